#!/bin/bash
# tools/gpu_suite.sh <label> [pytest args...] -- the GPU test suite, ONE pytest process, with whatever a GPU fault leaves behind
# brought home.  The HSA runtime writes `gpucore.<pid>` into the working directory when a GPU memory fault ends the process, and
# only the output directory comes back from the box, which is how round 3's gpucore.790 was lost.  After the run every core found
# is compressed and copied next to the test log when it fits in 40 MiB, to be examined off the box.  Never loops, never retries.
label=${1:?usage: tools/gpu_suite.sh <label> [pytest args...]}
shift
cd "$(dirname "$0")/.." || exit 2
mkdir -p gpurun_out
rm -f gpucore.*
python -m pytest tests -m gpu -x -q "$@" > "gpurun_out/${label}_gpu_tests.txt" 2>&1
rc=$?
tail -n 6 "gpurun_out/${label}_gpu_tests.txt"
for core in gpucore.*; do
    [ -e "$core" ] || continue
    gzip -1 -c "$core" > "/tmp/${core}.gz" && [ "$(stat -c %s "/tmp/${core}.gz")" -le $((40 << 20)) ] && cp "/tmp/${core}.gz" "gpurun_out/${label}_${core}.gz"
    echo "GPU core $core found"
done
exit $rc
