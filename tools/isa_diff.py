"""Kernel-by-kernel diff of two `make -C opencv-opencl_amd/csrc asm` outputs (parent, branch): labels renumbered, names of the
default-policy fused instantiations mapped onto their parent names; for every kernel only the branch has, its memory
instructions by cache-policy bits, VGPRs and scratch.
    python tools/isa_diff.py parent.s branch.s"""
import re,sys,collections
def kernels(path):
    out={}; cur=None; body=[]
    for line in open(path):
        m=re.match(r'^(_Z\w+):\s*(;.*)?$',line)
        if m:
            cur=m.group(1); body=[]; out[cur]=body; continue
        if cur is None: continue
        if line.startswith('.Lfunc_end'): cur=None; continue
        s=line.split(';')[0].strip()
        if not s or s.startswith('.') and not s.startswith('.LBB'): continue
        body.append(re.sub(r'\.LBB\d+_', '.LBB_', s))
    return out
def meta(path):
    d={}
    txt=open(path).read()
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel',txt,re.S):
        b=m.group(2)
        g=lambda k: re.search(k+r' (\d+)',b)
        d[m.group(1)]=dict(vgpr=int(g(r'\.amdhsa_next_free_vgpr').group(1)),scratch=int(g(r'\.amdhsa_private_segment_fixed_size').group(1)))
    return d
P,B=kernels(sys.argv[1]),kernels(sys.argv[2])
mp,mb=meta(sys.argv[1]),meta(sys.argv[2])
def key(n): return re.sub(r'(equalize_fused_kernelILi\d+)ELi0E',r'\1E',n)
Bk={key(n):n for n in B}
same=diff=0
for n in P:
    bn=Bk.get(key(n))
    if bn is None: print('MISSING in branch',n); continue
    pb=[l.replace(n,'K') for l in P[n]]; bb=[l.replace(bn,'K') for l in B[bn]]
    if pb==bb and mp[n]==mb[bn]: same+=1
    else: diff+=1; print('DIFF',n,len(pb),len(bb),mp[n],mb[bn])
print('parent kernels',len(P),'identical',same,'different',diff)
Pk={key(n) for n in P}
new=[n for n in B if key(n) not in Pk]
for n in new:
    body=B[n]
    c=collections.Counter()
    for l in body:
        m=re.match(r'(buffer_(?:load|store)_\w+|global_(?:load|store|atomic)_\w+|buffer_atomic\w+|flat_\w+)',l)
        if m:
            flags=' '.join(f for f in ('nt','sc0','sc1') if re.search(r'\b'+f+r'\b',l))
            c[(m.group(1),flags)]+=1
    print(n,mb[n])
    for k,v in sorted(c.items()): print('    ',k,v)
