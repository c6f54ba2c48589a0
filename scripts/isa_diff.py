"""Compare the device ISA of two builds function by function and kernel descriptor by kernel descriptor.
    for d in ...: hipcc --offload-arch=gfx950 -O3 -std=c++17 -DMF_D=$d --cuda-device-only -S mf_inst.hip -o DIR/inst_d$d.s   (both trees)
    python3 scripts/isa_diff.py DIR_A DIR_B        -> one DIFF line per function or descriptor whose text differs
Instruction text is compared without comments, .loc / .file / .cfi lines; files are matched by name."""
import re, sys, glob, os, hashlib
def funcs(path):
    out = {}; cur = None; buf = []
    for line in open(path, errors='replace'):
        m = re.match(r'^(_Z[\w$.]+):', line)
        if m and cur is None:
            cur = m.group(1); buf = []; continue
        if cur is not None:
            if line.startswith('.Lfunc_end'):
                out[cur] = buf; cur = None; continue
            l = line.split(';')[0].rstrip()
            if not l.strip() or l.strip().startswith(('.loc', '.file', '.cfi')): continue
            buf.append(l)
    # kernel descriptors
    for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', open(path, errors='replace').read(), re.S):
        out['desc:' + m.group(1)] = [l.strip() for l in m.group(2).split('\n')]
    return out
P, B = sys.argv[1], sys.argv[2]
tot = same = 0; diffs = []
for fb in sorted(glob.glob(B + '/*.s')):
    fp = os.path.join(P, os.path.basename(fb))
    if not os.path.exists(fp): print('missing parent', fp); continue
    a, b = funcs(fp), funcs(fb)
    for k in sorted(set(a) | set(b)):
        tot += 1
        if a.get(k) == b.get(k): same += 1
        else: diffs.append((os.path.basename(fb), k, len(a.get(k, [])), len(b.get(k, []))))
    print(os.path.basename(fb), 'functions+descriptors', len(set(a) | set(b)))
print('total', tot, 'identical', same)
for d in diffs: print('DIFF', *d)
