#!/usr/bin/env python3
"""Static mnemonic histogram of the (single) search kernel in each `hipcc -S --cuda-device-only` output given: the whole
kernel, and its hop loop -- the largest backward-branch region that holds the gather's 16 global_load_dwordx4.
usage: python profiles/hop_mnemonics.py parent.s branch.s [...]"""
import collections
import re
import sys

def load(p):
    L = [l.rstrip() for l in open(p)]
    s = next(i for i,l in enumerate(L) if re.match(r'^_ZN4dann\S*:', l))
    e = next(i for i in range(s, len(L)) if L[i].strip().startswith('s_endpgm'))
    # keep going to the last s_endpgm before .Lfunc_end
    fe = next(i for i in range(s, len(L)) if L[i].startswith('.Lfunc_end'))
    return L[s:fe]
def mn(l):
    t = l.strip()
    if not t or t.startswith(('.', ';', '_Z')) or t.endswith(':'): return None
    return t.split()[0]
def loops(L):
    lab = {m.group(1): i for i,l in enumerate(L) if (m := re.match(r'^(\.LBB\d+_\d+):', l))}
    out = []
    for i,l in enumerate(L):
        m = re.search(r's_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)', l)
        if m:
            t = lab.get(m.group(1) or m.group(2))
            if t is not None and t < i: out.append((t, i))
    return out
KEYS = ['s_and_saveexec_b64','s_or_saveexec_b64','s_cbranch_execz','s_cbranch_execnz','s_cbranch_scc0','s_cbranch_scc1','s_cbranch_vccz','s_cbranch_vccnz','s_branch','s_or_b64','s_and_b64','s_andn2_b64','s_xor_b64','s_mov_b64','v_readlane_b32','v_writelane_b32','v_readfirstlane_b32','v_cndmask_b32_e32','v_cndmask_b32_e64','s_barrier','s_waitcnt']
def report(p):
    L = load(p)
    ls = loops(L)
    def nload(a,b): return sum(1 for l in L[a:b+1] if 'global_load_dwordx4' in l)
    big = [x for x in ls if nload(*x) >= 16]
    # the hop loop: the outermost backward branch region holding the gather (largest span)
    hop = max(big, key=lambda x: x[1]-x[0]) if big else (0, len(L)-1)
    res = {}
    for name, (a,b) in (('kernel', (0, len(L)-1)), ('hop', hop)):
        c = collections.Counter(m for l in L[a:b+1] if (m := mn(l)))
        tot = sum(c.values())
        sal = sum(v for k,v in c.items() if k.startswith('s_') and not k.startswith(('s_cbranch','s_branch','s_waitcnt','s_nop','s_load','s_buffer_load','s_barrier','s_endpgm')))
        br = sum(v for k,v in c.items() if k.startswith(('s_cbranch','s_branch')))
        val = sum(v for k,v in c.items() if k.startswith('v_'))
        lds = sum(v for k,v in c.items() if k.startswith('ds_'))
        vm = sum(v for k,v in c.items() if k.startswith(('global_','flat_','buffer_')))
        res[name] = (c, dict(lines=b-a+1, total=tot, VALU=val, SALU=sal, branch=br, LDS=lds, VMEM=vm))
    return res
cols = sys.argv[1:]
R = [report(p) for p in cols]
for region in ('hop', 'kernel'):
    print(f'## {region} (static instruction counts)')
    print('mnemonic'.ljust(24) + ''.join(c.rsplit('/',1)[-1].ljust(24) for c in cols))
    for k in ['lines','total','VALU','SALU','branch','LDS','VMEM']:
        print(k.ljust(24) + ''.join(str(r[region][1][k]).ljust(24) for r in R))
    for k in KEYS:
        print(k.ljust(24) + ''.join(str(r[region][0].get(k,0)).ljust(24) for r in R))
