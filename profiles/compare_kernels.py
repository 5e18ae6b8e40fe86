#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of one translation unit (no GPU needed): for every kernel both objects
hold, the metadata (VGPRs, SGPRs, spills, scratch, static LDS) and a hash of the disassembled instructions.
usage: python profiles/compare_kernels.py <parent.o> <branch.o>   -> one line per kernel that differs, then a summary"""
import hashlib
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_object


def kernels(obj):
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                             capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]
        meta[g("name")] = tuple(g(k) for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                                               "private_segment_fixed_size", "group_segment_fixed_size"))
    text = {}
    name = None
    after_getpc = -1
    for line in dis.splitlines():
        m = re.match(r"^<?([_A-Za-z][\w.$]*)>?:$", line.strip())
        if m:
            name = m.group(1)
            text[name] = hashlib.sha1()
            continue
        if name and line.strip():
            # the trailing comment holds the instruction's address and encoding, and the two additions behind an
            # s_getpc_b64 hold the distance to a called function: both move with the kernel's place in the object
            ins = line.split("//")[0].strip()
            after_getpc = 2 if ins.startswith("s_getpc_b64") else after_getpc - 1
            if 0 <= after_getpc < 2 and ins.startswith(("s_add_u32", "s_addc_u32")):
                ins = re.sub(r"0x[0-9a-fA-F]+|\b\d+$", "REL", ins)
            text[name].update(ins.encode())
    return {k: (meta[k], text[k].hexdigest() if k in text else "?") for k in meta}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    both = sorted(set(a) & set(b))
    differ = [k for k in both if a[k] != b[k]]
    for k in differ:
        print(f"DIFFERS {k[:150]}\n  parent {a[k][0]}\n  branch {b[k][0]}")
    print(f"{len(both)} kernels in both objects, {len(differ)} differ; only in parent: {len(set(a) - set(b))}; "
          f"only in branch: {len(set(b) - set(a))}")
    for k in sorted(set(b) - set(a)):
        print(f"  new: {k[:150]}  (vgpr, sgpr, sgpr spills, vgpr spills, scratch, lds) = {b[k][0]}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
