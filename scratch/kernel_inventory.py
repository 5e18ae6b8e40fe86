"""One sorted line per gfx950 kernel of a translation unit: mangled name, VGPRs, SGPRs, AGPRs, private and group
segment bytes, and a hash of the kernel's disassembly.  Two inventories of one unit, before and after a change to host
code, are compared with diff: equal lines mean the same set of kernels and the same machine code for each.

    python scratch/kernel_inventory.py diskann_amd/csrc/paged_kernels.hip > paged.inv

A `.hip` argument is compiled device-only and unbundled with build.py's flags.  An object file that build.py left in
diskann_amd/build/ is accepted too: its gfx950 code object is taken out of the fat binary instead of compiled again.
It hashes and compares; it inspects nothing.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diskann_amd.build import FLAGS, _hipcc  # noqa: E402

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def code_object(src, tmp):
    co = os.path.join(tmp, "unit.co")
    if src.endswith(".o"):
        fb = os.path.join(tmp, "unit.hipfb")
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, src,
            os.path.join(tmp, "unit.o"))  # (with no output file llvm-objcopy rewrites its input)
        run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb,
            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co)
    else:
        run(_hipcc(), *FLAGS, "--offload-device-only", "--no-gpu-bundle-output", "-c", src, "-o", co)
    return co


def resources(co):
    """kernel name -> (vgpr, sgpr, agpr, private, group) from the code object's metadata note"""
    res, cur = {}, {}
    keys = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
    for line in run(os.path.join(LLVM, "llvm-readobj"), "--notes", co).splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s+(\S+)\s*$", line)
        if not m:
            continue
        k, v = m.groups()
        if k == ".name":
            cur["name"] = v.strip("'\"")
        elif k in keys:
            cur[k] = int(v)
        if k == ".wavefront_size":  # the last key of a kernel's map (keys are sorted; .name of an argument is earlier)
            res[cur.pop("name")] = tuple(cur.pop(x, 0) for x in keys)
            cur = {}
    return res


def hashes(co, kernels):
    """kernel name -> sha256 of its instructions: addresses, encodings and comments left out, the padding that follows
    the last instruction stripped, and the pc-relative offset of a constant table (the literal added to s_getpc_b64's
    result) masked, since like a branch target's address it moves with the order of the kernels in the file"""
    body, cur, getpc = {}, None, False
    text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-leading-addr", "--no-show-raw-insn", co)
    for line in text.splitlines():
        line = re.sub(r"\s*//.*$", "", line).strip()
        m = re.match(r"^<(.+)>:$", line)
        if m:
            cur = body.setdefault(m.group(1), []) if m.group(1) in kernels else None
        elif cur is not None and line:
            if getpc:
                line = re.sub(r"^(s_add_u32 \S+ \S+) 0x[0-9a-f]+$", r"\1 <pcrel>", line)
            getpc = line.startswith("s_getpc_b64")
            cur.append(line)
    out = {}
    for name, lines in body.items():
        while lines and (lines[-1] == "..." or lines[-1].startswith("s_nop") or lines[-1].startswith("s_code_end")):
            lines.pop()
        out[name] = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(sys.argv[1], tmp)
        res = resources(co)
        hs = hashes(co, res)
    for name in sorted(res):
        v, s, a, p, g = res[name]
        print(f"{name} vgpr {v} sgpr {s} agpr {a} private {p} group {g} sha {hs.get(name, 'missing')}")


if __name__ == "__main__":
    main()
