#!/usr/bin/env python
"""Are the gfx950 kernels of two builds of the library the same machine code?  (A refactor that only moves source must say yes.)

    python profiles/tools/code_identity.py BEFORE.so AFTER.so

Extracts the code objects the way tests/shake_standalone.py::kernel_inventory does (`llvm-objdump --offloading`), disassembles them
and compares, kernel by kernel: the instruction stream with addresses and encodings stripped, and the descriptor values of the
metadata note (VGPR / SGPR / AGPR counts, LDS bytes, scratch bytes, workgroup size).  Kernel order inside a code object is free.
Exit status 0 only if the kernel sets are equal and every kernel is identical.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = "/opt/rocm/llvm/bin"
DESCRIPTOR = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
              "sgpr_spill_count", "max_flat_workgroup_size", "kernarg_segment_size", "uses_dynamic_stack")


def kernels_of(lib_path):
    """{kernel symbol: (instruction lines, descriptor dict)} over every gfx950 code object in the library."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib_path, copy)
        subprocess.check_call([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", copy], stdout=subprocess.DEVNULL)
        objects = [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "amdgcn" in f]
        assert objects, "no gfx950 code object in " + lib_path
        for obj in objects:
            code, current = {}, None
            for line in subprocess.check_output([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", obj]).decode().splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    current = code.setdefault(m.group(1), [])
                elif current is not None and line.strip():
                    current.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())    # the comment holds address and encoding
            notes = subprocess.check_output([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", obj]).decode()
            for block in notes.split("\n  - .agpr_count:")[1:]:         # one list item of amdhsa.kernels per kernel
                values = dict(re.findall(r"^    \.(\w+): +(\S+)$", "    .agpr_count:" + block, re.M))   # its own fields, not .args'
                sym = values["symbol"][:-len(".kd")]
                assert sym in code and sym not in out, sym
                text = code[sym]
                while text and text[-1] in ("s_nop 0", "s_code_end", "..."):   # padding behind the kernel; the last one's runs to the section end
                    text = text[:-1]
                out[sym] = (text, {k: values[k] for k in DESCRIPTOR})
    return out


def main(before, after):
    a, b = kernels_of(before), kernels_of(after)
    print(f"{before}: {len(a)} kernels; {after}: {len(b)} kernels")
    bad = 0
    for sym in sorted(set(a) ^ set(b)):
        print(f"ONLY IN {'BEFORE' if sym in a else 'AFTER'}: {sym}")
        bad += 1
    for sym in sorted(set(a) & set(b)):
        if a[sym][1] != b[sym][1]:
            print(f"DESCRIPTOR DIFFERS: {sym}: {a[sym][1]} != {b[sym][1]}")
            bad += 1
        if a[sym][0] != b[sym][0]:
            first = next((i for i, (x, y) in enumerate(zip(a[sym][0], b[sym][0])) if x != y), min(len(a[sym][0]), len(b[sym][0])))
            print(f"CODE DIFFERS: {sym}: {len(a[sym][0])} vs {len(b[sym][0])} instructions, first difference at {first}")
            bad += 1
    n_instr = sum(len(v[0]) for v in a.values())
    print(f"{'IDENTICAL' if not bad else 'DIFFERENT'}: {len(set(a) & set(b))} common kernels, {n_instr} instructions before, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
