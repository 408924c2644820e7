"""The register, scratch, LDS and occupancy figures of every k_ism_* instantiation from hipcc's resource remarks, two builds side by side.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c -Rpass-analysis=kernel-resource-usage \
        audiblelight_amd/csrc/al_kernels.hip -o /dev/null 2> after.log        (the same at the commit before: before.log)
    python profiles/tools/shoebox_kernel_resources.py before.log after.log > profiles/shoebox_kernel_resources.txt

A kernel that exists in one build only has dashes in the other's columns.  No GPU is needed.
"""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPR"), ("TotalSGPRs", "SGPR"), ("SGPRs Spill", "sspill"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "waves"))


def resources(path):
    table, name = {}, None
    for line in open(path):
        m = re.search(r"remark: .*?: +(Function Name|[A-Za-z][A-Za-z /\[\]]*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2) if "k_ism_" in m.group(2) else None
            if name:
                table[name] = {}
        elif name:
            table[name][m.group(1)] = m.group(2)
    return table


def main(before_log, after_log):
    before, after = resources(before_log), resources(after_log)
    names = sorted(set(before) | set(after))
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    plain = [re.sub(r"^(void )?al::|\(al::\w+\)$", "", p) for p in plain]
    width = max(len(p) for p in plain)
    cols = "".join(f"{short:>8}" for _, short in FIELDS)
    print(f"{'kernel':<{width}} |{cols} |{cols} | note")
    print(f"{'':<{width}} |{'before':>{8 * len(FIELDS)}} |{'after':>{8 * len(FIELDS)}} |")
    for name, shown in sorted(zip(names, plain), key=lambda pair: pair[1]):
        b, a = before.get(name), after.get(name)
        row = lambda r: "".join(f"{(r[key] if r else '-'):>8}" for key, _ in FIELDS)     # noqa: E731
        note = ""
        if a and b:
            worse = [short for key, short in FIELDS[3:5] if int(a[key]) > int(b[key])] + (["waves"] if int(a[FIELDS[5][0]]) < int(b[FIELDS[5][0]]) else [])
            moved = [short for key, short in FIELDS[:2] if a[key] != b[key]]
            note = "WORSE: " + ", ".join(worse) if worse else ("moved: " + ", ".join(moved) if moved else "")
        print(f"{shown:<{width}} |{row(b)} |{row(a)} | {note}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
