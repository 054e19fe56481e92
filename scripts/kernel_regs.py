"""Register, LDS and scratch use of the kernels in one unit's device assembly.

    make -C libspm_amd/csrc asm UNIT=scan_filter
    python scripts/kernel_regs.py libspm_amd/csrc/scan_filter.gfx950.s [REGEX]

REGEX selects kernels by their demangled name (default: all of them)."""
import re
import subprocess
import sys

if len(sys.argv) < 2:
    sys.exit(__doc__)
pat = sys.argv[2] if len(sys.argv) > 2 else ""
txt = open(sys.argv[1]).read()
fields = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
rows = []
for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
    rows.append((m.group(1), [re.search(rf"\.amdhsa_{f} (\d+)", m.group(2)).group(1) for f in fields]))
names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
print(f"{'kernel':90s} {'vgpr':>5s} {'sgpr':>5s} {'lds':>6s} {'scratch':>7s}")
for (_, (v, s, lds, sc)), d in zip(rows, names):
    d = d.replace("void spm_hip::", "").split("(")[0]
    if re.search(pat, d):
        print(f"{d[:90]:90s} {v:>5s} {s:>5s} {lds:>6s} {sc:>7s}")
