"""Register, LDS and scratch use of the kernels in one unit's device assembly.

    make -C libspm_amd/csrc asm UNIT=filter_stream
    python scripts/kernel_regs.py libspm_amd/csrc/filter_stream.gfx950.s [REGEX]

REGEX selects kernels by their demangled name (default: all of them).  The units that hold the seed filter's kernels are
filter_stream, filter_dense, filter_resolve and filter_verify; scan_brute holds the brute-force kernels, jst, select,
jst_select, align, bgzf, bam_index, text, patterns, hits and comm their own.  scripts/kernel_diff.py compares two builds kernel by
kernel and reads the listings through kernel_table() below."""
import re
import subprocess
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernel_table(txt):
    """[(mangled name, [vgpr, sgpr, lds, scratch] as strings)] for every .amdhsa_kernel block of a listing, in file order."""
    rows = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        rows.append((m.group(1), [re.search(rf"\.amdhsa_{f} (\d+)", m.group(2)).group(1) for f in FIELDS]))
    return rows


def demangled(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    except OSError:  # no binutils: the mangled names will do
        out = list(names)
    return [d.replace("void spm_hip::", "").split("(")[0] for d in out[:len(names)]]


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    pat = argv[2] if len(argv) > 2 else ""
    rows = kernel_table(open(argv[1]).read())
    print(f"{'kernel':90s} {'vgpr':>5s} {'sgpr':>5s} {'lds':>6s} {'scratch':>7s}")
    for (_, (v, s, lds, sc)), d in zip(rows, demangled([r[0] for r in rows])):
        if re.search(pat, d):
            print(f"{d[:90]:90s} {v:>5s} {s:>5s} {lds:>6s} {sc:>7s}")


if __name__ == "__main__":
    main(sys.argv)
