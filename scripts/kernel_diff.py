"""Device code of two builds, kernel by kernel: is every kernel of the parent in the child, instruction for instruction?

    make -C libspm_amd/csrc asm UNIT=...          (in both trees, for every unit that holds device code)
    python scripts/kernel_diff.py PARENT.s CHILD.s [PARENT2.s CHILD2.s ...]

The listings are taken in pairs, but kernels are matched by mangled name across ALL parent files and ALL child files: a
kernel may move from one unit to another.  (Where a unit was split, name the parent's listing once per child listing: a
file given twice counts once.)  Per kernel the
comparison drops comments and debug directives and renames local labels (.LBB3_7, .Ltmp12, ..) in order of appearance,
since their numbers depend on what else the unit holds; for the same reason an unnamed string constant (.str.9) is compared
by what it holds, not by its number.  It prints one line per kernel: `identical`, or the instruction
counts parent -> child, VGPR, SGPR, LDS, scratch and the lines removed / added.  Exit status 1 if any kernel differs or is
missing on either side."""
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_regs import demangled, kernel_table  # noqa: E402

_DEBUG = re.compile(r"\.(loc|file|cfi_\w+|ident|addrsig\w*)\b")
_LABEL = re.compile(r"\.L[\w$.]+")
_STRING = re.compile(r"(?<![\w.])\.str(?:\.\d+)?(?![\w.])")


def string_constants(txt):
    """{symbol: its directive} of the unit's unnamed string constants (.str, .str.1, ..): numbered like the local labels."""
    return dict(re.findall(r"^(\.str(?:\.\d+)?):\n\s*(\.asci[iz]\s.*)$", txt, re.M))


def kernel_body(txt, name):
    """The normalised lines of kernel `name`: from its entry label to its descriptor (compared apart) or its end label."""
    m = re.search(rf"^{re.escape(name)}:.*?$(.*?)^(\.Lfunc_end\d+:|\s*\.amdhsa_kernel )", txt, re.S | re.M)
    if not m:
        return None
    lines, labels, strings = [], {}, string_constants(txt)
    for line in m.group(1).split("\n"):
        line = line.split(";")[0].strip()
        if not line or _DEBUG.match(line):
            continue
        line = _STRING.sub(lambda s: "{" + strings.get(s.group(0), s.group(0)) + "}", line)  # the constant for its number
        lines.append(_LABEL.sub(lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line))
    return lines


def instructions(lines):
    return sum(1 for l in lines if not l.startswith(".") and not l.endswith(":"))


def kernels(texts):
    """{mangled name: (normalised body, [vgpr, sgpr, lds, scratch])} over several listings."""
    out = {}
    for txt in texts:
        for name, regs in kernel_table(txt):
            out[name] = (kernel_body(txt, name), regs)
    return out


def compare(parent_texts, child_texts, out=sys.stdout):
    """Prints the per-kernel lines; -> (kernels compared, kernels that differ or are missing)."""
    P, C = kernels(parent_texts), kernels(child_texts)
    names = sorted(set(P) | set(C))
    bad = 0
    for name, shown in zip(names, demangled(names)):
        if name not in P or name not in C or P[name][0] is None or C[name][0] is None:
            bad += 1
            print(f"{shown}: missing in the {'parent' if name not in P or P[name][0] is None else 'child'}", file=out)
            continue
        (pb, pr), (cb, cr) = P[name], C[name]
        if pb == cb and pr == cr:
            print(f"{shown}: identical", file=out)
            continue
        bad += 1
        d = [l for l in difflib.unified_diff(pb, cb, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        regs = ", ".join(f"{f} {a}" if a == b else f"{f} {a}->{b}" for f, a, b in zip(("VGPR", "SGPR", "LDS", "scratch"), pr, cr))
        print(f"{shown}: instructions {instructions(pb)}->{instructions(cb)}, {regs}, "
              f"-{sum(l.startswith('-') for l in d)} / +{sum(l.startswith('+') for l in d)} lines", file=out)
    print(f"{len(names)} kernels, {len(names) - bad} identical, {bad} differing or missing", file=out)
    return len(names), bad


def main(argv):
    files = argv[1:]
    if not files or len(files) % 2:
        sys.exit(__doc__)
    read = lambda paths: [open(p).read() for p in paths]
    return 1 if compare(read(files[0::2]), read(files[1::2]))[1] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
