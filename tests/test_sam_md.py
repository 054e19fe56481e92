"""CPU: the MD string and the layout of spm_sam_extras (spm_hip_sam_md, no device needed).

The expected strings never come from the code under test.  The rule of spm_hip.h is written again here from the SAM
specification's description of MD (py_md): it does not look at the = / X of a transcript but compares the read with the
reference column by column, which is what a consumer without the transcript would do.  And for every case the reference
stretch is rebuilt from (SEQ, CIGAR, MD) alone and compared with the reference's slice: that is what MD is for."""
import re

import numpy as np

from cpp_programs import c_layout

INS, DEL, EQ, X = 1, 2, 7, 8
OP_CHAR = {INS: "I", DEL: "D", EQ: "=", X: "X"}
MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
OVERFLOW, INVALID = -5, -1


# ---------------------------------------------------------------------------------------------------------------------
# the rule again, and its inverse
# ---------------------------------------------------------------------------------------------------------------------
def letters(ranks, symbols="ACGT"):
    return "".join(symbols[r] if r < len(symbols) else "N" for r in np.asarray(ranks).tolist())


def cigar_of(words, merge=False):
    items = []
    for w in words:
        n, op = int(w) >> 4, OP_CHAR[int(w) & 15]
        if merge and op in "=X":
            if items and items[-1][1] == "M":
                items[-1][0] += n
                continue
            op = "M"
        items.append([n, op])
    return "".join(f"{n}{op}" for n, op in items)


def py_md(cigar, read, ref, begin, symbols="ACGT"):
    """MD of the alignment `cigar` (M, =, X, I, D) of the ranks `read` at reference position `begin`, by comparing columns"""
    out, c, q, r = [], 0, 0, int(begin)
    for n, op in re.findall(r"([0-9]+)([MIDX=])", cigar):
        n = int(n)
        if op == "I":
            q += n
        elif op == "D":
            out.append(f"{c}^{letters(ref[r:r + n], symbols)}")
            c, r = 0, r + n
        else:
            for i in range(n):
                if int(read[q + i]) == int(ref[r + i]):
                    c += 1
                else:
                    out.append(f"{c}{letters(ref[r + i:r + i + 1], symbols)}")
                    c = 0
            q, r = q + n, r + n
    return "".join(out) + str(c)


def rebuild_reference(seq, cigar, md):
    """the reference letters an alignment spans, from the line's SEQ (letters), CIGAR and MD alone"""
    columns = []                                                    # per reference position: None (as the read) or its letter
    for num, dele, sub in re.findall(r"([0-9]+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            columns += [None] * int(num)
        elif dele:
            columns += [("D", ch) for ch in dele]
        else:
            columns.append(("X", sub))
    columns = iter(columns)
    out, q = [], 0
    for n, op in re.findall(r"([0-9]+)([MIDX=])", cigar):
        n = int(n)
        if op == "I":
            q += n
            continue
        for _ in range(n):
            col = next(columns)
            if op == "D":
                assert col is not None and col[0] == "D", (cigar, md)
                out.append(col[1])
            else:
                assert col is None or col[0] == "X", (cigar, md)
                out.append(seq[q] if col is None else col[1])
                q += 1
    assert next(columns, "end") == "end" and q == len(seq), (cigar, md)
    return "".join(out)


def words_of(items):
    return np.array([n << 4 | op for n, op in items], dtype=np.uint32)


def random_alignment(rng, ref, sigma=4, max_words=12, max_run=40):
    """a transcript over a random stretch of ref and the read it describes -> (words, read ranks, begin)"""
    n_words = int(rng.integers(1, max_words + 1))
    ops, last = [], None
    for _ in range(n_words):
        op = int(rng.choice([o for o in (EQ, EQ, X, INS, DEL) if o != last]))
        last = op
        n = int(rng.integers(1, max_run + 1)) if op == EQ else int(rng.integers(1, 4)) if op != DEL else int(rng.integers(1, 9))
        ops.append((n, op))
    span = sum(n for n, op in ops if op != INS)
    begin = int(rng.integers(0, len(ref) - span + 1))
    read, r = [], begin
    for n, op in ops:
        if op == EQ:
            read += ref[r:r + n].tolist()
        elif op == X:
            read += [int((int(x) + 1 + int(rng.integers(0, sigma - 1))) % sigma) for x in ref[r:r + n]]
        elif op == INS:
            read += rng.integers(0, sigma, n).tolist()
        r += n if op != INS else 0
    return words_of(ops), np.array(read, dtype=np.uint8), begin


WORKED = [  # (transcript, the reference stretch it spans, MD)
    ([(20, EQ), (1, X), (11, EQ)], "T" * 20 + "G" + "T" * 11, "20G11"),
    ([(5, EQ), (2, X), (3, EQ), (2, DEL), (1, X), (4, EQ)], "TTTTT" + "AC" + "TTT" + "GT" + "A" + "TTTT", "5A0C3^GT0A4"),
    ([(3, X)], "ACG", "0A0C0G0"),
    ([(4, EQ), (2, INS), (4, EQ)], "CCCCCCCC", "8"),
    ([(30, INS)], "", "0"),
]


def _r(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
int main(void)
{
    printf("sizeof %zu\n", sizeof(spm_sam_extras));
    printf("qual %zu\n", offsetof(spm_sam_extras, qual));
    printf("n_qual %zu\n", offsetof(spm_sam_extras, n_qual));
    printf("reference %zu\n", offsetof(spm_sam_extras, reference));
    printf("flags %zu\n", offsetof(spm_sam_extras, flags));
    printf("reserved %zu\n", offsetof(spm_sam_extras, reserved));
    printf("SPM_SAM_MD %u\n", SPM_SAM_MD);
    return 0;
}
"""


def test_extras_layout_matches_the_header(spm, tmp_path):
    import ctypes
    got = {k: int(v) for k, v in c_layout(tmp_path, LAYOUT_C).items()}
    E = spm.capi.SamExtras
    assert got.pop("sizeof") == ctypes.sizeof(E) == 32
    assert got.pop("SPM_SAM_MD") == spm.capi.SAM_MD == 1
    assert got == {name: getattr(E, name).offset for name, _t in E._fields_}
    for name in ("spm_hip_jst_ref_loci_sam_ex", "spm_hip_jst_ref_loci_bam_ex", "spm_hip_sam_md"):
        assert name in spm.capi.EXPORTS


def test_python_rule_on_the_worked_cases():
    for items, stretch, md in WORKED:
        ref = np.concatenate([_r("GATTACA"), _r(stretch), _r("CAT")])
        words = words_of(items)
        read, r = [], 7
        for n, op in items:
            if op == EQ:
                read += ref[r:r + n].tolist()
            elif op == X:
                read += [(int(x) + 2) & 3 for x in ref[r:r + n]]
            elif op == INS:
                read += [1] * n
            r += n if op != INS else 0
        for merge in (False, True):
            assert py_md(cigar_of(words, merge), read, ref, 7) == md, (items, merge)
        assert rebuild_reference(letters(read), cigar_of(words), md) == stretch
        assert MD_RE.fullmatch(md)


def test_worked_cases(spm):
    for items, stretch, md in WORKED:
        ref = np.concatenate([_r("GATTACA"), _r(stretch), _r("CAT")])
        assert spm.sam_md(words_of(items), ref, 7) == md, items
    assert spm.sam_md([], _r("ACGT"), 2) == "0"
    assert spm.sam_md(words_of([(2, X)]), np.array([4, 9], np.uint8), 0) == "0N0N0"            # a rank >= sigma prints N
    assert spm.sam_md(words_of([(1, EQ), (2, DEL)]), _r("ACG"), 0, symbols="acgt") == "1^cg0"


def test_random_transcripts_against_the_python_rule_and_back(spm):
    rng = np.random.default_rng(2001)
    ref = rng.integers(0, 4, 3000, dtype=np.uint8)
    ref[rng.integers(0, len(ref), 40)] = 4                          # some N
    shapes = set()
    for i in range(3000):
        words, read, begin = random_alignment(rng, ref)
        got = spm.sam_md(words, ref, begin, "ACGT")
        cig = cigar_of(words)
        assert got == py_md(cig, read, ref, begin) == py_md(cigar_of(words, True), read, ref, begin), (i, cig, begin)
        assert MD_RE.fullmatch(got), got
        span = sum(int(w) >> 4 for w in words if int(w) & 15 != INS)
        assert rebuild_reference(letters(read), cig, got) == letters(ref[begin:begin + span]), (i, cig, got)
        ops = [int(w) & 15 for w in words]
        shapes |= {"begins_x"} if ops[0] == X else set()
        shapes |= {"ends_x"} if ops[-1] == X else set()
        shapes |= {"d_then_x"} if any(a == DEL and b == X for a, b in zip(ops, ops[1:])) else set()
        shapes |= {"eq_i_eq"} if any(t == (EQ, INS, EQ) for t in zip(ops, ops[1:], ops[2:])) else set()
        shapes |= {"all_i"} if ops == [INS] else set()
        shapes |= {"n"} if "N" in got else set()
    assert shapes == {"begins_x", "ends_x", "d_then_x", "eq_i_eq", "all_i", "n"}, shapes


def test_buffer_protocol_and_refusals(spm):
    import ctypes as C
    lib = spm.capi.lib()
    ref = _r("ACGTACGTAC")
    words = words_of([(3, EQ), (1, X), (2, DEL), (2, EQ)])
    want = spm.sam_md(words, ref, 1)
    assert want == "3A0^CG2"
    wp, rp = words.ctypes.data_as(C.POINTER(C.c_uint32)), ref.ctypes.data_as(C.POINTER(C.c_uint8))
    need = C.c_uint64()
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 1, b"ACGT", None, 0, C.byref(need)) == OVERFLOW and need.value == len(want)
    buf = C.create_string_buffer(b"#" * 16, 16)
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 1, b"ACGT", buf, len(want) - 1, C.byref(need)) == OVERFLOW
    assert buf.raw == b"#" * 16                                     # short by one byte: nothing is written
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 1, b"ACGT", buf, len(want), C.byref(need)) == 0
    assert buf.raw == want.encode() + b"#" * (16 - len(want))       # exact: not a byte beyond
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 2, b"ACGT", buf, 16, C.byref(need)) == 0   # ends at the last symbol
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 3, b"ACGT", buf, 16, C.byref(need)) == INVALID   # leaves the reference
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 11, b"ACGT", buf, 16, C.byref(need)) == INVALID
    assert lib.spm_hip_sam_md(None, 1, rp, len(ref), 0, b"ACGT", buf, 16, C.byref(need)) == INVALID
    assert lib.spm_hip_sam_md(wp, len(words), None, len(ref), 0, b"ACGT", buf, 16, C.byref(need)) == INVALID
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 0, None, buf, 16, C.byref(need)) == INVALID
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 0, b"ACGT", buf, 16, None) == INVALID
    assert lib.spm_hip_sam_md(wp, len(words), rp, len(ref), 0, b"ACGT", None, 16, C.byref(need)) == INVALID
    try:
        spm.sam_md(words, ref, 3)
    except spm.SpmError as e:
        assert "spm_hip_sam_md" in str(e)
    else:
        raise AssertionError("a transcript that leaves the reference was accepted")


def test_sam_extras_of_the_binding(spm):
    assert spm.sam_extras() == (None, None)
    e, keep = spm.sam_extras(np.array([[1, 2, 3], [4, 5, 93]], np.uint8))
    assert (e.n_qual, e.flags, e.reserved, e.reference) == (6, 0, 0, None) and keep.tolist() == [1, 2, 3, 4, 5, 93] and e.qual == keep.ctypes.data
    e, keep = spm.sam_extras([np.array([7], np.uint8), np.array([8, 9], np.uint8)], md=True)
    assert (e.n_qual, e.flags) == (3, 1) and keep.tolist() == [7, 8, 9]
