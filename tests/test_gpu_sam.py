"""SAM lines and MAPQ on the device: spm_hip_jst_ref_loci_sam behind the chain ... -> collapse -> reads [-> pairs [-> rescue]],
and its Python binding.

The expected text never comes from the code under test.  The rule of spm_hip.h is written again here (np_sam): the MAPQ
policy, which line a read reports with and without a used rescue, the mate fields, the secondary lines, every field of a line
with Python's own formatting.  Text and line records are compared byte for byte, in the host view and in the device view, and
across two calls.  Independently of that rule every line is matched against the SAM 1.6 grammar, and its CIGAR against its SEQ
and the reference range of its source."""
import copy
import ctypes
import re

import numpy as np
import pytest

from cpp_programs import download
from test_pairs import MAX_TLEN, MIN_TLEN, _chain, _free_stretches, _planted_chain, _planted_pairs
from test_jst_project import _make_tree, _plant
from test_rescue import K, K_SEARCH, NOT_CONCORDANT, NOTHING, RESCUED, _chain_of, _diverge, _planted_rescue, stranded
from test_sam import LINE, np_mapq
from test_strands import np_revcomp

gpu = pytest.mark.gpu
NONE = 0xFFFFFFFF
UNMAPPED, LOCUS, RESCUE, SECONDARY = 0, 1, 2, 3
COUNTS = ("n_lines", "n_bytes", "n_reported", "n_secondary", "n_unmapped", "n_rescue_lines")
UNSUPPORTED = -4


# ---------------------------------------------------------------------------------------------------------------------
# the rule again
# ---------------------------------------------------------------------------------------------------------------------
def np_cigar(words, merge):
    items = []
    for w in words:
        n, op = int(w) >> 4, {1: "I", 2: "D", 7: "=", 8: "X"}[int(w) & 15]
        if merge and op in "=X":
            if items and items[-1][1] == "M":
                items[-1][0] += n
                continue
            op = "M"
        items.append([n, op])
    return "".join(f"{n}{op}" for n, op in items)


def np_sam(loci, ops, members, reads, pairs, rescues, rescue_ops, needles, names, opts):
    """-> (the lines as bytes, the line records).  opts: dict(rname, symbols, strands, cigar_m, secondary, unique, multi);
    pairs / rescues / names may be None.  members: the member pool of the loci (XN is its share per locus)."""
    strands, symbols, merge = opts["strands"], opts["symbols"], opts["cigar_m"]
    unique, multi = opts.get("unique") or (60, 40, 30, 20), opts.get("multi") or (3, 1, 1, 0)
    paired = pairs is not None
    n_reads = len(reads)
    assert int(loci["n_haplotypes"].sum()) == len(members)
    mapq = lambda nb, nn: np_mapq(int(nb), int(nn), unique, multi)
    seq = lambda p: "".join(symbols[r] if r < len(symbols) else "N" for r in needles[p].tolist())
    words_of = lambda rec, pool: pool[int(rec["cigar_off"]):int(rec["cigar_off"]) + int(rec["cigar_len"])]
    qname = lambda r: (names[r // 2 if paired else r] if names is not None else str(r // 2 if paired else r))

    # ---- the reported line of every read: (kind, source, flag, mapq, x0, x1, pos, reverse), and its TLEN ----
    rep, tlen = [None] * n_reads, [0] * n_reads
    nothing = lambda flag: (UNMAPPED, NONE, flag, 0, 0, 0, 0, False)

    def locus_line(i, flag, nb, nn):
        return (LOCUS, i, flag, mapq(nb, nn), int(nb), int(nn), int(loci["ref_begin"][i]) + 1, bool(strands == 2 and loci["pattern"][i] & 1))

    if not paired:
        for r, R in enumerate(reads):
            i = int(R["primary"])
            rep[r] = nothing(4) if i == NONE else locus_line(i, 16 if strands == 2 and loci["pattern"][i] & 1 else 0, R["n_best"], R["n_next"])
    else:
        used_of = {}
        for j, U in enumerate(rescues if rescues is not None else []):
            if U["status"] == RESCUED:
                p = int(U["pair"])
                if p not in used_of or int(U["score"]) < int(rescues[used_of[p]]["score"]):
                    used_of[p] = j
        for p, P in enumerate(pairs):
            M = (reads[2 * p], reads[2 * p + 1])
            locus, flag = (int(P["locus1"]), int(P["locus2"])), (int(P["flag1"]), int(P["flag2"]))
            if p in used_of:
                j = used_of[p]
                U = rescues[j]
                y = (int(U["pattern"]) >> 1) & 1                   # the rescued mate
                a = 1 - y
                nb, nn = int(M[a]["n_best"]), int(M[a]["n_next"])  # both lines: the anchor read's counts
                q = mapq(nb, nn)
                rep[2 * p + y] = (RESCUE, j, int(U["flag"]), q, nb, nn, int(U["ref_begin"]) + 1, bool(U["flag"] & 0x10))
                f = ((flag[a] | 0x2) & ~0x8 & ~0x20) | (0x20 if U["flag"] & 0x10 else 0)
                A = int(U["anchor"])
                assert A == locus[a]
                rep[2 * p + a] = (LOCUS, A, f, q, nb, nn, int(loci["ref_begin"][A]) + 1, bool(loci["pattern"][A] & 1))
                t = int(U["tlen"])
            else:
                proper = bool(flag[0] & 2)
                for x in (0, 1):
                    if locus[x] == NONE:
                        rep[2 * p + x] = nothing(flag[x])
                    else:
                        nb, nn = (P["n_best"], P["n_next"]) if proper else (M[x]["n_best"], M[x]["n_next"])
                        rep[2 * p + x] = locus_line(locus[x], flag[x], nb, nn)
                t = int(P["tlen"])
            tlen[2 * p], tlen[2 * p + 1] = t, -t

    # ---- the lines ----
    text, recs = [], []

    def emit(r, kind, source, flag, q, x0, x1, line_tlen):
        other = rep[r ^ 1] if paired else None
        mate_pos = other[6] if paired and other[0] != UNMAPPED else 0
        mapped = kind != UNMAPPED
        if kind in (LOCUS, SECONDARY):
            X = loci[source]
            pos, cig = int(X["ref_begin"]) + 1, np_cigar(words_of(X, ops), merge)
            tags = [f"NM:i:{int(X['ref_score'])}", f"XH:i:{int(X['score'])}", f"XN:i:{int(X['n_haplotypes'])}"]
            sq = "*" if kind == SECONDARY else seq(int(X["pattern"]))
        elif kind == RESCUE:
            X = rescues[source]
            pos, cig = int(X["ref_begin"]) + 1, np_cigar(words_of(X, rescue_ops), merge)
            tags = [f"NM:i:{int(X['score'])}", "XR:i:1"]
            sq = seq(int(X["pattern"]))
        else:
            pos, cig, tags, sq = (mate_pos, "*", [], seq(strands * r))
        if kind in (LOCUS, RESCUE):
            tags += [f"X0:i:{x0}", f"X1:i:{x1}"]
        rname = opts["rname"] if mapped or mate_pos else "*"
        if not paired:
            rnext, pnext = "*", 0
        elif mate_pos:
            rnext, pnext = "=", mate_pos
        elif mapped:
            rnext, pnext = "=", pos
        else:
            rnext, pnext = "*", 0
        fields = [qname(r), str(flag), rname, str(pos), str(q), cig, rnext, str(pnext), str(line_tlen if mapped else 0), sq, "*"] + tags
        line = ("\t".join(fields) + "\n").encode()
        recs.append((sum(len(x) for x in text), len(line), r, source, flag, q, kind))
        text.append(line)

    for r in range(n_reads):
        kind, source, flag, q, x0, x1, _pos, _rev = rep[r]
        emit(r, kind, source, flag, q, x0, x1, tlen[r])
        if opts["secondary"]:
            R = reads[r]
            for i in range(int(R["first_locus"]), int(R["first_locus"]) + int(R["n_loci"])):
                if kind == LOCUS and i == source:
                    continue
                f = 0x100 | (0x10 if strands == 2 and loci["pattern"][i] & 1 else 0)
                if paired:
                    other = rep[r ^ 1]
                    f |= 0x1 | (0x80 if r & 1 else 0x40) | (0x8 if other[0] == UNMAPPED else (0x20 if other[7] else 0))
                emit(r, SECONDARY, i, f, 255, 0, 0, 0)
    return text, np.array(recs, dtype=LINE) if recs else np.zeros(0, LINE)


def test_rule_on_a_hand_worked_list():
    """the worked cases of spm_hip.h through np_sam"""
    L = np.zeros(3, dtype=[("ref_begin", "<u8"), ("ref_end", "<u8"), ("pattern", "<u4"), ("ref_score", "<i4"), ("score", "<i4"),
                           ("cigar_off", "<u4"), ("cigar_len", "<u4"), ("n_haplotypes", "<u4")])
    L["ref_begin"], L["ref_end"], L["pattern"] = [1000, 1170, 7000], [1004, 1174, 7004], [0, 3, 3]
    L["ref_score"], L["score"], L["cigar_off"], L["cigar_len"], L["n_haplotypes"] = [0, 1, 0], [0, 1, 0], [0, 1, 4], [1, 3, 1], 1
    ops = np.array([4 << 4 | 7, 2 << 4 | 7, 1 << 4 | 8, 1 << 4 | 7, 4 << 4 | 7], np.uint32)
    R = np.zeros(2, dtype=[("first_locus", "<u4"), ("n_loci", "<u4"), ("primary", "<u4"), ("n_best", "<u4"), ("n_next", "<u4")])
    R["first_locus"], R["n_loci"], R["primary"], R["n_best"], R["n_next"] = [0, 1], [1, 2], [0, 2], [1, 1], [0, 1]
    P = np.zeros(1, dtype=[("locus1", "<u4"), ("locus2", "<u4"), ("tlen", "<i4"), ("n_best", "<u4"), ("n_next", "<u4"),
                           ("flag1", "<u2"), ("flag2", "<u2")])
    P[0] = (0, 1, 174, 1, 0, 0x63, 0x93)
    needles = [np.array(x, np.uint8) for x in ([0, 1, 2, 3], [0, 1, 2, 3], [3, 3, 0, 7], [1, 1, 0, 0])]
    o = dict(rname="chr", symbols="ACGT", strands=2, cigar_m=False, secondary=True)
    text, recs = np_sam(L, ops, np.zeros(3), R, P, None, None, needles, None, o)
    assert text == [b"0\t99\tchr\t1001\t60\t4=\t=\t1171\t174\tACGT\t*\tNM:i:0\tXH:i:0\tXN:i:1\tX0:i:1\tX1:i:0\n",
                    b"0\t147\tchr\t1171\t60\t2=1X1=\t=\t1001\t-174\tCCAA\t*\tNM:i:1\tXH:i:1\tXN:i:1\tX0:i:1\tX1:i:0\n",
                    b"0\t401\tchr\t7001\t255\t4=\t=\t1001\t0\t*\t*\tNM:i:0\tXH:i:0\tXN:i:1\n"]
    assert recs.tolist() == [(0, len(text[0]), 0, 0, 99, 60, LOCUS), (len(text[0]), len(text[1]), 1, 1, 147, 60, LOCUS),
                             (len(text[0]) + len(text[1]), len(text[2]), 1, 2, 401, 255, SECONDARY)]
    text, _r = np_sam(L, ops, np.zeros(3), R, None, None, None, needles, ["a", "b"], dict(o, cigar_m=True, secondary=False))
    assert text == [b"a\t0\tchr\t1001\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:0\tXH:i:0\tXN:i:1\tX0:i:1\tX1:i:0\n",
                    b"b\t16\tchr\t7001\t40\t4M\t*\t0\t0\tCCAA\t*\tNM:i:0\tXH:i:0\tXN:i:1\tX0:i:1\tX1:i:1\n"]
    assert np_cigar([5 << 4 | 7, 2 << 4 | 1, 7 << 4 | 7, 1 << 4 | 8], True) == "5M2I8M"


# ---------------------------------------------------------------------------------------------------------------------
# the grammar of SAM 1.6 (section 1.4, the mandatory fields), independent of the rule
# ---------------------------------------------------------------------------------------------------------------------
RNAME_RE = r"[0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*"
FIELDS_RE = [re.compile(x) for x in (r"[!-?A-~]{1,254}", r"[0-9]+", r"\*|" + RNAME_RE, r"[0-9]+", r"[0-9]+", r"\*|([0-9]+[MIDNSHPX=])+",
                                     r"\*|=|" + RNAME_RE, r"[0-9]+", r"-?[0-9]+", r"\*|[A-Za-z=.]+", r"[!-~]+")]
TAG_RE = re.compile(r"[A-Za-z][A-Za-z0-9]:i:[-+]?[0-9]+")


def _check_grammar(text, recs, loci, rescues, needles):
    for line, rec in zip(text, recs):
        assert line.endswith(b"\n") and line.count(b"\n") == 1
        f = line[:-1].decode("ascii").split("\t")
        assert len(f) >= 11, line
        for x, rx in zip(f, FIELDS_RE):
            assert rx.fullmatch(x), (x, rx.pattern, line)
        assert all(TAG_RE.fullmatch(x) for x in f[11:]) and len({x[:2] for x in f[11:]}) == len(f[11:])
        flag, pos, q, pnext, tl = int(f[1]), int(f[3]), int(f[4]), int(f[7]), int(f[8])
        assert flag < 1 << 16 and pos < 1 << 31 and q <= 255 and pnext < 1 << 31 and abs(tl) < 1 << 31
        kind = int(rec["kind"])
        if kind == UNMAPPED:
            assert flag & 4 and f[5] == "*" and len(f) == 11 and q == 0
            continue
        assert not flag & 4 and f[5] != "*" and (flag & 0x100 != 0) == (kind == SECONDARY)
        src = (rescues if kind == RESCUE else loci)[int(rec["source"])]
        items = re.findall(r"([0-9]+)([MIDNSHPX=])", f[5])
        q_len = sum(int(n) for n, op in items if op in "MIS=X")
        r_len = sum(int(n) for n, op in items if op in "MDN=X")
        assert r_len == int(src["ref_end"]) - int(src["ref_begin"]) and pos == int(src["ref_begin"]) + 1
        assert q_len == len(needles[int(src["pattern"])])
        if kind != SECONDARY:
            assert q_len == len(f[9])


# ---------------------------------------------------------------------------------------------------------------------
# one call against the rule
# ---------------------------------------------------------------------------------------------------------------------
def _views(lc, rd, pr, rs):
    loci, ops, members = lc.view(), lc.ops, lc.members
    pairs = pr.view() if pr is not None else None
    rescues, rops = rs.view() if rs is not None else (None, None)
    return loci, ops, members, rd.view(), pairs, rescues, rops


def _check_sam(ctx, lc, rd, ps, needles, strands, pr=None, rs=None, names=None, cigar_m=False, secondary=False, tables=None,
               rname="chr7", symbols="ACGT"):
    """-> (the result, the expected lines, the expected records)"""
    loci, ops, members, reads, pairs, rescues, rops = _views(lc, rd, pr, rs)
    opts = dict(rname=rname, symbols=symbols, strands=strands, cigar_m=cigar_m, secondary=secondary,
                unique=tables[0] if tables else None, multi=tables[1] if tables else None)
    want, recs = np_sam(loci, ops, members, reads, pairs, rescues, rops, needles, names, opts)
    call = lambda: lc.sam(rd, ps, rname, pairs=pr, rescues=rs, names=names, symbols=symbols, cigar_m=cigar_m, secondary=secondary,
                          mapq_unique=tables[0] if tables else None, mapq_multi=tables[1] if tables else None)
    s = call()
    got, lines = s.text(), s.lines()
    assert lines.dtype == LINE and len(lines) == len(recs) == len(s)
    if got != b"".join(want):
        have = got.split(b"\n")
        bad = [(i, have[i] if i < len(have) else None, w) for i, w in enumerate(want) if i >= len(have) or have[i] + b"\n" != w][:4]
        raise AssertionError(bad)
    assert lines.tobytes() == recs.tobytes(), [(i, g, w) for i, (g, w) in enumerate(zip(lines.tolist(), recs.tolist())) if g != w][:6]
    d_text, n_bytes, d_lines, n_lines = s.device()
    assert n_bytes == len(got) and n_lines == len(recs)
    assert download(ctx, d_text, n_bytes, np.uint8).tobytes() == got and download(ctx, d_lines, n_lines, LINE).tobytes() == recs.tobytes()
    again = call()                                                 # a pure function of its inputs
    assert again.text() == got and again.lines().tobytes() == recs.tobytes()
    again.close()
    st = s.stats()
    kinds = recs["kind"]
    assert {c: int(getattr(st, c)) for c in COUNTS} == dict(
        n_lines=len(recs), n_bytes=len(got), n_reported=int(np.isin(kinds, (LOCUS, RESCUE)).sum()), n_secondary=int((kinds == SECONDARY).sum()),
        n_unmapped=int((kinds == UNMAPPED).sum()), n_rescue_lines=int((kinds == RESCUE).sum()))
    assert st.ms_host > 0 and st.ms_total >= 0
    _check_grammar(want, recs, loci, rescues, needles)
    return s, want, recs


def _fields(line):
    return line[:-1].decode().split("\t")


# ---------------------------------------------------------------------------------------------------------------------
# GPU 1: single-end, stranded
# ---------------------------------------------------------------------------------------------------------------------
POSITIONS = (9, 10, 99, 100, 999, 1000, 9999, 10000)
_single = {}


def _single_end_reads():
    """the tree, the reads and {class: read index}"""
    if _single:
        return _single["t"], _single["reads"], _single["at"]
    t = _make_tree(6101, 12_000, 4, 6, 8)
    rng = np.random.default_rng(1401)
    ref = t["ref"]
    apos = t["alleles"]["pos"].astype(np.int64)
    for pos in POSITIONS:                                          # the stretches the POS reads are cut from hold no allele
        assert np.all((apos < pos - 1 - 40) | (apos > pos - 1 + 32 + 40)), pos
    free = [s for s in _free_stretches(t, 400, 12, first=1100) if not any(s - 60 <= p - 1 <= s + 460 for p in POSITIONS)]
    assert len(free) >= 9
    spots = iter(free)
    # two best loci: the same 33 symbols at two places; a next-stratum locus: a copy with one substitution
    a, b = next(spots) + 30, next(spots) + 30
    ref[b:b + 33] = ref[a:a + 33]
    c, d = next(spots) + 30, next(spots) + 30
    ref[d:d + 34] = ref[c:c + 34]
    ref[d + 17] = (int(ref[d + 17]) + 1) & 3
    reads, at = [], {}

    def add(name, r):
        at[name] = len(reads)
        reads.append(np.ascontiguousarray(r, np.uint8))

    for pos in POSITIONS:
        add(f"pos{pos}", ref[pos - 1:pos - 1 + 30 + pos % 7])      # 30 .. 36 symbols
    for m in (63, 64, 65, 300):                                    # the lane-stride edges of SEQ; 300: five passes of a wave
        x = next(spots) + 40
        add(f"m{m}", ref[x:x + m] if m != 64 else np_revcomp(ref[x:x + m]))
    add("unmapped", rng.integers(0, 4, 33, dtype=np.uint8))
    add("two_best", ref[a:a + 33])
    add("next_stratum", ref[c:c + 34])
    x = next(spots) + 40
    add("reverse", np_revcomp(ref[x:x + 35]))
    add("deletion", np.delete(ref[x + 100:x + 136], 17))           # one reference symbol the read lacks: a D
    add("insertion", np.insert(ref[x + 200:x + 233], 15, (int(ref[x + 215]) + 2) & 3))
    for r in _plant(t, 1402, 32, 2, per_kind=1):                   # across the alleles of every kind
        add(f"allele{len(reads)}", r)
    _single.update(t=t, reads=reads, at=at)
    return t, reads, at


NAME_ALPHABET = "".join(chr(c) for c in range(33, 127) if chr(c) != "@")


def _names(n):
    """names of 1 .. 254 symbols over every legal byte: the first has 1, the second 254"""
    out = []
    for i in range(n):
        m = (1, 254, 2, 63, 64, 65, 7)[i % 7]
        out.append("".join(NAME_ALPHABET[(i * 31 + j * 7) % len(NAME_ALPHABET)] for j in range(m)))
    out[2] = "*" * 2                                               # a name may hold a *, it may not BE one
    return out


def test_planted_inputs_hold_their_cases(oracle):
    """CPU: the reads are where they were planted, by the oracle alone"""
    t, reads, at = _single_end_reads()
    ref = t["ref"]
    for pos in POSITIONS:
        r = reads[at[f"pos{pos}"]]
        h = oracle.sellers(ref, r, 0)
        assert h["pos"].tolist() == [pos - 1 + len(r)]
    assert len(oracle.sellers(ref, reads[at["two_best"]], 0)) == 2
    h = oracle.sellers(ref, reads[at["next_stratum"]], 1)
    (exact,) = h["pos"][h["score"] == 0].tolist()                 # one exact place; one more, a substitution away, elsewhere
    assert len({int(e) for e in h["pos"].tolist() if abs(int(e) - exact) > 40}) == 1
    assert len(oracle.sellers(ref, reads[at["unmapped"]], 2)) == 0 and len(oracle.sellers(ref, np_revcomp(reads[at["unmapped"]]), 2)) == 0
    assert [len(reads[at[f"m{m}"]]) for m in (63, 64, 65, 300)] == [63, 64, 65, 300]
    # the long rescue of test 3: the planted mate lies within 40 edits of its place, and has more than 32 of them
    t3, reads3, planted = _rescue_reads()
    p, lo, hi, end = planted["long"]
    mate = np_revcomp(reads3[2 * p + 1])
    assert len(mate) == 150
    h = oracle.sellers(t3["ref"][lo:hi], mate, 40)
    d = dict(zip((h["pos"].astype(np.int64) + lo).tolist(), h["score"].tolist()))
    assert end in d and 33 <= d[end] <= 40


@gpu
def test_single_end_stranded(spm, ctx):
    t, reads, at = _single_end_reads()
    needles = stranded(reads)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    names = _names(len(reads))
    first = None
    for nm in (None, names):
        for cigar_m in (False, True):
            for secondary in (False, True):
                s, want, recs = _check_sam(ctx, lc, rd, ps, needles, 2, names=nm, cigar_m=cigar_m, secondary=secondary)
                if first is None:
                    first = (s, want, recs)
                else:
                    s.close()
    s, want, recs = first
    assert len(want) == len(reads) and recs["read"].tolist() == list(range(len(reads)))
    f = [_fields(x) for x in want]
    for pos in POSITIONS:
        assert f[at[f"pos{pos}"]][1:5] == ["0", "chr7", str(pos), "60"], f[at[f"pos{pos}"]]
    for m in (63, 65, 300):
        assert f[at[f"m{m}"]][5] == f"{m}=" and len(f[at[f"m{m}"]][9]) == m and f[at[f"m{m}"]][1] == "0"
    assert f[at["m64"]][1] == "16" and len(f[at["m64"]][9]) == 64
    assert f[at["unmapped"]][1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"] and len(f[at["unmapped"]]) == 11
    assert f[at["two_best"]][4] == "3" and f[at["two_best"]][-2:] == ["X0:i:2", "X1:i:0"]
    assert f[at["next_stratum"]][4] == "40" and f[at["next_stratum"]][-2:] == ["X0:i:1", "X1:i:1"]
    assert f[at["reverse"]][1] == "16" and f[at["reverse"]][9] == "".join("ACGT"[c] for c in np_revcomp(reads[at["reverse"]]))
    assert re.fullmatch(r"[0-9]+=1D[0-9]+=", f[at["deletion"]][5]) and re.fullmatch(r"[0-9]+=1I[0-9]+=", f[at["insertion"]][5])
    assert all(x[6:9] == ["*", "0", "0"] for x in f)
    s.close()
    # an overridden table reaches the lines; another alphabet, another name of the reference
    s, want, _r = _check_sam(ctx, lc, rd, ps, needles, 2, tables=((11, 12, 13, 14), (21, 22, 23, 24)), rname="x|y@z", symbols="acgt")
    f = [_fields(x) for x in want]
    assert f[at["two_best"]][4] == "21" and f[at["next_stratum"]][4] == "12" and f[at["pos9"]][4] == "11" and f[at["pos9"]][2] == "x|y@z"
    assert f[at["pos9"]][9] == "".join("acgt"[c] for c in reads[at["pos9"]])
    s.close()
    # the same loci summarised as a plain set of 2n reads (strands == 1): read = pattern, every locus forward
    rd1 = lc.reads(2 * len(reads), 1)
    s, want, recs = _check_sam(ctx, lc, rd1, ps, needles, 1, secondary=True)
    assert len(want) >= 2 * len(reads) and np.array_equal(np.unique(recs["read"]), np.arange(2 * len(reads)))
    assert _fields(want[int(np.nonzero(recs["read"] == 2 * at["reverse"] + 1)[0][0])])[1] == "0"
    for x in (s, rd1, rd, lc, ps, ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 2: paired, no rescues
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_paired_without_rescues(spm, ctx):
    t, reads, classes = _planted_pairs()
    needles = stranded(reads)
    lc, rd, rest = _planted_chain(spm, ctx)
    ps = rest[1]
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    names = _names(len(reads) // 2)
    first = None
    for nm, cigar_m, secondary in ((None, False, False), (names, True, False), (None, False, True), (names, True, True)):
        s, want, recs = _check_sam(ctx, lc, rd, ps, needles, 2, pr=pr, names=nm, cigar_m=cigar_m, secondary=secondary)
        if first is None:
            first = (want, recs)
        s.close()
    want, recs = first
    f = [_fields(x) for x in want]
    assert len(f) == len(reads)
    line = lambda p, mate: f[2 * p + mate]
    for p, tlen in classes["proper_forward"]:
        assert (line(p, 0)[1], line(p, 1)[1]) == ("99", "147") and (line(p, 0)[8], line(p, 1)[8]) == (str(tlen), str(-tlen))
        assert line(p, 0)[6] == "=" and line(p, 0)[7] == line(p, 1)[3] and line(p, 1)[7] == line(p, 0)[3] and line(p, 0)[4] == "60"
    for p, tlen in classes["proper_reverse"]:
        assert (line(p, 0)[1], line(p, 1)[1]) == ("83", "163") and (line(p, 0)[8], line(p, 1)[8]) == (str(-tlen), str(tlen))
    for p, _t in classes["two_best"]:                              # the pair's counts, on both lines
        assert line(p, 0)[4] == line(p, 1)[4] == "3" and line(p, 0)[-2:] == line(p, 1)[-2:] == ["X0:i:2", "X1:i:0"]
    for p, _t in classes["unmapped"]:
        assert (line(p, 0)[1:9], line(p, 1)[1:9]) == (["77", "*", "0", "0", "*", "*", "0", "0"], ["141", "*", "0", "0", "*", "*", "0", "0"])
    (p1, _), (p2, _) = classes["one_mate"]                         # this mate mapped, the other not -- and the other's line
    assert line(p1, 0)[1] == "73" and line(p1, 0)[6:9] == ["=", line(p1, 0)[3], "0"]
    assert line(p1, 1)[1:9] == ["133", "chr7", line(p1, 0)[3], "0", "*", "=", line(p1, 0)[3], "0"] and len(line(p1, 1)) == 11
    assert line(p2, 1)[1] == "153" and line(p2, 0)[1:9] == ["101", "chr7", line(p2, 1)[3], "0", "*", "=", line(p2, 1)[3], "0"]
    for p, _t in classes["outside"] + classes["same_strand"]:      # both mapped, not proper: each mate's own counts, TLEN 0
        assert line(p, 0)[6:9] == ["=", line(p, 1)[3], "0"] and line(p, 1)[6:9] == ["=", line(p, 0)[3], "0"] and not int(line(p, 0)[1]) & 2
    signs = {np.sign(int(x[8])) for x in f}
    assert signs == {-1, 0, 1}
    for x in (pr, rd, lc) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 3: paired with rescues
# ---------------------------------------------------------------------------------------------------------------------
_rescue = {}


def _rescue_reads():
    """the planted rescues of test_rescue.py on a copy of their tree, and behind them: two discordant pairs with BOTH jobs
    rescued (5 and 3 edits: the second record wins; 4 and 4: the first does), and a pair whose mate 2 has 150 symbols and
    about 35 scattered substitutions.  -> (tree, reads, {name: ...})"""
    if _rescue:
        return _rescue["t"], _rescue["reads"], _rescue["planted"]
    t0, reads0, _classes = _planted_rescue()
    t = copy.deepcopy(t0)                                          # (the planted tree is shared with test_rescue.py: not touched)
    reads = [r.copy() for r in reads0]
    ref = t["ref"]
    rng = np.random.default_rng(1403)
    spots = _free_stretches(t, 240, 30, first=400)[22:]            # the planted reads use the first 22
    assert len(spots) >= 5
    planted = {}
    for name, (s1, s2), (e1, e2) in (("second_wins", spots[0:2], (5, 3)), ("tie", spots[2:4], (4, 4))):
        x, far, la, ly = s1 + 20, s2 + 170, 33, 35
        # mate 1 forward at x, mate 2 reverse at far: discordant.  Beside mate 2 a copy of mate 1 with e1 substitutions,
        # beside mate 1 a copy of mate 2 with e2
        ref[far + ly - 150:far + ly - 150 + la] = _diverge(rng, ref[x:x + la], e1)
        ref[x + 150 - ly:x + 150] = _diverge(rng, ref[far:far + ly], e2)
        planted[name] = (len(reads) // 2, e1, e2)
        reads += [ref[x:x + la].copy(), np_revcomp(ref[far:far + ly])]
    x = spots[4] + 20
    src = ref[x + 175 - 150:x + 175].copy()
    for i in range(35):                                            # 35 substitutions, never adjacent: 71 CIGAR words
        at = 2 + 4 * i + int(rng.integers(0, 2))
        src[at] = (int(src[at]) + 1 + int(rng.integers(0, 3))) & 3
    planted["long"] = (len(reads) // 2, x, x + MAX_TLEN, x + 175)  # pair, the window [lo, hi) of the job, the planted end
    reads += [ref[x:x + 34].copy(), np_revcomp(src)]
    reads += [rng.integers(0, 4, 31, dtype=np.uint8), rng.integers(0, 4, 36, dtype=np.uint8)]   # the last pair: unmapped
    reads = [np.ascontiguousarray(r, np.uint8) for r in reads]
    _rescue.update(t=t, reads=reads, planted=planted)
    return t, reads, planted


@gpu
def test_paired_with_rescues(spm, ctx):
    t, reads, planted = _rescue_reads()
    needles = stranded(reads)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    rescues, _ops = rs.view()
    assert {RESCUED, NOTHING, NOT_CONCORDANT} <= set(rescues["status"].tolist())
    by_pair = lambda p: rescues[rescues["pair"] == p]
    for name, pick in (("second_wins", 1), ("tie", 0)):
        p, e1, e2 = planted[name]
        both = by_pair(p)
        assert both["status"].tolist() == [RESCUED, RESCUED] and both["score"].tolist() == [e1, e2], (name, both)
    names = _names(len(reads) // 2)
    first = None
    for nm, cigar_m, secondary in ((None, False, False), (names, True, False), (None, False, True), (names, True, True)):
        s, want, recs = _check_sam(ctx, lc, rd, ps, needles, 2, pr=pr, rs=rs, names=nm, cigar_m=cigar_m, secondary=secondary)
        if first is None:
            first = (want, recs)
        s.close()
    want, recs = first
    f = [_fields(x) for x in want]
    pairs = pr.view()
    for name, pick in (("second_wins", 1), ("tie", 0)):            # the used record: the smaller score, on a tie the first
        p, e1, e2 = planted[name]
        j = int(np.nonzero(rescues["pair"] == p)[0][pick])
        y = (int(rescues[j]["pattern"]) >> 1) & 1
        assert y == pick                                           # the first record rescues mate 1
        assert recs[2 * p + y].tolist()[3:] == (j, int(rescues[j]["flag"]), recs[2 * p + y]["mapq"], RESCUE)
        assert recs[2 * p + 1 - y]["kind"] == LOCUS and recs[2 * p + 1 - y]["source"] == rescues[j]["anchor"]
        assert f[2 * p + y][11:13] == [f"NM:i:{(e1, e2)[pick]}", "XR:i:1"] and int(f[2 * p][1]) & 2 and int(f[2 * p + 1][1]) & 2
        assert int(f[2 * p][8]) == -int(f[2 * p + 1][8]) == int(rescues[j]["tlen"]) != 0
        assert f[2 * p][7] == f[2 * p + 1][3] and f[2 * p + 1][7] == f[2 * p][3] and f[2 * p][4] == f[2 * p + 1][4]
    kinds = recs["kind"]
    assert int((kinds == RESCUE).sum()) >= 12 and int((kinds == UNMAPPED).sum()) >= 4
    # a pair whose only record is NONE or NOT_CONCORDANT prints what it printed without rescues
    plain, want_plain, recs_plain = _check_sam(ctx, lc, rd, ps, needles, 2, pr=pr)
    plain.close()
    untouched = [p for p in range(len(pairs)) if not np.any((rescues["pair"] == p) & (rescues["status"] == RESCUED))]
    assert len(untouched) >= 8 and any(len(by_pair(p)) for p in untouched)
    for p in untouched:
        assert want[2 * p] == want_plain[2 * p] and want[2 * p + 1] == want_plain[2 * p + 1]
    # k = 40: every needle of at most 40 symbols is short, the 150-symbol mate is found with its 35 substitutions: a transcript
    # of more than 64 words, with and without M
    rs40 = pr.rescue(lc, rd, ref_text, ps, 40, MIN_TLEN, MAX_TLEN)
    r40, _o = rs40.view()
    p, lo, hi, end = planted["long"]
    (rec,) = r40[r40["pair"] == p]
    assert rec["status"] == RESCUED and rec["ref_end"] == end and rec["cigar_len"] > 64 and 33 <= rec["score"] <= 40
    assert int((r40["status"] == RESCUED).sum()) == 1
    for cigar_m in (False, True):
        s, want40, recs40 = _check_sam(ctx, lc, rd, ps, needles, 2, pr=pr, rs=rs40, cigar_m=cigar_m, secondary=True)
        g = _fields(want40[int(np.nonzero((recs40["read"] == 2 * p + 1) & (recs40["kind"] == RESCUE))[0][0])])
        n_items = len(re.findall(r"[0-9]+[=XIDM]", g[5]))
        if cigar_m:
            assert n_items < int(rec["cigar_len"]) and "=" not in g[5] and "X" not in g[5]
        else:
            assert n_items == int(rec["cigar_len"]) > 64
        assert len(g[9]) == 150
        s.close()
    for x in (rs40, rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 4: what is refused
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(spm, ctx):
    t, reads, planted = _rescue_reads()
    needles = stranded(reads)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    lib = spm.capi.lib()
    err = lambda: lib.spm_hip_last_error(ctx._h)
    n_pairs = len(reads) // 2
    good = lc.sam(rd, ps, "chr7", pairs=pr, rescues=rs)
    good_text = good.text()

    def opts_of(rname=b"chr7", symbols=b"ACGT", names=None, offs=None, n_names=None, **kw):
        o = spm.sam_opts(rname if rname is not None else b"x", symbols if symbols is not None else b"ACGT")
        if rname is None:
            o.rname = None
        if symbols is None:
            o.symbols = None
        keep = []
        if names is not None:
            blob = ctypes.create_string_buffer(names, len(names) + 1)
            keep.append(blob)
            o.names = ctypes.addressof(blob)
        if offs is not None:
            arr = np.asarray(offs, dtype=np.uint64)
            keep.append(arr)
            o.name_off = arr.ctypes.data
        if n_names is not None:
            o.n_names = n_names
        for k, v in kw.items():
            setattr(o, k, v)
        o._keep = keep
        return o

    def call(l=lc, r=rd, p=pr, x=rs, pats=ps, opts=None, no_opts=False):
        out = ctypes.c_void_p(1)                                   # (a refusal leaves NULL behind)
        h = lambda v: v._h if v is not None else None
        o = None if no_opts else ctypes.byref(opts if opts is not None else opts_of())
        rc = lib.spm_hip_jst_ref_loci_sam(h(l), h(r), h(p), h(x), h(pats), o, ctypes.byref(out))
        return rc, out

    def refused(word, code=-1, **kw):
        rc, out = call(**kw)
        assert rc == code and not out.value, (rc, out.value, err())
        assert word in err(), err()

    rc, out = call()                                               # the arguments of every refusal below, unchanged: accepted
    assert rc == 0 and out.value
    lib.spm_hip_sam_destroy(out)
    refused(b"NULL", r=None)
    refused(b"NULL", pats=None)
    refused(b"NULL", no_opts=True)
    refused(b"rname", opts=opts_of(rname=None))
    refused(b"symbols", opts=opts_of(symbols=None))
    assert lib.spm_hip_jst_ref_loci_sam(None, rd._h, pr._h, rs._h, ps._h, ctypes.byref(opts_of()), ctypes.byref(ctypes.c_void_p())) == -1
    assert lib.spm_hip_jst_ref_loci_sam(lc._h, rd._h, pr._h, rs._h, ps._h, ctypes.byref(opts_of()), None) == -1
    refused(b"flag", opts=opts_of(flags=4))
    refused(b"flag", opts=opts_of(flags=0x80000001))
    refused(b"reserved", opts=opts_of(reserved=1))
    refused(b"mapq_defaults", opts=opts_of(mapq_defaults=2))
    refused(b"rescues without pairs", p=None)
    other = spm.Context(0)                                         # a handle of another context
    other_ps = other.patterns(spm.ALGO_MYERS, reads, k=K_SEARCH, both_strands=True)
    refused(b"context", pats=other_ps)
    other_ps.close()
    other.close()
    few = reads[:8]
    lc4, rd4, ref4, ps4, rest4 = _chain_of(spm, ctx, t, few)       # another collapse with fewer loci
    assert 0 < len(lc4.view()) < len(lc.view())
    refused(b"loci", l=lc4)
    refused(b"loci", r=rd4)
    fewer = lc.reads(len(reads) - 2, 2)
    refused(b"pairs", r=fewer)
    plain = lc.reads(2 * len(reads), 1)
    refused(b"pairs", r=plain)
    refused(b"needles", r=fewer, p=None, x=None)                   # single-end: the set is not the set of these reads
    half = ctx.patterns(spm.ALGO_MYERS, reads[:-2], k=K_SEARCH, both_strands=True)
    refused(b"needles", pats=half)
    prefix = ctx.patterns(spm.ALGO_MYERS_PREFIX, reads, k=K_SEARCH, both_strands=True)
    refused(b"MYERS_PREFIX", code=UNSUPPORTED, pats=prefix)
    refused(b"symbols", opts=opts_of(symbols=b"ACG"))
    refused(b"symbols", opts=opts_of(symbols=b"ACGTN"))
    for bad in (b"", b"*", b"chr 7", b"chr\t7", b"chr\n", b"\x7f", b"x" * 255):
        refused(b"rname", opts=opts_of(rname=bad))
    ok_offs = np.arange(n_pairs + 1, dtype=np.uint64) * 2
    ok_names = b"ab" * n_pairs
    rc, out = call(opts=opts_of(names=b"@b" * n_pairs, offs=ok_offs, n_names=n_pairs))          # '@' is allowed
    assert rc == 0 and out.value
    lib.spm_hip_sam_destroy(out)
    refused(b"names", opts=opts_of(names=ok_names, offs=ok_offs, n_names=n_pairs - 1))
    refused(b"names", opts=opts_of(names=ok_names, offs=ok_offs, n_names=2 * n_pairs))          # one per pair, not per read
    refused(b"names", opts=opts_of(names=ok_names, n_names=n_pairs))                            # names without name_off
    refused(b"names", opts=opts_of(offs=ok_offs, n_names=n_pairs))
    refused(b"names", opts=opts_of(n_names=n_pairs))
    refused(b"names", p=None, x=None, opts=opts_of(names=ok_names, offs=ok_offs, n_names=n_pairs))   # single-end: one per read
    down = ok_offs.copy()
    down[3] = 3
    refused(b"ascend", opts=opts_of(names=ok_names, offs=down, n_names=n_pairs))
    refused(b"ascend", opts=opts_of(names=ok_names, offs=ok_offs + 1, n_names=n_pairs))
    empty = ok_offs.copy()
    empty[5] = empty[4]
    refused(b"name 4", opts=opts_of(names=ok_names, offs=empty, n_names=n_pairs))
    for bad in (b"a ", b"\ta", b"a\n", b"\x80a"):
        refused(b"name 1", opts=opts_of(names=b"ab" + bad + ok_names[4:], offs=ok_offs, n_names=n_pairs))
    star = ok_offs.copy()
    star[1:] -= 1
    refused(b"name 0", opts=opts_of(names=b"*" + ok_names[2:], offs=star, n_names=n_pairs))
    long_offs = ok_offs.copy()
    long_offs[1:] += 253
    refused(b"name 0", opts=opts_of(names=b"x" * 253 + ok_names, offs=long_offs, n_names=n_pairs))
    # records corrupted in the device buffers: counted, not followed
    hip = ctypes.CDLL("libamdhip64.so")
    PAIR, RESC = spm.JST_PAIR_DTYPE, spm.JST_RESCUE_DTYPE

    def with_broken(d_ptr, host, broken):
        ctx.synchronize()
        assert hip.hipMemcpy(ctypes.c_void_p(d_ptr), broken.ctypes.data_as(ctypes.c_void_p), broken.nbytes, 1) == 0
        refused(b"disagree")
        assert hip.hipMemcpy(ctypes.c_void_p(d_ptr), host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1) == 0

    d_pairs, n = pr.device()
    host = download(ctx, d_pairs, n, PAIR)
    broken = host.copy()
    broken["locus1"][int(np.nonzero(host["locus1"] != NONE)[0][0])] = len(lc.view()) + 5        # a locus outside the loci
    with_broken(d_pairs, host, broken)
    d_resc, n_resc, _d_ops, n_rops = rs.device()
    host = download(ctx, d_resc, n_resc, RESC)
    for field, value in (("pair", n_pairs + 3), ("anchor", len(lc.view()) + 1), ("cigar_off", n_rops)):
        broken = host.copy()
        j = int(np.nonzero(host["status"] == RESCUED)[0][-1])
        broken[field][j] = value
        with_broken(d_resc, host, broken)
    broken = host.copy()
    broken[[0, 1]] = host[[1, 0]]                                  # records out of order
    with_broken(d_resc, host, broken)
    # accessors on NULL, and after all of this the call still answers as before
    assert lib.spm_hip_sam_view(None, None, None, None, None) == -1 and lib.spm_hip_sam_device(None, None, None, None, None) == -1
    assert lib.spm_hip_sam_stats(None, None) == -1
    lib.spm_hip_sam_destroy(None)
    with pytest.raises(spm.SpmError, match="-1"):
        lc.sam(rd, ps, "chr 7", pairs=pr)
    after = lc.sam(rd, ps, "chr7", pairs=pr, rescues=rs)
    assert after.text() == good_text
    for x in (after, good, prefix, half, plain, fewer, rd4, lc4, ps4, ref4) + rest4 + (rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 5: zero reads, no loci, lifetimes
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_zero_reads_and_no_loci(spm, ctx):
    t, _reads, _c = _planted_pairs()
    rng = np.random.default_rng(1405)
    absent = [rng.integers(0, 4, 31 + i, dtype=np.uint8) for i in range(6)]
    ref_text = ctx.upload(t["ref"], sigma=4)
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS, absent, k=1, both_strands=True)
    jst.index(max(ps.window_size(p) for p in range(len(ps))), 64)
    h = jst.search_device(ps, max_hits=1 << 21)
    assert len(h) == 0
    lc = _chain(h, best=1, across=True, strands=True)
    rd = lc.reads(6, 2)
    needles = stranded(absent)
    seqs = ["".join("ACGT"[c] for c in r) for r in absent]
    s, want, recs = _check_sam(ctx, lc, rd, ps, needles, 2, secondary=True, cigar_m=True)       # single-end: flag 4
    assert want == [f"{r}\t4\t*\t0\t0\t*\t*\t0\t0\t{seqs[r]}\t*\n".encode() for r in range(6)]
    s.close()
    pr = lc.pairs(rd, 1, 10)
    s, want, recs = _check_sam(ctx, lc, rd, ps, needles, 2, pr=pr, names=["p", "q", "r"])        # paired: 0x4D and 0x8D
    assert want == [f"{'pqr'[r // 2]}\t{(0x4D, 0x8D)[r & 1]}\t*\t0\t0\t*\t*\t0\t0\t{seqs[r]}\t*\n".encode() for r in range(6)]
    rs = pr.rescue(lc, rd, ref_text, ps, 3, 1, 10)                 # no jobs: an empty rescues handle changes nothing
    s2, want2, _r = _check_sam(ctx, lc, rd, ps, needles, 2, pr=pr, rs=rs, names=["p", "q", "r"])
    assert want2 == want and s2.stats().n_unmapped == 6
    s2.close()
    # zero reads
    rd0 = lc.reads(0, 2)
    ps0 = ctx.patterns(spm.ALGO_MYERS, [], k=1, both_strands=True)
    pr0 = lc.pairs(rd0, 1, 10)
    for kw in ({}, {"pairs": pr0}):
        e = lc.sam(rd0, ps0, "chr7", **kw)
        assert e.text() == b"" and len(e.lines()) == 0 and e.device()[1] == 0 and e.device()[3] == 0 and e.stats().n_lines == 0
        assert e.header(len(t["ref"])) == b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr7\tLN:12000\n"
        e.close()
    # the result outlives every input
    for x in (rs, pr0, ps0, rd0, pr, rd, lc, h, ps, jst, ref_text):
        x.close()
    assert s.text() == b"".join(want) and s.lines().tobytes() == recs.tobytes()
    d_text, n_bytes, _d, _n = s.device()
    assert download(ctx, d_text, n_bytes, np.uint8).tobytes() == b"".join(want)
    s.close()
