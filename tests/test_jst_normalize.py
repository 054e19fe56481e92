"""Left-normalised projected pan-genome alignments (spm_hip_jst_ref_alns_normalize, JstRefAlignments.normalize).

The expected answer never comes from the code under test: `np_normalize` below is the rule of the header in COLUMN form -- a
list of one op per column, rewritten one step at a time -- and shares nothing with libspm_amd/csrc/jst_normalize_core.hpp,
which works on a stack of words.  Every GPU row compares records and pool with it byte for byte, in the host view and in the
device view, replays every transcript against the reference, and asserts -- with counters the reference computes -- that it
holds the case it is named for.
"""
import ctypes

import numpy as np
import pytest

from cpp_programs import c_layout, download
from test_align import replay
from test_jst_collapse import REF_ALN, _alleles, _loci_where, _members, _records, np_collapse
from test_jst_project import (DEL, EQ, INS, X, _cig, _hap, _make_tree, _open, _plant, _r, _row1_tree, _runs, _window)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: layout
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define S(f) printf("%s %zu\n", #f, offsetof(spm_jst_normalize_stats, f))
int main(void)
{
    S(ms_total); S(ms_slots); S(ms_normalize); S(ms_offsets); S(ms_gather); S(ms_compact); S(ms_host); S(reserved); S(n_alns);
    S(n_slots); S(n_ops_in); S(n_ops); S(n_changed); S(n_steps); S(n_joined); S(n_pinned);
    printf("sizeof.stats %zu\n", sizeof(spm_jst_normalize_stats));
    return 0;
}
"""
CALLS = ("spm_hip_jst_ref_alns_normalize", "spm_hip_jst_ref_alns_normalize_stats")


def test_stats_layout_matches_the_header(spm, tmp_path):
    assert ctypes.sizeof(spm.capi.JstNormalizeStats) == 96
    want = c_layout(tmp_path, LAYOUT_C)
    assert int(want.pop("sizeof.stats")) == 96
    for name, off in want.items():
        assert getattr(spm.capi.JstNormalizeStats, name).offset == int(off), name
    assert len(want) == len(spm.capi.JstNormalizeStats._fields_) == 16
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    assert hasattr(spm.JstRefAlignments, "normalize") and hasattr(spm.JstRefAlignments, "normalize_stats")


# ---------------------------------------------------------------------------------------------------------------------
# the reference: one op per column, one step at a time
# ---------------------------------------------------------------------------------------------------------------------
def _columns(words):
    return [int(w) & 15 for w in words for _ in range(int(w) >> 4)]


def np_normalize(P, ref, ref_begin, words):
    """The rule of the header on one transcript.  Returns (words, counters): steps, joined, pinned, and whether an I run and a
    D run stepped."""
    col = _columns(words)
    n = len(col)
    cnt = {"steps": 0, "joined": 0, "pinned": 0, "i_stepped": 0, "d_stepped": 0}
    at = 0
    while at < n:
        op = col[at]
        if op not in (INS, DEL):
            at += 1
            continue
        c = at
        assert c == 0 or col[c - 1] != op                       # (runs are maximal and treated left to right)
        L = 0
        while c + L < n and col[c + L] == op:
            L += 1
        stepped = False
        while True:
            i = sum(1 for o in col[:c] if o in (EQ, X, INS))
            r = ref_begin + sum(1 for o in col[:c] if o in (EQ, X, DEL))
            same = c >= 1 and col[c - 1] == EQ and (int(P[i - 1]) == int(P[i + L - 1]) if op == INS else
                                                    int(ref[r - 1]) == int(ref[r + L - 1]))
            if not (c >= 2 and same):
                cnt["pinned"] += int(c == 1 and same)
                break
            col[c - 1], col[c - 1 + L] = op, EQ                 # columns [c-1, c-1+L) are the gap, column c-1+L is =
            c -= 1
            cnt["steps"] += 1
            stepped = True
            if c >= 1 and col[c - 1] == op:                     # the new left neighbour is a run of the same op: one run
                cnt["joined"] += 1
                while c >= 1 and col[c - 1] == op:
                    c -= 1
                    L += 1
        cnt["i_stepped" if op == INS else "d_stepped"] += int(stepped)
        at = c + L
    return _runs(np.array(col, dtype=np.uint32)) if n else np.zeros(0, np.uint32), cnt


def _words(s):
    """'8=1D5=' -> words"""
    out, num = [], ""
    for ch in s:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num) << 4) | {"I": INS, "D": DEL, "=": EQ, "X": X}[ch])
            num = ""
    return np.array(out, dtype=np.uint32)


def _consumes(words):
    col = _columns(words)
    return sum(o in (EQ, X, INS) for o in col), sum(o in (EQ, X, DEL) for o in col), sum(o != EQ for o in col)


def _true_columns(P, ref, ref_begin, words):
    """every = / X column says the truth, the words consume exactly P, and no two adjacent words share an op"""
    i, r = 0, ref_begin
    for o in _columns(words):
        if o in (EQ, X):
            assert (int(P[i]) == int(ref[r])) == (o == EQ)
        i += o in (EQ, X, INS)
        r += o in (EQ, X, DEL)
    assert i == len(P)
    ops = [int(w) & 15 for w in words]
    assert all(a != b for a, b in zip(ops, ops[1:])) and all(int(w) >> 4 for w in words)
    return r


REP = "ACT"
WORKED = [  # ref, needle, ref_begin, sources, result
    ("GATTCGCAAAAGTCCATG", "TTCGCAAAGTCCA", 2, ["8=1D5=", "6=1D7=", "5=1D8="], "5=1D8="),
    ("GGAC" + REP * 5 + "GGTC", "AC" + REP * 4 + "GG", 2, [f"{2 + 3 * j}=3D{14 - 3 * j}=" for j in range(5)], "2=3D14="),
    ("GATCCGT", "ATCCCG", 1, ["4=1I1=", "3=1I2="], "2=1I3="),
    ("GACGTCGTA", "ACGTCGTCGTA", 1, ["7=3I1="], "1=3I7="),
    ("CAAAAG", "AAAG", 1, ["3=1D1="], "1=1D3="),
    ("CAAAAAAG", "AAAAG", 1, ["2=1D1=1D2=", "1=1D2=1D2=", "4=2D1="], "1=2D4="),
    ("GACGTTA", "ACGATTA", 1, ["3=1X1I2="], "3=1X1I2="),
]


def test_reference_on_the_worked_cases():
    for ref, P, rb, sources, want in WORKED:
        ref, P = _r(ref), _r(P)
        for s in sources:
            w = _words(s)
            re = _true_columns(P, ref, rb, w)                   # (the case itself is a true alignment)
            out, cnt = np_normalize(P, ref, rb, w)
            assert _cig(out) == want, (s, _cig(out), want)
            assert _true_columns(P, ref, rb, out) == re
            assert _cig(np_normalize(P, ref, rb, out)[0]) == want
    assert np_normalize(_r("AAAG"), _r("CAAAAG"), 1, _words("3=1D1="))[1]["pinned"] == 1
    assert np_normalize(_r("AAAAG"), _r("CAAAAAAG"), 1, _words("2=1D1=1D2="))[1]["joined"] == 1
    assert np_normalize(_r("ACGT"), _r("ACGT"), 2, _words("4I"))[0].tolist() == _words("4I").tolist()   # inside an insertion


def _random_alignment(rng, sigma, n_cols, p_edit):
    """a true alignment made column by column: (P, ref, ref_begin, words)"""
    ref_begin = int(rng.integers(0, 4))
    ref = list(rng.integers(0, sigma, ref_begin))
    P, col = [], []
    for _ in range(n_cols):
        u = rng.random()
        if u >= p_edit:
            s = int(rng.integers(0, sigma))
            ref.append(s)
            P.append(s)
            col.append(EQ)
        elif u < p_edit / 3 and sigma > 1:
            s = int(rng.integers(0, sigma))
            ref.append(s)
            P.append((s + 1 + int(rng.integers(0, sigma - 1))) % sigma)
            col.append(X)
        elif u < 2 * p_edit / 3:
            P.append(int(rng.integers(0, sigma)))
            col.append(INS)
        else:
            ref.append(int(rng.integers(0, sigma)))
            col.append(DEL)
    if not P:
        P.append(0)
        col.append(INS)
    ref += list(rng.integers(0, sigma, 3))
    return np.array(P, np.uint8), np.array(ref, np.uint8), ref_begin, _runs(np.array(col, dtype=np.uint32))


def test_reference_invariants_on_random_alignments():
    rng = np.random.default_rng(2027)
    tot = {"changed": 0, "grew": 0, "shrank": 0, "joined": 0, "pinned": 0, "i_stepped": 0, "d_stepped": 0}
    for it in range(6000):
        sigma = (1, 2, 4)[it % 3]
        P, ref, rb, w = _random_alignment(rng, sigma, int(rng.integers(1, 40)), 0.25)
        re = _true_columns(P, ref, rb, w)
        out, cnt = np_normalize(P, ref, rb, w)
        assert _true_columns(P, ref, rb, out) == re             # consumes exactly P and ref[rb, re); = / X still true
        replay(P, ref, rb, re, out, _consumes(out)[2])
        a, b = _columns(w), _columns(out)
        assert all(a.count(o) == b.count(o) for o in (EQ, X, INS, DEL))
        assert len(out) <= 2 * len(w)
        again, cnt2 = np_normalize(P, ref, rb, out)
        assert again.tolist() == out.tolist() and cnt2["steps"] == 0 and cnt2["joined"] == 0
        assert (cnt["steps"] > 0) == (out.tolist() != w.tolist())
        # a function of (P, ref, ref_begin, words) only: the flanks do not enter
        ref2 = np.concatenate([ref[:rb], ref[rb:re], (ref[re:] + 1) % max(sigma, 2)]).astype(np.uint8)
        assert np_normalize(P, ref2, rb, w)[0].tolist() == out.tolist()
        tot["changed"] += out.tolist() != w.tolist()
        tot["grew"] += len(out) > len(w)
        tot["shrank"] += len(out) < len(w)
        for k in ("joined", "pinned", "i_stepped", "d_stepped"):
            tot[k] += cnt[k] > 0
    print(tot)
    assert all(v > 20 for v in tot.values()), tot


def test_collapse_case1_is_one_locus_after_normalisation():
    ref = _r("GATTCGCAAAAGTCCATG")
    al, pool, cov = _alleles([(10, 1, "", (0,))], 2)
    needles = [_r("TTCGCAAAGTCCA")]
    rv, rops = _records(ref, al, pool, cov, 2, needles, 1)
    before = _loci_where(np_collapse(rv, rops), ref_begin=2, ref_end=16)
    assert [c for _i, c in before] == ["5=1D8=", "8=1D5="]
    nv, nops, _cnt = np_normalize_view(rv, rops, needles, ref)
    want = np_collapse(nv, nops)
    got = _loci_where(want, ref_begin=2, ref_end=16)
    assert [c for _i, c in got] == ["5=1D8="], got
    l = want["loci"][got[0][0]]
    assert int(l["n_records"]) == 2 and _members(want, got[0][0]) == [(0, 0), (1, 1)]


def np_normalize_view(rv, rops, needles, ref):
    """np_normalize on a projection's view: the same records with new cigar_off / cigar_len, one transcript per distinct
    source slot in source pool order, and the counters summed over the slots."""
    rops = np.asarray(rops, dtype=np.uint32)
    out = rv.copy()
    tot = {"slots": 0, "changed": 0, "steps": 0, "joined": 0, "pinned": 0, "grew": 0, "shrank": 0, "i_stepped": 0, "d_stepped": 0,
           "slots_joined": 0, "slots_pinned": 0}
    pool, place, memo = [], {}, {}
    first = {}
    for i, off in enumerate(rv["cigar_off"].tolist()):
        first.setdefault(off, i)
    for off in sorted(first):
        r = rv[first[off]]
        w = rops[off:off + int(r["cigar_len"])]
        key = (int(r["pattern"]), int(r["ref_begin"]), w.tobytes())
        if key not in memo:
            memo[key] = np_normalize(needles[int(r["pattern"])], ref, int(r["ref_begin"]), w)
        nw, cnt = memo[key]
        place[off] = (len(pool), len(nw))
        pool += nw.tolist()
        tot["slots"] += 1
        tot["changed"] += nw.tolist() != w.tolist()
        tot["grew"] += len(nw) > len(w)
        tot["shrank"] += len(nw) < len(w)
        for k in ("steps", "joined", "pinned"):
            tot[k] += cnt[k]
        tot["i_stepped"] += cnt["i_stepped"] > 0
        tot["d_stepped"] += cnt["d_stepped"] > 0
        tot["slots_joined"] += cnt["joined"] > 0
        tot["slots_pinned"] += cnt["pinned"] > 0
    for i, off in enumerate(rv["cigar_off"].tolist()):
        out["cigar_off"][i], out["cigar_len"][i] = place[off]
    return out, np.array(pool, dtype=np.uint32), tot


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _norm_checked(spm, ctx, t, needles, pr, close=True):
    """pr (JstRefAlignments, a projection): its normalisation against np_normalize of its host view, in both views; every
    transcript replayed; sharing; the stats.  Returns (normalised view, pool, counters, bytes of the host view)."""
    rv, rops = pr.view(), pr.ops
    ref = t["ref"]
    want_v, want_ops, cnt = np_normalize_view(rv, rops, needles, ref)
    nz = pr.normalize()
    try:
        gv, gops = nz.view(), nz.ops
        assert gv.dtype == REF_ALN and len(gv) == len(rv)
        for f in REF_ALN.names:
            assert np.array_equal(gv[f], want_v[f]), f
        assert gv.tobytes() == want_v.tobytes() and gops.tobytes() == want_ops.tobytes()
        # the device view: record i belongs to record i of the source's device view; the pool is the same pool
        sp, sn, _so, _sno = pr.device()
        dp, dn, do, dno = nz.device()
        assert (dn, dno) == (len(rv), len(want_ops)) and sn == dn
        if dn:
            dsrc, dgot = download(ctx, sp, sn, REF_ALN), download(ctx, dp, dn, REF_ALN)
            place = {int(a): (int(b), int(c)) for a, b, c in zip(rv["cigar_off"], want_v["cigar_off"], want_v["cigar_len"])}
            dwant = dsrc.copy()
            for i, off in enumerate(dsrc["cigar_off"].tolist()):
                dwant["cigar_off"][i], dwant["cigar_len"][i] = place[off]
            assert dgot.tobytes() == dwant.tobytes()
            assert download(ctx, do, dno, np.dtype("<u4")).tobytes() == want_ops.tobytes()
        # every distinct transcript replays against the reference
        seen = set()
        for r in gv:
            key = (int(r["pattern"]), int(r["cigar_off"]))
            if key in seen:
                continue
            seen.add(key)
            w = gops[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])]
            replay(needles[int(r["pattern"])], ref, int(r["ref_begin"]), int(r["ref_end"]), w, int(r["ref_score"]))
        # sharing: equal source slots <=> equal result slots, the pool in source pool order and holding nothing else
        if len(rv):
            pairs = np.unique(np.stack([rv["cigar_off"].astype(np.int64), gv["cigar_off"].astype(np.int64)]), axis=1)
            assert len(np.unique(pairs[0])) == len(np.unique(pairs[1])) == pairs.shape[1] == cnt["slots"]
            assert np.all(np.diff(pairs[1]) > 0)
            last = int(np.argmax(gv["cigar_off"]))
            assert int(gv["cigar_off"][last]) + int(gv["cigar_len"][last]) == len(gops)
        st, ps = nz.normalize_stats(), nz.stats()
        assert (st.n_alns, st.n_slots, st.n_ops_in, st.n_ops) == (len(rv), cnt["slots"], len(rops), len(want_ops))
        assert (st.n_changed, st.n_steps, st.n_joined, st.n_pinned) == (cnt["changed"], cnt["steps"], cnt["joined"], cnt["pinned"])
        assert (ps.n_alns, ps.n_projected, ps.n_ops, ps.ms_total, ps.ms_host) == (len(rv), cnt["slots"], len(want_ops), 0, 0)
        assert len(nz) == len(rv)
        print(f"records {len(rv)}, slots {st.n_slots}, words {st.n_ops_in} -> {st.n_ops}; {cnt}; device ms slots "
              f"{st.ms_slots:.3f} normalise {st.ms_normalize:.3f} offsets {st.ms_offsets:.3f} gather {st.ms_gather:.3f} compact "
              f"{st.ms_compact:.3f}, host {st.ms_host:.3f}")
        return gv, gops, cnt, (gv.tobytes(), gops.tobytes())
    finally:
        if close:
            nz.close()


def _search_normalize(spm, ctx, t, needles, k, block, algo=None, shard=None, select=None):
    """search -> align (or select + align_selected) -> project -> normalise, checked.  Returns what _norm_checked returns
    plus the projection's (view, pool)."""
    ref_text, jst, ps = _open(spm, ctx, t, needles, k, algo)
    try:
        jst.index(_window(ps, len(needles)), block, *(shard or ()))
        h = jst.search_device(ps, alignable=select is None, max_hits=1 << 21)
        if select is None:
            sel, a = None, h.align()
        else:
            sel = h.select(best=0 if select else 1, across=select)
            assert 0 < len(sel) < len(h)
            a = sel.align_selected()
        pr = a.project()
        try:
            assert len(pr) >= 1
            return _norm_checked(spm, ctx, t, needles, pr) + ((pr.view(), pr.ops),)
        finally:
            for x in (pr, a, sel, h):
                if x is not None:
                    x.close()
    finally:
        jst.close()
        ps.close()
        ref_text.close()


HOMO = "GATTCGCAAAAGTCCATG"


@pytest.mark.gpu
def test_row1_collapse_case1_on_the_device(spm, ctx):
    """the header's two-haplotype tree between random flanks: two loci without normalize(), one with it"""
    at = 2000
    t = _make_tree(911, 4_000, 2, 8, 0, extra=[(at + 10, 1, [], (0,))])
    t["ref"][at:at + len(HOMO)] = _r(HOMO)                      # (before any haplotype is materialised)
    needles = [_r("TTCGCAAAGTCCA")]
    ref_text, jst, ps = _open(spm, ctx, t, needles, 1)
    jst.index(_window(ps, 1), 64)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    a = h.align()
    pr = a.project()
    nz = pr.normalize()
    plain, merged = pr.collapse(), nz.collapse()

    def loci(lc):
        v, ops = lc.view(), lc.ops
        return [(i, lc.cigar(i, v, ops)) for i, l in enumerate(v) if (int(l["ref_begin"]), int(l["ref_end"])) == (at + 2, at + 16)]

    assert [c for _i, c in loci(plain)] == ["5=1D8=", "8=1D5="]
    got = loci(merged)
    assert [c for _i, c in got] == ["5=1D8="], got
    l = merged.view()[got[0][0]]
    hm, hs = merged.haplotypes(got[0][0])
    assert int(l["n_haplotypes"]) == 2 and int(l["n_records"]) == 2 and int(l["ref_score"]) == 1
    assert list(zip(hm.tolist(), hs.tolist())) == [(0, 0), (1, 1)]
    assert len(merged) == len(plain) - 1
    # and the device collapse of the normalised records is the reference collapse of the reference normalisation
    nv, nops, _cnt = np_normalize_view(pr.view(), pr.ops, needles, t["ref"])
    want = np_collapse(nv, nops)
    assert merged.view().tobytes() == want["loci"].tobytes() and merged.ops.tobytes() == want["ops"].tobytes()
    assert merged.members.tobytes() == want["members"].tobytes() and merged.member_scores.tobytes() == want["member_scores"].tobytes()
    for x in (merged, plain, nz, pr, a, h, jst, ps, ref_text):
        x.close()


def _low_complexity_tree():
    """A random reference with homopolymer and tandem-repeat stretches (unit 1-4, 5-20 copies, at most 28 symbols).  Per
    stretch, hand-made alleles INSIDE it: two deletions of one or two units at different copies, carried by different
    haplotype subsets that overlap (so some haplotypes carry two alleles in one stretch) -- or an insertion of a unit and a
    deletion -- and, behind every second stretch, a SNP (an X directly behind a gap run: the word count grows).  Needles are
    cut from the haplotypes across the stretches, some beginning inside one."""
    rng = np.random.default_rng(1201)
    n_ref, n_hap, n_st = 8_000, 8, 24
    ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
    extra, stretches = [], []
    for j in range(n_st):
        p = 300 + 300 * j
        u = 1 + j % 4
        unit = rng.integers(0, 4, u, dtype=np.uint8)
        while u > 1 and len(set(unit.tolist())) == 1:
            unit = rng.integers(0, 4, u, dtype=np.uint8)
        copies = min(int(rng.integers(5, 21)), max(5, 28 // u))
        ref[p:p + u * copies] = np.tile(unit, copies)
        ref[p - 1] = (int(unit[-1]) + 1) & 3                    # the stretch ends where it says
        ref[p + u * copies] = (int(unit[0]) + 1) & 3
        a, b = sorted(rng.choice(np.arange(1, copies - 1), size=2, replace=False).tolist())
        if b == a + 1:
            a, b = (a - 1, b) if a > 1 else (a, min(b + 1, copies - 2))
        if b <= a + 1:
            a, b = 1, copies - 2
        n_b = 2 if (j % 3 == 0 and b + 2 <= copies) else 1
        if j % 2 == 0:                                          # two deletions: carriers {0,1,2} and {2,3,4}
            extra.append((p + u * a, u, [], (0, 1, 2)))
            extra.append((p + u * b, u * n_b, [], (2, 3, 4)))
        else:                                                   # an insertion of a unit and a deletion
            extra.append((p + u * a, 0, unit.copy(), (0, 1, 2)))
            extra.append((p + u * b, u * n_b, [], (2, 3, 4)))
        if j % 2 == 1 or j % 4 == 0:
            q = p + u * copies
            extra.append((q, 1, [(int(ref[q]) + 2) & 3], (1, 3, 5)))
        stretches.append((p, u, copies))
    t = _make_tree(1202, n_ref, n_hap, 8, 0, extra=extra)
    t = dict(t, ref=ref)
    needles, seen = [], set()
    for p, u, copies in stretches:
        for h in (0, 2, 3, 6):
            hp, J = _hap(t, h)
            x0 = int(np.searchsorted(J.org, p))
            for o in (x0 - 10, x0 - 3, x0 + 1, x0 + u + 1):     # across the stretch, and beginning inside it
                nd = hp[o:o + 40].copy()
                if nd.tobytes() not in seen:
                    seen.add(nd.tobytes())
                    needles.append(nd)
    return t, needles


@pytest.mark.gpu
def test_row2_low_complexity(spm, ctx):
    t, needles = _low_complexity_tree()
    gv, gops, cnt, _b, (rv, rops) = _search_normalize(spm, ctx, t, needles, 2, 64)
    for k in ("i_stepped", "d_stepped", "grew", "shrank", "slots_joined", "slots_pinned"):
        assert cnt[k] >= 1, (k, cnt)
    before, after = np_collapse(rv, rops), np_collapse(gv, gops)
    print(f"loci {len(before['loci'])} -> {len(after['loci'])}")
    assert len(after["loci"]) < len(before["loci"]), "normalisation merged nothing: the row shows nothing"


_shared = {}


def _row1(spm, ctx):
    if "row1" not in _shared:
        t, needles = _row1_tree()
        _shared["row1"] = _search_normalize(spm, ctx, t, needles, 2, 64)
    return _shared["row1"]


@pytest.mark.gpu
def test_row3_every_allele_kind_idempotence_and_sharing(spm, ctx):
    t, needles = _row1_tree()
    ref_text, jst, ps = _open(spm, ctx, t, needles, 2)
    jst.index(_window(ps, len(needles)), 64)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    a = h.align()
    pr = a.project()
    gv, gops, cnt, blob = _norm_checked(spm, ctx, t, needles, pr)
    _shared.setdefault("row1", (gv, gops, cnt, blob, (pr.view(), pr.ops)))
    assert cnt["slots"] < len(gv), "no transcript is shared: the row shows nothing about sharing"
    assert cnt["changed"] > 0
    n1 = pr.normalize()
    n2 = n1.normalize()                                         # normalising a normalised result changes nothing
    assert (n2.view().tobytes(), n2.ops.tobytes()) == (n1.view().tobytes(), n1.ops.tobytes()) == blob
    s2 = n2.normalize_stats()
    assert (s2.n_changed, s2.n_steps, s2.n_joined, s2.n_ops_in, s2.n_ops) == (0, 0, 0, len(gops), len(gops))
    _norm_checked(spm, ctx, t, needles, n1)                     # (and the reference says the same about it)
    n3 = pr.normalize()                                         # two calls: identical bytes
    assert (n3.view().tobytes(), n3.ops.tobytes()) == blob
    for x in (n3, n2, n1, pr, a, h, jst, ps, ref_text):
        x.close()


@pytest.mark.gpu
def test_row4_long_needles_wave_class_kernels(spm, ctx):
    t = _make_tree(401, 20_000, 8, 8, 200)
    needles = _plant(t, 402, 300, 12, per_kind=1)
    _gv, _go, cnt, _b, _src = _search_normalize(spm, ctx, t, needles, 12, 64)
    assert cnt["changed"] > 0 and cnt["steps"] > 0


@pytest.mark.gpu
def test_row4_one_needle_of_1024_symbols(spm, ctx):
    t = _make_tree(451, 6_000, 4, 8, 60)
    needles = _plant(t, 452, 1024, 64, per_kind=1, kinds=("del",))[:1]
    assert len(needles) == 1 and len(needles[0]) == 1024
    _gv, _go, cnt, _b, _src = _search_normalize(spm, ctx, t, needles, 64, 64)
    assert cnt["slots"] >= 1


@pytest.mark.gpu
def test_row5_exact_set(spm, ctx):
    """exact needles on the low-complexity tree: every gap of a transcript is a carried allele, and those still shift"""
    t, needles = _low_complexity_tree()
    needles = list({nd[:32].tobytes(): nd[:32].copy() for nd in needles}.values())
    gv, _go, cnt, _b, _src = _search_normalize(spm, ctx, t, needles, 0, 64, algo=spm.ALGO_SHIFTOR)
    assert any(int(s) > 0 for s in gv["ref_score"]) and cnt["d_stepped"] > 0 and cnt["i_stepped"] > 0, cnt


@pytest.mark.gpu
def test_row5_dna5_reference_with_n_runs(spm, ctx):
    t = _make_tree(601, 16_000, 6, 8, 160, sigma=5, n_runs=60)
    needles = _plant(t, 602, 40, 2)
    assert any(4 in nd for nd in needles), "no needle holds an N"
    _search_normalize(spm, ctx, t, needles, 2, 64)


@pytest.mark.gpu
def test_row5_block_shard(spm, ctx):
    t, needles = _row1_tree()
    n_blocks = -(-len(t["ref"]) // 64)
    _search_normalize(spm, ctx, t, needles, 2, 64, shard=(n_blocks // 3, 2 * n_blocks // 3))


@pytest.mark.gpu
@pytest.mark.parametrize("across", [False, True])
def test_row5_selections(spm, ctx, across):
    t, needles = _row1_tree()
    _search_normalize(spm, ctx, t, needles, 2, 64, select=across)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 0])
def test_row6_slot_counts_around_a_workgroup(spm, ctx, n):
    t = _make_tree(1101, 16_000, 1, 8, 160)
    hp, _J = _hap(t, 0)
    rng = np.random.default_rng(1102)
    if n:
        starts = rng.choice(len(hp) - 32, size=n, replace=False)
        needles = [hp[int(o):int(o) + 32].copy() for o in starts]
    else:
        needles = [np.tile(np.array([0, 0, 1, 3, 2, 2, 1, 0], np.uint8), 4)]
    ref_text, jst, ps = _open(spm, ctx, t, needles, 0, spm.ALGO_SHIFTOR)
    jst.index(_window(ps, len(needles)), 64)
    h = jst.search_device(ps, alignable=True)
    a = h.align()
    assert len(a) == n, "a 32-mer occurs twice (or the absent one occurs): choose another seed"
    pr = a.project()
    gv, gops, cnt, _b = _norm_checked(spm, ctx, t, needles, pr)
    assert cnt["slots"] == n == len(gv)
    if n == 0:
        nz = pr.normalize()
        assert len(nz) == 0 and len(nz.ops) == 0 and nz.device()[1] == 0 and nz.device()[3] == 0
        lc = nz.collapse()
        assert len(lc) == 0
        lc.close()
        nz.close()
    for x in (pr, a, h, jst, ps, ref_text):
        x.close()


@pytest.mark.gpu
def test_row7_refusals_and_lifetimes(spm, ctx):
    t, needles = _row1_tree()
    ref_text, jst, ps = _open(spm, ctx, t, needles, 2)
    jst.index(_window(ps, len(needles)), 64)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    a = h.align()
    pr = a.project()
    lib = spm.capi.lib()
    out = ctypes.c_void_p()
    # unknown flags through the raw ABI; NULL arguments; the stats of a plain projection
    assert lib.spm_hip_jst_ref_alns_normalize(pr._h, 1, ctypes.byref(out)) == -1 and not out.value
    assert b"flag" in lib.spm_hip_last_error(ctx._h)
    assert lib.spm_hip_jst_ref_alns_normalize(None, 0, ctypes.byref(out)) == -1 and not out.value
    assert lib.spm_hip_jst_ref_alns_normalize(pr._h, 0, None) == -1
    st = spm.capi.JstNormalizeStats()
    assert lib.spm_hip_jst_ref_alns_normalize_stats(pr._h, ctypes.byref(st)) == -1
    assert lib.spm_hip_jst_ref_alns_normalize_stats(None, ctypes.byref(st)) == -1
    with pytest.raises(spm.SpmError):
        pr.normalize_stats()
    _gv, _go, _cnt, base = _norm_checked(spm, ctx, t, needles, pr)
    # the tree indexed again with another block length: the reference text belongs to no index generation
    jst.index(_window(ps, len(needles)), 16)
    with pytest.raises(spm.SpmError):
        a.project()                                             # (the projection does refuse the new generation)
    nz = pr.normalize()
    assert (nz.view().tobytes(), nz.ops.tobytes()) == base
    rv, rops = pr.view(), pr.ops
    want_v, want_ops, _c = np_normalize_view(rv, rops, needles, t["ref"])
    want = np_collapse(want_v, want_ops)
    # closed tree or needle set: Python refuses
    jst.close()
    with pytest.raises(spm.SpmError):
        pr.normalize()
    with pytest.raises(spm.SpmError):
        nz.normalize()
    ps.close()
    with pytest.raises(spm.SpmError):
        pr.normalize()
    # the result is usable and collapsible after source, tree and set are closed
    for x in (pr, a, h, ref_text):
        x.close()
    assert (nz.view().tobytes(), nz.ops.tobytes()) == base
    lc = nz.collapse()
    assert lc.view().tobytes() == want["loci"].tobytes() and lc.ops.tobytes() == want["ops"].tobytes()
    assert lc.locus_of.tobytes() == want["locus_of"].tobytes()
    lc.close()
    nz.close()
    with pytest.raises(spm.SpmError):
        nz.view()
