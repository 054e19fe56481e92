"""Projected pan-genome alignments collapsed to one record per locus (spm_hip_jst_ref_alns_collapse, JstRefAlignments.collapse).

The expected answer never comes from the code under test: `np_collapse` below collapses the host view and the pool of the
PROJECTION by the rule of the header, with tuples and `sorted`; in the same test `_check` of test_jst_project pins that
projection to the NumPy projection and the replayer.  Every GPU row compares records, the three pools and the map with that
reference byte for byte, and asserts -- with counters the reference computes -- that it holds the case it is named for.
"""
import ctypes

import numpy as np
import pytest

from cpp_programs import c_layout, download
from test_align import replay
from test_gpu_jst import _apply
from test_jst_project import (ALL_KINDS, DEL, EQ, INS, X, Journal, _check, _cig, _global_dp, _hap, _make_tree, _open,
                              _plant, _r, _row1_tree, _window, np_project)


LOCUS = np.dtype([("ref_begin", "<u8"), ("ref_end", "<u8"), ("pattern", "<u4"), ("ref_score", "<i4"), ("score", "<i4"),
                  ("n_records", "<u4"), ("cigar_off", "<u4"), ("cigar_len", "<u4"), ("member_off", "<u4"), ("n_haplotypes", "<u4")])
REF_ALN = np.dtype([("ref_begin", "<u8"), ("ref_end", "<u8"), ("haplotype", "<u4"), ("pattern", "<u4"), ("score", "<i4"),
                    ("ref_score", "<i4"), ("cigar_off", "<u4"), ("cigar_len", "<u4")])

# ---------------------------------------------------------------------------------------------------------------------
# CPU: layout
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define F(f) printf("%s %zu\n", #f, offsetof(spm_jst_ref_locus, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_jst_collapse_stats, f))
int main(void)
{
    F(ref_begin); F(ref_end); F(pattern); F(ref_score); F(score); F(n_records); F(cigar_off); F(cigar_len); F(member_off);
    F(n_haplotypes);
    S(ms_total); S(ms_slots); S(ms_order); S(ms_records); S(ms_emit); S(ms_host); S(n_alns); S(n_slots); S(n_loci); S(n_members);
    S(n_ops); S(n_multi_slot); S(max_run);
    printf("sizeof.locus %zu\nsizeof.stats %zu\n", sizeof(spm_jst_ref_locus), sizeof(spm_jst_collapse_stats));
    return 0;
}
"""
CALLS = ("spm_hip_jst_ref_alns_collapse", "spm_hip_jst_ref_loci_view", "spm_hip_jst_ref_loci_device", "spm_hip_jst_ref_loci_map",
         "spm_hip_jst_ref_loci_stats", "spm_hip_jst_ref_loci_destroy")


def test_record_layout_matches_the_header(spm, tmp_path):
    assert ctypes.sizeof(spm.capi.JstRefLocus) == 48 == spm.JST_REF_LOCUS_DTYPE.itemsize
    assert spm.JST_REF_LOCUS_DTYPE == LOCUS
    assert ctypes.sizeof(spm.capi.JstCollapseStats) == 80
    want = c_layout(tmp_path, LAYOUT_C)
    assert int(want.pop("sizeof.locus")) == 48 and int(want.pop("sizeof.stats")) == 80
    n_rec = n_st = 0
    for name, off in want.items():
        if name.startswith("stats."):
            assert getattr(spm.capi.JstCollapseStats, name[6:]).offset == int(off), name
            n_st += 1
        else:
            assert getattr(spm.capi.JstRefLocus, name).offset == int(off), name
            assert spm.JST_REF_LOCUS_DTYPE.fields[name][1] == int(off), name
            n_rec += 1
    assert n_rec == len(spm.capi.JstRefLocus._fields_) == len(spm.JST_REF_LOCUS_DTYPE.names) == 10
    assert n_st == len(spm.capi.JstCollapseStats._fields_) == 13
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    assert hasattr(spm.JstRefAlignments, "collapse")
    for name in ("view", "ops", "members", "member_scores", "locus_of", "cigar", "haplotypes", "device", "stats", "close"):
        assert hasattr(spm.JstRefLoci, name), name


# ---------------------------------------------------------------------------------------------------------------------
# the reference: tuples and sorted
# ---------------------------------------------------------------------------------------------------------------------
def np_collapse(rv, rops):
    """The rule of the header on the host view `rv` (REF_ALN records) and pool `rops` of a projection.  Returns a dict:
    loci (LOCUS records), ops, members, member_scores, locus_of, and the counters the rows assert their cases with."""
    rops = np.asarray(rops, dtype=np.uint32)
    content = []
    for r in rv:
        w = tuple(int(x) for x in rops[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])])
        assert len(w) == int(r["cigar_len"])
        content.append((int(r["pattern"]), int(r["ref_begin"]), int(r["ref_end"]), int(r["ref_score"]), len(w), w))
    order = sorted(set(content))
    number = {c: i for i, c in enumerate(order)}
    locus_of = np.array([number[c] for c in content], dtype=np.uint32)
    loci = np.zeros(len(order), dtype=LOCUS)
    ops, members, scores = [], [], []
    by_locus = [[] for _ in order]
    for i, l in enumerate(locus_of.tolist()):
        by_locus[l].append(i)
    n_multi_slot = n_mixed = n_twice = n_inside_merged = 0
    for l, (c, recs) in enumerate(zip(order, by_locus)):
        best = {}
        for i in recs:
            h, s = int(rv["haplotype"][i]), int(rv["score"][i])
            best[h] = min(best.get(h, s), s)
        haps = sorted(best)
        loci[l] = (c[1], c[2], c[0], c[3], min(best.values()), len(recs), len(ops), c[4], len(members), len(haps))
        ops += list(c[5])
        members += haps
        scores += [best[h] for h in haps]
        slots = {int(rv["cigar_off"][i]) for i in recs}
        n_multi_slot += len(slots) > 1
        n_mixed += len(set(best.values())) > 1
        n_twice += len(recs) > len(haps)
        n_inside_merged += c[1] == c[2] and len(recs) > 1
    runs = {}
    for c, off in {(c[:5], int(r["cigar_off"])) for c, r in zip(content, rv)}:
        runs[c] = runs.get(c, 0) + 1
    return {"loci": loci, "ops": np.array(ops, dtype=np.uint32), "members": np.array(members, dtype=np.uint32),
            "member_scores": np.array(scores, dtype=np.int32), "locus_of": locus_of,
            "n_slots": len({int(x) for x in rv["cigar_off"]}) if len(rv) else 0, "n_multi_slot": int(n_multi_slot),
            "n_mixed": int(n_mixed), "n_twice": int(n_twice), "n_inside_merged": int(n_inside_merged),
            "max_run": max(runs.values()) if runs else 0,
            "max_slots_per_locus": max((len({int(rv["cigar_off"][i]) for i in recs}) for recs in by_locus), default=0)}


def _invariants(want, rv, rops):
    """what the contract promises about any result, checked on the reference itself"""
    L, n = want["loci"], len(want["loci"])
    assert np.array_equal(L["cigar_off"], np.concatenate([[0], np.cumsum(L["cigar_len"])[:-1]]).astype(np.uint32)[:n])
    assert np.array_equal(L["member_off"], np.concatenate([[0], np.cumsum(L["n_haplotypes"])[:-1]]).astype(np.uint32)[:n])
    assert int(L["n_records"].sum()) == len(rv) and int(L["cigar_len"].sum()) == len(want["ops"])
    assert int(L["n_haplotypes"].sum()) == len(want["members"]) == len(want["member_scores"])
    keys = [(int(l["pattern"]), int(l["ref_begin"]), int(l["ref_end"]), int(l["ref_score"]), int(l["cigar_len"]),
             tuple(want["ops"][int(l["cigar_off"]):int(l["cigar_off"]) + int(l["cigar_len"])].tolist())) for l in L]
    assert all(a < b for a, b in zip(keys, keys[1:])), "loci are not strictly ascending"
    for l in L:
        m = want["members"][int(l["member_off"]):int(l["member_off"]) + int(l["n_haplotypes"])]
        s = want["member_scores"][int(l["member_off"]):int(l["member_off"]) + int(l["n_haplotypes"])]
        assert np.all(np.diff(m.astype(np.int64)) > 0) and int(s.min()) == int(l["score"]) and l["n_records"] >= l["n_haplotypes"]
    for i, r in enumerate(rv):
        l = L[int(want["locus_of"][i])]
        assert (l["pattern"], l["ref_begin"], l["ref_end"], l["ref_score"], l["cigar_len"]) == \
               (r["pattern"], r["ref_begin"], r["ref_end"], r["ref_score"], r["cigar_len"])
        assert np.array_equal(want["ops"][int(l["cigar_off"]):int(l["cigar_off"]) + int(l["cigar_len"])],
                              rops[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])])


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the worked cases of the header, records from the tests' own DP and projection
# ---------------------------------------------------------------------------------------------------------------------
def _dist(P, T):
    return _global_dp(P, T)[1]


def _records(ref, alleles, pool, cov, n_hap, needles, k):
    """Every hit of every needle on every haplotype with distance <= k, as the search defines it (an end, its distance, the
    LARGEST begin with that distance), aligned by the global DP of test_jst_project and projected by np_project: a
    projection's host view and pool, one slot per record."""
    recs, ops = [], []
    for h in range(n_hap):
        hap = _apply(ref, alleles, pool, cov, h)
        J = Journal(len(ref), alleles, cov, h)
        for p, P in enumerate(needles):
            m = len(P)
            for e in range(1, len(hap) + 1):
                cands = [(_dist(P, hap[b:e]), -b) for b in range(max(0, e - m - k), e + 1)]
                d, nb = min(cands)
                if d > k:
                    continue
                b = -nb
                words, d2 = _global_dp(P, hap[b:e])
                assert d2 == d
                rb, re, score, out, _kinds = np_project(J, ref, b, words, P)
                replay(P, ref, rb, re, out, score)
                recs.append((rb, re, h, p, d, score, len(ops), len(out)))
                ops += out.tolist()
    return np.array(recs, dtype=REF_ALN), np.array(ops, dtype=np.uint32)


def _alleles(rows, n_hap):
    al = np.zeros(len(rows), dtype=[("pos", "<u8"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("alt_off", "<u8")])
    cov = np.zeros((len(rows), 1), dtype=np.uint64)
    pool = []
    for i, (pos, rl, alt, hs) in enumerate(rows):
        al[i] = (pos, rl, len(alt), len(pool))
        pool += list(_r(alt))
        for h in hs:
            cov[i, 0] |= np.uint64(1) << np.uint64(h)
    return al, np.array(pool, dtype=np.uint8), cov


def _loci_where(want, **eq):
    out = []
    for i, l in enumerate(want["loci"]):
        if all(int(l[f]) == v for f, v in eq.items()):
            out.append((i, _cig(want["ops"][int(l["cigar_off"]):int(l["cigar_off"]) + int(l["cigar_len"])])))
    return out


def _members(want, i):
    l = want["loci"][i]
    lo, hi = int(l["member_off"]), int(l["member_off"]) + int(l["n_haplotypes"])
    return list(zip(want["members"][lo:hi].tolist(), want["member_scores"][lo:hi].tolist()))


def test_reference_case1_same_range_different_transcripts():
    ref = _r("GATTCGCAAAAGTCCATG")
    al, pool, cov = _alleles([(10, 1, "", (0,))], 2)
    rv, rops = _records(ref, al, pool, cov, 2, [_r("TTCGCAAAGTCCA")], 1)
    want = np_collapse(rv, rops)
    _invariants(want, rv, rops)
    got = _loci_where(want, ref_begin=2, ref_end=16)
    assert [c for _i, c in got] == ["5=1D8=", "8=1D5="], got          # two loci, in word order (5= < 8=)
    (i0, _), (i1, _) = got
    assert i1 == i0 + 1 and want["loci"][i0]["ref_score"] == want["loci"][i1]["ref_score"] == 1
    assert _members(want, i0) == [(1, 1)] and _members(want, i1) == [(0, 0)]


def test_reference_case2_one_haplotype_twice():
    ref = _r("GATTCGCATGTCCATG")
    al, pool, cov = _alleles([(8, 0, "G", (0,))], 1)
    rv, rops = _records(ref, al, pool, cov, 1, [_r("ATTCGCA")], 1)
    want = np_collapse(rv, rops)
    _invariants(want, rv, rops)
    got = _loci_where(want, ref_begin=1, ref_end=8)
    assert [c for _i, c in got] == ["7="], got
    l = want["loci"][got[0][0]]
    assert (int(l["n_records"]), int(l["n_haplotypes"]), int(l["score"])) == (2, 1, 0) and _members(want, got[0][0]) == [(0, 0)]
    assert sorted(rv["score"][want["locus_of"] == got[0][0]].tolist()) == [0, 1]      # 7= and 7=1D, the D on the inserted G
    assert want["n_twice"] >= 1


def test_reference_case3_one_member_score_per_haplotype():
    rng = np.random.default_rng(31)
    ref = rng.integers(0, 4, 60, dtype=np.uint8)
    snp = "ACGT"[(int(ref[30]) + 1) & 3]
    al, pool, cov = _alleles([(30, 1, snp, (1,))], 3)
    carrier = _apply(ref, al, pool, cov, 1)
    rv, rops = _records(ref, al, pool, cov, 3, [carrier[20:40].copy()], 1)
    want = np_collapse(rv, rops)
    _invariants(want, rv, rops)
    got = _loci_where(want, ref_begin=20, ref_end=40)
    assert [c for _i, c in got] == ["10=1X9="], got
    l = want["loci"][got[0][0]]
    assert int(l["score"]) == 0 and int(l["ref_score"]) == 1 and int(l["n_records"]) == 3
    assert _members(want, got[0][0]) == [(0, 1), (1, 0), (2, 1)] and want["n_mixed"] >= 1


def test_reference_case4_inside_an_insertion():
    rng = np.random.default_rng(41)
    ref = rng.integers(0, 4, 50, dtype=np.uint8)
    unit = "ACGTTGCATC"
    al, pool, cov = _alleles([(25, 0, unit + unit + "A", (0, 2))], 3)
    rv, rops = _records(ref, al, pool, cov, 3, [_r(unit[1:9])], 0)
    want = np_collapse(rv, rops)
    _invariants(want, rv, rops)
    got = _loci_where(want, ref_begin=25, ref_end=25)
    assert [c for _i, c in got] == ["8I"], got          # both copies, on both carriers: pattern and anchor agree
    l = want["loci"][got[0][0]]
    assert (int(l["n_records"]), int(l["n_haplotypes"])) == (4, 2) and _members(want, got[0][0]) == [(0, 0), (2, 0)]
    assert want["n_inside_merged"] == 1 and len(want["loci"]) == 1


def test_reference_is_a_function_of_the_record_set():
    """about 2 000 random record sets over few distinct values (so that records merge), each in several arrival orders and
    pool layouts -- shuffled records, shuffled slots, slots shared or private: one result"""
    rng = np.random.default_rng(2026)
    merged = multi = 0
    for _ in range(2000):
        n_content = int(rng.integers(1, 8))
        contents = []
        for _c in range(n_content):
            w = [(int(rng.integers(1, 3)) << 4) | int(rng.choice([EQ, X, INS, DEL])) for _w in range(int(rng.integers(1, 4)))]
            contents.append((int(rng.integers(0, 2)), int(rng.integers(0, 3)), 3 + int(rng.integers(0, 2)), int(rng.integers(0, 2)), w))
        n = int(rng.integers(1, 25))
        picks = [(int(rng.integers(0, n_content)), int(rng.integers(0, 5)), int(rng.integers(0, 3))) for _i in range(n)]
        first = None
        for _order in range(3):
            perm = rng.permutation(n)
            share = bool(rng.integers(0, 2))
            slot_of, ops, recs = {}, [], []
            for j in perm.tolist():
                c, h, s = picks[j]
                key = c if share else (c, j)
                if key not in slot_of:
                    slot_of[key] = len(ops)
                    ops += contents[c][4]
                p, b, e, sc, w = contents[c]
                recs.append((b, e, h, p, s, sc, slot_of[key], len(w)))
            rv, rops = np.array(recs, dtype=REF_ALN), np.array(ops, dtype=np.uint32)
            want = np_collapse(rv, rops)
            _invariants(want, rv, rops)
            back = np.empty(n, dtype=np.uint32)
            back[perm] = want["locus_of"]               # the map in the order of `picks`
            blob = (want["loci"].tobytes(), want["ops"].tobytes(), want["members"].tobytes(), want["member_scores"].tobytes(),
                    back.tobytes())
            if first is None:
                first = blob
            assert blob == first
            merged += len(want["loci"]) < n
            multi += want["n_multi_slot"] > 0
    assert merged > 1000 and multi > 500


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _blob(lc):
    return (lc.view().tobytes(), lc.ops.tobytes(), lc.members.tobytes(), lc.member_scores.tobytes(), lc.locus_of.tobytes())


def _compare(lc, want, rv):
    got, st = lc.view(), lc.stats()
    assert got.dtype == LOCUS and len(got) == len(want["loci"]), (len(got), len(want["loci"]))
    for f in LOCUS.names:
        assert np.array_equal(got[f], want["loci"][f]), f
    assert got.tobytes() == want["loci"].tobytes()
    assert lc.ops.tobytes() == want["ops"].tobytes()
    assert lc.members.tobytes() == want["members"].tobytes()
    assert lc.member_scores.tobytes() == want["member_scores"].tobytes()
    assert lc.locus_of.tobytes() == want["locus_of"].tobytes()
    assert (st.n_alns, st.n_loci, st.n_members, st.n_ops) == (len(rv), len(got), len(want["members"]), len(want["ops"]))
    assert (st.n_slots, st.n_multi_slot, st.max_run) == (want["n_slots"], want["n_multi_slot"], want["max_run"])
    assert len(lc) == len(got)
    print(f"records {len(rv)}, slots {st.n_slots} -> loci {st.n_loci}, members {st.n_members}, words {st.n_ops}; multi-slot "
          f"{st.n_multi_slot}, max run {st.max_run}; device ms slots {st.ms_slots:.3f} order {st.ms_order:.3f} records "
          f"{st.ms_records:.3f} emit {st.ms_emit:.3f}, host {st.ms_host:.3f}")


def _collapse_checked(spm, ctx, t, needles, src, block, need=(), min_shared=True):
    """src (JstAlignments): its projection pinned by _check; its collapse compared with the reference.  Returns
    (reference result, projected host view, blob of the device result)."""
    _check(spm, ctx, t, needles, src, block, need, min_shared)
    pr = src.project()
    rv, rops = pr.view(), pr.ops
    want = np_collapse(rv, rops)
    lc = pr.collapse()
    try:
        _compare(lc, want, rv)
        # every projected slot has a pool offset of its own, so the collapse finds the projection's slots again: both number
        # them with the one stage of transcript_slots.hpp
        assert lc.stats().n_slots == pr.stats().n_projected
        return want, rv, _blob(lc)
    finally:
        lc.close()
        pr.close()


def _search_collapse(spm, ctx, t, needles, k, block, need=(), algo=None, shard=None, min_shared=True, engine=None):
    ref_text, jst, ps = _open(spm, ctx, t, needles, k, algo)
    try:
        jst.index(_window(ps, len(needles)), block, *(shard or ()))
        h = jst.search_device(ps, alignable=True, max_hits=1 << 21, **({} if engine is None else {"engine": engine}))
        if engine is not None:
            assert ps.filterable and jst.stats().engine_used == engine, "the row does not run the engine it is named for"
        a = h.align()
        try:
            return _collapse_checked(spm, ctx, t, needles, a, block, need, min_shared)
        finally:
            a.close()
            h.close()
    finally:
        jst.close()
        ps.close()
        ref_text.close()


_shared = {}


def _row1(spm, ctx):
    """the row-1 search, collapsed once and shared (read-only) by the rows that compare with it"""
    if "row1" not in _shared:
        t, needles = _row1_tree()
        _shared["row1"] = _search_collapse(spm, ctx, t, needles, 2, 64, ALL_KINDS)
    return _shared["row1"]


@pytest.mark.gpu
def test_row1_every_allele_kind(spm, ctx):
    want, rv, _b = _row1(spm, ctx)
    assert want["n_multi_slot"] > 0, "no locus merges several slots"
    assert want["n_mixed"] > 0, "no locus has mixed member scores"
    assert len(want["loci"]) < len(rv), "nothing merged"


HOMO, TWICE = "GATTCGCAAAAGTCCATG", "GATTCGCATGTCCATG"


@pytest.mark.gpu
def test_row2_hand_made_alleles(spm, ctx):
    rng = np.random.default_rng(7)
    unit = rng.integers(0, 4, 40, dtype=np.uint8)
    big = np.concatenate([unit, unit])                        # an 80-symbol insertion that holds every 24-mer of `unit` twice
    p_homo, p_twice = 2000, 3000
    extra = [(p_homo + 10, 1, [], (0,)), (p_twice + 8, 0, _r("G"), (0,)), (5000, 0, big, (1, 3))]
    t = _make_tree(211, 16_000, 6, 8, 60, extra=extra)
    t["ref"][p_homo:p_homo + len(HOMO)] = _r(HOMO)            # (before any haplotype is materialised)
    t["ref"][p_twice:p_twice + len(TWICE)] = _r(TWICE)
    needles = _plant(t, 212, 40, 1, per_kind=1)
    n0 = len(needles)
    needles += [_r("TTCGCAAAGTCCA"), _r("ATTCGCA"), unit[3:27].copy()]
    want, rv, _b = _search_collapse(spm, ctx, t, needles, 1, 64, ("inside",))
    # the homopolymer deletion: two loci with one range, in word order
    got = _loci_where(want, pattern=n0, ref_begin=p_homo + 2, ref_end=p_homo + 16)
    assert [c for _i, c in got] == ["5=1D8=", "8=1D5="] and got[1][0] == got[0][0] + 1, got
    assert _members(want, got[0][0]) == [(h, 1) for h in range(1, 6)] and _members(want, got[1][0]) == [(0, 0)]
    # the insertion behind the needle's end: haplotype 0 twice in one locus
    got = _loci_where(want, pattern=n0 + 1, ref_begin=p_twice + 1, ref_end=p_twice + 8)
    assert [c for _i, c in got] == ["7="], got
    l = want["loci"][got[0][0]]
    assert int(l["n_haplotypes"]) == 6 and int(l["n_records"]) == 7 and _members(want, got[0][0]) == [(h, 0) for h in range(6)]
    mine = rv[want["locus_of"] == got[0][0]]
    assert sorted(mine[mine["haplotype"] == 0]["score"].tolist()) == [0, 1] and want["n_twice"] >= 1
    # needles inside the insertion: every copy on both carriers merges at the anchor
    got = _loci_where(want, pattern=n0 + 2, ref_begin=5000, ref_end=5000)
    assert [c for _i, c in got] == ["24I"], got
    l = want["loci"][got[0][0]]
    assert int(l["n_haplotypes"]) == 2 and int(l["n_records"]) >= 4 and want["n_inside_merged"] >= 1
    assert [h for h, _s in _members(want, got[0][0])] == [1, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["block16", "block128", "again"])
def test_row3_invariance(spm, ctx, variant):
    _w, _rv, base = _row1(spm, ctx)
    t, needles = _row1_tree()
    block = {"block16": 16, "block128": 128}.get(variant, 64)
    _want, _rv2, blob = _search_collapse(spm, ctx, t, needles, 2, block)
    # (the host map belongs to the projection's host view, which is in the order of every host view of pan-genome hits)
    assert blob == base, variant


@pytest.mark.gpu
def test_row3_brute_against_filter_engine(spm, ctx):
    t, _needles = _row1_tree()
    needles = _plant(t, 103, 64, 2)                           # (long enough for the seed filter to take the set)
    _w1, _r1, brute = _search_collapse(spm, ctx, t, needles, 2, 64, engine=spm.ENGINE_BRUTE)
    want, rv, filt = _search_collapse(spm, ctx, t, needles, 2, 64, engine=spm.ENGINE_FILTER)
    assert brute == filt and len(want["loci"]) < len(rv)


@pytest.mark.gpu
@pytest.mark.parametrize("across", [False, True])
def test_row4_selections(spm, ctx, across):
    full, frv, _b = _row1(spm, ctx)
    t, needles = _row1_tree()
    ref_text, jst, ps = _open(spm, ctx, t, needles, 2)
    jst.index(_window(ps, len(needles)), 64)
    h = jst.search_device(ps, alignable=False, max_hits=1 << 21)
    sel = h.select(best=0 if across else 1, across=across)
    assert 0 < len(sel) < len(h)
    b = sel.align_selected()
    want, rv, _blob2 = _collapse_checked(spm, ctx, t, needles, b, 64, min_shared=False)
    # every such locus is a locus of the full result, with a subset of its members
    key = lambda R, l: (int(l["pattern"]), int(l["ref_begin"]), int(l["ref_end"]),
                        R["ops"][int(l["cigar_off"]):int(l["cigar_off"]) + int(l["cigar_len"])].tobytes())
    index = {key(full, l): i for i, l in enumerate(full["loci"])}
    assert 0 < len(want["loci"]) <= len(full["loci"])
    for i, l in enumerate(want["loci"]):
        j = index[key(want, l)]
        have = dict(_members(full, j))
        assert all(h in have and s >= have[h] for h, s in _members(want, i))   # (a haplotype's kept records are some of its records)
    for x in (b, sel, h, jst, ps, ref_text):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 0])
def test_row5_locus_counts_around_a_workgroup(spm, ctx, n):
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
    want, _rv, _b = _collapse_checked(spm, ctx, t, needles, a, 64, min_shared=False)
    assert len(want["loci"]) == n
    if n == 0:
        pr = a.project()
        lc = pr.collapse()
        d = lc.device()
        assert len(lc) == 0 and len(lc.ops) == 0 and len(lc.members) == 0 and len(lc.locus_of) == 0
        assert d["n"] == d["n_ops"] == d["n_members"] == d["n_alns"] == 0 and lc.stats().n_slots == 0 == pr.stats().n_projected
        lc.close()
        pr.close()
    for x in (a, h, jst, ps, ref_text):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_hap", [63, 64, 65, 70, 1100])
def test_row5_members_per_locus(spm, ctx, n_hap):
    """haplotypes without alleles near the read: every one of them is a member of the read's locus, so the member list crosses
    a wave (64), a coverage word (64) and a haplotype group (1 024)"""
    n_ref = 4_000
    t = _make_tree(500 + n_hap, n_ref, n_hap, 8, 24)
    pos = np.sort(t["alleles"]["pos"].astype(np.int64))
    gaps = np.diff(np.concatenate([[0], pos, [n_ref]]))
    g = int(np.argmax(gaps))
    lo = int(np.concatenate([[0], pos])[g])
    assert gaps[g] > 200
    at = lo + int(gaps[g]) // 2 - 20
    read = t["ref"][at:at + 40].copy()
    want, _rv, _b = _search_collapse(spm, ctx, t, [read], 1, 64, min_shared=False)
    got = _loci_where(want, ref_begin=at, ref_end=at + 40)
    assert [c for _i, c in got] == ["40="], got
    assert _members(want, got[0][0]) == [(h, 0) for h in range(n_hap)]


def _no_repeat(rng, n):
    """n symbols, no two adjacent ones equal: a one-base deletion inside has exactly one optimal alignment"""
    out = [int(rng.integers(0, 4))]
    while len(out) < n:
        out.append((out[-1] + 1 + int(rng.integers(0, 3))) & 3)
    return np.array(out, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("n_hap", [140, 63, 64, 65])
def test_row6_long_runs(spm, ctx, n_hap):
    """Every haplotype carries a private one-base deletion at a distinct position inside one read (k = 1): as many distinct
    transcripts with one range, NM and length as there are haplotypes -- one run that the words alone order; with 140
    haplotypes it crosses two waves.  (The read has 160 symbols: 140 distinct interior positions do not fit into 120.)  A
    second read next to private SNPs OUTSIDE its span gives the opposite: many slots, one locus."""
    rng = np.random.default_rng(600 + n_hap)
    L, at, at2 = 160, 1000, 2560 - 38                          # the second read ends 2 symbols into block 2560 / 64
    n_snp = min(n_hap, 50)
    extra = [(at + 10 + h, 1, [], (h,)) for h in range(n_hap)]
    t = _make_tree(601, 4_000, n_hap, 8, 0, extra=extra)
    t["ref"][at:at + L] = _no_repeat(rng, L)
    for h in range(n_snp):                                     # private SNPs behind the second read, in the block of its end
        p = 2560 + 6 + h
        extra.append((p, 1, [(int(t["ref"][p]) + 1) & 3], (h,)))
    t = dict(_make_tree(601, 4_000, n_hap, 8, 0, extra=extra), ref=t["ref"])
    needles = [t["ref"][at:at + L].copy(), t["ref"][at2:at2 + 40].copy()]
    want, rv, _b = _search_collapse(spm, ctx, t, needles, 1, 64, min_shared=False)
    run = _loci_where(want, pattern=0, ref_begin=at, ref_end=at + L)
    assert len(run) == n_hap and want["max_run"] == n_hap, (len(run), want["max_run"])
    assert n_hap < 129 or len(run) >= 129
    idx = [i for i, _c in run]
    assert idx == list(range(idx[0], idx[0] + n_hap))          # one contiguous run ...
    L_ = want["loci"][idx]
    assert len(set(L_["cigar_len"].tolist())) == 1 and set(L_["ref_score"].tolist()) == {2} and set(L_["n_records"].tolist()) == {1}
    words = [tuple(want["ops"][int(l["cigar_off"]):int(l["cigar_off"]) + int(l["cigar_len"])].tolist()) for l in L_]
    assert words == sorted(words) and len(set(words)) == n_hap  # ... in word order
    assert [c for _i, c in run][0] == f"10=1I1D{L - 11}="      # the deletion nearest the read's begin has the smallest first word
    one = _loci_where(want, pattern=1, ref_begin=at2, ref_end=at2 + 40)
    assert [c for _i, c in one] == ["40="], one
    assert _members(want, one[0][0]) == [(h, 0) for h in range(n_hap)]
    slots = {int(r["cigar_off"]) for r in rv[want["locus_of"] == one[0][0]]}
    assert len(slots) >= n_snp and want["max_slots_per_locus"] >= n_snp, (len(slots), n_snp)


@pytest.mark.gpu
def test_row7_exact_set(spm, ctx):
    t, _ = _row1_tree()
    needles = _plant(t, 502, 32, 0)
    want, rv, _b = _search_collapse(spm, ctx, t, needles, 0, 64, ALL_KINDS, algo=spm.ALGO_SHIFTOR)
    assert len(want["loci"]) < len(rv) and any(int(l["ref_score"]) > 0 for l in want["loci"])


@pytest.mark.gpu
def test_row7_dna5_reference_with_n_runs(spm, ctx):
    t = _make_tree(601, 16_000, 6, 8, 160, sigma=5, n_runs=60)
    needles = _plant(t, 602, 40, 2)
    assert any(4 in nd for nd in needles), "no needle holds an N"
    want, rv, _b = _search_collapse(spm, ctx, t, needles, 2, 64, ALL_KINDS)
    assert len(want["loci"]) < len(rv)


@pytest.mark.gpu
def test_row7_block_shard(spm, ctx):
    t, needles = _row1_tree()
    n_blocks = -(-len(t["ref"]) // 64)
    want, rv, _b = _search_collapse(spm, ctx, t, needles, 2, 64, (), shard=(n_blocks // 3, 2 * n_blocks // 3), min_shared=False)
    assert 0 < len(want["loci"]) < len(rv)


@pytest.mark.gpu
def test_row8_refusals_lifetimes_and_the_device_view(spm, ctx):
    t, needles = _row1_tree()
    ref_text, jst, ps = _open(spm, ctx, t, needles, 2)
    jst.index(_window(ps, len(needles)), 64)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    a = h.align()
    pr = a.project()
    rv, rops = pr.view(), pr.ops
    want = np_collapse(rv, rops)
    lib = spm.capi.lib()
    # nonzero flags through the raw ABI; NULL arguments
    out = ctypes.c_void_p()
    assert lib.spm_hip_jst_ref_alns_collapse(pr._h, 1, ctypes.byref(out)) == -1 and not out.value
    assert b"flag" in lib.spm_hip_last_error(ctx._h)
    assert lib.spm_hip_jst_ref_alns_collapse(None, 0, ctypes.byref(out)) == -1 and not out.value
    assert lib.spm_hip_jst_ref_alns_collapse(pr._h, 0, None) == -1
    n64 = ctypes.c_uint64()
    assert lib.spm_hip_jst_ref_loci_view(None, None, None, None, None, None, None, None) == -1
    assert lib.spm_hip_jst_ref_loci_device(None, None, None, None, None, None, None, None) == -1
    assert lib.spm_hip_jst_ref_loci_map(None, None, None, ctypes.byref(n64)) == -1
    assert lib.spm_hip_jst_ref_loci_stats(None, None) == -1
    lib.spm_hip_jst_ref_loci_destroy(None)
    # two calls in a row: identical bytes
    l1, l2 = pr.collapse(), pr.collapse()
    assert _blob(l1) == _blob(l2)
    _compare(l1, want, rv)
    # the device view equals the host view; the device map belongs to the source's DEVICE view
    d = l1.device()
    assert (d["n"], d["n_ops"], d["n_members"], d["n_alns"]) == (len(want["loci"]), len(want["ops"]), len(want["members"]), len(rv))
    assert download(ctx, d["records"], d["n"], LOCUS).tobytes() == want["loci"].tobytes()
    assert download(ctx, d["ops"], d["n_ops"], np.dtype("<u4")).tobytes() == want["ops"].tobytes()
    assert download(ctx, d["members"], d["n_members"], np.dtype("<u4")).tobytes() == want["members"].tobytes()
    assert download(ctx, d["member_scores"], d["n_members"], np.dtype("<i4")).tobytes() == want["member_scores"].tobytes()
    dmap = download(ctx, d["locus_of"], d["n_alns"], np.dtype("<u4"))
    rp, rn, _ro, _rno = pr.device()
    drv = download(ctx, rp, rn, REF_ALN)
    dwant = np_collapse(drv, rops)                            # (the same set of records in another order: the same loci)
    assert dwant["loci"].tobytes() == want["loci"].tobytes() and dmap.tobytes() == dwant["locus_of"].tobytes()
    assert l1.cigar(0) == _cig(want["ops"][:int(want["loci"][0]["cigar_len"])])
    hm, hs = l1.haplotypes(0)
    assert list(zip(hm.tolist(), hs.tolist())) == _members(want, 0)
    # the result outlives source, alignments, search, tree and needle set; a fresh collapse needs neither tree nor set
    l2.close()
    for x in (a, h, jst, ps, ref_text):
        x.close()
    l3 = pr.collapse()
    _compare(l3, want, rv)
    pr.close()
    _compare(l1, want, rv)
    _compare(l3, want, rv)
    assert download(ctx, d["records"], d["n"], LOCUS).tobytes() == want["loci"].tobytes()
    # a closed source
    with pytest.raises(spm.SpmError):
        pr.collapse()
    l1.close()
    l3.close()
    with pytest.raises(spm.SpmError):
        l1.view()
