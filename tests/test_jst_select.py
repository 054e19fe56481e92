"""Selection of pan-genome hits on the device (spm_hip_jst_hits_select / spm_hip_jst_records_select; contract in
include/spm_hip.h, scheme in DESIGN.md 4.7): one record per locus of every haplotype -- the locus is (haplotype, pattern) --
and the best error stratum per (haplotype, pattern), or per pattern across all haplotypes.

The yardsticks never come from the code under test:
  (a) `rule` of test_select -- the literal definition of plain selection -- applied to the records of one haplotype at a
      time (`jrule` below);
  (b) the route that needs no tree: every haplotype spelled out by the NumPy allele walk of test_gpu_jst, uploaded, scanned
      and selected with the existing Hits.select().
SPM_SELECT_ACROSS has no per-haplotype route: its yardstick is (a) for LOCI, then the stratum test against the minimum
taken per pattern over ALL input records."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_gpu_jst import _apply, _random_alleles
from test_select import HAND, HIT, rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JH = np.dtype([("pos", "<u8"), ("haplotype", "<u4"), ("pattern", "<u4"), ("score", "<i4"), ("reserved", "<u4")])
gpu = pytest.mark.gpu


def host_order(a):
    """the order of every spm_hip_jst_hits_view: (haplotype, pos, pattern, score)"""
    return a[np.lexsort((a["score"], a["pattern"], a["pos"], a["haplotype"]))]


def device_order(a):
    """the order of a selection's device view: (haplotype, pattern, pos)"""
    return a[np.lexsort((a["pos"], a["pattern"], a["haplotype"]))]


def jrecs(rows):
    """rows of (haplotype, pattern, pos, score) -> JH records in host order"""
    a = np.zeros(len(rows), dtype=JH)
    for i, (h, p, pos, s) in enumerate(rows):
        a[i] = (pos, h, p, s, 0)
    return host_order(a)


def jrows(a):
    return [(int(h), int(p), int(x), int(s)) for h, p, x, s in zip(a["haplotype"], a["pattern"], a["pos"], a["score"])]


def jrule(v, w, best=None, loci=True, across=False):
    """Yardstick (a).  v: JH records; w: one window, or one per pattern.  `rule` sees the records of one haplotype at a time,
    as plain HIT records sorted by (pattern, pos); what it keeps is picked out of v by (pattern, pos), which is unique within
    a haplotype.  across: rule does LOCI only, and the stratum test uses the minimum per pattern over all of v."""
    assert not across or best is not None
    out = []
    for h in np.unique(v["haplotype"]):
        sub = v[v["haplotype"] == h]
        sub = sub[np.lexsort((sub["pos"], sub["pattern"]))]
        plain = np.zeros(len(sub), dtype=HIT)
        for f in ("pos", "pattern", "score"):
            plain[f] = sub[f]
        kept = rule(plain, w, best=None if across else best, loci=loci)
        places = np.unique(plain["pos"])                       # (pattern, rank of the position): no two records share it
        key = lambda a: a["pattern"].astype(np.int64) * len(places) + np.searchsorted(places, a["pos"])
        out.append(sub[np.isin(key(plain), key(kept))])
    out = np.concatenate(out) if out else v[:0]
    if across and len(v):
        mn = np.full(int(v["pattern"].max()) + 1, np.iinfo(np.int64).max)
        np.minimum.at(mn, v["pattern"].astype(np.int64), v["score"].astype(np.int64))
        out = out[out["score"].astype(np.int64) <= mn[out["pattern"].astype(np.int64)] + best]
    return host_order(out)


# ------------------------------------------------------------------------------------------------------------------
# CPU: layouts, the rule on hand-worked lists
# ------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
int main(void)
{
    int (*a)(spm_jst_hits *, const spm_select_opts *, spm_jst_hits **) = spm_hip_jst_hits_select;
    int (*b)(spm_ctx *, const void *, uint64_t, const spm_patterns *, const spm_select_opts *, spm_jst_hits **) =
        spm_hip_jst_records_select;
    int (*c)(const spm_jst_hits *, spm_select_stats *) = spm_hip_jst_hits_select_stats;
    printf("flags %u %u %u %u\n", SPM_SELECT_LOCI, SPM_SELECT_BEST, SPM_SELECT_ACROSS, SPM_SELECT_WINDOW_K);
    printf("hit %zu %zu %zu %zu %zu %zu\n", sizeof(spm_jst_hit), offsetof(spm_jst_hit, pos), offsetof(spm_jst_hit, haplotype),
           offsetof(spm_jst_hit, pattern), offsetof(spm_jst_hit, score), offsetof(spm_jst_hit, reserved));
    printf("opts %zu stats %zu %zu %zu %zu %zu\n", sizeof(spm_select_opts), sizeof(spm_select_stats),
           offsetof(spm_select_stats, n_in), offsetof(spm_select_stats, n_loci), offsetof(spm_select_stats, n_out),
           offsetof(spm_select_stats, key_bits));
    return !(a && b && c);
}
"""


def test_layouts_and_flags_match_the_header(spm, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    lib = os.path.join(ROOT, "libspm_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-L" + lib, "-l:libspm_hip.so", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    got = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [int(x) for x in got["flags"].split()] == [1, 2, 4, 0xFFFFFFFF]
    assert (spm.capi.SELECT_LOCI, spm.capi.SELECT_BEST, spm.capi.SELECT_ACROSS, spm.capi.SELECT_WINDOW_K) == (1, 2, 4, 0xFFFFFFFF)
    assert spm.SELECT_ACROSS == 4
    assert [int(x) for x in got["hit"].split()] == [24] + [JH.fields[f][1] for f in JH.names] == [24, 0, 8, 12, 16, 20]
    assert spm.JST_HIT_DTYPE == JH and ctypes.sizeof(spm.capi.JstHit) == 24
    S = spm.capi.SelectStats
    assert [int(x) for x in got["opts"].split()[:1]] == [ctypes.sizeof(spm.capi.SelectOpts)] == [16]
    assert [int(x) for x in got["opts"].split()[2:]] == [ctypes.sizeof(S), S.n_in.offset, S.n_loci.offset, S.n_out.offset,
                                                         S.key_bits.offset]
    for name in ("spm_hip_jst_hits_select", "spm_hip_jst_records_select", "spm_hip_jst_hits_select_stats"):
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    assert callable(spm.JstHits.select) and callable(spm.JstHits.select_stats) and callable(spm.JstHits.device)
    assert callable(spm.select_jst_records)


SIX = [(0, 0, 10, 1), (0, 0, 11, 1), (0, 0, 50, 2), (1, 0, 10, 2), (1, 0, 60, 3), (0, 1, 20, 0), (1, 1, 20, 1)]
JHAND = [
    # name, records (haplotype, pattern, pos, score), kwargs of jrule, the kept records in host order -- worked by hand
    ("one pattern on two adjacent haplotypes within w: both kept",
     [(0, 0, 5, 0), (0, 1, 100, 1), (1, 1, 101, 2)], dict(w=3), [(0, 0, 5, 0), (0, 1, 100, 1), (1, 1, 101, 2)]),
    ("the same with n_patterns = 1", [(0, 0, 100, 1), (1, 0, 101, 2)], dict(w=3), [(0, 0, 100, 1), (1, 0, 101, 2)]),
    # (within one haplotype the pair is one locus)
    ("the same two records on one haplotype", [(1, 0, 100, 1), (1, 0, 101, 2)], dict(w=3), [(1, 0, 100, 1)]),
    # hap 0 / pattern 0: 11 ties with 10 and lies right of it; nothing else is within 3 of anything
    ("LOCI on the list of seven", SIX, dict(w=3), [(0, 0, 10, 1), (0, 1, 20, 0), (0, 0, 50, 2), (1, 0, 10, 2), (1, 1, 20, 1), (1, 0, 60, 3)]),
    # minima per (haplotype, pattern): (0,0) 1, (1,0) 2, (0,1) 0, (1,1) 1
    ("BEST per haplotype", SIX, dict(w=3, best=0), [(0, 0, 10, 1), (0, 1, 20, 0), (1, 0, 10, 2), (1, 1, 20, 1)]),
    # minima per pattern over both haplotypes: pattern 0 -> 1, pattern 1 -> 0
    ("ACROSS on the same list", SIX, dict(w=3, best=0, across=True), [(0, 0, 10, 1), (0, 1, 20, 0)]),
    ("ACROSS strata 1", SIX, dict(w=3, best=1, across=True), [(0, 0, 10, 1), (0, 1, 20, 0), (0, 0, 50, 2), (1, 0, 10, 2), (1, 1, 20, 1)]),
    ("BEST per haplotype strata 1", SIX, dict(w=3, best=1),
     [(0, 0, 10, 1), (0, 1, 20, 0), (0, 0, 50, 2), (1, 0, 10, 2), (1, 1, 20, 1), (1, 0, 60, 3)]),
    ("BEST alone: LOCI's loser stays", SIX, dict(w=3, best=0, loci=False),
     [(0, 0, 10, 1), (0, 0, 11, 1), (0, 1, 20, 0), (1, 0, 10, 2), (1, 1, 20, 1)]),
    ("ACROSS without LOCI", SIX, dict(w=3, best=0, loci=False, across=True), [(0, 0, 10, 1), (0, 0, 11, 1), (0, 1, 20, 0)]),
    ("neither flag: a sorted copy", [(1, 1, 5, 1), (1, 0, 5, 2), (0, 0, 11, 2), (0, 0, 10, 2)], dict(w=3, loci=False),
     [(0, 0, 10, 2), (0, 0, 11, 2), (1, 0, 5, 2), (1, 1, 5, 1)]),
    # the last record of haplotype 0 and the first of haplotype 1 are one apart: they never see each other
    ("two haplotypes, one pattern, a border inside w",
     [(0, 0, 500, 2), (0, 0, 1000, 2), (1, 0, 1001, 1), (1, 0, 1500, 0)], dict(w=3),
     [(0, 0, 500, 2), (0, 0, 1000, 2), (1, 0, 1001, 1), (1, 0, 1500, 0)]),
    ("... with BEST", [(0, 0, 500, 2), (0, 0, 1000, 2), (1, 0, 1001, 1), (1, 0, 1500, 0)], dict(w=3, best=0),
     [(0, 0, 500, 2), (0, 0, 1000, 2), (1, 0, 1500, 0)]),
    ("w = 0 keeps everything", [(2, 1, 10, 3), (2, 1, 11, 2), (2, 1, 12, 2)], dict(w=0), [(2, 1, 10, 3), (2, 1, 11, 2), (2, 1, 12, 2)]),
]
# ... and the plain hand-worked lists of test_select (one window, no segments) moved to haplotype 2 of three
for _name, _given, _kw, _want in HAND:
    if "segs" not in _kw and np.isscalar(_kw["w"]):
        _side = [(0, 0, 10, 9), (3, 0, 10, 9)]
        JHAND.append(("plain: " + _name, [(2, p, x, s) for p, x, s in _given] + _side, _kw,
                      [_side[0]] + sorted([(2, p, x, s) for p, x, s in _want], key=lambda r: (r[2], r[1])) + [_side[1]]))


@pytest.mark.parametrize("case", JHAND, ids=[c[0] for c in JHAND])
def test_rule_per_haplotype_on_hand_worked_lists(case):
    _, given, kw, want = case
    kw = dict(kw)
    assert jrows(jrule(jrecs(given), kw.pop("w"), **kw)) == want


# ------------------------------------------------------------------------------------------------------------------
# the trees of the GPU tests, built on the host alone
# ------------------------------------------------------------------------------------------------------------------
ROWS = [
    # name, seed, n_ref, n_hap, n_var, max allele length, algo, |P|, k, needles, sigma
    ("one haplotype", 101, 20_000, 1, 60, 8, "myers", 64, 2, 24, 4),
    ("five haplotypes, |P| = 100", 102, 30_000, 5, 150, 12, "myers", 100, 4, 24, 4),
    ("seventy haplotypes: two coverage words", 103, 24_000, 70, 120, 10, "myers", 64, 4, 24, 4),
    ("|P| = 200", 1044, 60_000, 5, 200, 12, "myers", 200, 2, 24, 4),
    ("a single needle", 2095, 20_000, 5, 100, 8, "myers", 100, 2, 1, 4),
    ("shift-or with tandem stretches", 106, 20_000, 5, 300, 3, "shiftor", 24, 0, 24, 4),
    ("dna5", 107, 20_000, 5, 100, 8, "myers", 64, 2, 24, 5),
]
# (the seeds are validated by test_tree_seeds_are_not_vacuous_by_the_oracle_alone)
TANDEM = [(5000, [0]), (9000, [0, 1]), (13000, [2, 3, 1])]     # shift-or row: 80 bases of each unit in the reference


def _needle(rng, hp, L, k, myers):
    """L symbols cut from hp with at most k - 1 edits (one of them an insertion or a deletion, every other time): the
    occurrence ends within k at its own end and at both neighbours, so every needle comes back as a cluster."""
    o = int(rng.integers(0, len(hp) - L - 4))
    nd = hp[o:o + L + 2].copy()
    edits = int(rng.integers(0, k)) if myers and k else 0
    if edits and rng.integers(0, 2):
        at = int(rng.integers(3, L - 3))
        nd = np.delete(nd, at) if rng.integers(0, 2) else np.insert(nd, at, (int(nd[at]) + 1 + int(rng.integers(0, 3))) & 3)
        edits -= 1
    nd = nd[:L].copy()
    for at in rng.choice(L, size=edits, replace=False):
        nd[at] = (int(nd[at]) + 1 + int(rng.integers(0, 3))) & 3
    return nd.astype(np.uint8)


_trees = {}


def tree_of(row):
    """reference, alleles, the haplotypes spelled out, needles: NumPy alone, the same on every machine"""
    if row[0] in _trees:
        return _trees[row[0]]
    name, seed, n_ref, n_hap, n_var, max_len, algo, L, k, n_needles, sigma = row
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
    if algo == "shiftor":
        for at, unit in TANDEM:
            ref[at:at + 80] = np.tile(np.array(unit, dtype=np.uint8), 80)[:80]
    alleles, pool, cov = _random_alleles(rng, n_ref, n_hap, n_var, max_len)
    if sigma == 5:                                           # as test_jst_align's dna5 row: 4 is a base, 3 is rare
        ref[ref == 3] = 4
        ref[rng.integers(0, n_ref, 60)] = 3
        pool[pool == 3] = 4
    haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
    needles = []
    while len(needles) < n_needles:
        nd = _needle(rng, haps[int(rng.integers(0, n_hap))], L, k, algo == "myers")
        if sigma == 4 or not np.any(nd == 3):                # (dna5: needles without the rare symbol)
            needles.append(nd)
    if algo == "shiftor":
        needles[-3:] = [np.tile(np.array(unit, dtype=np.uint8), L)[:L] for _, unit in TANDEM]
    t = dict(ref=ref, alleles=alleles, pool=pool, cov=cov, haps=haps, needles=needles, myers=algo == "myers", L=L, k=k,
             n_hap=n_hap, sigma=sigma, small_block=128 if L == 200 else L // 2)
    _trees[row[0]] = t
    return t


def _hap_coord(alleles, cov, h, r):
    """haplotype h's coordinate of reference position r; None where r lies in or at an allele h carries"""
    shift = 0
    for i, a in enumerate(alleles):
        p, rl, al = int(a["pos"]), int(a["ref_len"]), int(a["alt_len"])
        if p > r:
            break
        if not (int(cov[i, h >> 6]) >> (h & 63)) & 1:
            continue
        if p == r or p + rl > r:
            return None
        shift += al - rl
    return r + shift


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_tree_seeds_are_not_vacuous_by_the_oracle_alone(oracle, row):
    """No device involved: the oracle's scan of every spelled-out haplotype plus the rule.  Every needle has a cluster of at
    least two ends somewhere (LOCI has something to drop); some needle has loci on two haplotypes; at the small block
    length some cluster has ends on both sides of a block border.  A seed that fails is replaced, the conditions stay."""
    t = tree_of(row)
    O = oracle
    v = []
    for h, hp in enumerate(t["haps"]):
        r = O.scan_multi(O.MYERS if t["myers"] else O.SHIFTOR, hp, t["needles"], k=t["k"], sigma=t["sigma"], threads=4)
        a = np.zeros(len(r), dtype=JH)
        a["pos"], a["pattern"], a["score"], a["haplotype"] = r["pos"], r["pattern"], r["score"], h
        v.append(a)
    v = host_order(np.concatenate(v))
    n_needles = len(t["needles"])
    assert set(v["pattern"].tolist()) == set(range(n_needles))
    w = t["k"] if t["myers"] else 2
    loci = jrule(v, w)
    assert len(loci) < len(v) and set(loci["pattern"].tolist()) == set(range(n_needles))
    if not t["myers"]:
        return                                               # (the exact row: only the tandem needles cluster, by design)
    clustered, straddles = set(), 0
    checked = range(min(t["n_hap"], 5))                      # haplotypes whose block borders are worked out
    borders = {}
    for h in checked:
        at = [_hap_coord(t["alleles"], t["cov"], h, r) for r in range(0, len(t["ref"]), t["small_block"])]
        borders[h] = np.array([c for c in at if c is not None], dtype=np.int64)
    for h in range(t["n_hap"]):
        sub = v[v["haplotype"] == h]
        sub = sub[np.lexsort((sub["pos"], sub["pattern"]))]
        pos, pat = sub["pos"].astype(np.int64), sub["pattern"].astype(np.int64)
        cut = np.flatnonzero((np.diff(pat) != 0) | (np.diff(pos) > w)) + 1
        for a, b in zip(np.r_[0, cut], np.r_[cut, len(sub)]):
            if b - a >= 2:
                clustered.add(int(pat[a]))
                if h in checked:
                    lo, hi = int(pos[a]), int(pos[b - 1])        # ends are exclusive: symbol e - 1 is the last one
                    straddles += int(np.any((lo <= borders[h]) & (borders[h] < hi)))
    assert clustered == set(range(n_needles))
    assert straddles > 0
    if t["n_hap"] > 1:
        per_pattern = {}
        for h, p in zip(loci["haplotype"].tolist(), loci["pattern"].tolist()):
            per_pattern.setdefault(p, set()).add(h)
        assert any(len(s) >= 2 for s in per_pattern.values())
        # ... and the best place of some needle is better on one haplotype than on another: ACROSS differs from BEST
        assert len(jrule(v, w, best=0, across=True)) < len(jrule(v, w, best=0))


# ------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ------------------------------------------------------------------------------------------------------------------
def device_view(ctx, h):
    """the records behind JstHits.device(), downloaded in their device order"""
    import torch
    n = h.device()[1]
    buf = torch.zeros((max(n, 1), 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                 # (torch fills on its own stream, the library copies on the context's)
    assert h.copy_to(buf.data_ptr(), n) == n
    ctx.synchronize()
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:n].copy().view(JH).reshape(-1)


def upload_records(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 3).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def check(ctx, sel, want):
    """host view == the yardstick in host order, device view == the yardstick in (haplotype, pattern, pos) order, bytes"""
    got = sel.view()
    assert len(got) == len(want), (len(got), len(want))
    assert got.tobytes() == want.tobytes()
    dv = device_view(ctx, sel)
    assert dv.tobytes() == device_order(want).tobytes()
    assert np.array_equal(np.lexsort((dv["pos"], dv["pattern"], dv["haplotype"])), np.arange(len(dv)))   # the device order
    st = sel.select_stats()
    assert st.n_out == len(want) == len(sel) and st.n_in >= st.n_loci >= st.n_out
    return st


def _select_records(spm, ctx, a, kw, w, ps=None):
    buf = upload_records(a) if len(a) else None
    sel = spm.select_jst_records(ctx, buf.data_ptr() if buf is not None else 0, len(a), ps, loci=kw.get("loci", True), window=w,
                                 best=kw.get("best"), across=kw.get("across", False))
    return sel, buf


# ------------------------------------------------------------------------------------------------------------------
# GPU: the records route
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", JHAND, ids=[c[0] for c in JHAND])
def test_hand_worked_lists_through_select_jst_records(spm, ctx, case):
    _, given, kw, want = case
    kw = dict(kw)
    w = kw.pop("w")
    a = jrecs(given)
    a = a[np.random.default_rng(3).permutation(len(a))]      # arrival order is not sorted
    sel, _buf = _select_records(spm, ctx, a, kw, w)
    assert jrows(sel.view()) == want
    assert jrows(device_view(ctx, sel)) == sorted(want)      # (haplotype, pattern, pos)
    check(ctx, sel, jrecs(want))


@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_record_counts_around_one_tile(spm, ctx, n):
    rng = np.random.default_rng(n)
    given = [(3, 1, 2 * i + int(rng.integers(0, 2)), int(rng.integers(0, 4))) for i in range(n)]
    a = jrecs(given)
    a = a[rng.permutation(n)]
    for kw in (dict(), dict(best=0), dict(loci=False), dict(best=1, across=True)):
        sel, _buf = _select_records(spm, ctx, a, kw, 3)
        st = check(ctx, sel, jrule(host_order(a), 3, **kw))
        assert st.n_in == n


@gpu
def test_one_group_of_700_walks_beyond_the_halo_on_both_sides(spm, ctx):
    """700 consecutive positions of one (haplotype, pattern), scores falling to 0 at the middle and rising again, w = 200:
    three tiles; the walk to the left finds nothing better for 200 records, the one to the right reaches the minimum only
    for the last records -- both leave the 32 staged records behind."""
    given = [(1, 2, 1000 + i, abs(i - 350)) for i in range(700)]
    given += [(0, 0, 1000 + 3 * i, 5) for i in range(10)] + [(1, 3, 1000, 1), (2, 2, 1350, 7)]
    a = jrecs(given)
    a = a[np.random.default_rng(7).permutation(len(a))]
    sel, _buf = _select_records(spm, ctx, a, {}, 200)
    want = jrule(host_order(a), 200)
    assert jrows(want) == [(0, 0, 1000, 5), (1, 3, 1000, 1), (1, 2, 1350, 0), (2, 2, 1350, 7)]
    check(ctx, sel, want)
    # ... and with plateaus of equal scores, where only the leftmost record of a plateau can survive
    given = [(1, 2, 1000 + i, abs(i - 350) // 100) for i in range(700)] + [(1, 1, 5, 0)]
    a = jrecs(given)
    a = a[np.random.default_rng(8).permutation(len(a))]
    for w in (200, 33, 31):
        sel, _buf = _select_records(spm, ctx, a, dict(best=1), w)
        check(ctx, sel, jrule(host_order(a), w, best=1))


@gpu
@pytest.mark.parametrize("change", ["pattern", "haplotype"])
def test_group_change_exactly_at_sorted_index_256(spm, ctx, change):
    rng = np.random.default_rng(256)
    first = [(4, 6, 10 + i, int(rng.integers(0, 5))) for i in range(256)]
    second = [(4, 7, 260 + i, int(rng.integers(0, 5))) for i in range(120)] if change == "pattern" else \
             [(5, 6, 260 + i, int(rng.integers(0, 5))) for i in range(120)]
    a = jrecs(first + second)
    assert jrows(device_order(a))[256] == second[0]
    a = a[rng.permutation(len(a))]
    for kw in (dict(), dict(best=0), dict(best=0, across=True), dict(loci=False, best=1)):
        sel, _buf = _select_records(spm, ctx, a, kw, 5)
        check(ctx, sel, jrule(host_order(a), 5, **kw))


@gpu
def test_records_with_per_needle_windows_and_ranges_read_off_the_buffer(spm, ctx):
    """SPM_SELECT_WINDOW_K with a set; haplotype 65 534 and a position of 40 bits: the key is planned from what the range
    kernel finds"""
    ks = [1, 2, 0]
    ps = ctx.patterns(spm.ALGO_MYERS, [np.arange(40, dtype=np.uint8) % 4 for _ in ks], k=np.asarray(ks, dtype=np.uint16))
    big = 1 << 40
    given = [(0, 0, 10, 0), (0, 0, 12, 1), (0, 1, 10, 0), (0, 1, 12, 1), (0, 2, 10, 0), (0, 2, 11, 1),
             (65534, 1, big, 1), (65534, 1, big + 2, 0), (65534, 1, big + 5, 1)]
    a = jrecs(given)
    sel, _buf = _select_records(spm, ctx, a[::-1].copy(), {}, None, ps)
    want = jrule(a, np.asarray(ks, dtype=np.int64))
    assert jrows(want) == [(0, 0, 10, 0), (0, 1, 10, 0), (0, 2, 10, 0), (0, 2, 11, 1), (0, 0, 12, 1),
                           (65534, 1, big + 2, 0), (65534, 1, big + 5, 1)]
    st = check(ctx, sel, want)
    assert st.key_bits == 16 + 2 + 41
    bad = a.copy()
    bad["pattern"][0] = 3                                    # outside the set of three
    with pytest.raises(spm.SpmError, match="-1"):
        _select_records(spm, ctx, bad, {}, None, ps)


# ------------------------------------------------------------------------------------------------------------------
# GPU: trees
# ------------------------------------------------------------------------------------------------------------------
MODES = [dict(), dict(best=0), dict(best=1), dict(loci=False, best=0), dict(loci=False)]
ACROSS = [dict(best=0, across=True), dict(best=1, across=True), dict(loci=False, best=0, across=True)]


def _route_b(spm, ctx, t, ps, kw):
    """yardstick (b): every spelled-out haplotype uploaded, scanned, selected by the existing Hits.select()"""
    out = []
    for h, hp in enumerate(t["haps"]):
        text = ctx.upload(hp, sigma=t["sigma"])
        r = spm.scan(ctx, text, ps, engine=spm.ENGINE_BRUTE, max_hits=1 << 20)
        per_mode = []
        for m in kw:
            s = r.select(**m)
            v = s.view()
            a = np.zeros(len(v), dtype=JH)
            a["pos"], a["pattern"], a["score"], a["haplotype"] = v["pos"], v["pattern"], v["score"], h
            per_mode.append(a)
            s.close()
        out.append(per_mode)
        r.close()
        text.close()
    return [host_order(np.concatenate([out[h][i] for h in range(len(out))])) for i in range(len(kw))]


@gpu
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_tree_rows_equal_both_yardsticks(spm, ctx, row):
    t = tree_of(row)
    myers, L, k = t["myers"], t["L"], t["k"]
    n_needles = len(t["needles"])
    ref_text = ctx.upload(t["ref"], sigma=t["sigma"])
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS if myers else spm.ALGO_SHIFTOR, t["needles"], k=k, sigma=t["sigma"])
    window = max(ps.window_size(p) for p in range(n_needles))
    modes = list(MODES) + ([] if myers else [dict(window=2), dict(window=2, best=0)])
    w_of = lambda m: m.get("window", k if myers else 0)

    want_a, src0 = None, None
    for blk, engine in ((0, spm.ENGINE_AUTO), (0, spm.ENGINE_BRUTE), (t["small_block"], spm.ENGINE_AUTO),
                        (t["small_block"], spm.ENGINE_BRUTE)):
        jst.index(window, blk)
        h = jst.search_device(ps, engine=engine, max_hits=1 << 20)
        src = h.view()
        if want_a is None:                                   # the yardsticks, once per row
            src0 = src
            want_a = [jrule(src, w_of(m), best=m.get("best"), loci=m.get("loci", True)) for m in modes]
            want_b = _route_b(spm, ctx, t, ps, modes)
            for m, a, b in zip(modes, want_a, want_b):
                assert a.tobytes() == b.tobytes(), m
                assert set(a["pattern"].tolist()) == set(range(n_needles)), m    # every planted needle keeps a record
            reducing = want_a[0] if myers else want_a[len(MODES)]
            assert len(reducing) < len(src)                   # n_out < n_in: the row shows something
            want_x = [jrule(src, w_of(m), best=m["best"], loci=m.get("loci", True), across=True) for m in ACROSS]
            assert 0 < len(want_x[0]) < len(want_a[1]) or not myers or t["n_hap"] == 1
            assert set(want_x[0]["pattern"].tolist()) == set(range(n_needles))
        else:
            assert src.tobytes() == src0.tobytes()
        for m, want in list(zip(modes, want_a)) + list(zip(ACROSS, want_x)):
            sel = h.select(**m)
            st = check(ctx, sel, want)
            assert st.n_in == len(src)
            if not m.get("loci", True):
                assert st.n_loci == st.n_in
            sel.close()
        if not myers:                                        # SPM_SELECT_WINDOW_K is 0 for exact sets: everything stays
            assert len(want_a[0]) == len(src) and len(want_a[len(MODES)]) < len(src)
        h.close()
    jst.close()
    ps.close()
    ref_text.close()


@gpu
def test_two_block_shards_selected_on_one_buffer(spm, ctx):
    """The sharded shape on one device: two block shards searched one after the other, their records copied into one
    buffer, spm_hip_jst_records_select on it == select() of the unsharded search."""
    import torch
    t = tree_of(ROWS[1])
    ref_text = ctx.upload(t["ref"])
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS, t["needles"], k=t["k"])
    window = t["L"] + t["k"]
    n_blocks = jst.index(window, 64).n_blocks
    whole = jst.search_device(ps, max_hits=1 << 20)
    src = whole.view()
    cut = n_blocks // 2 + 1
    buf = torch.zeros((len(src), 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    at = 0
    for b0, b1 in ((0, cut), (cut, n_blocks)):
        assert jst.index(window, 64, b0, b1).n_blocks == b1 - b0
        part = jst.search_device(ps, max_hits=1 << 20)
        assert 0 < len(part) < len(src)
        at += part.copy_to(buf.data_ptr() + 24 * at, len(src) - at)
        ctx.synchronize()
        part.close()
    assert at == len(src)
    for m in (dict(), dict(best=0), dict(best=0, across=True)):
        both = spm.select_jst_records(ctx, buf.data_ptr(), at, ps, **m)
        one = whole.select(**m)
        want = jrule(src, t["k"], **m)
        assert len(want) < len(src)
        check(ctx, both, want)
        check(ctx, one, want)
        assert device_view(ctx, both).tobytes() == device_view(ctx, one).tobytes()
    jst.close()


# ------------------------------------------------------------------------------------------------------------------
# GPU: object rules
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_object_rules_and_refusals(spm, ctx):
    import torch
    t = tree_of(ROWS[1])
    k = t["k"]
    ref_text = ctx.upload(t["ref"])
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS, t["needles"], k=k)
    jst.index(t["L"] + k, 256)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
    src = h.view()
    want = jrule(src, k)
    with pytest.raises(spm.SpmError, match="-1"):            # select_stats on a search's own result
        h.select_stats()
    assert len(h.align()) == len(src)                        # the source is alignable ...
    once = h.select()
    with pytest.raises(spm.SpmError, match=r"error -1: .*selection"):   # ... its selection is not, and says so
        once.align()
    # a selection of a selection: idempotent, whatever the flags add
    check(ctx, once, want)
    twice = once.select()
    check(ctx, twice, want)
    check(ctx, once.select(best=0), jrule(src, k, best=0))
    check(ctx, once.select(best=0, across=True), jrule(src, k, best=0, across=True))
    assert twice.select_stats().n_in == len(want)
    # the source destroyed before the result is read; a later search reuses what it gave back
    s2 = h.select(best=1)
    h.close()
    h3 = jst.search_device(ps, max_hits=1 << 20)
    check(ctx, s2, jrule(src, k, best=1))
    check(ctx, once, want)
    # the documented codes
    L = spm.capi.lib()
    out = ctypes.c_void_p()
    O = spm.capi.SelectOpts
    assert L.spm_hip_jst_hits_select(h3._h, None, ctypes.byref(out)) == -1
    assert L.spm_hip_jst_hits_select(None, ctypes.byref(O()), ctypes.byref(out)) == -1
    for bad in (O(flags=4, window=1, strata=0, reserved=0),                       # ACROSS without BEST
                O(flags=5, window=1, strata=0, reserved=0),
                O(flags=8, window=1, strata=0, reserved=0),                       # unknown flag bits
                O(flags=0xDEADBEEF, window=0xABCD, strata=7, reserved=0),
                O(flags=1, window=1, strata=0, reserved=1)):
        assert L.spm_hip_jst_hits_select(h3._h, ctypes.byref(bad), ctypes.byref(out)) == -1
    with pytest.raises(spm.SpmError, match="-1"):
        h3.select(across=True)
    buf = upload_records(np.concatenate([src[:100], src[:1]]))
    with pytest.raises(spm.SpmError, match="-1"):            # the window of the needles needs the needles
        spm.select_jst_records(ctx, buf.data_ptr(), 100, None)
    with pytest.raises(spm.SpmError, match="-1"):            # records that are not 8-byte aligned
        spm.select_jst_records(ctx, buf.data_ptr() + 4, 100, ps)
    ok = spm.select_jst_records(ctx, buf.data_ptr() + 8, 0, None, window=3)      # no records: an empty result
    assert len(ok) == 0 and len(ok.view()) == 0 and ok.select_stats().n_in == 0 and len(ok.select(window=3, best=0)) == 0
    # plain selection still refuses flag bit 4
    T = np.random.default_rng(1).integers(0, 4, 1 << 14, dtype=np.uint8)
    plain = spm.scan(ctx, ctx.upload(T), ctx.patterns(spm.ALGO_MYERS, [T[100:164].copy()], k=2))
    assert len(plain.view()) > 0
    for flags in (4, 6, 7):
        bad = O(flags=flags, window=1, strata=0, reserved=0)
        assert L.spm_hip_hits_select(plain._h, ctypes.byref(bad), ctypes.byref(out)) == -1
        assert L.spm_hip_records_select(ctx._h, plain.device()[0], plain.device()[1], None, ctypes.byref(bad), ctypes.byref(out)) == -1
    # ACROSS keeps one minimum per pattern index: a raw buffer without a set that names a huge index is refused, not tried
    far = src[:4].copy()
    far["pattern"][3] = 1 << 30
    fbuf = upload_records(far)
    with pytest.raises(spm.SpmError, match="-4"):
        spm.select_jst_records(ctx, fbuf.data_ptr(), 4, None, window=3, best=0, across=True)
    check(ctx, spm.select_jst_records(ctx, fbuf.data_ptr(), 4, None, window=3, best=0), jrule(host_order(far), 3, best=0))
    # gatherv and copies take the result unchanged: copy_to is what device_view uses; a short buffer takes the first records
    small = torch.zeros((5, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert once.copy_to(small.data_ptr(), 5) == len(want)
    ctx.synchronize()
    assert small.cpu().numpy().copy().view(JH).reshape(-1).tobytes() == device_order(want)[:5].tobytes()
    # with an explicit window the needle set is not read: it may be gone when a result is selected (raw call; Python's
    # select() refuses a closed set whatever the window)
    ps.close()
    ow = O(flags=3, window=k, strata=0, reserved=0)
    assert L.spm_hip_jst_hits_select(once._h, ctypes.byref(ow), ctypes.byref(out)) == 0
    late = spm.JstHits(ctx, ctypes.c_void_p(out.value))
    check(ctx, late, jrule(src, k, best=0))
    h3.close()
    jst.close()


# ------------------------------------------------------------------------------------------------------------------
# GPU: one scale row
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_scale_c5_shape_over_a_million_records(spm, ctx):
    """The C5 shape of test_gpu_jst (|P| = 1024, k = 64, 64 haplotypes over 400 000 bases) with 160 needles of at most 8
    substitutions: every occurrence comes back as a cluster of more than a hundred ends on every haplotype, over 10^6 records
    -- the sort and the scans take their multi-block paths, and with the needles' own window of 64 every walk leaves the
    halo.  Yardstick (a) only."""
    n_ref, n_hap, L, k, n_needles = 400_000, 64, 1024, 64, 160
    rng = np.random.default_rng(5)
    ref_text = ctx.generate(0x5EED0001, 0, n_ref)
    ref = ref_text.download(0, n_ref)
    alleles, pool, cov = spm.synth_variants(0x5EED0001, 0x5EED0003, 0, n_ref, n_hap)
    cov2 = cov.reshape(-1, 1)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov2, n_hap)
    needles = []
    for _ in range(n_needles):
        hp = _apply(ref, alleles, pool, cov2, int(rng.integers(0, n_hap)))
        o = int(rng.integers(0, len(hp) - L))
        nd = hp[o:o + L].copy()
        at = rng.choice(L, size=int(rng.integers(0, 9)), replace=False)
        nd[at] = (nd[at] + 1 + rng.integers(0, 3, len(at))) & 3
        needles.append(nd.astype(np.uint8))
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    jst.index(L + k, 1024)
    h = jst.search_device(ps, max_hits=1 << 21)
    src = h.view()
    print("scale source:", len(src), "records")
    assert len(src) >= 1_000_000
    sel = h.select()
    st = check(ctx, sel, jrule(src, k))
    print("n_in", st.n_in, "n_loci", st.n_loci, "n_out", st.n_out, "key bits", st.key_bits, "ms order/select", st.ms_order,
          st.ms_select, "host", st.ms_host)
    assert st.n_in == len(src) and st.n_in >= st.n_loci >= st.n_out == len(sel) and st.n_out < st.n_in // 50
    assert st.n_out >= n_needles and set(sel.view()["pattern"].tolist()) == set(range(n_needles))
    best = h.select(best=0, across=True)
    sb = best.select_stats()
    assert sb.n_in == len(src) and sb.n_loci == st.n_loci and n_needles <= sb.n_out <= st.n_out
    jst.close()
