"""Selection of hits on the device (spm_hip_hits_select / spm_hip_records_select; contract in include/spm_hip.h, scheme in
DESIGN.md 4.7): one record per locus, the best error stratum per needle, sorted.

The yardstick is `rule` below: the literal definition of the contract, vectorised as shifted comparisons over the
(pattern, pos)-sorted records.  CPU tests pin the rule itself on hand-worked lists whose answers are written out here;
GPU tests compare -- byte for byte -- the derived result's host view, its device view (downloaded) and the rule applied to
the source's view()."""
import ctypes
import itertools

import numpy as np
import pytest

HIT = np.dtype([("pos", "<u8"), ("pattern", "<u4"), ("score", "<i4")])
SEED_TEXT, SEED_PAT = 0x5EED0001, 0x5EED0002


def recs(rows):
    """rows of (pattern, pos, score) -> HIT records sorted by (pattern, pos)"""
    a = np.zeros(len(rows), dtype=HIT)
    for i, (p, pos, s) in enumerate(sorted(rows)):
        a[i] = (pos, p, s)
    return a


def rows(a):
    return [(int(p), int(pos), int(s)) for pos, p, s in zip(a["pos"].astype(np.int64), a["pattern"], a["score"])]


def segment_of(pos, segs, myers):
    """Myers: seg_off[s] < p <= seg_off[s+1] (p is an end); exact sets: seg_off[s] <= p < seg_off[s+1]."""
    segs = np.asarray(segs, dtype=np.int64)
    sym = np.where(pos > 0, pos - 1, pos) if myers else pos
    return np.clip(np.searchsorted(segs, sym, side="right") - 1, 0, len(segs) - 2)


def rule(h, w, best=None, loci=True, segs=None, myers=True, pos_offset=0):
    """The contract, literally.  h: HIT records sorted by (pattern, pos), (pattern, pos) unique.  w: one window, or one per
    pattern.  LOCI: r is dropped iff a record r' of the same pattern (and segment) has |pos' - pos| <= w and
    (score', pos') < (score, pos).  BEST (after LOCI): kept iff score <= min over the pattern's INPUT records + best."""
    n = len(h)
    pos = h["pos"].astype(np.int64)
    pat = h["pattern"].astype(np.int64)
    sc = h["score"].astype(np.int64)
    assert np.all((np.diff(pat) > 0) | ((np.diff(pat) == 0) & (np.diff(pos) > 0))), "sorted, unique (pattern, pos)"
    keep = np.ones(n, dtype=bool)
    if loci and n:
        wi = np.full(n, w, dtype=np.int64) if np.isscalar(w) else np.asarray(w, dtype=np.int64)[pat]
        seg = segment_of(pos - pos_offset, segs, myers) if segs is not None else np.zeros(n, dtype=np.int64)
        # (pattern, pos) is unique, so a record within w positions is within w places in sorted order
        for d in range(1, n):
            near = (pat[d:] == pat[:-d]) & (pos[d:] - pos[:-d] <= np.maximum(wi[d:], wi[:-d]))
            if not near.any():
                break
            same = (pat[d:] == pat[:-d]) & (seg[d:] == seg[:-d])
            dist = pos[d:] - pos[:-d]
            # r = the right record, r' = the left one: pos' < pos, so r' is better iff score' <= score
            keep[d:] &= ~(same & (dist <= wi[d:]) & (sc[:-d] <= sc[d:]))
            # r = the left record, r' = the right one: better iff score' < score
            keep[:-d] &= ~(same & (dist <= wi[:-d]) & (sc[d:] < sc[:-d]))
    if best is not None and n:
        mn = np.full(int(pat.max()) + 1, np.iinfo(np.int64).max)
        np.minimum.at(mn, pat, sc)
        keep &= sc <= mn[pat] + best
    return h[keep]


# ------------------------------------------------------------------------------------------------------------------
# CPU: the rule on hand-worked lists, the struct layouts
# ------------------------------------------------------------------------------------------------------------------
HAND = [
    # name, records (pattern, pos, score), kwargs of the rule, the kept records -- worked by hand
    ("descending plateau 3,2,2,1 inside one window", [(0, 10, 3), (0, 11, 2), (0, 12, 2), (0, 13, 1)], dict(w=3), [(0, 13, 1)]),
    # w = 1: 10 loses to 11; 11 has no better neighbour (12 ties but lies right); 12 loses to 11 (tie, left) and to 13
    ("descending plateau, w = 1: the leftmost of the tie survives", [(0, 10, 3), (0, 11, 2), (0, 12, 2), (0, 13, 1)], dict(w=1),
     [(0, 11, 2), (0, 13, 1)]),
    ("ascending plateau 1,2,2,3", [(0, 10, 1), (0, 11, 2), (0, 12, 2), (0, 13, 3)], dict(w=3), [(0, 10, 1)]),
    # w = 1: 12 is dropped by 11, which is itself dropped by 10 -- strict suppression
    ("ascending plateau, w = 1: dominated by a dominated record", [(0, 10, 1), (0, 11, 2), (0, 12, 2), (0, 13, 3)], dict(w=1),
     [(0, 10, 1)]),
    ("a chain of dominations", [(0, 0, 0), (0, 2, 1), (0, 4, 2), (0, 6, 3), (0, 8, 4)], dict(w=2), [(0, 0, 0)]),
    ("exactly w apart", [(0, 100, 1), (0, 103, 2)], dict(w=3), [(0, 100, 1)]),
    ("w + 1 apart", [(0, 100, 1), (0, 104, 2)], dict(w=3), [(0, 100, 1), (0, 104, 2)]),
    ("w = 0 keeps everything", [(0, 10, 3), (0, 11, 2), (0, 12, 2), (0, 13, 1)], dict(w=0),
     [(0, 10, 3), (0, 11, 2), (0, 12, 2), (0, 13, 1)]),
    ("two needles at adjacent positions", [(0, 50, 1), (1, 51, 0)], dict(w=3), [(0, 50, 1), (1, 51, 0)]),
    ("per-needle windows", [(0, 10, 0), (0, 12, 1), (1, 10, 0), (1, 12, 1)], dict(w=[1, 2]), [(0, 10, 0), (0, 12, 1), (1, 10, 0)]),
    # Myers: end 100 closes segment [0, 100), end 101 is the first end of segment [100, 200)
    ("a segment boundary between two records <= w apart (Myers)", [(0, 99, 1), (0, 100, 2), (0, 101, 0)],
     dict(w=3, segs=[0, 100, 200], myers=True), [(0, 99, 1), (0, 101, 0)]),
    ("the same records without segments", [(0, 99, 1), (0, 100, 2), (0, 101, 0)], dict(w=3), [(0, 101, 0)]),
    # exact sets: begin 100 is the first symbol of segment [100, 200)
    ("a segment boundary, exact set", [(0, 99, 0), (0, 100, 0), (0, 101, 0)], dict(w=3, segs=[0, 100, 200], myers=False),
     [(0, 99, 0), (0, 100, 0)]),
    # AAAA in A x 10: begins 0..6, all score 0
    ("overlapping exact occurrences in poly-A, window k = 0", [(0, b, 0) for b in range(7)], dict(w=0), [(0, b, 0) for b in range(7)]),
    # ... an explicit window collapses the plateau: 1, 2 lose to 0; 3 loses to 1 although 1 is dropped; and so on
    ("overlapping exact occurrences in poly-A, w = 2", [(0, b, 0) for b in range(7)], dict(w=2), [(0, 0, 0)]),
    ("BEST strata 0 after LOCI", [(0, 10, 1), (0, 11, 2), (0, 50, 2), (0, 90, 3), (1, 20, 0), (1, 60, 0), (1, 100, 2)],
     dict(w=3, best=0), [(0, 10, 1), (1, 20, 0), (1, 60, 0)]),
    ("BEST strata 1 after LOCI", [(0, 10, 1), (0, 11, 2), (0, 50, 2), (0, 90, 3), (1, 20, 0), (1, 60, 0), (1, 100, 2)],
     dict(w=3, best=1), [(0, 10, 1), (0, 50, 2), (1, 20, 0), (1, 60, 0)]),
    ("BEST alone: the minimum is taken over the input", [(0, 10, 1), (0, 11, 2), (0, 50, 2)], dict(w=3, best=0, loci=False), [(0, 10, 1)]),
    ("neither flag: a sorted copy", [(1, 5, 1), (0, 11, 2), (0, 10, 2)], dict(w=3, loci=False), [(0, 10, 2), (0, 11, 2), (1, 5, 1)]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_rule_on_hand_worked_lists(case):
    _, given, kw, want = case
    kw = dict(kw)
    assert rows(rule(recs(given), kw.pop("w"), **kw)) == want


def test_rule_properties_on_random_lists():
    """Kept records of one pattern are more than w apart; LOCI never removes a pattern's minimum."""
    rng = np.random.default_rng(11)
    for w in (1, 2, 5):
        given = sorted({(int(p), int(x)) for p, x in zip(rng.integers(0, 4, 400), rng.integers(0, 300, 400))})
        h = recs([(p, x, int(rng.integers(0, 4))) for p, x in given])
        out = rule(h, w)
        for p in range(4):
            x = out["pos"][out["pattern"] == p].astype(np.int64)
            assert np.all(np.diff(x) > w)
            assert out["score"][out["pattern"] == p].min() == h["score"][h["pattern"] == p].min()
        assert np.array_equal(rule(h, w, best=0), rule(out, w, best=0, loci=False))


def test_select_struct_layouts(spm):
    assert ctypes.sizeof(spm.capi.SelectOpts) == 16
    assert ctypes.sizeof(spm.capi.SelectStats) == 48
    assert spm.capi.SelectStats.n_in.offset == 16 and spm.capi.SelectStats.key_bits.offset == 40
    assert spm.capi.SELECT_WINDOW_K == 0xFFFFFFFF and (spm.capi.SELECT_LOCI, spm.capi.SELECT_BEST) == (1, 2)
    for name in ("spm_hip_hits_select", "spm_hip_records_select", "spm_hip_hits_select_stats"):
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    assert callable(spm.Hits.select) and callable(spm.Hits.select_stats) and callable(spm.select_records)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def device_view(ctx, h):
    """the records behind Hits.device(), downloaded in their device order"""
    import torch
    n = h.device()[1]
    buf = torch.zeros((max(n, 1), 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                             # (torch fills on its own stream, the library copies on the context's)
    assert h.copy_to(buf.data_ptr(), n) == n
    ctx.synchronize()
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:n].copy().view(HIT).reshape(-1)


def upload_records(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 2).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def check(ctx, sel, want):
    """host view == device view == the rule, byte for byte"""
    got = sel.view()
    assert len(got) == len(want), (len(got), len(want))
    assert got.tobytes() == want.tobytes()
    assert device_view(ctx, sel).tobytes() == want.tobytes()
    st = sel.select_stats()
    assert st.n_out == len(want) and sel.stats().n_hits == len(want)
    return st


def ks_of(ps_k, n):
    return np.full(n, ps_k, dtype=np.int64) if np.isscalar(ps_k) else np.asarray(ps_k, dtype=np.int64)


UNSEGMENTED = [c for c in HAND if "segs" not in c[2]]     # (raw records have no segment table: real scans below)


@gpu
@pytest.mark.parametrize("case", UNSEGMENTED, ids=[c[0] for c in UNSEGMENTED])
def test_hand_worked_lists_through_select_records(spm, ctx, case):
    _, given, kw, want = case
    kw = dict(kw)
    w = kw.pop("w")
    rng = np.random.default_rng(3)
    a = recs(given)
    a = a[rng.permutation(len(a))]                       # arrival order is not sorted
    buf = upload_records(a)
    if np.isscalar(w):
        sel = spm.select_records(ctx, buf.data_ptr(), len(a), None, loci=kw.get("loci", True), window=w, best=kw.get("best"))
    else:                                                # per-needle windows: a Myers set with those k
        needles = [np.arange(40, dtype=np.uint8) % 4 for _ in w]
        ps = ctx.patterns(spm.ALGO_MYERS, needles, k=np.asarray(w, dtype=np.uint16))
        sel = spm.select_records(ctx, buf.data_ptr(), len(a), ps, loci=True, window=None, best=kw.get("best"))
    assert rows(sel.view()) == want
    assert rows(device_view(ctx, sel)) == want
    with pytest.raises(spm.SpmError, match="-1"):        # no alignment context: SPM_E_INVALID
        sel.align()


def _select_records(spm, ctx, a, w, **kw):
    """a: records in arrival order -> (the selection, the device buffer it reads, to be kept alive by the caller)"""
    buf = upload_records(a) if len(a) else None
    sel = spm.select_records(ctx, buf.data_ptr() if buf is not None else 0, len(a), None, loci=kw.get("loci", True), window=w,
                             best=kw.get("best"))
    return sel, buf


@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_record_counts_around_one_tile(spm, ctx, n):
    """one pattern, n records: an empty list, one lane, one lane short of a tile, a full tile, one record in a second tile"""
    rng = np.random.default_rng(n)
    a = recs([(1, 2 * i + int(rng.integers(0, 2)), int(rng.integers(0, 4))) for i in range(n)])
    srt = a.copy()
    a = a[rng.permutation(n)]
    for kw in (dict(best=0), dict(), dict(best=1, loci=False)):
        sel, _buf = _select_records(spm, ctx, a, 3, **kw)
        st = check(ctx, sel, rule(srt, 3, **kw))
        assert st.n_in == n


@gpu
def test_one_pattern_of_700_walks_beyond_the_halo_on_both_sides(spm, ctx):
    """700 consecutive positions of one pattern, scores falling to 0 at the middle and rising again: three tiles.  With
    w = 200 and w = 33 the walks of the middle record find nothing better for w records on either side and leave the 32
    staged records behind, across the tile borders at 256 and 512 for w = 200.  The two data sets after it make a walk FIND
    its suppressor out there: to the left (isolated low records) and to the right (plateaus)."""
    given = [(1, 1000 + i, abs(i - 350)) for i in range(700)] + [(0, 1000 + 3 * i, 5) for i in range(10)] + [(2, 1350, 7)]
    srt = recs(given)
    a = srt[np.random.default_rng(7).permutation(len(srt))]
    for w in (200, 33):
        sel, _buf = _select_records(spm, ctx, a, w)
        want = rule(srt, w)
        assert rows(want)[-2:] == [(1, 1350, 0), (2, 1350, 7)]
        assert [r for r in rows(want) if r[0] == 1] == [(1, 1350, 0)]       # the descent on either side suppresses the rest
        check(ctx, sel, want)
    # ... the mirror image: a record whose suppressor lies to its LEFT, behind more than 32 worse records, in the tile
    # before its own and outside that tile's halo (tile 1 stages sorted indices 224.., tile 2 480..): low records at 200 and
    # 470, the contenders 60 places after them at 260 and 530, one more at 300 that loses to 260 inside the tile
    score = {200: 0, 260: 3, 300: 5, 470: 1, 530: 4}
    srt = recs([(1, 1000 + i, score.get(i, 9)) for i in range(700)])
    a = srt[np.random.default_rng(9).permutation(len(srt))]
    kept_at = {200: [200, 470], 60: [0, 200, 470], 59: [0, 200, 260, 470, 530], 33: [0, 200, 260, 300, 470, 530]}
    for w, at in kept_at.items():
        want = rule(srt, w)
        assert rows(want) == [(1, 1000 + i, score.get(i, 9)) for i in at], w   # (record 0 loses only at w = 200, to record 200)
        sel, _buf = _select_records(spm, ctx, a, w)
        check(ctx, sel, want)
    # ... and with plateaus of equal scores, where only the leftmost record of a plateau can survive
    srt = recs([(1, 1000 + i, abs(i - 350) // 100) for i in range(700)] + [(0, 5, 0)])
    a = srt[np.random.default_rng(8).permutation(len(srt))]
    for w in (200, 33):
        for kw in (dict(), dict(best=1)):
            sel, _buf = _select_records(spm, ctx, a, w, **kw)
            check(ctx, sel, rule(srt, w, **kw))


@gpu
def test_pattern_change_exactly_at_sorted_index_256(spm, ctx):
    """two patterns whose boundary is the tile border, records within w of each other across it: no record is suppressed by
    the other pattern's records, and each pattern's BEST minimum is its own"""
    rng = np.random.default_rng(256)
    first = [(6, 10 + i, int(rng.integers(1, 5))) for i in range(256)]
    second = [(7, 260 + i, int(rng.integers(0, 5))) for i in range(120)]
    second[40] = (7, 300, 0)
    srt = recs(first + second)
    assert rows(srt)[256] == second[0] and rows(srt)[255] == first[-1]
    assert abs(second[0][1] - first[-1][1]) <= 5 and min(s for _, _, s in first) != min(s for _, _, s in second)
    a = srt[rng.permutation(len(srt))]
    for kw in (dict(), dict(best=0), dict(best=1, loci=False)):
        sel, _buf = _select_records(spm, ctx, a, 5, **kw)
        want = rule(srt, 5, **kw)
        check(ctx, sel, want)
    # the head of the second pattern would lose to the last record of the first, 5 positions on, if the two saw each other
    first[-1] = (6, 265, 0)                                                 # the best of its window in pattern 6
    second[:6] = [(7, 260, 3)] + [(7, 261 + i, 4) for i in range(5)]        # ... and the head the best of its own
    srt = recs(first + second)
    assert rows(srt)[255] == first[-1] and rows(srt)[256] == second[0]
    sel, _buf = _select_records(spm, ctx, srt[rng.permutation(len(srt))], 5)
    want = rule(srt, 5)
    assert first[-1] in rows(want) and second[0] in rows(want)
    check(ctx, sel, want)


def plant(rng, n_text, specs, gap=None):
    """Uniform text with every needle of `specs` (length, k) planted three times with <= k random edits, the copies at
    least 4 (|P| + k) apart.  Returns text, needles, ks, planted [(needle, end of the planted copy)]."""
    T = rng.integers(0, 4, n_text, dtype=np.uint8)
    needles = [rng.integers(0, 4, L, dtype=np.uint8) for L, _ in specs]
    ks = np.array([k for _, k in specs], dtype=np.uint16)
    slot = n_text // (3 * len(specs))
    longest = max(L + k for L, k in specs)
    assert slot >= 6 * longest
    order = rng.permutation(3 * len(specs))
    planted = []
    for s, j in enumerate(order):
        p = int(j) // 3
        L, k = specs[p]
        copy = list(needles[p])
        for _ in range(int(rng.integers(0, k + 1))):
            at = int(rng.integers(0, len(copy)))
            op = int(rng.integers(0, 3))
            if op == 0:
                copy[at] = (copy[at] + 1 + int(rng.integers(0, 3))) % 4
            elif op == 1:
                copy.insert(at, int(rng.integers(0, 4)))
            elif len(copy) > 1:
                del copy[at]
        site = s * slot + int(rng.integers(0, slot - 5 * longest))   # >= 5 longest - |copy| >= 4 (|P| + k) between copies
        T[site:site + len(copy)] = copy
        planted.append((p, site + len(copy)))
    return T, needles, ks, planted


# Kept because the reference alone (test_planted_seed_holds_for_the_reference_alone) gives exactly one locus per planted
# copy for it.  20240607 did not: two copies out of 1 536 came with two loci (ends two apart around a non-hit, k = 1), which
# the rule at w = k rightly keeps apart; such a seed is replaced, not excused.
PLANT_SEED = 20240608


def planted_specs(rng):
    """512 needles, |P| in 40...150, per-needle k in 0...6 -- as far as the needle keeps k + 1 seeds of 9 symbols, so that
    the set runs on the seed-filter engine too (|P| >= 63 admits every k)"""
    out = []
    for _ in range(512):
        L = int(rng.integers(40, 151))
        out.append((L, int(rng.integers(0, min(6, L // 9 - 1) + 1))))
    return out


def one_locus_per_planted(loci, ks, planted):
    """every planted occurrence has exactly one locus within 2k of its planted end"""
    by_pat = {}
    for p, pos in zip(loci["pattern"], loci["pos"].astype(np.int64)):
        by_pat.setdefault(int(p), []).append(int(pos))
    bad = []
    for p, end in planted:
        k = int(ks[p])
        if sum(abs(x - end) <= 2 * k for x in by_pat.get(p, [])) != 1:
            bad.append((p, end, k, by_pat.get(p)))
    return bad


def test_planted_seed_holds_for_the_reference_alone(oracle):
    """The seed of the planted-ground-truth test: the oracle's Sellers DP plus the rule, no device involved, already gives
    exactly one locus within 2k of every planted end."""
    rng = np.random.default_rng(PLANT_SEED)
    specs = planted_specs(rng)
    T, needles, ks, planted = plant(rng, 1 << 22, specs)
    out = []
    for p, end in planted:
        L, k = specs[p]
        lo, hi = max(0, end - 3 * (L + k)), min(len(T), end + 2 * (L + k))
        r = oracle.sellers(T[lo:hi], needles[p], k)
        near = np.abs(r["pos"].astype(np.int64) + lo - end) <= 4 * k + 1   # (what the rule needs around the planted end)
        out += [(p, int(x) + lo, int(s)) for x, s in zip(r["pos"][near], r["score"][near])]
    h = recs(sorted(set(out)))
    assert not one_locus_per_planted(rule(h, ks.astype(np.int64)), ks, planted)


@gpu
def test_planted_ground_truth_both_engines(spm, ctx):
    rng = np.random.default_rng(PLANT_SEED)
    specs = planted_specs(rng)
    T, needles, ks, planted = plant(rng, 1 << 22, specs)
    text = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=ks)
    outs = []
    for engine in (spm.ENGINE_FILTER, spm.ENGINE_BRUTE):
        h = spm.scan(ctx, text, ps, engine=engine, max_hits=1 << 22)
        assert h.stats().engine_used == engine
        src = h.view()
        sel = h.select()
        want = rule(src, ks.astype(np.int64))
        st = check(ctx, sel, want)
        assert st.n_in == len(src) and st.n_loci == len(want) and st.n_loci < st.n_in
        bad = one_locus_per_planted(sel.view(), ks, planted)
        assert not bad, bad[:5]
        best = h.select(best=0)
        check(ctx, best, rule(src, ks.astype(np.int64), best=0))
        outs.append(sel.view().tobytes())
    assert outs[0] == outs[1]                              # filter engine and brute engine: identical bytes after selection


def _c3r(spm, ctx, n, ppm, n_pat, L=100, k=3):
    text = ctx.generate_repeats(SEED_TEXT, 0, n, ppm)
    needles = [spm.synth_repeat_pattern(SEED_TEXT, SEED_PAT, n, p, L, k, ppm)[0] for p in range(n_pat)]
    return text, needles


def tandem_needles(L):
    """Every primitive unit of 1...4 bases in every rotation (4 + 12 + 60 + 240 needles), tiled to L bases: the needles
    that a tandem repeat of that unit matches at every end position -- the unit-1 ones are the homopolymers."""
    out = []
    for u in range(1, 5):
        for unit in itertools.product(range(4), repeat=u):
            if any(u % d == 0 and unit == unit[:d] * (u // d) for d in range(1, u)):
                continue                                 # a repetition of a shorter unit: that needle is there already
            out.append(np.tile(np.array(unit, dtype=np.uint8), -(-L // u))[:L])
    return out


@gpu
def test_repeat_rich_text(spm, ctx):
    """c3r-shaped, 64 MiB at 5 %: millions of hits, long plateaus, homopolymer needles.

    The c3r needles alone are cut from single places of the text and bring a few thousand hits.  The millions come from
    the text's 12 000 tandem stretches (units of 1...6 bases, 16...256 long) and as many low-complexity ones: a needle
    tiled from a stretch's unit ends a match at every position of it once the stretch is longer than the needle, in
    every rotation of the unit (scores 0, 1, 2, 1 along the plateau for a unit of 4), and a homopolymer needle of 40
    finds ragged runs of ends in the 7/8-pure stretches.  The oracle's scan of the same text with the 316 short needles
    gives 2.7 million records."""
    n, k = 1 << 26, 3
    text, needles = _c3r(spm, ctx, n, 50000, 256)
    needles += [np.full(100, b, dtype=np.uint8) for b in range(4)]            # homopolymers
    needles += [np.tile(np.array([0, 1], dtype=np.uint8), 50), np.tile(np.array([2, 3, 1], dtype=np.uint8), 34)[:100]]
    needles += tandem_needles(40)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    h = spm.scan(ctx, text, ps, max_hits=1 << 26)
    src = h.view()
    print("repeat-rich source:", len(src), "hits")
    assert len(src) > 2_000_000
    for kw in (dict(), dict(best=0), dict(window=1), dict(window=40, best=1), dict(loci=False)):
        sel = h.select(**kw)
        w = kw.get("window", None)
        want = rule(src, k if w is None else w, best=kw.get("best"), loci=kw.get("loci", True))
        st = check(ctx, sel, want)
        print(kw, "n_in", st.n_in, "n_loci", st.n_loci, "n_out", st.n_out, "ms order/select", st.ms_order, st.ms_select)
        if kw.get("loci", True):
            ww = k if w is None else w
            got = sel.view()
            same = got["pattern"][1:] == got["pattern"][:-1]
            assert np.all(np.diff(got["pos"].astype(np.int64))[same] > ww)   # kept records of one needle: more than w apart
        sel.close()


@gpu
def test_long_needles_windows_cross_tiles_and_halos(spm, ctx):
    """The C5 needle shape: |P| = 1024, k = 64 in 16 MiB -- windows of 64 reach beyond the staged halo."""
    n, L, k = 1 << 24, 1024, 64
    text = ctx.generate(SEED_TEXT, 0, n)
    needles = [spm.synth_pattern(SEED_TEXT, SEED_PAT, n, p, L, k)[0] for p in range(256)]
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    h = spm.scan(ctx, text, ps, max_hits=1 << 22)
    src = h.view()
    assert len(src) > 256 * 20
    for kw in (dict(), dict(best=2), dict(window=31), dict(window=33), dict(window=200)):
        w = kw.get("window", k)
        sel = h.select(**kw)
        check(ctx, sel, rule(src, w, best=kw.get("best")))
        sel.close()
    loci = h.select().view()
    assert set(loci["pattern"].tolist()) == set(range(256))


@gpu
def test_source_kinds(spm, ctx):
    rng = np.random.default_rng(77)
    n = 1 << 20
    T = rng.integers(0, 4, n, dtype=np.uint8)
    needles = [T[o:o + 64].copy() for o in rng.integers(0, n - 64, 300)]
    ks = rng.integers(0, 5, 300).astype(np.uint16)
    text = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=ks)
    kw = ks.astype(np.int64)
    whole = spm.scan(ctx, text, ps)
    src = whole.view()

    # a deferred source is completed first
    d = spm.scan(ctx, text, ps, engine=spm.ENGINE_FILTER, flags=spm.SCAN_DEFER)
    sel = d.select()
    check(ctx, sel, rule(src, kw))
    assert d.view().tobytes() == src.tobytes()

    # a sub-range with left context and pos_offset
    b, e, off = 300001, n - 7777, 1 << 40
    sub = spm.scan(ctx, text, ps, b, e, left_context=True, pos_offset=off)
    ssrc = sub.view()
    assert len(ssrc) and int(ssrc["pos"].min()) > off
    check(ctx, sub.select(best=1), rule(ssrc, kw, best=1))

    # two shards with left context, their device records concatenated: select_records == select of the whole scan
    import torch
    cut = n // 2 + 13
    parts = [spm.scan(ctx, text, ps, 0, cut), spm.scan(ctx, text, ps, cut, n, left_context=True)]
    tot = sum(p.device()[1] for p in parts)
    assert tot == len(src)
    buf = torch.zeros((tot, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    at = 0
    for p in parts:
        at += p.copy_to(buf.data_ptr() + 16 * at, tot - at)
    ctx.synchronize()
    both = spm.select_records(ctx, buf.data_ptr(), tot, ps, best=0)
    check(ctx, both, rule(src, kw, best=0))
    assert both.view().tobytes() == whole.select(best=0).view().tobytes()
    # ... a locus that straddles the cut is why per-shard selection is not the same thing
    with pytest.raises(spm.SpmError, match="-1"):
        both.align()
    with pytest.raises(spm.SpmError, match="-1"):        # the window of the needles needs the needles
        spm.select_records(ctx, buf.data_ptr(), tot, None)

    # segmented: segments shorter than a window apart (cuts inside occurrences)
    ends = np.sort(src["pos"].astype(np.int64))
    cuts = sorted({0, n} | {int(x) - 1 for x in ends[::7]} | {int(x) + 2 for x in ends[3::11] if x + 2 < n})
    seg = spm.scan_segments(ctx, text, ps, cuts)
    gsrc = seg.view()
    assert len(gsrc)
    check(ctx, seg.select(), rule(gsrc, kw, segs=cuts, myers=True))
    check(ctx, seg.select(window=9, best=0), rule(gsrc, 9, best=0, segs=cuts, myers=True))

    # the source destroyed before the derived result is read
    h2 = spm.scan(ctx, text, ps)
    s2 = h2.select()
    h2.close()
    h3 = spm.scan(ctx, text, ps)                          # (reuses what h2 gave back)
    check(ctx, s2, rule(src, kw))
    h3.close()

    # dna5
    T5 = rng.integers(0, 5, 1 << 18, dtype=np.uint8)
    n5 = [T5[o:o + 50].copy() for o in rng.integers(0, (1 << 18) - 50, 64)]
    t5 = ctx.upload(T5, sigma=5)
    p5 = ctx.patterns(spm.ALGO_MYERS, n5, k=2, sigma=5)
    h5 = spm.scan(ctx, t5, p5)
    check(ctx, h5.select(), rule(h5.view(), 2))


@gpu
def test_exact_and_prefix_sets(spm, ctx):
    A = np.zeros(1 << 12, dtype=np.uint8)                  # poly-A
    text = ctx.upload(A)
    for algo in (spm.ALGO_SHIFTOR, spm.ALGO_HORSPOOL):
        ps = ctx.patterns(algo, [np.zeros(4, dtype=np.uint8), np.zeros(9, dtype=np.uint8)])
        h = spm.scan(ctx, text, ps)
        src = h.view()
        assert len(src) == (len(A) - 3) + (len(A) - 8)
        check(ctx, h.select(), src)                        # SPM_SELECT_WINDOW_K is 0 for exact sets: everything stays
        sel = h.select(window=2)
        check(ctx, sel, rule(src, 2, myers=False))
        assert rows(sel.view()) == [(0, 0, 0), (1, 0, 0)]
        segs = [0, 100, 101, 4000, len(A)]
        g = spm.scan_segments(ctx, text, ps, segs)
        check(ctx, g.select(window=5), rule(g.view(), 5, segs=segs, myers=False))
    # a segment boundary between two records <= w apart, by a real scan: AAAA with k = 1 in two poly-A haystacks of 50.
    # Ends 3 (one error) and 4..50 (none) in the first, 53 and 54..100 in the second; ends 50 and 54 are 4 apart.
    pm = ctx.patterns(spm.ALGO_MYERS, [np.zeros(4, dtype=np.uint8)], k=1)
    g = spm.scan_segments(ctx, ctx.upload(A[:100]), pm, [0, 50, 100])
    gs = g.view()
    assert rows(gs) == [(0, 3, 1)] + [(0, e, 0) for e in range(4, 51)] + [(0, 53, 1)] + [(0, e, 0) for e in range(54, 101)]
    assert rows(rule(gs, 4)) == [(0, 4, 0)] and rows(rule(gs, 4, segs=[0, 50, 100])) == [(0, 4, 0), (0, 54, 0)]
    sel = g.select(window=4)
    check(ctx, sel, rule(gs, 4, segs=[0, 50, 100]))
    assert rows(sel.view()) == [(0, 4, 0), (0, 54, 0)]
    rng = np.random.default_rng(5)
    T = rng.integers(0, 4, 1 << 16, dtype=np.uint8)
    needles = [T[o:o + 48].copy() for o in (0, 3, 5)] + [T[100:148].copy()]
    pp = ctx.patterns(spm.ALGO_MYERS_PREFIX, needles, k=4)
    hp = spm.scan(ctx, ctx.upload(T), pp)
    psrc = hp.view()
    assert len(psrc)
    check(ctx, hp.select(), rule(psrc, 4))
    with pytest.raises(spm.SpmError, match="-4"):        # the refusals are inherited
        hp.select().align()


@gpu
def test_stateful_chunk_walk(spm, ctx):
    rng = np.random.default_rng(9)
    n = 1 << 18
    T = rng.integers(0, 4, n, dtype=np.uint8)
    needles = [T[o:o + 70].copy() for o in rng.integers(0, n - 70, 40)]
    text = ctx.upload(T)
    for algo, k in ((spm.ALGO_MYERS, 3), (spm.ALGO_SHIFTOR, 0)):
        ps = ctx.patterns(algo, needles, k=k)
        state = ps.initial_state()
        total = 0
        for a, b in zip(range(0, n, 50001), list(range(50001, n, 50001)) + [n]):
            hits, state = spm.scan(ctx, text, ps, a, b, state_in=state, want_state=True)
            src = hits.view()
            total += len(src)
            sel = hits.select()
            check(ctx, sel, rule(src, k, myers=algo == spm.ALGO_MYERS))
            with pytest.raises(spm.SpmError, match="-4"):
                sel.align()
        assert total >= 40


@gpu
def test_select_then_align_equals_the_rows_the_rule_keeps(spm, ctx):
    rng = np.random.default_rng(21)
    n = 1 << 20
    T = rng.integers(0, 4, n, dtype=np.uint8)
    needles = []
    for o in rng.integers(0, n - 120, 200):
        nd = T[o:o + 100].copy()
        nd[rng.integers(0, 100, 2)] ^= 1
        needles.append(np.delete(nd, int(rng.integers(0, 100))))
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=4)
    text = ctx.upload(T)
    h = spm.scan(ctx, text, ps)
    src = h.view()
    key = lambda a: a["pattern"].astype(np.int64) << 40 | a["pos"].astype(np.int64)
    keep = np.isin(key(src), key(rule(src, 4)))
    assert 0 < keep.sum() < len(src)
    sel = h.select()
    for begin_only in (False, True):
        full, part = h.align(begin_only=begin_only), sel.align(begin_only=begin_only)
        fr, fo, pr, po = full.view(), full.ops, part.view(), part.ops
        want = fr[keep]
        assert len(pr) == len(want)
        for f in ("begin", "end", "pattern", "score"):
            assert np.array_equal(pr[f], want[f]), f
        if not begin_only:
            idx = np.flatnonzero(keep)
            for j in range(0, len(pr), max(1, len(pr) // 150)):
                assert part.cigar(j, pr, po) == full.cigar(int(idx[j]), fr, fo)


@gpu
def test_lifetimes_and_errors(spm, ctx, oracle):
    rng = np.random.default_rng(2)
    T = rng.integers(0, 4, 1 << 18, dtype=np.uint8)
    needles = [T[o:o + 64].copy() for o in rng.integers(0, (1 << 18) - 64, 100)]
    text = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=2)
    h = spm.scan(ctx, text, ps)
    with pytest.raises(spm.SpmError, match="-1"):        # select_stats on a plain scan
        h.select_stats()
    small = spm.scan(ctx, text, ps, max_hits=10)           # an overflowed source returns its SPM_E_OVERFLOW
    with pytest.raises(spm.SpmError, match="-5"):
        small.select()
    L = spm.capi.lib()
    out = ctypes.c_void_p()
    assert L.spm_hip_hits_select(h._h, None, ctypes.byref(out)) == -1          # null opts
    for bad in (spm.capi.SelectOpts(flags=4, window=1, strata=0, reserved=0),
                spm.capi.SelectOpts(flags=0xDEADBEEF, window=0xABCD, strata=7, reserved=0x1234),
                spm.capi.SelectOpts(flags=1, window=1, strata=0, reserved=1)):
        assert L.spm_hip_hits_select(h._h, ctypes.byref(bad), ctypes.byref(out)) == -1
    assert L.spm_hip_hits_select(None, ctypes.byref(spm.capi.SelectOpts()), ctypes.byref(out)) == -1
    # an empty result selects to an empty result
    none = spm.scan(ctx, text, ctx.patterns(spm.ALGO_MYERS, [np.array([0, 1, 2, 3] * 30, dtype=np.uint8)], k=0), 0, 64)
    e = none.select(best=0)
    assert len(e.view()) == 0 and e.select_stats().n_in == 0 and e.device()[1] == 0
    # a selection can be selected again: LOCI is idempotent
    once = h.select()
    check(ctx, once.select(), once.view())
    # the other accessors take the result unchanged
    import torch
    v = once.view()
    buf = torch.full((len(v) + 1, 2), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert once.copy_fused(buf.data_ptr(), len(v)) == len(v)
    ctx.synchronize()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert host[0, 0] == len(v) and host[1:].copy().view(HIT).reshape(-1).tobytes() == v.tobytes()
    buf.fill_(-1)
    torch.cuda.synchronize()
    once.copy_fused_device(buf.data_ptr(), len(v))
    ctx.synchronize()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert host[0, 0] == len(v) and host[0, 1] == 0 and host[1:].copy().view(HIT).reshape(-1).tobytes() == v.tobytes()
    assert once.checksum() == oracle.checksum(v)


@gpu
def test_full_size_c4_shape(spm, ctx):
    """Beside the other full-size tests: 8 GiB x 100 000 needles of 150, k <= 3."""
    N, L, kmax, n_pat = 1 << 33, 150, 3, 100_000
    made = [spm.synth_pattern(SEED_TEXT, SEED_PAT, N, p, L, kmax) for p in range(n_pat)]
    planted = np.array([m[1] for m in made], dtype=np.int64)
    text = ctx.generate(SEED_TEXT, 0, N)
    ps = ctx.patterns(spm.ALGO_MYERS, np.stack([m[0] for m in made]), k=kmax)
    h = spm.scan(ctx, text, ps, max_hits=1 << 22)
    src = h.view()
    sel = h.select()
    st = check(ctx, sel, rule(src, kmax))
    print("c4 select: n_in", st.n_in, "n_loci", st.n_loci, "key bits", st.key_bits, "ms order/select", st.ms_order, st.ms_select)
    assert st.n_loci < st.n_in
    got = sel.view()
    key = got["pattern"].astype(np.int64) << 40 | got["pos"].astype(np.int64)
    assert np.all(np.diff(key) > 0)                        # sorted
    near = np.abs(got["pos"].astype(np.int64) - (planted[got["pattern"]] + L)) <= kmax
    assert len(np.unique(got["pattern"][near])) == n_pat   # every planted needle keeps a locus
    check(ctx, h.select(best=0), rule(src, kmax, best=0))
