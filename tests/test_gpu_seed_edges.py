"""GPU: the seed filter on worst-case occurrences -- occurrences that keep exactly one intact seed (two where the needle
carries k + 2) -- at every phase around every border of the streaming kernels, for every kernel variant (tests/seed_edges.py
builds them; tests/test_seed_edges.py checks the builder on the CPU).  Needles with random edits keep two or more seeds
nearly always, and that redundancy hides the loss of one; here nothing is redundant: a key window the kernel does not
look up, a carry it drops at a span's start, a pruning that rejects at its exact boundary -- each loses a planted hit.
A brute-force re-scan would find what the filter lost, so every scan also asserts that none happened."""
import os

import numpy as np
import pytest

import seed_edges as E
from test_host_index import _selftest

pytestmark = pytest.mark.gpu

OFFSET = 1 << 40


class V:
    """One kernel variant: the shape and knobs that select it, and what the index must then report."""

    def __init__(self, name, m, k, expect, env=None, algo="MYERS", sigma=4, packed=False, n_kinds=False, min_launches=1):
        self.name, self.m, self.k, self.expect, self.env = name, m, k, expect, env or {}
        self.algo, self.sigma, self.packed, self.n_kinds, self.min_launches = algo, sigma, packed, n_kinds, min_launches
        self.alphabet = {4: E.DNA4, 5: E.DNA5, 15: E.DNA15}[sigma]
        self.exact = algo != "MYERS"

    def __repr__(self):
        return self.name


def X(stride, key_len, hv, dense=0):
    return dict(stride=stride, key_len=key_len, hash_variant=hv, dense=dense)


S8, S4, S2, S1 = ({"SPM_HIP_FILTER_STRIDE": s} for s in "8421")
NO_DENSE = {"SPM_HIP_FILTER_DENSE": "0"}
# hash variants: 1 Bloom cascade, 2 fingerprint table, 3 dense pass, 4 presence bits as level 1
VARIANTS = [
    # fingerprint table, 1-byte text
    V("table_s8", 100, 3, X(8, 16, 2), S8),
    V("table_s16_shiftor", 32, 0, X(16, 16, 2), algo="SHIFTOR"),
    V("table_s16_horspool", 32, 0, X(16, 16, 2), algo="HORSPOOL"),
    V("table_s4", 80, 3, X(4, 16, 2), S4),
    # ... over the packed shadow: seed_filter_packed_kernel<16,4>, <8,4>, <4,2>
    V("packed_s16", 32, 0, X(16, 16, 2), algo="SHIFTOR", packed=True),
    V("packed_s8", 100, 3, X(8, 16, 2), S8, packed=True),
    V("packed_s4", 80, 3, X(4, 16, 2), S4, packed=True),
    # presence bits as level 1
    V("bits_s2_masked", 60, 3, X(2, 14, 4)),
    V("bits_s2_key16", 100, 3, X(2, 16, 4), S2),
    V("bits_s1_masked", 48, 3, X(1, 12, 4)),
    V("bits_s1_key16", 68, 3, X(1, 16, 4), {**S1, **NO_DENSE}),     # (64 / 4 = 16-symbol seeds get 15-symbol keys)
    V("bits_s1_whole_seed", 44, 3, X(1, 11, 4)),
    # Bloom cascade
    V("bloom_s8", 100, 3, X(8, 16, 1), {**S8, "SPM_HIP_FILTER_HASH": "1"}),
    V("bloom_s2", 60, 3, X(2, 14, 1), {"SPM_HIP_FILTER_HASH": "1"}),
    # dense pass; 150 / 3 anchors on three dimers: two or three anchor patterns
    V("dense", 100, 3, X(1, 16, 3, dense=1), {"SPM_HIP_FILTER_DENSE": "2"}),
    V("dense_patterns", 150, 3, X(1, 16, 3, dense=1), {"SPM_HIP_FILTER_DENSE": "2"}),
    # anchored stride-1 passes
    V("anchored", 150, 3, X(1, 16, 2), {**S1, **NO_DENSE, "SPM_HIP_FILTER_MAX_KEYS": "4096"}, min_launches=3),
    # surplus seeds with band merging; the piece count's top case
    V("surplus_150_8", 150, 8, X(1, 14, 4)),
    V("pieces_128_7", 128, 7, X(1, 15, 4)),
    # dna5, dna15: an N beside the seed
    V("dna5_s8", 100, 3, X(8, 16, 2), S8, sigma=5, n_kinds=True),
    V("dna5_s1", 48, 3, X(1, 12, 2), sigma=5, n_kinds=True),
    V("dna15_s8", 100, 3, X(8, 16, 2), S8, sigma=15, n_kinds=True),
    V("dna15_s1", 48, 3, X(1, 12, 2), sigma=15, n_kinds=True),
]
EDGE_VARIANTS = [v for v in VARIANTS if v.name in ("table_s8", "bits_s1_masked", "dense", "packed_s8")]


def _patterns(spm, ctx, v, needles):
    """The needle set under the variant's knobs, and the proof that it is the variant: build stats + the hash variant of the
    host self-test on the same needles."""
    algo = getattr(spm, "ALGO_" + v.algo)
    saved = {a: os.environ.get(a) for a in v.env}
    os.environ.update(v.env)
    try:
        ps = ctx.patterns(algo, needles, k=v.k, sigma=v.sigma)
        rc, st = _selftest(spm, algo, needles, v.k, v.sigma)
    finally:
        for a, b in saved.items():
            os.environ.pop(a, None) if b is None else os.environ.__setitem__(a, b)
    bs = ps.build_stats()
    assert ps.filterable and rc == 0 and st["missing"] == 0
    got = dict(stride=int(bs.stride), key_len=int(bs.key_len), hash_variant=st["hash_variant"], dense=int(bool(bs.dense)))
    assert got == v.expect and (int(bs.stride), int(bs.key_len), int(bs.passes)) == (st["stride"], st["key_len"], st["passes"]), (got, st)
    if v.name == "dense_patterns":      # 3, 5, 6 or 7 sixteenths of the dimers: no single pattern covers that
        assert int(bs.anchor_sixteenths) in (3, 5, 6, 7), int(bs.anchor_sixteenths)
    if v.name == "anchored":
        assert int(bs.passes) >= 3 and int(bs.anchor_sixteenths) >= 1
    return ps


def _upload(ctx, v, T):
    text = ctx.upload(T, sigma=v.sigma)
    if v.packed:
        text.pack()
        assert text.packed
    return text


def _filter_scan(spm, ctx, v, text, ps, *args, **kw):
    h = spm.scan(ctx, text, ps, *args, engine=spm.ENGINE_FILTER, **kw)
    st = h.stats()
    # conditions, not measurements: a brute-force re-scan would find what the filter lost
    assert (int(st.engine_used), int(st.fell_back), int(st.fallback_spans)) == (spm.ENGINE_FILTER, 0, 0)
    assert int(st.main_launches) >= v.min_launches
    if v.packed:    # the packed kernel ran: spans of whole groups of four p-chunks
        assert int(st.span_symbols) % (4 * 4096) == 0 and int(st.span_symbols) > 0
    return h.view(), st


def _n_decorations(v):
    """dna5 / dna15: every kind of N beside the kept seed, one at a time (layout `hug`: the edit of a neighbouring piece
    touches the seed), after the plain sweep of all four layouts.  Returns [(name, edit_for, decorate, layouts)]."""
    if not v.n_kinds:
        return [("", None, None, None)]
    n, q = E.plan(v.m, v.k)
    assert n * q == v.m     # (no tail: what follows the last seed is outside the occurrence)
    N = 3 if v.sigma == 5 else 8

    def before(T, c, occ, at, q_):    # kept piece 0: the symbol in front of the occurrence
        if c.keep[0] == 0:
            T[c.start - 1] = N
        assert T[c.border + c.phase - 1] == N

    def after(T, c, occ, at, q_):
        if c.keep[0] == n - 1:
            T[c.end] = N
        assert T[c.border + c.phase + q_] == N

    def around(T, c, occ, at, q_):
        T[c.start - 1] = T[c.end] = N

    hug = ("hug",)
    return [("no N", None, None, None),     # the plain sweep: all four layouts
            ("N before the seed", lambda kp: {kp[0] - 1: N} if kp[0] > 0 else {}, before, hug),
            ("N after the seed", lambda kp: {kp[0] + 1: N} if kp[0] + 1 < n else {}, after, hug),
            ("N around the occurrence", None, around, hug)]


def _rows(hits):
    return {(int(p), int(x)): int(s) for p, x, s in zip(hits["pattern"], hits["pos"], hits["score"])}


def _window_ref(oracle, v, T, needles, c):
    """(ws, we, pos, score): the oracle on the case's window; positions in text coordinates, only those it is exact for."""
    ws, we = E.window(c, len(T))
    if v.exact:
        pos = np.sort(oracle.naive_exact(T[ws:we], needles[c.pattern]).astype(np.int64)) + ws
        return ws, we, pos, np.zeros(len(pos), np.int64)
    w = oracle.myers(T[ws:we], needles[c.pattern], v.k, sigma=v.sigma)
    w = w[w["pos"] >= v.m + v.k]
    return ws, we, w["pos"].astype(np.int64) + ws, w["score"].astype(np.int64)


def _check(v, got, cases, refs, planted, offset=0):
    """got: the filter's hits (sorted by pattern, pos).  planted: the cases whose hit must be there; refs: {case index:
    window reference} for the cases whose whole window the scan covers."""
    rows = _rows(got)
    for c in planted:
        key = (c.pattern, (c.start if v.exact else c.end) + offset)
        assert key in rows and rows[key] <= v.k, ("planted occurrence lost", v, c)
    pat = got["pattern"]
    pos = got["pos"].astype(np.int64) - offset
    for i, (ws, we, rpos, rscore) in refs.items():
        c = cases[i]
        a, b = np.searchsorted(pat, c.pattern), np.searchsorted(pat, c.pattern, side="right")
        p, s = pos[a:b], got["score"][a:b]
        keep = (p >= ws) & (p <= we - v.m) if v.exact else (p >= ws + v.m + v.k) & (p <= we)
        assert np.array_equal(p[keep], rpos) and np.array_equal(s[keep], rscore), ("window != oracle", v, c)


@pytest.mark.parametrize("v", VARIANTS, ids=repr)
def test_sweep(spm, ctx, oracle, v):
    for kind, edit_for, decorate, only in _n_decorations(v):
        classes = ("a", "b", "c", "d") if v.packed else ("a", "b", "c")
        span = 16384 if v.packed else 8192
        for again in range(2):      # the span depends on the device and on the text's length: lay out, scan, read it, lay out again
            T, needles, cases = E.lay_out(v.m, v.k, span, classes, seed=len(v.name) + 5, alphabet=v.alphabet, decorate=decorate,
                                          edit_for=edit_for, only_layouts=only)
            assert len(T) <= 16 << 20
            text = _upload(ctx, v, T)
            ps = _patterns(spm, ctx, v, needles)
            got, st = _filter_scan(spm, ctx, v, text, ps)
            if int(st.span_symbols) == span:
                break
            span = int(st.span_symbols)
        assert int(st.span_symbols) == span, "the layout's span borders are not the scan's"
        # 1. ground truth from the construction  2. the brute-force engine  3. the oracle on every case's window
        brute = spm.scan(ctx, text, ps, engine=spm.ENGINE_BRUTE).view()
        refs = {i: _window_ref(oracle, v, T, needles, c) for i, c in enumerate(cases)}
        _check(v, got, cases, refs, cases)
        assert np.array_equal(got, brute), (v, kind)
        # a sub-range that begins and ends inside plants: cold, and with left context == that part of the whole scan
        lo, hi = cases[len(cases) // 3].start + v.m // 2, cases[2 * len(cases) // 3].start + v.m // 2 + 1
        last = got["pos"].astype(np.int64) + (v.m - 1 if v.exact else -1)       # the hit's last symbol
        part = got[(last >= lo) & (last < hi)].copy()
        part["pos"] += OFFSET
        inner = {i: r for i, r in refs.items() if r[0] >= lo and r[1] <= hi}
        assert len(inner) > len(cases) // 4
        for warm in (False, True):
            sub, _ = _filter_scan(spm, ctx, v, text, ps, lo, hi, left_context=warm, pos_offset=OFFSET)
            bsub = spm.scan(ctx, text, ps, lo, hi, engine=spm.ENGINE_BRUTE, left_context=warm, pos_offset=OFFSET).view()
            assert np.array_equal(sub, bsub), (v, kind, warm)
            if warm:
                assert np.array_equal(sub, part), (v, kind)
            planted = [c for c in cases if (lo < c.end <= hi if warm else lo <= c.start and c.end <= hi)]
            _check(v, sub, cases, inner, planted, OFFSET)
        ps.close()
        text.close()


# ---- range, haystack and segment edges: a text of 64 Ki symbols ----
def _edge_setup(spm, ctx, v, seed, n_text=1 << 16, fillers=12):
    """A random text and a few needles that occur nowhere; the tests plant occurrences with the kept seed at either end of
    the needle (`ins` / `del` put the seed's diagonal k away from the occurrence's first / last symbol)."""
    rng = np.random.default_rng(seed)
    alpha = np.array(v.alphabet, np.uint8)
    T = alpha[rng.integers(0, 4, n_text)]
    n, q = E.plan(v.m, v.k)
    needles = [alpha[rng.integers(0, 4, v.m)] for _ in range(fillers)]
    return rng, alpha, T, n, needles


def _plant(T, needles, v, rng, keep, layout, start=None, end=None):
    alpha = np.array(v.alphabet, np.uint8)
    P = alpha[rng.integers(0, 4, v.m)]
    occ, at = E.occurrence(P, v.k, (keep,), layout, rng, v.alphabet)
    start = end - len(occ) if start is None else start
    T[start:start + len(occ)] = occ
    needles.append(P)
    return len(needles) - 1, start, start + len(occ)


def _sorted(h):
    return h[np.lexsort((h["pos"], h["pattern"]))]


@pytest.mark.parametrize("v", EDGE_VARIANTS, ids=repr)
def test_range_and_haystack_edges(spm, ctx, oracle, v):
    """begin at every value in [start - 17, start + 17], end at every value in [e - 17, e + 17], cold and warm: the range's
    first window, base0, the windows in front of lo, and the haystack bounds of the whole-seed check and of the piece
    count -- flush, one inside, one outside, and at distance exactly k."""
    rng, alpha, T, n, needles = _edge_setup(spm, ctx, v, 77)
    plants = []
    at = 8192
    for layout in ("hug", "ins", "del"):
        for keep in (0, n - 1):
            # start 5 past a multiple of 1 KiB: the begin sweep crosses it; the next plant's end 3 past one: the end sweep does
            if keep == 0:
                plants.append(_plant(T, needles, v, rng, keep, layout, start=at + 5))
            else:
                plants.append(_plant(T, needles, v, rng, keep, layout, end=at + 3))
            assert (plants[-1][1] - 17) // 1024 != (plants[-1][1] + 17) // 1024 or (plants[-1][2] - 17) // 1024 != (plants[-1][2] + 17) // 1024
            assert (plants[-1][1] - 17) // 1024 == (plants[-1][1] + 17) // 1024 or (plants[-1][2] - 17) // 1024 == (plants[-1][2] + 17) // 1024
            at += 4096
    text = _upload(ctx, v, T)
    ps = _patterns(spm, ctx, v, needles)
    whole = oracle.scan_multi(oracle.MYERS, T, needles, k=v.k, sigma=v.sigma, threads=4)
    for p, start, e in plants:
        assert ((whole["pattern"] == p) & (whole["pos"] == e)).any()
        ranges = [(b, e + 1500) for b in range(start - 17, start + 18)] + [(start - 1500, x) for x in range(e - 17, e + 18)]
        for b, x in ranges:
            for warm in (False, True):
                got, _ = _filter_scan(spm, ctx, v, text, ps, b, x, left_context=warm)
                if warm:
                    want = whole[(whole["pos"] > b) & (whole["pos"] <= x)]
                else:
                    want = oracle.scan_multi(oracle.MYERS, T[b:x], needles, k=v.k, sigma=v.sigma)
                    want["pos"] += b
                assert np.array_equal(got, want), (v, p, start, e, b, x, warm)
                # the plant is reported when the range holds it (cold: all of it; warm: its last symbol)
                if (b < e <= x) if warm else (b <= start and e <= x):
                    assert ((got["pattern"] == p) & (got["pos"] == e)).any(), (v, p, start, e, b, x, warm)


@pytest.mark.parametrize("v", EDGE_VARIANTS, ids=repr)
@pytest.mark.parametrize("how", ["uploaded", "wrapped"])
def test_ragged_ends(spm, ctx, oracle, v, how):
    """Sixteen texts of length L0 + r: each ends exactly at an occurrence whose kept seed is the last piece and whose last
    symbols are a poly-A tail; the text's end also cuts a second needle's occurrence short; and a poly-A needle must not
    match the symbols past the end (the kernels read them as 0 = A)."""
    import torch
    n, q = E.plan(v.m, v.k)
    L0 = 5 * 1024 + 357
    for r in range(16):
        rng, alpha, T, n, needles = _edge_setup(spm, ctx, v, 100 + r, n_text=L0 + r, fillers=4)
        tail = 12
        P = alpha[rng.integers(0, 4, v.m)]
        P[-tail:] = 0
        occ, _ = E.occurrence(P, v.k, (n - 1,), "mid", rng, v.alphabet)
        T[len(T) - len(occ):] = occ
        cut = np.concatenate([T[len(T) - (2 * q + 5):], alpha[rng.integers(0, 4, v.m - (2 * q + 5))]])    # two whole seeds fit
        needles += [P, cut, np.zeros(v.m, np.uint8)]
        T[1000:1000 + v.m - 1] = 0      # a poly-A stretch the poly-A needle does match (with one error)
        want = oracle.scan_multi(oracle.MYERS, T, needles, k=v.k, sigma=v.sigma)
        assert ((want["pattern"] == 4) & (want["pos"] == len(T))).any() and not (want["pattern"] == 5).any()
        assert (want["pattern"] == 6).any() and not ((want["pattern"] == 6) & (want["pos"] > 2000)).any()
        if how == "uploaded":
            text = _upload(ctx, v, T)
        else:   # a borrowed buffer with foreign symbols right behind the text
            buf = torch.full((len(T) + 256,), 3, dtype=torch.uint8, device="cuda")
            buf[:len(T)] = torch.from_numpy(T).to("cuda")
            torch.cuda.synchronize()
            text = ctx.wrap(buf.data_ptr(), len(T), sigma=v.sigma, keepalive=buf)
            if v.packed:
                text.pack()
                assert text.packed
        ps = _patterns(spm, ctx, v, needles)
        got, _ = _filter_scan(spm, ctx, v, text, ps)
        assert np.array_equal(got, want), (v, how, r)
        ps.close()
        text.close()


@pytest.mark.parametrize("v", EDGE_VARIANTS, ids=repr)
def test_segment_edges(spm, ctx, oracle, v):
    """scan_segments: segments that begin at start - 1, start, start + 1 and end at e - 1, e, e + 1 of plants with the kept
    seed at either end, an empty segment and one shorter than a key among them; per segment == the oracle on it alone."""
    rng, alpha, T, n, needles = _edge_setup(spm, ctx, v, 55)
    offs, at, plants = [0], 2048, []
    for keep in (0, n - 1):
        for layout in ("hug", "ins", "del"):
            for db in (-1, 0, 1):
                for de in (-1, 0, 1):
                    p, start, e = _plant(T, needles, v, rng, keep, layout, start=at)
                    plants.append((p, start, e, db, de))
                    offs += [start + db, e + de]
                    if len(plants) % 5 == 0:
                        offs += [e + de, e + de + 5]      # an empty segment, and one of 5 symbols
                    at += 1024
    offs.append(len(T))
    assert at < len(T) and all(a <= b for a, b in zip(offs, offs[1:]))
    text = _upload(ctx, v, T)
    ps = _patterns(spm, ctx, v, needles)
    h = spm.scan_segments(ctx, text, ps, np.array(offs, np.uint64), engine=spm.ENGINE_FILTER)
    st = h.stats()
    assert (int(st.engine_used), int(st.fell_back), int(st.fallback_spans)) == (spm.ENGINE_FILTER, 0, 0)
    got = h.view()
    ref = []
    for b, e in zip(offs, offs[1:]):
        if e > b:
            w = oracle.scan_multi(oracle.MYERS, T[b:e], needles, k=v.k, sigma=v.sigma)
            w["pos"] += b
            ref.append(w)
    want = _sorted(np.concatenate(ref))
    assert np.array_equal(got, want), v
    for p, start, e, db, de in plants:      # reported when the segment holds the whole occurrence
        if db <= 0 and de >= 0:
            assert ((got["pattern"] == p) & (got["pos"] == e)).any(), (v, p, db, de)
