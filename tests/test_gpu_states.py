"""GPU: captured matcher states (the restorable matchers' capture()/restore() blobs) and the prefix matcher, against the DP.

Every state blob the product hands back is decoded with the documented layout (oracle/states.py) and compared with the
oracle's resumable state -- which tests/test_state_reference.py pins to the Sellers column and to the Shift-Or
definition -- after every chunk: rows below |P|, score, set-wide n_words and the padding rule.  Blobs the product did not
write are restored too.  Widths cover every brute-force bucket (1 .. 64 32-bit words) at both ends."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import states as ST

pytestmark = pytest.mark.gpu

HIT_DTYPE = np.dtype([("pos", "<u8"), ("pattern", "<u4"), ("score", "<i4")])
# (lo, hi) |P| of every brute-force width bucket: NW = 1, 2, 4, 8, 16, 32, 64 words of 32 rows
BUCKETS = [(1, 32), (33, 64), (65, 128), (129, 256), (257, 512), (513, 1024), (1025, 2048)]

_pool = None


def _map(fn, items):
    """The oracle runs one needle per call; ctypes releases the GIL, so the needles of a set run side by side."""
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
    return list(_pool.map(fn, items))


class Ref:
    """The oracle's resumable matchers for a whole needle set (Myers: full width, variant 1)."""

    def __init__(self, O, algo, needles, ks, sigma=4):
        self.O, self.algo, self.needles, self.ks, self.sigma = O, algo, needles, list(ks), sigma
        self.max_m = max(len(p) for p in needles)
        self.myers = ST.is_myers(algo)
        self.mode = O.PREFIX if algo == ST.ALGO_MYERS_PREFIX else O.INFIX
        if self.myers:
            self.st = [O.myers_state(len(p), k) for p, k in zip(needles, self.ks)]
        else:
            self.st = [O.shiftor_state(len(p)) for p in needles]

    def restore(self, records):
        """Continue from decoded records (bits >= |P| are ignored, as the product must ignore them)."""
        for i, rec in enumerate(records):
            m = len(self.needles[i])
            low = (1 << m) - 1
            if self.myers:
                self.st[i] = ST.oracle_from_record(dict(rec, vp=rec["vp"] & low, vn=rec["vn"] & low), m, self.ks[i])
            else:
                own = (1 << (32 * ((m + 31) // 32))) - 1
                self.st[i] = ST.shiftor_oracle_from_register(rec["r"] & low | own ^ low, m)

    def advance(self, chunk, offset):
        """Hits of the next chunk (sorted by (pattern, pos), like the product's view); the states move on."""
        O = self.O

        def one(i):
            p = self.needles[i]
            if self.myers:
                h = O.myers(chunk, p, self.ks[i], sigma=self.sigma, mode=self.mode, variant=1, state=self.st[i],
                            text_offset=offset)
                pos, score = h["pos"], h["score"]
            else:
                pos = O.shiftor(chunk, p, sigma=self.sigma, state=self.st[i], text_offset=offset)
                score = 0
            out = np.zeros(len(pos), dtype=HIT_DTYPE)
            out["pos"], out["pattern"], out["score"] = pos, i, score
            return out

        return np.concatenate(_map(one, range(len(self.needles))))

    def records(self):
        nw = ST.n_words(self.algo, self.max_m)
        out = []
        for i, p in enumerate(self.needles):
            m = len(p)
            if self.myers:
                out.append(dict(ST.record_from_oracle(self.st[i], m), n_words=nw))
            else:
                low = (1 << m) - 1
                r = ST.shiftor_oracle_register(self.st[i]) & low | ((1 << (32 * nw)) - 1) ^ low
                out.append({"n_words": nw, "pad": 0, "r": r})
        return out

    def blob(self, rng=None):
        """The reference state as a blob; with rng, the bits at and above |P| of each record hold garbage."""
        recs = self.records()
        if rng is not None:
            nw = ST.n_words(self.algo, self.max_m)
            for i, rec in enumerate(recs):
                m = len(self.needles[i])
                for f in ("vp", "vn") if self.myers else ("r",):
                    bits = (64 if self.myers else 32) * nw
                    junk = int.from_bytes(rng.bytes(bits // 8), "little") & ~((1 << m) - 1)
                    rec[f] = (rec[f] & ((1 << m) - 1)) | junk
        return ST.encode(recs, self.algo, self.max_m)


def check_state(ref, blob, where):
    """The product's blob == the reference state: every record, every documented field, the padding rule."""
    got = ST.decode(blob, ref.algo, len(ref.needles), ref.max_m)
    want = ref.records()
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        m = len(ref.needles[i])
        if ref.myers:
            pad_ok = (g["vp"] >> m) == 0 and (g["vn"] >> m) == 0  # bits >= |P| are zero on output
            same = (g["score"], g["vp"], g["vn"], g["n_words"]) == (w["score"], w["vp"], w["vn"], w["n_words"])
        else:
            low = (1 << m) - 1
            pad_ok = (g["r"] | low) == (1 << (32 * w["n_words"])) - 1  # bits >= |P| are set
            same = (g["r"], g["n_words"]) == (w["r"], w["n_words"])
        if not (same and pad_ok):
            bad.append((i, m, ref.ks[i], "data" if not same else "padding"))
    assert not bad, f"{where}: {len(bad)} records differ from the reference, first {bad[:4]}"


def make_set(rng, lo, hi, n, sigma=4, exact=False, short_long=False):
    """n needles, |P| in [lo, hi] with both ends present.  Myers k per needle: 0 and small k; |P| - 1, |P| and |P| + 2
    (hits almost or exactly everywhere) on three needles of length lo only, so that the window stays close to max|P|."""
    lengths = [lo, hi, lo, lo, lo] + [int(x) for x in rng.integers(lo, hi + 1, n - 5)]
    if short_long:  # |P| 1..5 next to |P| = 2048: the short ones sit at the top of a 64-word column
        lengths = [2048 if i % 4 == 1 else 1 + i % 5 for i in range(n)]
    needles = [rng.integers(0, sigma, m, dtype=np.uint8) for m in lengths]
    ks = []
    for i, m in enumerate(lengths):
        if exact:
            ks.append(0)
        elif 2 <= i <= 4:
            ks.append([max(0, m - 1), m, m + 2][i - 2])
        else:
            ks.append([0, 1, 4, min(m // 10, 12), min(m - 1, 2)][i % 5] if m > 1 else 0)
    return needles, ks


def window(needles, ks, exact):
    return max(len(p) + (0 if exact else k) for p, k in zip(needles, ks))


def plant_long_span(rng, T, end, pat, k, W):
    """Plant pat with c > W - |P| inserted symbols so that it ends at T[end - 1]: an optimal alignment of the needle's
    rows spans more than the window, which a warm-up of only W symbols misses."""
    m = len(pat)
    c = W - m + 4 + m // 8
    occ = pat.copy()
    for j in sorted(rng.choice(np.arange(1, m + 1), size=c, replace=True))[::-1]:
        occ = np.insert(occ, j, rng.integers(0, 4))
    if len(occ) > end:
        return False
    T[end - len(occ):end] = occ
    return True


def walk(spm, ctx, O, algo, needles, ks, T, cuts, sigma=4, engine=None, ref=None, state=None, check_engine=None, base=0):
    """Chunked restorable scan of T along `cuts`, twice: chunks uploaded one by one (pos_offset), and sub-ranges of one
    uploaded text.  After every chunk: hits == the oracle's from the carried state, the blob == the reference state.
    T[0] has the global position `base` (a restored state stands for the symbols before it)."""
    engine = spm.ENGINE_AUTO if engine is None else engine
    ps = ctx.patterns(algo, needles, k=ks, sigma=sigma)
    ref = ref or Ref(O, algo, needles, ks, sigma)
    st0 = ps.initial_state() if state is None else state
    if state is None:
        check_state(ref, st0, "initial state")
    whole = ctx.upload(T, sigma=sigma)
    states = [st0, st0.copy()]
    cap = len(needles) * (max(b - a for a, b in zip(cuts[:-1], cuts[1:])) + 1) + 64
    for a, b in zip(cuts[:-1], cuts[1:]):
        want = ref.advance(T[a:b], base + a)
        for mode in (0, 1):
            if mode == 0:
                hits, states[0] = spm.scan(ctx, ctx.upload(T[a:b], sigma=sigma), ps, state_in=states[0],
                                           want_state=True, pos_offset=base + a, engine=engine, max_hits=cap)
            else:
                hits, states[1] = spm.scan(ctx, whole, ps, a, b, state_in=states[1], want_state=True, engine=engine,
                                           pos_offset=base, max_hits=cap)
            got = hits.view()
            assert np.array_equal(got, want), (f"chunk [{a},{b}) {'upload' if mode == 0 else 'sub-range'}: "
                                               f"{len(got)} hits vs {len(want)}")
            if check_engine is not None and b - a >= check_engine[0]:
                assert int(hits.stats().engine_used) == check_engine[1], (a, b)
            check_state(ref, states[mode], f"after chunk [{a},{b}) {'upload' if mode == 0 else 'sub-range'}")
    return ref, ps


def _cuts_for(W, big=True, extra=()):
    sizes = [0, 1, max(1, W - 1), W, W + 1, 0, 1, 3 * W + 17] + list(extra)
    if big:
        sizes += [65535, 65536, 65537]
    cuts = [0]
    for s in sizes:
        cuts.append(cuts[-1] + s)
    return cuts


def _matrix_case(spm, ctx, O, algo, bucket, sigma, short_long=False, seed=0, big=True):
    lo, hi = BUCKETS[bucket]
    rng = np.random.default_rng(1000 * bucket + 10 * algo + sigma + seed)
    n = 65 + (bucket * 11) % 66  # 65 .. 130 needles: two or three lane groups, the last one partly filled
    exact = not ST.is_myers(algo)
    needles, ks = make_set(rng, lo, hi, n, sigma=sigma, exact=exact, short_long=short_long)
    W = window(needles, ks, exact)
    cuts = _cuts_for(W, big=big)
    T = rng.integers(0, sigma, cuts[-1], dtype=np.uint8)
    # occurrences ending at chunk ends (exact ones for the exact matchers), and alignments longer than the window
    longest = [i for i in np.argsort([-len(p) for p in needles]) if ks[i] < len(needles[i])][:4]
    ends = [cuts[4], cuts[5], cuts[8], cuts[-2], cuts[-1], cuts[-3]]
    for j, e in enumerate(ends):
        i = longest[j % len(longest)]
        if exact:
            m = len(needles[i])
            if m <= e:
                T[e - m:e] = needles[i]
        elif algo == ST.ALGO_MYERS:
            plant_long_span(rng, T, e, needles[i], ks[i], W)
    if exact:
        for i in range(0, n, 7):  # occurrences that straddle a cut
            m, e = len(needles[i]), cuts[3 + i % 8] + len(needles[i]) // 2
            if m <= e <= len(T):
                T[e - m:e] = needles[i]
    walk(spm, ctx, O, algo, needles, ks, T, cuts, sigma=sigma)


# ---- the width matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket", range(len(BUCKETS)))
def test_myers_states_every_width(spm, ctx, oracle, bucket):
    _matrix_case(spm, ctx, oracle, ST.ALGO_MYERS, bucket, 4)


@pytest.mark.parametrize("bucket", range(len(BUCKETS)))
def test_prefix_states_every_width(spm, ctx, oracle, bucket):
    _matrix_case(spm, ctx, oracle, ST.ALGO_MYERS_PREFIX, bucket, 4)


@pytest.mark.parametrize("bucket", range(len(BUCKETS)))
def test_shiftor_states_every_width(spm, ctx, oracle, bucket):
    _matrix_case(spm, ctx, oracle, ST.ALGO_SHIFTOR, bucket, 4)


@pytest.mark.parametrize("algo,bucket,sigma", [(ST.ALGO_MYERS, 6, 5), (ST.ALGO_MYERS, 5, 15), (ST.ALGO_MYERS, 1, 15),
                                               (ST.ALGO_MYERS_PREFIX, 2, 5), (ST.ALGO_MYERS_PREFIX, 5, 15),
                                               (ST.ALGO_SHIFTOR, 6, 5), (ST.ALGO_SHIFTOR, 5, 15),
                                               (ST.ALGO_HORSPOOL, 3, 4)])
def test_states_other_alphabets_and_horspool(spm, ctx, oracle, algo, bucket, sigma):
    _matrix_case(spm, ctx, oracle, algo, bucket, sigma)


@pytest.mark.parametrize("algo", [ST.ALGO_MYERS, ST.ALGO_MYERS_PREFIX])
def test_states_short_needles_next_to_2048(spm, ctx, oracle, algo):
    _matrix_case(spm, ctx, oracle, algo, 6, 4, short_long=True, seed=1, big=False)


def test_dna15_over_1024_is_refused_by_the_brute_engine(spm, ctx, oracle):
    """A dna15 set with |P| > 1024 needs more LDS than the brute engine has: a clear error, never hits."""
    rng = np.random.default_rng(15)
    needles = [rng.integers(0, 15, m, dtype=np.uint8) for m in (1025, 40, 2048)]
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=2, sigma=15)
    text = ctx.upload(rng.integers(0, 15, 5000, dtype=np.uint8), sigma=15)
    calls = [dict(engine=spm.ENGINE_BRUTE), dict(want_state=True), dict(state_in=ps.initial_state(), want_state=True)]
    for kw in calls:
        with pytest.raises(spm.capi.SpmError, match="error -4"):
            spm.scan(ctx, text, ps, **kw)


# ---- the stateful seed-filter path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", [(1024, 64), (100, 3)])
def test_states_through_the_stateful_filter(spm, ctx, oracle, m, k):
    """A chunk of >= 2^18 symbols of a filterable set under ENGINE_AUTO: the seed filter takes it, the brute kernel its
    first window - 1 symbols and the exit state (tail pass).  An alignment longer than the window ends at that cut."""
    rng = np.random.default_rng(m + k)
    n = 65 + m % 7
    needles = [rng.integers(0, 4, m - (i % 3), dtype=np.uint8) for i in range(n)]
    ks = [k - (i % 2) for i in range(n)]
    W = window(needles, ks, False)
    cuts = [0, 3 * W + 5, 3 * W + 5 + (1 << 18) + 77, 3 * W + 5 + (1 << 18) + 77 + 2 * W]
    T = rng.integers(0, 4, cuts[-1], dtype=np.uint8)
    for j in range(12):  # planted occurrences with edits, some across the cuts
        i = int(rng.integers(0, n))
        at = cuts[1 + j % 2] - len(needles[i]) // 2 if j % 3 == 0 else int(rng.integers(0, cuts[-1] - 2 * m))
        occ = needles[i].copy()
        occ[len(occ) // 3] = (occ[len(occ) // 3] + 1) & 3
        T[at:at + len(occ)] = occ
    assert plant_long_span(rng, T, cuts[2], needles[0], ks[0], W)
    # the planted alignment does matter: a cold start one window before the cut ends in another column
    cold = oracle.myers_state(len(needles[0]), ks[0])
    oracle.myers(T[cuts[2] - W:cuts[2]], needles[0], ks[0], variant=1, state=cold)
    full = oracle.myers_state(len(needles[0]), ks[0])
    oracle.myers(T[:cuts[2]], needles[0], ks[0], variant=1, state=full)
    assert ST.record_from_oracle(cold, m) != ST.record_from_oracle(full, m)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=ks)
    assert ps.filterable
    walk(spm, ctx, oracle, ST.ALGO_MYERS, needles, ks, T, cuts, check_engine=(1 << 18, spm.ENGINE_FILTER))


# ---- restoring states the product did not write -----------------------------------------------------------------------
@pytest.mark.parametrize("algo,bucket", [(ST.ALGO_MYERS, 6), (ST.ALGO_MYERS, 2), (ST.ALGO_MYERS_PREFIX, 4),
                                         (ST.ALGO_SHIFTOR, 6), (ST.ALGO_SHIFTOR, 0)])
def test_restore_a_reference_state(spm, ctx, oracle, algo, bucket):
    """A reference state after a random prefix X that the product never saw, encoded with garbage in every bit at or
    above |P|, restored on a different haystack Y: hits and exit state == the oracle continuing from the same state."""
    lo, hi = BUCKETS[bucket]
    rng = np.random.default_rng(77 + 3 * bucket + algo)
    exact = not ST.is_myers(algo)
    needles, ks = make_set(rng, lo, hi, 70, exact=exact)
    ref = Ref(oracle, algo, needles, ks)
    X = rng.integers(0, 4, int(rng.integers(hi, 3 * hi + 50)), dtype=np.uint8)
    i0 = 1  # the prefix ends inside an occurrence of the longest needle, which Y completes
    half = len(needles[i0]) // 2
    X[len(X) - half:] = needles[i0][:half]
    ref.advance(X, 0)
    blob = ref.blob(rng)
    W = window(needles, ks, exact)
    for n_y in (W + 300, 70001):  # one pass, and the resume pass + tail pass
        ref_y = Ref(oracle, algo, needles, ks)
        ref_y.restore(ST.decode(blob, algo, len(needles), ref.max_m))
        Y = rng.integers(0, 4, n_y, dtype=np.uint8)
        Y[:len(needles[i0]) - half] = needles[i0][half:]
        walk(spm, ctx, oracle, algo, needles, ks, Y, [0, n_y], ref=ref_y, state=blob.copy(), base=len(X))


# ---- the prefix matcher ------------------------------------------------------------------------------------------------
def _prefix_set(rng):
    """Mixed lengths up to 300; the longest needle (k = 0) alone has the largest window."""
    lengths = [300] + [int(x) for x in rng.integers(1, 250, 69)]
    needles = [rng.integers(0, 4, m, dtype=np.uint8) for m in lengths]
    ks = [0] + [[0, max(0, m - 1), m, m + 2, min(3, m)][i % 5] for i, m in enumerate(lengths[1:])]
    ks = [min(k, 299 - len(p)) if i else k for i, (p, k) in enumerate(zip(needles, ks))]
    return needles, ks


def _prefix_hits(O, needles, ks, text, offset):
    ref = Ref(O, ST.ALGO_MYERS_PREFIX, needles, ks)
    return ref.advance(text, offset), ref


def test_prefix_matcher_ranges_segments_and_left_context(spm, ctx, oracle):
    rng = np.random.default_rng(2024)
    needles, ks = _prefix_set(rng)
    W = window(needles, ks, False)
    assert W == 300 and all(len(p) + k < W for p, k in zip(needles[1:], ks[1:]))
    ps = ctx.patterns(spm.ALGO_MYERS_PREFIX, needles, k=ks)
    n = 4000
    T = rng.integers(0, 4, n, dtype=np.uint8)
    starts = [0, 7, 500, 1200, 2600]
    for j, s in enumerate(starts):  # a needle (with an edit) at the start of every sub-range
        p = needles[(13 * j) % 70].copy()
        p[len(p) // 2] = (p[len(p) // 2] + 1) & 3
        T[s:s + len(p)] = p
    text = ctx.upload(T)
    # sub-ranges with left_context = 0: each is a haystack of its own
    for a, b in [(0, n), (7, 400), (500, 500 + W - 1), (500, 500 + W + 1), (1200, 1203), (2600, n)]:
        want, ref = _prefix_hits(oracle, needles, ks, T[a:b], a)
        hits, st = spm.scan(ctx, text, ps, a, b, want_state=True, max_hits=1 << 20)
        assert np.array_equal(hits.view(), want), (a, b)
        check_state(ref, st, f"prefix range [{a},{b})")
    # left_context = 1: the whole text's hits whose last symbol lies in [begin, end), and the state after text[0:end).
    # The longest needle (k = 0) ends at begin - 1 + 1 symbol: a warm-up that starts one window before begin would take
    # its first symbol for the haystack start.
    for begin in (3, W - 2, W - 1, W, W + 10, 1500):
        if begin >= W:
            T2 = T.copy()
            T2[begin - W + 1:begin + 1] = needles[0]
        else:
            T2 = T
        t2 = ctx.upload(T2)
        end = begin + 700
        whole, ref = _prefix_hits(oracle, needles, ks, T2[:end], 0)
        want = whole[whole["pos"] > begin]
        hits, st = spm.scan(ctx, t2, ps, begin, end, left_context=True, want_state=True, max_hits=1 << 20)
        got = hits.view()
        assert np.array_equal(got, want), f"left context, begin {begin}: {got[:4]} vs {want[:4]}"
        if begin >= W:
            assert len(got) == 0
        check_state(ref, st, f"prefix left context [{begin},{end})")
        # stateless: the same hits (past the first window, the scan has nothing to report and runs nothing)
        got = spm.scan(ctx, t2, ps, begin, end, left_context=True, max_hits=1 << 20).view()
        assert np.array_equal(got, want), f"stateless left context, begin {begin}: {got[:4]} vs {want[:4]}"
        # with a state, left_context changes nothing: the tile resumes at begin
        h0, s0 = spm.scan(ctx, t2, ps, begin, end, state_in=st, want_state=True, max_hits=1 << 20)
        h1, s1 = spm.scan(ctx, t2, ps, begin, end, left_context=True, state_in=st, want_state=True, max_hits=1 << 20)
        assert np.array_equal(h0.view(), h1.view()) and np.array_equal(s0, s1), begin
    # segments shorter and longer than |P| + k + 1
    lens = [3, W - 1, W, W + 1, 2 * W + 5, 40, 1]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    S = rng.integers(0, 4, int(offs[-1]), dtype=np.uint8)
    for s in range(len(lens)):
        p = needles[(5 * s + 1) % 70]
        L = min(len(p), lens[s])
        S[int(offs[s]):int(offs[s]) + L] = p[:L]
    parts = [_prefix_hits(oracle, needles, ks, S[int(offs[s]):int(offs[s + 1])], int(offs[s]))[0]
             for s in range(len(lens))]
    want = np.concatenate(parts)
    want = want[np.lexsort((want["pos"], want["pattern"]))]
    got = spm.scan_segments(ctx, ctx.upload(S), ps, offs, max_hits=1 << 20).view()
    assert np.array_equal(got, want)
    assert len(want) > 0


def test_prefix_chunked_walk_equals_sellers(spm, ctx, oracle):
    """The restorable prefix matcher chunk by chunk == Sellers PREFIX carrying its column (hits and every column)."""
    rng = np.random.default_rng(99)
    needles, ks = _prefix_set(rng)
    ps = ctx.patterns(spm.ALGO_MYERS_PREFIX, needles, k=ks)
    T = rng.integers(0, 4, 1500, dtype=np.uint8)
    T[:len(needles[3])] = needles[3]
    cuts = [0, 0, 1, 2, 50, 299, 300, 301, 302, 700, 1500]
    cols = [ST.initial_column(len(p)) for p in needles]
    state = ps.initial_state()
    n_hits = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        hits, state = spm.scan(ctx, ctx.upload(T[a:b]), ps, state_in=state, want_state=True, pos_offset=a)
        got = hits.view()
        want = []
        for i, p in enumerate(needles):
            h, cols[i] = ST.sellers_column(T[a:b], p, ks[i], mode=oracle.PREFIX, col=cols[i], text_offset=a)
            want += [(i, int(x), int(s)) for x, s in zip(h["pos"], h["score"])]
        assert [(int(p), int(x), int(s)) for p, x, s in zip(got["pattern"], got["pos"], got["score"])] == want
        recs = ST.decode(state, ST.ALGO_MYERS_PREFIX, len(needles), 300)
        for i, p in enumerate(needles):
            assert np.array_equal(ST.column_from_record(recs[i], len(p)), cols[i]), (a, b, i)
            assert recs[i]["vp"] >> len(p) == 0 and recs[i]["vn"] >> len(p) == 0
        n_hits += len(want)
    assert n_hits >= 20


# ---- left_context = 1 with want_state ---------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [ST.ALGO_MYERS, ST.ALGO_SHIFTOR])
def test_left_context_state_equals_state_after_the_prefix(spm, ctx, oracle, algo):
    """left_context = 1, want_state, no state_in: the state after text[0:end), whatever the range's length and engine.
    With state_in, left_context = 1 gives what left_context = 0 gives."""
    rng = np.random.default_rng(41 + algo)
    exact = algo == ST.ALGO_SHIFTOR
    n = 66
    needles = [rng.integers(0, 4, 100 + (i % 51), dtype=np.uint8) for i in range(n)]
    ks = [0] * n if exact else [3 - (i % 4) for i in range(n)]
    W = window(needles, ks, exact)
    N = 90000
    T = rng.integers(0, 4, N, dtype=np.uint8)
    # short ranges whose one pass would cold-start W - 1 symbols before begin (and after the haystack start), longer ones,
    # a long one that takes the tail pass, one that starts inside the first window, and an empty one
    short = [(5000, 5001), (6000, 6008)]
    ranges = short + [(6500, 6500 + W // 2), (7000, 7000 + W + 1), (8000, 8000 + 2 * W + 3), (9000, 9000 + 3000),
                      (100, 100 + 70000), (10, 200), (5000, 5000)]
    for j, (a, b) in enumerate(ranges[len(short):]):
        if b > a and not exact:
            plant_long_span(rng, T, b, needles[j], ks[j], W)
        elif b > a:
            T[b - 30:b] = needles[j][:30]
    if not exact:
        # The needle with the least slack (largest |P| + k), planted with a long-span alignment at the end of each short
        # range.  A cold start one window before begin ends in another column for it: without the tail pass, a short
        # range's one-pass state would be wrong.
        tight = max(range(n), key=lambda i: (len(needles[i]) + ks[i], len(needles[i])))
        p, kt = needles[tight], ks[tight]
        for a, b in short:
            assert plant_long_span(rng, T, b, p, kt, W)
            cold, full = oracle.myers_state(len(p), kt), oracle.myers_state(len(p), kt)
            oracle.myers(T[a - (W - 1):b], p, kt, variant=1, state=cold)
            oracle.myers(T[:b], p, kt, variant=1, state=full)
            assert ST.record_from_oracle(cold, len(p)) != ST.record_from_oracle(full, len(p)), (a, b)
    text = ctx.upload(T)
    ps = ctx.patterns(algo, needles, k=ks)
    engines = [spm.ENGINE_BRUTE] + ([spm.ENGINE_FILTER] if ps.filterable else [])
    assert exact or len(engines) == 2
    for a, b in ranges:
        ref = Ref(oracle, algo, needles, ks)
        whole = ref.advance(T[:b], 0)
        lo = a + 1 if not exact else a  # Myers: pos = exclusive end; exact: pos = begin, owned by its last symbol
        want = whole[whole["pos"] >= lo] if not exact else whole[whole["pos"] + np.array([len(needles[p]) for p in whole["pattern"]], dtype=np.uint64) > a]
        for engine in engines:
            if engine == spm.ENGINE_FILTER and b == a:
                continue
            hits, st = spm.scan(ctx, text, ps, a, b, engine=engine, left_context=True, want_state=True,
                                max_hits=1 << 20)
            assert np.array_equal(hits.view(), want), (a, b, engine)
            check_state(ref, st, f"left context [{a},{b}) engine {engine}")
    # with state_in, left_context is irrelevant
    ref = Ref(oracle, algo, needles, ks)
    ref.advance(T[:3000], 0)
    blob = ref.blob()
    for a, b in [(3000, 3000 + W // 2), (3000, 3000 + 4000), (3000, 3000 + 70000)]:
        outs = [spm.scan(ctx, text, ps, a, b, engine=spm.ENGINE_BRUTE, left_context=lc, state_in=blob.copy(),
                         want_state=True, max_hits=1 << 20) for lc in (False, True)]
        assert np.array_equal(outs[0][0].view(), outs[1][0].view())
        assert np.array_equal(outs[0][1], outs[1][1])
        r2 = Ref(oracle, algo, needles, ks)
        r2.restore(ST.decode(blob, algo, n, ref.max_m))
        assert np.array_equal(outs[1][0].view(), r2.advance(T[a:b], a))
        check_state(r2, outs[1][1], f"state_in + left context [{a},{b})")
