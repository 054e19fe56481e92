"""Begins and CIGAR transcripts of hits (spm_hip_hits_align, Hits.align, the C++ mirror's locate).

The reference answer is built here: a NumPy DP over hits that computes ED(P, T[e-j, e)) for every j (and so the largest
begin b* at the hit's distance), and a replayer that checks a transcript consumes exactly P and T[b*, e), that its = / X
agree with the symbols and that its cost is the hit's distance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cpp_programs import build_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {1: "I", 2: "D", 7: "=", 8: "X"}


# ---------------------------------------------------------------------------------------------------------------------
# reference answer
# ---------------------------------------------------------------------------------------------------------------------
def ref_begins(T, needles, pats, ends, dists, los):
    """b* = max{b in [lo, e] : ED(P, T[b, e)) = d} for every hit, vectorised over the hits of one needle length.
    Also checks that d is the minimum over b >= lo (else the hit is not a hit of that scan)."""
    out = np.full(len(ends), -1, dtype=np.int64)
    lens = np.array([len(needles[p]) for p in pats], dtype=np.int64)
    for m in np.unique(lens):
        idx = np.nonzero(lens == m)[0]
        for c0 in range(0, len(idx), 4096):
            sel = idx[c0:c0 + 4096]
            e = ends[sel].astype(np.int64)
            d = dists[sel].astype(np.int64)
            lo = los[sel].astype(np.int64)
            J = int(m + d.max())
            jj = np.arange(J + 1)
            lim = np.minimum(m + d, e - lo)                           # j <= lim
            tpos = e[:, None] - jj[None, 1:]                          # text symbol of column j (1-based): T[e - j]
            tsym = T[np.clip(tpos, 0, len(T) - 1)].astype(np.int16)
            tsym[tpos < 0] = -1
            P = np.stack([needles[p] for p in pats[sel]]).astype(np.int16)
            big = 1 << 20
            row = np.broadcast_to(jj, (len(sel), J + 1)).astype(np.int64)  # D[0][j] = j
            for i in range(1, m + 1):
                pc = P[:, m - i]                                      # reversed needle
                diag = row[:, :-1] + (tsym != pc[:, None])
                up = row + 1
                x = np.empty_like(row)
                x[:, 0] = i
                x[:, 1:] = np.minimum(diag, up[:, 1:])
                row = np.minimum.accumulate(x - jj[None, :], axis=1) + jj[None, :]
            row = np.where(jj[None, :] <= lim[:, None], row, big)
            assert np.array_equal(row.min(axis=1), d), "a hit's distance is not the minimum over its begins"
            first = np.argmax(row == d[:, None], axis=1)
            out[sel] = e - first
    return out


def replay(P, T, b, e, words, d):
    """A transcript consumes exactly P and T[b, e), = / X agree with the symbols, runs are merged, cost = d."""
    i = j = 0
    cost = 0
    prev = None
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        assert n > 0 and op in OPS and op != prev, (words, "empty or unmerged run")
        prev = op
        if op in (7, 8):
            a, t = P[i:i + n], T[b + j:b + j + n]
            assert len(a) == n and len(t) == n and b + j + n <= e
            assert np.all(a == t) if op == 7 else np.all(a != t), "=/X disagree with the symbols"
            i += n
            j += n
            cost += n if op == 8 else 0
        elif op == 1:
            i += n
            cost += n
        else:
            j += n
            cost += n
    assert i == len(P) and b + j == e, "the transcript does not consume P and T[b, e)"
    assert cost == d, f"cost {cost} != distance {d}"


def _r(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


# (text, needle, end, distance, lo) -> (begin, CIGAR)
HAND = {
    "mismatch": ("TTTACGATTT", "ACCA", 7, 1, 0, 3, "2=1X1="),
    "insertion": ("TTTACGATTT", "ACCGA", 7, 1, 0, 3, "1=1I3="),
    "deletion": ("TTTACGATTT", "ACA", 7, 1, 0, 3, "2=1D1="),
    "tie_two_begins": ("TTTTCGATTT", "ACGA", 7, 1, 0, 4, "1I3="),
    "clipped_by_lo": ("TTTACGATTT", "ACGA", 7, 1, 4, 4, "1I3="),
}


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_record_layout(spm):
    assert ctypes.sizeof(spm.capi.Aln) == 32
    assert spm.ALN_DTYPE.itemsize == 32
    assert ctypes.sizeof(spm.capi.AlignStats) == 64


@pytest.mark.parametrize("case", sorted(HAND))
def test_reference_dp_and_replayer_on_hand_worked_cases(case):
    text, needle, e, d, lo, want_b, want_cigar = HAND[case]
    T, P = _r(text), _r(needle)
    b = ref_begins(T, [P], np.array([0]), np.array([e]), np.array([d]), np.array([lo]))
    assert int(b[0]) == want_b
    words = [int(n) << 4 | {"=": 7, "X": 8, "I": 1, "D": 2}[op]
             for n, op in __import__("re").findall(r"(\d+)([=XID])", want_cigar)]
    replay(P, T, want_b, e, words, d)
    with pytest.raises(AssertionError):
        replay(P, T, want_b, e, words, d + 1)


def test_reference_dp_rejects_a_distance_that_is_not_minimal():
    T, P = _r("TTTACGATTT"), _r("ACGA")
    with pytest.raises(AssertionError):
        ref_begins(T, [P], np.array([0]), np.array([7]), np.array([1]), np.array([0]))


LOCATE_CPP = r"""
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include <libspm/matcher/hip_batch.hpp>
#include <libspm/matcher/myers_matcher.hpp>
#include <libspm/seqan/alphabet.hpp>

// usage: locate text.bin needles.bin L k  -> one line per hit: needle begin end errors cigar operator()_begin
int main(int argc, char ** argv)
{
    if (argc < 5)
        return 2;
    std::ifstream ft(argv[1], std::ios::binary), fn(argv[2], std::ios::binary);
    std::vector<char> t((std::istreambuf_iterator<char>(ft)), std::istreambuf_iterator<char>());
    std::vector<char> nd((std::istreambuf_iterator<char>(fn)), std::istreambuf_iterator<char>());
    std::size_t const L = std::stoul(argv[3]), k = std::stoul(argv[4]);
    std::vector<spm::dna4> text(t.size());
    for (std::size_t i = 0; i < t.size(); ++i)
        text[i].assign_rank(static_cast<std::uint8_t>(t[i]));
    std::vector<std::vector<spm::dna4>> needles(nd.size() / L, std::vector<spm::dna4>(L));
    for (std::size_t p = 0; p < needles.size(); ++p)
        for (std::size_t i = 0; i < L; ++i)
            needles[p][i].assign_rank(static_cast<std::uint8_t>(nd[p * L + i]));
    auto batch = spm::batch_myers_matcher{needles, k};
    std::vector<std::size_t> plain;
    batch(text, [&](std::size_t, auto const & f) { plain.push_back(seqan2::beginPosition(f)); });
    std::size_t i = 0;
    batch.locate(text, [&](std::size_t needle, auto const & f, spm::alignment const & a) {
        std::printf("%zu %zu %zu %d %s %zu\n", needle, seqan2::beginPosition(f), seqan2::endPosition(f), a.errors(),
                    a.cigar_string().c_str(), i < plain.size() ? plain[i] : std::size_t{0});
        ++i;
    });
    // the single-needle matcher and the resident haystack: the same begins for needle 0
    spm::hip::resident_haystack const hs{text};
    spm::myers_matcher single{needles[0], k};
    std::size_t n0 = 0;
    single.locate(hs, [&](auto const & f, spm::alignment const & a) {
        if (a.begin_position() != seqan2::beginPosition(f) || a.cigar().empty())
            std::printf("MISMATCH\n");
        ++n0;
    });
    std::printf("single %zu\n", n0);
    return i == plain.size() ? 0 : 1;
}
"""


def _build_locate(tmp_path):
    src = tmp_path / "locate.cpp"
    src.write_text(LOCATE_CPP)
    return build_mirror(str(src), tmp_path, fixtures=False)


def test_locate_program_compiles_with_reference_flags(spm, tmp_path):
    assert _build_locate(tmp_path).exists()


def test_locate_is_a_compile_error_for_the_prefix_matcher(spm, tmp_path):
    """restorable_myers_prefix_matcher has no alignments: calling locate() on it must not compile (not abort at run time)"""
    src = tmp_path / "prefix_locate.cpp"
    src.write_text(r"""
#include <vector>
#include <libspm/matcher/myers_prefix_matcher_restorable.hpp>
#include <libspm/seqan/alphabet.hpp>
int main()
{
    std::vector<spm::dna4> needle(8), text(64);
    spm::restorable_myers_prefix_matcher m{needle, 1u};
    m.locate(text, [](auto const &, spm::alignment const &) {});
}
""")
    r = subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-pedantic", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "locate() is not available for this matcher" in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _align(hits, begin_only=False):
    a = hits.align(begin_only=begin_only)
    try:
        return a.view(), a.ops, a.stats()
    finally:
        a.close()


def _check_all(T, needles, hv, rec, ops, lo_of, check_dp=True):
    """every record against its hit, the DP's b* and the replayer"""
    assert len(rec) == len(hv)
    assert np.array_equal(rec["end"], hv["pos"]) and np.array_equal(rec["pattern"], hv["pattern"])
    assert np.array_equal(rec["score"], hv["score"])
    if len(rec) == 0:
        return
    assert np.all(rec["cigar_len"] <= 2 * rec["score"] + 1)
    offs = np.concatenate([[0], np.cumsum(2 * hv["score"].astype(np.int64) + 1)[:-1]])
    assert np.array_equal(rec["cigar_off"], offs)
    ends = hv["pos"].astype(np.int64)
    los = lo_of(ends)
    if check_dp:
        want = ref_begins(T, needles, hv["pattern"], ends, hv["score"], los)
        assert np.array_equal(rec["begin"].astype(np.int64), want)
    for r in rec:
        o = int(r["cigar_off"])
        replay(needles[r["pattern"]], T, int(r["begin"]), int(r["end"]), ops[o:o + int(r["cigar_len"])], int(r["score"]))


@pytest.mark.gpu
@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_worked_cases_brute(spm, ctx, case):
    """the hand-worked cases as they stand: needles of 3-5 symbols (too short for the seed filter)"""
    text, needle, e, d, lo, want_b, want_cigar = HAND[case]
    rng = np.random.default_rng(7)
    T = np.concatenate([_r(text), rng.integers(0, 4, 1 << 16, dtype=np.uint8)])
    P = _r(needle)
    tx = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, [P], k=d)
    h = spm.scan(ctx, tx, ps, begin=lo, engine=spm.ENGINE_BRUTE)
    hv = h.view()
    a = h.align()
    rec, ops = a.view(), a.ops
    i = np.nonzero(hv["pos"] == e)[0]
    assert len(i) == 1 and hv["score"][i[0]] == d
    assert int(rec["begin"][i[0]]) == want_b
    assert a.cigar(int(i[0])) == want_cigar
    _check_all(T, [P], hv, rec, ops, lambda ends: np.full(len(ends), lo))
    a.close()
    h.close()


# the single-edit cases inside 40 random symbols on either side (ending / starting with T, which the middles do not hold):
# long enough for the seed filter.  (case -> CIGAR)
WRAPPED = {"mismatch": "42=1X41=", "insertion": "41=1I43=", "deletion": "42=1D41="}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(WRAPPED))
def test_hand_worked_cases_inside_long_needles_both_engines(spm, ctx, case):
    text, needle, e, d, lo, b, _ = HAND[case]
    rng = np.random.default_rng(17)
    A = rng.integers(0, 4, 40, dtype=np.uint8)
    B = rng.integers(0, 4, 40, dtype=np.uint8)
    A[-1], B[0] = 3, 3
    X = rng.integers(0, 4, 1000, dtype=np.uint8)
    T = np.concatenate([X, A, _r(text)[b:e], B, rng.integers(0, 4, 1 << 16, dtype=np.uint8)])
    P = np.concatenate([A, _r(needle), B])
    end = len(X) + 40 + (e - b) + 40
    tx = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, [P], k=d)
    assert ps.filterable, "an 84-symbol needle with k = 1 should admit the seed filter"
    got = []
    for engine in (spm.ENGINE_BRUTE, spm.ENGINE_FILTER):
        h = spm.scan(ctx, tx, ps, engine=engine)
        assert int(h.stats().engine_used) == engine
        hv = h.view()
        a = h.align()
        rec, ops = a.view(), a.ops
        i = np.nonzero(hv["pos"] == end)[0]
        assert len(i) == 1 and hv["score"][i[0]] == d
        assert int(rec["begin"][i[0]]) == len(X)
        assert a.cigar(int(i[0]), rec, ops) == WRAPPED[case]
        _check_all(T, [P], hv, rec, ops, lambda ends: np.zeros(len(ends), np.int64))
        got.append((rec.tobytes(), ops.tobytes()))
        a.close()
        h.close()
    assert got[0] == got[1]


@pytest.mark.gpu
def test_hits_keep_their_text_and_needles_alive(spm, ctx):
    """Hits.align() after the caller dropped every reference to the scan's text and needle set"""
    import gc
    rng = np.random.default_rng(23)
    T = rng.integers(0, 4, 1 << 18, dtype=np.uint8)
    needles = [np.delete(T[a:a + 120].copy(), [30]) for a in rng.integers(0, len(T) - 200, 32)]
    h = spm.scan(ctx, ctx.upload(T), ctx.patterns(spm.ALGO_MYERS, needles, k=3))
    gc.collect()
    _ = [ctx.upload(rng.integers(0, 4, 1 << 18, dtype=np.uint8)) for _ in range(4)]  # (reuse of freed memory, were it freed)
    hv = h.view()
    rec, ops, _ = _align(h)
    assert len(hv) >= 32
    _check_all(T, needles, hv, rec, ops, lambda ends: np.zeros(len(ends), np.int64))
    segs = np.array([0, len(T) // 2, len(T)], dtype=np.uint64)
    h2 = spm.scan_segments(ctx, ctx.upload(T), ctx.patterns(spm.ALGO_MYERS, needles, k=3), segs)
    gc.collect()
    rec2, ops2, _ = _align(h2)
    _check_all(T, needles, h2.view(), rec2, ops2,
               lambda ends: segs[np.searchsorted(segs, ends - 1, side="right") - 1].astype(np.int64))
    h.close()
    h2.close()


def _planted(spm, ctx, n, lengths, n_needles, kmax, seed=0xA11C0001):
    text = ctx.generate(seed, 0, n)
    T = text.download(0, n)
    needles, origins, ks = [], [], []
    for p in range(n_needles):
        L = lengths[p % len(lengths)]
        k = p % (kmax + 1)
        nd, o = spm.synth_pattern(seed, seed + 1, n, p, L, k)
        needles.append(nd)
        origins.append(o)
        ks.append(k)
    return text, T, needles, np.array(origins), np.array(ks)


def _run_sets(spm, ctx, text, T, needles, ks, groups, check_dp=True):
    """align every group (a needle set) on every engine it admits; returns {group: (hits, records, ops)}"""
    out = {}
    for name, idx in groups.items():
        sub = [needles[i] for i in idx]
        ps = ctx.patterns(spm.ALGO_MYERS, sub, k=ks[idx])
        results = []
        engines = [spm.ENGINE_BRUTE] + ([spm.ENGINE_FILTER] if ps.filterable else [])
        for engine in engines:
            h = spm.scan(ctx, text, ps, engine=engine)
            hv = h.view()
            rec, ops, st = _align(h)
            rec2, ops2, _ = _align(h)
            assert rec.tobytes() == rec2.tobytes() and ops.tobytes() == ops2.tobytes(), "two calls differ"
            assert st.n_alns == len(hv)
            _check_all(T, sub, hv, rec, ops, lambda ends: np.zeros(len(ends), np.int64), check_dp)
            results.append((hv, rec, ops))
            h.close()
        for hv, rec, ops in results[1:]:
            assert hv.tobytes() == results[0][0].tobytes()
            assert rec.tobytes() == results[0][1].tobytes() and ops.tobytes() == results[0][2].tobytes(), \
                "engines disagree"
        out[name] = (results[0], idx, len(engines))
        ps.close()
    return out


@pytest.mark.gpu
def test_planted_needles_both_engines(spm, ctx):
    n = 4 << 20
    lengths = [24, 64, 65, 100, 150, 200]
    text, T, needles, origins, ks = _planted(spm, ctx, n, lengths, 512, 8)
    lens = np.array([len(x) for x in needles])
    groups = {"short": np.nonzero(lens == 24)[0], "mid": np.nonzero((lens == 64) | (lens == 65))[0],
              "long": np.nonzero(lens >= 100)[0]}
    res = _run_sets(spm, ctx, text, T, needles, ks, groups)
    assert res["long"][2] == 2, "the |P| >= 100 set should admit the seed filter"
    for name, ((hv, rec, _), idx, _) in res.items():
        for local, p in enumerate(idx):
            r = rec[rec["pattern"] == local]
            o, L = int(origins[p]), len(needles[p])
            assert np.any((r["begin"] < o + L + ks[p]) & (r["end"] > o)), f"needle {p}: no alignment over its origin"


@pytest.mark.gpu
def test_long_needles_wave_and_global_paths(spm, ctx):
    n = 4 << 20
    text, T, needles, origins, ks = _planted(spm, ctx, n, [1024], 64, 64, seed=0xA11C0002)
    res = _run_sets(spm, ctx, text, T, needles, ks, {"c5": np.arange(64)})
    text2, T2, needles2, _, _ = _planted(spm, ctx, n, [2048], 8, 100, seed=0xA11C0003)
    ks2 = np.array([100 - 12 * i for i in range(8)])
    res2 = _run_sets(spm, ctx, text2, T2, needles2, ks2, {"l2048": np.arange(8)})
    assert len(res["c5"][0][1]) >= 64 and len(res2["l2048"][0][1]) >= 8
    ps2 = ctx.patterns(spm.ALGO_MYERS, needles2, k=ks2)  # (the set must outlive the align call)
    h = spm.scan(ctx, text2, ps2, engine=spm.ENGINE_BRUTE)
    st = _align(h)[2]
    h.close()
    ps2.close()
    assert st.begin_wave == st.n_alns and st.cigar_wave > 0 and st.cigar_wave_global > 0


@pytest.mark.gpu
def test_boundaries(spm, ctx):
    rng = np.random.default_rng(11)
    n = 1 << 18
    T = rng.integers(0, 4, n, dtype=np.uint8)
    L, k = 100, 6
    needles, starts = [], []
    for i in range(64):
        at = int(rng.integers(1000, n - 2000))
        nd = T[at:at + L].copy()
        nd[rng.integers(0, L, 3)] = rng.integers(0, 4, 3)
        needles.append(np.delete(nd, [10, 50]) if i % 2 else np.insert(nd, 20, 2))
        starts.append(at)
    tx = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    # left_context = 0 with begin > 0: a scan that starts inside planted occurrences (clipped alignments)
    for b0 in (starts[0] + 2, starts[1] + 1):
        h = spm.scan(ctx, tx, ps, begin=b0, engine=spm.ENGINE_BRUTE)
        hv = h.view()
        rec, ops, _ = _align(h)
        _check_all(T, needles, hv, rec, ops, lambda ends: np.full(len(ends), b0))
        assert np.any(rec["begin"] == b0), "no alignment clipped at the scan's begin"
        h.close()
    # left_context = 1 with pos_offset != 0: lo is 0, positions shifted
    off = 1 << 40
    for engine in (spm.ENGINE_BRUTE, spm.ENGINE_FILTER):
        h = spm.scan(ctx, tx, ps, begin=n // 2, engine=engine, left_context=True, pos_offset=off)
        hv = h.view()
        rec, ops, _ = _align(h)
        hv2 = hv.copy()
        hv2["pos"] -= off
        rec2 = rec.copy()
        rec2["begin"] -= off
        rec2["end"] -= off
        _check_all(T, needles, hv2, rec2, ops, lambda ends: np.zeros(len(ends), np.int64))
        h.close()
    # segments: alignments clipped at segment starts
    segs = np.array([0] + [s + 1 for s in starts[:16]] + [n], dtype=np.uint64)
    segs = np.unique(segs)
    h = spm.scan_segments(ctx, tx, ps, segs, engine=spm.ENGINE_BRUTE)
    hv = h.view()
    rec, ops, _ = _align(h)
    seg_lo = lambda ends: segs[np.searchsorted(segs, ends - 1, side="right") - 1].astype(np.int64)  # noqa: E731
    _check_all(T, needles, hv, rec, ops, seg_lo)
    assert np.any(np.isin(rec["begin"], segs[1:-1])), "no alignment clipped at a segment start"
    h.close()
    # a deferred scan: align completes it
    h = spm.scan(ctx, tx, ps, engine=spm.ENGINE_FILTER, flags=spm.SCAN_DEFER)
    rec, ops, _ = _align(h)
    hv = h.view()
    _check_all(T, needles, hv, rec, ops, lambda ends: np.zeros(len(ends), np.int64))
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [5, 15])
def test_dna5_dna15(spm, ctx, sigma):
    rng = np.random.default_rng(sigma)
    n = 1 << 18
    T = rng.integers(0, sigma, n, dtype=np.uint8)
    needles = []
    for i in range(48):
        at = int(rng.integers(0, n - 300))
        L = [40, 90, 130, 300][i % 4]
        nd = T[at:at + L].copy()
        nd[rng.integers(0, L, 2)] = rng.integers(0, sigma, 2)
        needles.append(np.delete(nd, [L // 3]))
    tx = ctx.upload(T, sigma=sigma)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=4, sigma=sigma)
    h = spm.scan(ctx, tx, ps, engine=spm.ENGINE_BRUTE)
    hv = h.view()
    rec, ops, _ = _align(h)
    assert len(hv) >= 48
    _check_all(T, needles, hv, rec, ops, lambda ends: np.zeros(len(ends), np.int64))
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["SHIFTOR", "HORSPOOL"])
def test_exact_sets_and_begin_only(spm, ctx, algo):
    rng = np.random.default_rng(3)
    n = 1 << 20
    T = rng.integers(0, 4, n, dtype=np.uint8)
    needles = [T[a:a + 32].copy() for a in rng.integers(0, n - 64, 100)]
    tx = ctx.upload(T)
    ps = ctx.patterns(getattr(spm, "ALGO_" + algo), needles)
    h = spm.scan(ctx, tx, ps)
    hv = h.view()
    rec, ops, _ = _align(h)
    assert np.array_equal(rec["begin"], hv["pos"]) and np.array_equal(rec["end"], hv["pos"] + 32)
    assert np.all(rec["cigar_len"] == 1) and np.all(ops[rec["cigar_off"]] == (32 << 4 | 7))
    rb, ob, _ = _align(h, begin_only=True)
    assert np.array_equal(rb["begin"], rec["begin"]) and np.all(rb["cigar_len"] == 0) and len(ob) == 0
    h.close()
    # Myers: begin-only gives the same begins
    ps2 = ctx.patterns(spm.ALGO_MYERS, [np.delete(x, 5) for x in needles], k=2)
    h = spm.scan(ctx, tx, ps2)
    rec, _, _ = _align(h)
    rb, ob, st = _align(h, begin_only=True)
    assert np.array_equal(rb["begin"], rec["begin"]) and np.all(rb["cigar_len"] == 0) and len(ob) == 0
    assert st.n_ops == 0
    h.close()


@pytest.mark.gpu
def test_refusals(spm, ctx):
    rng = np.random.default_rng(5)
    n = 1 << 16
    T = rng.integers(0, 4, n, dtype=np.uint8)
    tx = ctx.upload(T)
    needles = [T[100:140].copy(), T[5000:5040].copy()]
    ps = ctx.patterns(spm.ALGO_MYERS_PREFIX, needles, k=2)
    h = spm.scan(ctx, tx, ps)
    with pytest.raises(spm.SpmError, match=r"error -4: .*PREFIX"):
        h.align()
    h.close()
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=2)
    h, _ = spm.scan(ctx, tx, ps, state_in=ps.initial_state(), want_state=True)
    with pytest.raises(spm.SpmError, match=r"error -4: .*stateful"):
        h.align()
    h.close()
    ps = ctx.patterns(spm.ALGO_MYERS, [T[:8].copy()], k=3)
    h = spm.scan(ctx, tx, ps, max_hits=4, engine=spm.ENGINE_BRUTE)
    with pytest.raises(spm.SpmError, match=r"error -5: .*max_hits"):
        h.align()
    h.close()


@pytest.mark.gpu
def test_scale_c4_shape(spm, ctx):
    n = 256 << 20
    seed = 0x5EED0001
    text = ctx.generate(seed, 0, n)
    mat = np.stack([spm.synth_pattern(seed, 0x5EED0003, n, p, 150, 3)[0] for p in range(100_000)])
    ps = ctx.patterns(spm.ALGO_MYERS, mat, k=3)
    h = spm.scan(ctx, text, ps, max_hits=1 << 21)
    hv = h.view()
    rec, ops, st = _align(h)
    h.close()
    assert len(hv) >= 100_000 and st.n_alns == len(hv)
    assert np.array_equal(rec["end"], hv["pos"]) and np.array_equal(rec["score"], hv["score"])
    # every transcript: vectorised run-level checks (lengths consumed, cost)
    L = (ops >> 4).astype(np.int64)
    op = ops & 15
    nz = rec["cigar_len"] > 0
    assert np.all(nz)
    lens = rec["cigar_len"].astype(np.int64)
    rid = np.repeat(np.arange(len(rec)), lens)
    sel = np.repeat(rec["cigar_off"].astype(np.int64), lens) + np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
    Ls, os_ = L[sel], op[sel]
    assert np.all(Ls > 0) and np.all(np.isin(os_, [1, 2, 7, 8]))
    q = np.bincount(rid, weights=Ls * np.isin(os_, [1, 7, 8]), minlength=len(rec))
    r = np.bincount(rid, weights=Ls * np.isin(os_, [2, 7, 8]), minlength=len(rec))
    c = np.bincount(rid, weights=Ls * np.isin(os_, [1, 2, 8]), minlength=len(rec))
    assert np.all(q == 150)
    assert np.array_equal(r.astype(np.int64), (rec["end"] - rec["begin"]).astype(np.int64))
    assert np.array_equal(c.astype(np.int64), rec["score"].astype(np.int64))
    # every = / X run against the symbols, vectorised in chunks of records (positions of each run's first symbols)
    Tall = text.download(0, n)
    flat = mat.reshape(-1)
    m_all = mat.shape[1]
    q_len = np.where(np.isin(os_, [1, 7, 8]), Ls, 0)
    r_len = np.where(np.isin(os_, [2, 7, 8]), Ls, 0)
    first = np.repeat(np.cumsum(lens) - lens, lens)              # index of each run's record's first run
    q0 = np.cumsum(q_len) - q_len
    r0 = np.cumsum(r_len) - r_len
    q0 -= q0[first]                                              # needle offset of each run inside its record
    r0 -= r0[first]                                              # text offset
    diag = np.nonzero(np.isin(os_, [7, 8]))[0]
    for c0 in range(0, len(diag), 1 << 18):
        rr = diag[c0:c0 + (1 << 18)]
        n_sym = Ls[rr]
        base_q = np.repeat(rec["pattern"][rid[rr]].astype(np.int64) * m_all + q0[rr], n_sym)
        base_t = np.repeat(rec["begin"][rid[rr]].astype(np.int64) + r0[rr], n_sym)
        step = np.arange(n_sym.sum()) - np.repeat(np.cumsum(n_sym) - n_sym, n_sym)
        eq = flat[base_q + step] == Tall[base_t + step]
        want_eq = np.repeat(os_[rr] == 7, n_sym)
        assert np.array_equal(eq, want_eq), "an = / X run disagrees with the symbols"
    del Tall
    # symbol-level replay and DP begins on a 20 000-hit sample
    rng = np.random.default_rng(1)
    samp = np.sort(rng.choice(len(rec), size=min(20_000, len(rec)), replace=False))
    lo_b, hi_b = max(0, int(rec["begin"][samp].min()) - 512), int(rec["end"][samp].max())
    T = text.download(lo_b, hi_b - lo_b)
    pats = rec["pattern"][samp]
    want = ref_begins(T, mat, pats, hv["pos"][samp].astype(np.int64) - lo_b, hv["score"][samp],
                      np.full(len(samp), -lo_b, np.int64))
    assert np.array_equal(rec["begin"][samp].astype(np.int64) - lo_b, want)
    for s in samp[:2000]:
        o = int(rec["cigar_off"][s])
        replay(mat[rec["pattern"][s]], T, int(rec["begin"][s]) - lo_b, int(rec["end"][s]) - lo_b,
               ops[o:o + int(rec["cigar_len"][s])], int(rec["score"][s]))


@pytest.mark.gpu
def test_cpp_locate_matches_python(spm, ctx, tmp_path):
    exe = _build_locate(tmp_path)
    n = 1 << 20
    text, T, needles, _, _ = _planted(spm, ctx, n, [100], 64, 3, seed=0xA11C0004)
    L, k = 100, 3
    (tmp_path / "t.bin").write_bytes(T.tobytes())
    (tmp_path / "n.bin").write_bytes(np.concatenate(needles).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "t.bin"), str(tmp_path / "n.bin"), str(L), str(k)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "MISMATCH" not in r.stdout
    rows = [x.split() for x in lines if x and not x.startswith("single")]
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    h = spm.scan(ctx, text, ps)
    hv = h.view()
    a = h.align()
    rec, ops = a.view(), a.ops
    assert len(rows) == len(rec)
    indel = 0
    for i, row in enumerate(rows):
        p, b, e, err, cg, plain = int(row[0]), int(row[1]), int(row[2]), int(row[3]), row[4], int(row[5])
        assert (p, b, e, err) == (int(rec["pattern"][i]), int(rec["begin"][i]), int(rec["end"][i]), int(rec["score"][i]))
        assert cg == a.cigar(i, rec, ops)
        assert plain == max(0, e - L)
        if "I" in cg or "D" in cg:
            indel += 1
        if e - b != L:
            assert b != plain, "a hit whose span differs from |P| must differ from end - |P|"
    assert indel > 0 and any(int(r_[1]) != int(r_[5]) for r_ in rows)
    a.close()
    h.close()
