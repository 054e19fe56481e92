"""CPU: the reference side of the matcher state blobs (oracle/states.py) pinned to definitions, so that the GPU state tests
(test_gpu_states.py) can compare the product's blobs with something outside the product.

* the fast oracle's resumable Myers state (variant 1, every block) == the Sellers DP column carried across the same ragged
  chunks, infix and prefix mode, |P| around every 64-bit word border up to SPM_MAX_NEEDLE;
* the oracle's resumable Shift-Or register == its definition (bit j clear iff P[0..j] equals the last j + 1 symbols);
* the blob encoder and decoder against the layout include/spm_hip.h documents."""
import numpy as np
import pytest

MS = [1, 63, 64, 65, 127, 128, 129, 1024, 2047, 2048]


def _cuts(rng, n, m):
    """Ragged cut points of [0, n): chunks of 0 and 1 symbols, of |P| - 1, |P|, |P| + 1, and random ones."""
    sizes = [0, 1, max(0, m - 1), m, m + 1, 0, 1]
    cuts = [0]
    for s in sizes:
        cuts.append(min(n, cuts[-1] + s))
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + int(rng.integers(1, 2 * m + 40))))
    return cuts


def _text_with_occurrences(rng, pat, n):
    """Random dna4 text with the needle planted exactly, with a substitution, and with |P|/4 + 1 insertions."""
    m = len(pat)
    T = rng.integers(0, 4, n, dtype=np.uint8)
    ins = pat.copy()
    for j in sorted(rng.choice(m + 1, size=m // 4 + 1, replace=True))[::-1]:
        ins = np.insert(ins, j, rng.integers(0, 4))
    sub = pat.copy()
    sub[m // 2] = (sub[m // 2] + 1) & 3
    at = 0
    for piece in (pat, sub, ins):
        at += int(rng.integers(5, 40))
        if at + len(piece) > n:
            break
        T[at:at + len(piece)] = piece
        at += len(piece)
    return T


@pytest.mark.parametrize("mode", ["infix", "prefix"])
@pytest.mark.parametrize("m", MS)
def test_oracle_myers_state_equals_sellers_column(oracle, m, mode):
    from oracle import states as ST
    md = oracle.INFIX if mode == "infix" else oracle.PREFIX
    rng = np.random.default_rng(31 * m + md)
    P = rng.integers(0, 4, m, dtype=np.uint8)
    n = 3 * m + 600 if mode == "infix" else 2 * m + 200
    T = _text_with_occurrences(rng, P, n)
    for k in sorted({0, min(3, m), m // 3, m - 1 if m > 1 else 0, m, m + 2}):
        st = oracle.myers_state(m, k)
        col = ST.initial_column(m)
        assert ST.record_from_oracle(st, m) == ST.record_from_column(col)
        cuts = _cuts(rng, n, m)
        n_hits = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            got = oracle.myers(T[a:b], P, k, mode=md, variant=1, state=st, text_offset=a)
            want, col = ST.sellers_column(T[a:b], P, k, mode=md, col=col, text_offset=a)
            assert np.array_equal(got, want), (k, a, b)
            rec = ST.record_from_oracle(st, m)
            assert rec == ST.record_from_column(col), (k, a, b)
            assert np.array_equal(ST.column_from_record(rec, m), col)
            if md == oracle.PREFIX:
                assert col[0] == b  # row 0 of a prefix column counts the symbols read
            n_hits += len(got)
        if k >= m and mode == "infix":
            assert n_hits == n
        elif k > 0 and mode == "infix":
            assert n_hits >= 2


@pytest.mark.parametrize("m", MS)
def test_oracle_myers_restores_a_sellers_column(oracle, m):
    """A column the oracle did not compute, turned into a MyersState, continues exactly like Sellers from it."""
    from oracle import states as ST
    rng = np.random.default_rng(7 + m)
    P = rng.integers(0, 4, m, dtype=np.uint8)
    k = max(0, m // 4)
    for md in (oracle.INFIX, oracle.PREFIX):
        X = _text_with_occurrences(rng, P, m + 300)
        _, col = ST.sellers_column(X, P, k, mode=md)
        st = ST.oracle_from_record(ST.record_from_column(col), m, k)
        Y = _text_with_occurrences(rng, P, 2 * m + 100)
        got = oracle.myers(Y, P, k, mode=md, variant=1, state=st, text_offset=len(X))
        want, col = ST.sellers_column(Y, P, k, mode=md, col=col, text_offset=len(X))
        assert np.array_equal(got, want)
        assert ST.record_from_oracle(st, m) == ST.record_from_column(col)


@pytest.mark.parametrize("m", [1, 5, 31, 32, 33, 64, 100, 512, 513, 1025, 2048])
def test_oracle_shiftor_state_equals_definition(oracle, m):
    from oracle import states as ST
    rng = np.random.default_rng(500 + m)
    P = rng.integers(0, 4, m, dtype=np.uint8)
    if m > 4:
        P[: m // 2] = P[0]  # a long run: many rows clear at once
    n = 3 * m + 300
    T = rng.integers(0, 4, n, dtype=np.uint8)
    for at in (17, m + 60, 2 * m + 100):
        if at + m <= n:
            T[at:at + m] = P
    T[n - m // 2:] = P[:m // 2]  # a partial occurrence at the end: low rows clear in the last state
    state = oracle.shiftor_state(m)
    assert ST.shiftor_oracle_register(state) == ST.shiftor_register(T[:0], P)
    n_hits = 0
    cuts = _cuts(rng, n, m)
    for a, b in zip(cuts[:-1], cuts[1:]):
        got = oracle.shiftor(T[a:b], P, state=state, text_offset=a)
        want = oracle.naive_exact(T[:b], P)
        want = want[want + m > a]
        assert np.array_equal(got, want)
        assert ST.shiftor_oracle_register(state) == ST.shiftor_register(T[:b], P), (a, b)
        n_hits += len(got)
    assert n_hits >= 1
    r = ST.shiftor_register(T, P)
    assert r & ((1 << m) - 1) != (1 << m) - 1 or m == 1


def test_blob_layout_round_trip(oracle):
    """Encoder and decoder agree with each other and with the documented layout: set-wide n_words, strides, offsets."""
    from oracle import states as ST
    rng = np.random.default_rng(3)
    assert [ST.n_words(ST.ALGO_MYERS, m) for m in (1, 64, 65, 2048)] == [1, 1, 2, 32]
    assert [ST.n_words(ST.ALGO_SHIFTOR, m) for m in (1, 32, 33, 2048)] == [1, 1, 2, 64]
    assert ST.stride(ST.ALGO_MYERS, 65) == 8 + 2 * 16
    assert ST.stride(ST.ALGO_SHIFTOR, 65) == 8 + 4 * 4  # 3 words, padded to an even count
    assert ST.stride(ST.ALGO_SHIFTOR, 64) == 8 + 4 * 2
    for algo in (ST.ALGO_MYERS, ST.ALGO_MYERS_PREFIX, ST.ALGO_SHIFTOR):
        lengths = [1, 5, 70, 130]
        mx = max(lengths)
        nw = ST.n_words(algo, mx)
        recs = []
        for m in lengths:
            if ST.is_myers(algo):
                col = np.cumsum(np.concatenate([[int(rng.integers(0, 9))], rng.integers(-1, 2, m)])).astype(np.int32)
                recs.append(dict(ST.record_from_column(col), n_words=nw))
                assert np.array_equal(ST.column_from_record(recs[-1], m), col)
            else:
                recs.append({"n_words": nw, "pad": 0, "r": int(rng.integers(0, 1 << 62)) | (((1 << (32 * nw)) - 1) ^ ((1 << m) - 1))})
        blob = ST.encode(recs, algo, mx)
        assert len(blob) == ST.stride(algo, mx) * len(lengths)
        assert ST.decode(blob, algo, len(lengths), mx) == recs
        # field offsets of record 1, by hand
        st = ST.stride(algo, mx)
        r1 = blob[st:2 * st]
        if ST.is_myers(algo):
            assert r1[0:4].view(np.int32)[0] == recs[1]["score"] and r1[4:8].view(np.uint32)[0] == nw
            assert int(r1[8:16].view(np.uint64)[0]) == recs[1]["vp"] & ((1 << 64) - 1)
            assert int(r1[8 + 8 * nw:16 + 8 * nw].view(np.uint64)[0]) == recs[1]["vn"] & ((1 << 64) - 1)
        else:
            assert r1[0:4].view(np.uint32)[0] == nw
            assert int(r1[8:12].view(np.uint32)[0]) == recs[1]["r"] & 0xFFFFFFFF
