"""CPU: the generator of worst-case occurrences (tests/seed_edges.py) that tests/test_gpu_seed_edges.py sweeps the seed
filter with.  For every (needle length, k, layout) used there: every kept piece is intact at its intended place and every
other piece is intact nowhere within +-k of its place (checked on the symbols), the oracle reports the plant, and the
oracle on a window around the plant reports what the oracle on the whole text reports -- which is what makes the cheap
window a legitimate reference on the GPU side."""
import numpy as np
import pytest

import seed_edges as E

# (m, k, alphabet, sigma): every shape of test_gpu_seed_edges.py
SHAPES = [(100, 3, E.DNA4, 4), (80, 3, E.DNA4, 4), (60, 3, E.DNA4, 4), (68, 3, E.DNA4, 4), (48, 3, E.DNA4, 4),
          (44, 3, E.DNA4, 4), (150, 3, E.DNA4, 4), (150, 8, E.DNA4, 4), (128, 7, E.DNA4, 4), (32, 0, E.DNA4, 4),
          (100, 3, E.DNA5, 5), (48, 3, E.DNA5, 5), (100, 3, E.DNA15, 15), (48, 3, E.DNA15, 15)]


def test_plan_mirrors_plan_seeds():
    assert E.plan(100, 3) == (4, 25) and E.plan(32, 0) == (1, 32) and E.plan(128, 7) == (8, 16) and E.plan(44, 3) == (4, 11)
    assert E.plan(150, 8) == (10, 15) and E.plan(1024, 64) == (66, 15)      # k >= 8: k + 2 seeds ...
    assert E.plan(80, 8) == (9, 8) and E.plan(89, 8) == (9, 9) and E.plan(90, 8) == (10, 9) and E.plan(99, 9) == (11, 9)    # ... if they keep 9 symbols
    assert E.keeps(100, 3) == [(0,), (1,), (2,), (3,)]
    assert E.keeps(150, 8) == [(j, j + 1) for j in range(9)] + [(0, 9)]
    assert list(E.phases(25)) == list(range(-41, 16))


@pytest.mark.parametrize("m,k,alphabet,sigma", SHAPES)
def test_occurrences_keep_exactly_the_kept_pieces(oracle, m, k, alphabet, sigma):
    rng = np.random.default_rng(m * 131 + k)
    n, q = E.plan(m, k)
    alpha = np.array(alphabet, dtype=np.uint8)
    for kp in E.keeps(m, k):
        for lay in E.layouts(k):
            for _ in range(8):
                P = alpha[rng.integers(0, 4, m)]
                occ, at = E.occurrence(P, k, kp, lay, rng, alphabet)     # (asserts the invariants: check_occurrence)
                assert len(occ) == m + {"ins": k, "del": -k}.get(lay, 0)
                assert sorted(at) == sorted(kp)
                if lay in ("mid", "hug"):
                    assert int(np.count_nonzero(occ != P)) == k and all(at[j] == j * q for j in kp)
                if lay == "hug" and k:
                    # the intact stretch around a kept piece is exactly the piece
                    for j in kp:
                        if j > 0 and j - 1 not in kp:
                            assert occ[j * q - 1] != P[j * q - 1]
                        if j + 1 < n and j + 1 not in kp:
                            assert occ[(j + 1) * q] != P[(j + 1) * q]
                # the diagonal of the first kept piece is displaced by the indels in front of it, up to k
                shift = at[kp[0]] - kp[0] * q
                before = sum(1 for j in range(kp[0]) if j not in kp)
                assert shift == {"ins": before, "del": -before}.get(lay, 0)
                # edit distance: the oracle finds the needle at the end of the occurrence, with at most k errors
                hits = oracle.myers(np.concatenate([occ]), P, k, sigma=sigma)
                assert any(int(h["pos"]) == len(occ) and int(h["score"]) <= k for h in hits)
    # an N as the edit beside the kept piece (dna5 / dna15): still exactly k edits, the neighbours of the seed are the Ns
    if sigma != 4 and k and n * q == m:
        N = 3 if sigma == 5 else 8
        for j in range(n):
            P = alpha[rng.integers(0, 4, m)]
            occ, at = E.occurrence(P, k, (j,), "hug", rng, alphabet, {x: N for x in (j - 1, j + 1) if 0 <= x < n})
            assert int(np.count_nonzero(occ != P)) == k
            assert (j == 0 or occ[j * q - 1] == N) and (j == n - 1 or occ[(j + 1) * q] == N)


@pytest.mark.parametrize("m,k,alphabet,sigma", SHAPES)
def test_layout_places_every_case_and_the_oracle_reports_it(oracle, m, k, alphabet, sigma):
    """The full layout the GPU sweep uses (spans of 8 KiB; with the packed shadow's borders: 16 KiB): every case present,
    at its border and phase, reported by the windowed oracle at its end with score <= k."""
    n, q = E.plan(m, k)
    classes = ("a", "b", "c", "d") if (m, k, sigma) == (100, 3, 4) else ("a", "b", "c")
    span = 16384 if "d" in classes else 8192
    T, needles, cases = E.lay_out(m, k, span, classes, seed=7, alphabet=alphabet)
    assert len(cases) == len(needles) == len(E.keeps(m, k)) * len(E.layouts(k)) * (q + 32) * len(classes)
    assert len(T) <= 16 << 20
    seen = set()
    for c in cases:
        seen.add((c.keep, c.layout, c.cls, c.phase))
        B = c.border
        assert {"a": B % 16 == 0 and B % 1024 != 0, "b": B % 1024 == 0 and B % span != 0, "c": B % span == 0,
                "d": B % 4096 == 0 and B % span != 0}[c.cls]
        j = c.keep[0]
        assert np.array_equal(T[B + c.phase:B + c.phase + q], needles[c.pattern][j * q:(j + 1) * q])
        ws, we = E.window(c, len(T))
        hits = oracle.myers(T[ws:we], needles[c.pattern], k, sigma=sigma)
        assert any(int(h["pos"]) + ws == c.end and int(h["score"]) <= k for h in hits), c
    assert len(seen) == len(cases)
    # class b covers the chunk borders inside a group of 2 or 4 chunks and those between groups; class d two p-chunks
    inner = {c.border % span // 1024 for c in cases if c.cls == "b"}
    assert inner == ({2, 3, 5, 6} if "d" in classes else {2, 3, 4, 5, 6})
    assert "d" not in classes or {c.border % span for c in cases if c.cls == "d"} == {8192, 12288}


@pytest.mark.parametrize("m,k,alphabet,sigma", SHAPES)
def test_windowed_oracle_equals_whole_text_oracle(oracle, m, k, alphabet, sigma):
    """On a short text (two phases per kept set and layout, all border classes) the whole-text oracle is affordable: for
    every needle its hits with end in [ws + m + k, we] are the windowed oracle's hits with pos >= m + k."""
    T, needles, cases = E.lay_out(m, k, 16384, ("a", "b", "c", "d"), seed=11, alphabet=alphabet, only_phases=(-1, 0))
    whole = oracle.scan_multi(oracle.MYERS, T, needles, k=k, sigma=sigma, threads=4)
    assert len(whole) >= len(cases)
    for c in cases:
        ws, we = E.window(c, len(T))
        w = oracle.myers(T[ws:we], needles[c.pattern], k, sigma=sigma)
        w = w[w["pos"] >= m + k]
        mine = whole[(whole["pattern"] == c.pattern) & (whole["pos"] >= ws + m + k) & (whole["pos"] <= we)]
        assert np.array_equal(mine["pos"], w["pos"] + ws) and np.array_equal(mine["score"], w["score"]), c
        assert c.end in set(int(x) for x in mine["pos"])
