"""Worst-case occurrences for the seed filter (a helper module of tests/test_seed_edges.py and tests/test_gpu_seed_edges.py,
not a test file).

The filter rests on the pigeonhole argument: an occurrence with at most k edits leaves one of the needle's k + 1 seeds
intact (two of k + 2 when k >= 8).  A *worst-case occurrence* is one that leaves exactly that and nothing more: one edit
inside every seed but the kept one(s).  Losing the kept seed's key window -- at one text phase, at one border of the
streaming kernels -- loses the occurrence, with no second seed to hide the loss.  The generator places such occurrences
so that the kept seed starts at every phase around every kind of border.
"""
from __future__ import annotations

import numpy as np

LAYOUTS = ("mid", "hug", "ins", "del")
DNA4 = (0, 1, 2, 3)
DNA5 = (0, 1, 2, 4)       # A C G T; 3 is N
DNA15 = (0, 2, 4, 11)     # A C G T; every other code stands in for N
PLANT_GAP = 1024          # plants sit at least this far apart


def plan(m: int, k: int):
    """(n, q): the seeds of a needle -- n pieces of q symbols, piece j = [j q, (j + 1) q).  Mirrors plan_seeds
    (libspm_amd/csrc/filter_shared.hpp)."""
    n = k + 2 if (8 <= k <= 1000 and m // (k + 2) >= 9) else k + 1
    return n, m // n


def keeps(m: int, k: int):
    """The sets of kept pieces: every single piece for k + 1 plans; for k + 2 plans every adjacent pair and (0, n - 1)."""
    n, _ = plan(m, k)
    if n == k + 1:
        return [(j,) for j in range(n)]
    return [(j, j + 1) for j in range(n - 1)] + [(0, n - 1)]


def layouts(k: int):
    return LAYOUTS if k > 0 else ("mid",)     # (no edits: the four layouts are one)


def _other(rng, alphabet, *avoid):
    c = [a for a in alphabet if a not in avoid]
    assert c, "no symbol left"
    return c[int(rng.integers(0, len(c)))]


def occurrence(P, k: int, keep, layout: str, rng=None, alphabet=DNA4, edit_symbol=None, check=True):
    """The text spelling of needle P with exactly k edits, one inside every piece not in `keep`.

    Returns (occ, at): the symbols, and at[j] = where piece j of `keep` starts inside occ.
    edit_symbol: {piece: symbol} -- the substitution of that killed piece writes this symbol (an N next to the seed)."""
    P = np.asarray(P, dtype=np.uint8)
    m = len(P)
    n, q = plan(m, k)
    keep = tuple(keep)
    assert layout in LAYOUTS and len(keep) == n - k and all(0 <= j < n for j in keep) and len(set(keep)) == len(keep)
    rng = rng or np.random.default_rng(0)
    edit_symbol = edit_symbol or {}
    out, at, edits = [], {}, 0
    for j in range(n + 1):
        piece = P[j * q:(j + 1) * q] if j < n else P[n * q:]      # (j == n: what m / n leaves over, never edited)
        piece = [int(x) for x in piece]
        if j in keep:
            at[j] = sum(len(x) for x in out)
        elif j < n:
            mid = q // 2
            if layout in ("mid", "hug") or j in edit_symbol:
                i = mid
                if layout == "hug":
                    right, left = j + 1 in keep, j - 1 in keep
                    assert not (right and left), "a killed piece between two kept ones has one edit only"
                    i = q - 1 if right else 0 if left else mid
                piece[i] = edit_symbol.get(j, _other(rng, alphabet, piece[i]))
                assert piece[i] != int(P[j * q + i])
            elif layout == "ins":     # a text symbol the needle lacks, unlike both neighbours
                piece.insert(mid, _other(rng, alphabet, piece[mid - 1], piece[mid]))
            else:                     # del: a needle symbol the text lacks
                del piece[mid]
            edits += 1
        out.append(piece)
    assert edits == k
    occ = np.array([x for piece in out for x in piece], dtype=np.uint8)
    if check:
        check_occurrence(P, k, keep, occ, at)
    return occ, at


def check_occurrence(P, k, keep, occ, at):
    """The invariants of a worst-case occurrence, on the symbols: every kept piece is intact at its intended place, every
    other piece is intact nowhere within +-k of its place (its place: on the diagonal of the nearest kept piece)."""
    m = len(P)
    n, q = plan(m, k)
    P = np.asarray(P, dtype=np.uint8)
    for j in keep:
        assert np.array_equal(occ[at[j]:at[j] + q], P[j * q:(j + 1) * q]), ("kept piece not intact", j)
    for j in range(n):
        if j in keep:
            continue
        # the diagonal of kept piece a puts piece j at at[a] + (j - a) q
        places = [at[a] + (j - a) * q for a in keep]
        lo, hi = max(0, min(places) - k), min(len(occ) - q, max(places) + k)
        if lo <= hi:
            found = (np.lib.stride_tricks.sliding_window_view(occ[lo:hi + q], q) == P[j * q:(j + 1) * q]).all(axis=1)
            if found.any():
                raise NotWorstCase(("killed piece intact", j, lo + int(np.argmax(found))))


class NotWorstCase(AssertionError):
    """A killed piece is intact after all: the needle repeats itself there.  (Nothing else about a draw may be wrong.)"""


class Case:
    __slots__ = ("pattern", "keep", "layout", "cls", "border", "phase", "start", "end", "k", "m")

    def __repr__(self):
        return (f"case(pattern={self.pattern}, keep={self.keep}, {self.layout}, border {self.cls}={self.border}, "
                f"phase {self.phase}, [{self.start}, {self.end}))")


def phases(q: int):
    return range(-(q + 16), 16)


def combos(m: int, k: int, only_layouts=None, only_phases=None):
    """(keep, layout, phase) of one border class: every kept set x every layout x every phase, unless the caller names the
    layouts (the N tests: `hug`) or the phases (the CPU tests compare with a whole-text oracle on a short text)."""
    _, q = plan(m, k)
    return [(kp, lay, d) for kp in keeps(m, k) for lay in (only_layouts or layouts(k)) for d in (only_phases or phases(q))]


def text_length(n_combos: int, span: int):
    return (n_combos + 2) * span


# (chunk of border b, chunk of border a) inside a span of 8 chunks: b runs over every inner multiple of 1 KiB that leaves
# the plants 1 KiB apart -- borders inside a group of 2 or 4 chunks (3, 5) and between groups (2, 4, 6)
_BA = ((2, 5), (3, 5), (4, 2), (5, 2), (6, 3))


def borders(i: int, span: int, classes):
    """Combination i owns the span that starts at (i + 1) span: its border of every class.
    a: a multiple of 16, no multiple of 1024;  b: a multiple of 1024 that is no span border (with class d in use: and no
    multiple of 4096);  c: the span border;  d: a multiple of 4096 that is no span border (the p-chunks of the packed
    shadow: the third and the fourth of a span in turn)."""
    base = (i + 1) * span
    assert span % 8192 == 0 and ("d" not in classes or span >= 16384)
    pairs = [x for x in _BA if x[0] != 4] if "d" in classes else _BA
    b, a = pairs[i % len(pairs)]
    at = {"c": base, "b": base + 1024 * b, "a": base + 1024 * a + 16 * (1 + i % 31), "d": base + 8192 + 4096 * (i % 2)}
    assert at["a"] % 16 == 0 and at["a"] % 1024 and at["b"] % 1024 == 0 and at["b"] % span
    assert "d" not in classes or (at["b"] % 4096 and at["d"] % 4096 == 0 and at["d"] % span)
    return {c: at[c] for c in classes}


def lay_out(m: int, k: int, span: int, classes=("a", "b", "c"), seed=1, alphabet=DNA4, decorate=None, edit_for=None,
            only_layouts=None, only_phases=None):
    """A uniform random text with one needle per case: case = (kept piece(s), layout, border, phase); the first kept piece
    starts at border + phase.  Returns (T, needles, cases).

    decorate(T, case, occ, at, q): called after a plant is written (the dna5 / dna15 tests put an N beside it);
    edit_for(keep) -> {piece: symbol}: see occurrence()."""
    rng = np.random.default_rng(seed)
    n, q = plan(m, k)
    todo = combos(m, k, only_layouts, only_phases)
    L = text_length(len(todo), span)
    alpha = np.array(alphabet, dtype=np.uint8)
    T = alpha[rng.integers(0, 4, L)]
    needles, cases, last_end = [], [], 0
    for i, (kp, lay, d) in enumerate(todo):
        for cls, B in sorted(borders(i, span, classes).items(), key=lambda x: x[1]):
            # a needle that repeats itself (a run of one symbol across a piece's middle) keeps the piece intact beside an
            # indel: such a draw is no worst case for this layout.  The case stays; the needle is drawn again.
            for attempt in range(8):
                P = alpha[rng.integers(0, 4, m)]
                occ, at = occurrence(P, k, kp, lay, rng, alphabet, edit_for(kp) if edit_for else None, check=False)
                try:
                    check_occurrence(P, k, kp, occ, at)
                    break
                except NotWorstCase:
                    assert attempt < 7, "no worst-case needle in eight draws"
            c = Case()
            c.pattern, c.keep, c.layout, c.cls, c.border, c.phase, c.k, c.m = len(needles), kp, lay, cls, B, d, k, m
            c.start = B + d - at[kp[0]]
            c.end = c.start + len(occ)
            assert c.start >= last_end + PLANT_GAP and c.start >= 2 * m and c.end + 2 * m <= L, c
            T[c.start:c.end] = occ
            assert np.array_equal(T[B + d:B + d + q], P[kp[0] * q:(kp[0] + 1) * q])
            if decorate:
                decorate(T, c, occ, at, q)
            last_end = c.end
            needles.append(P)
            cases.append(c)
    assert len(cases) == len(todo) * len(classes)       # no case skipped
    return T, needles, cases


def window(c: Case, L: int):
    """The oracle's window of a case: [ws, we) = [start - 2m, end + 2m); its hits with pos >= m + k (pos in the window) are
    exact -- a cold start there reports what a scan of the whole text reports."""
    ws, we = c.start - 2 * c.m, c.end + 2 * c.m
    assert 0 <= ws and we <= L
    return ws, we
