"""Pan-genome alignments in reference coordinates (spm_hip_jst_alns_project, JstAlignments.project).

The expected answer never comes from the code under test:
  (a) the NumPy reference of this file builds the explicit column list of the alignment haplotype ~ reference (the journal:
      paired, inserted and deleted columns) and composes the transcript's columns over it;
  (b) every projected transcript is replayed, independently of (a), against ref[ref_begin, ref_end) with the replayer of
      test_align: it consumes exactly P and that stretch, = / X agree with the symbols, runs are merged, cost = ref_score.
"""
import ctypes

import numpy as np
import pytest

from cpp_programs import c_layout, download
from test_align import replay
from test_gpu_jst import _apply, _random_alleles

INS, DEL, EQ, X = 1, 2, 7, 8

# ---------------------------------------------------------------------------------------------------------------------
# CPU: layout
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define F(f) printf("%s %zu\n", #f, offsetof(spm_jst_ref_aln, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_jst_project_stats, f))
int main(void)
{
    F(ref_begin); F(ref_end); F(haplotype); F(pattern); F(score); F(ref_score); F(cigar_off); F(cigar_len);
    S(ms_total); S(ms_representatives); S(ms_count); S(ms_emit); S(ms_gather); S(ms_host); S(n_alns); S(n_projected); S(n_ops);
    S(n_inside_insertion); S(n_changed);
    printf("sizeof.aln %zu\nsizeof.stats %zu\n", sizeof(spm_jst_ref_aln), sizeof(spm_jst_project_stats));
    return 0;
}
"""


def test_record_layout_matches_the_header(spm, tmp_path):
    assert ctypes.sizeof(spm.capi.JstRefAln) == 40 == spm.JST_REF_ALN_DTYPE.itemsize
    assert ctypes.sizeof(spm.capi.JstProjectStats) == 64
    want = c_layout(tmp_path, LAYOUT_C)
    assert int(want.pop("sizeof.aln")) == 40 and int(want.pop("sizeof.stats")) == 64
    n_rec = n_st = 0
    for name, off in want.items():
        if name.startswith("stats."):
            assert getattr(spm.capi.JstProjectStats, name[6:]).offset == int(off), name
            n_st += 1
        else:
            assert getattr(spm.capi.JstRefAln, name).offset == int(off), name
            assert spm.JST_REF_ALN_DTYPE.fields[name][1] == int(off), name
            n_rec += 1
    assert n_rec == len(spm.capi.JstRefAln._fields_) == len(spm.JST_REF_ALN_DTYPE.names) == 8
    assert n_st == len(spm.capi.JstProjectStats._fields_) == 11
    for name in ("spm_hip_jst_alns_project", "spm_hip_jst_ref_alns_view", "spm_hip_jst_ref_alns_device",
                 "spm_hip_jst_ref_alns_stats", "spm_hip_jst_ref_alns_destroy"):
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    assert hasattr(spm.JstAlignments, "project") and hasattr(spm.JstRefAlignments, "cigar")


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy reference: the journal as an explicit column list, and the composition over it
# ---------------------------------------------------------------------------------------------------------------------
class Journal:
    """The alignment of haplotype h against the reference as columns (haplotype index or -1, reference position or -1):
    paired (x, r), inserted (x, -1), deleted (-1, r).  The deleted columns of an allele stand directly before the next paired
    column -- the contract's order: an inserted stretch directly behind a deletion comes first.  Per haplotype symbol: the
    anchor (its own position if paired) and the reference position it stems from (an alt symbol: its allele's)."""

    def __init__(self, n_ref, alleles, cov, h):
        hx, rp, anchor, org, pend = [], [], [], [], []
        self.n = 0

        def paired(r0, n, origin=None):
            if n <= 0:
                return
            for piece in pend:
                hx.append(np.full(len(piece), -1, np.int64))
                rp.append(piece)
            pend.clear()
            pos = np.arange(r0, r0 + n, dtype=np.int64)
            hx.append(np.arange(self.n, self.n + n, dtype=np.int64))
            rp.append(pos)
            anchor.append(pos)
            org.append(pos if origin is None else np.full(n, origin, np.int64))
            self.n += n

        r = 0
        for i, a in enumerate(alleles):
            if not (int(cov[i, h >> 6]) >> (h & 63)) & 1:
                continue
            p, al = int(a["pos"]), int(a["alt_len"])
            rl = min(int(a["ref_len"]), n_ref - p)
            paired(r, p - r)
            mn = min(rl, al)
            paired(p, mn, p)
            if al > rl:
                hx.append(np.arange(self.n, self.n + al - rl, dtype=np.int64))
                rp.append(np.full(al - rl, -1, np.int64))
                anchor.append(np.full(al - rl, p + mn, np.int64))
                org.append(np.full(al - rl, p, np.int64))
                self.n += al - rl
            if rl > al:
                pend.append(np.arange(p + al, p + rl, dtype=np.int64))
            r = p + rl
        paired(r, n_ref - r)
        for piece in pend:
            hx.append(np.full(len(piece), -1, np.int64))
            rp.append(piece)
        z = np.zeros(0, np.int64)
        self.hx, self.rp = np.concatenate(hx + [z]), np.concatenate(rp + [z])
        self.anchor, self.org = np.concatenate(anchor + [z]), np.concatenate(org + [z])
        self.col_of = np.nonzero(self.hx >= 0)[0]
        self.n_ref = n_ref
        assert len(self.col_of) == self.n == len(self.anchor)


def _runs(ops):
    ops = np.asarray(ops, dtype=np.uint32)
    if len(ops) == 0:
        return np.zeros(0, np.uint32)
    cut = np.concatenate([[0], np.nonzero(ops[1:] != ops[:-1])[0] + 1, [len(ops)]])
    return ((np.diff(cut).astype(np.uint32) << 4) | ops[cut[:-1]]).astype(np.uint32)


def np_project(J, ref, begin, words, P):
    """(ref_begin, ref_end, ref_score, words, kinds) of the transcript `words` of P against hap[begin, ...) through J"""
    words = np.asarray(words, dtype=np.uint32)
    t_op = np.repeat(words & 15, words >> 4)
    on_h, on_p = np.isin(t_op, (EQ, X, DEL)), np.isin(t_op, (EQ, X, INS))
    t_x = np.where(on_h, begin + np.cumsum(on_h) - 1, -1)
    t_i = np.where(on_p, np.cumsum(on_p) - 1, -1)
    assert int(on_p.sum()) == len(P)
    out, used = [], []          # projected ops; the paired journal columns the alignment consumes
    kinds = {"gap_d": 0, "x_from_eq": 0, "i_from_ins": 0, "inside": 0}
    for op, x, i in zip(t_op.tolist(), t_x.tolist(), t_i.tolist()):
        if x < 0:
            out.append(INS)
            continue
        c = int(J.col_of[x])
        if J.rp[c] >= 0:
            if used:
                nd = int(np.count_nonzero(J.hx[used[-1] + 1:c] < 0))   # the deleted columns between the two
                out += [DEL] * nd
                kinds["gap_d"] += nd
            used.append(c)
            if op == DEL:
                out.append(DEL)
            else:
                same = P[i] == ref[J.rp[c]]
                out.append(EQ if same else X)
                kinds["x_from_eq"] += int(op == EQ and not same)
        elif op != DEL:
            out.append(INS)
            kinds["i_from_ins"] += 1
    if used:
        rb, re = int(J.rp[used[0]]), int(J.rp[used[-1]]) + 1
    else:
        rb = re = int(J.anchor[begin]) if begin < J.n else J.n_ref
        kinds["inside"] = 1
    return rb, re, sum(1 for o in out if o != EQ), _runs(out), kinds


def _r(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


def _cig(words):
    return "".join(f"{int(w) >> 4}{'?ID????=X'[int(w) & 15]}" for w in words)


def _one_allele(pos, ref_len, alt):
    al = np.array([(pos, ref_len, len(alt), 0)], dtype=[("pos", "<u8"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("alt_off", "<u8")])
    return al, _r(alt), np.array([[1]], dtype=np.uint64)


# allele (pos, ref_len, alt), needle, hap range -> projected CIGAR, ref range, ref_score
HAND = [
    ((5, 1, "T"), "CGTT", (3, 7), "2=1X1=", (3, 7), 1),
    ((4, 2, ""), "CCTT", (2, 6), "2=2D2=", (2, 8), 2),
    ((4, 0, "TTT"), "CTTTG", (3, 8), "1=3I1=", (3, 5), 3),
    ((4, 0, "TTT"), "TT", (4, 6), "2I", (4, 4), 2),
    ((4, 2, "TAC"), "CTACT", (3, 8), "1=2X1I1=", (3, 7), 3),
]


def test_reference_on_the_hand_worked_cases():
    ref = _r("AACCGGTTAACC")
    for (pos, rl, alt), needle, (b, e), cigar, (rb, re), score in HAND:
        al, pool, cov = _one_allele(pos, rl, alt)
        hap = _apply(ref, al, pool, cov, 0)
        P = _r(needle)
        assert np.array_equal(hap[b:e], P), "the table's needle is not the haplotype slice"
        J = Journal(len(ref), al, cov, 0)
        got = np_project(J, ref, b, np.array([len(P) << 4 | EQ], np.uint32), P)
        assert (_cig(got[3]), (got[0], got[1]), got[2]) == (cigar, (rb, re), score), (needle, got)
        replay(P, ref, got[0], got[1], got[3], got[2])


def _global_dp(P, T):
    """edit-distance alignment of all of P against all of T: transcript words (needle = query, T = reference)"""
    m, n = len(P), len(T)
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    D[0] = np.arange(n + 1)
    ar = np.arange(n + 1)
    for i in range(1, m + 1):
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, :-1] + (T != P[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(t - ar) + ar
    ops, i, j = [], m, n
    while i or j:
        if i and j and D[i, j] == D[i - 1, j - 1] + int(P[i - 1] != T[j - 1]):
            ops.append(EQ if P[i - 1] == T[j - 1] else X)
            i, j = i - 1, j - 1
        elif i and D[i, j] == D[i - 1, j] + 1:
            ops.append(INS)
            i -= 1
        else:
            ops.append(DEL)
            j -= 1
    return _runs(ops[::-1]), int(D[m, n])


def test_reference_on_random_alignments_replays_against_the_reference():
    rng = np.random.default_rng(20260)
    seen = {"inside": 0, "gap_d": 0, "x_from_eq": 0, "i_from_ins": 0}
    n_done = 0
    while n_done < 2000:
        n_ref, n_hap = 400, 4
        ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
        alleles, pool, cov = _random_alleles(rng, n_ref, n_hap, 24, 10)
        journals = [Journal(n_ref, alleles, cov, h) for h in range(n_hap)]
        haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
        for _ in range(50):
            h = int(rng.integers(0, n_hap))
            hp, J = haps[h], journals[h]
            assert len(hp) == J.n
            L = int(rng.integers(3, 30))
            b = int(rng.integers(0, len(hp) - L))
            T = hp[b:b + L]
            P = T.copy()
            for _e in range(int(rng.integers(0, 4))):        # a few edits: the transcript has X, I and D of its own
                kind, at = int(rng.integers(0, 3)), int(rng.integers(0, max(1, len(P))))
                if kind == 0 and len(P):
                    P[at] = (int(P[at]) + 1 + int(rng.integers(0, 3))) & 3
                elif kind == 1:
                    P = np.insert(P, at, rng.integers(0, 4)).astype(np.uint8)
                elif len(P) > 2:
                    P = np.delete(P, at)
            words, d = _global_dp(P, T)
            replay(P, hp, b, b + L, words, d)
            rb, re, score, out, kinds = np_project(J, ref, b, words, P)
            replay(P, ref, rb, re, out, score)
            if kinds["inside"]:
                assert rb == re and np.array_equal(out, [len(P) << 4 | INS])
            for k in seen:
                seen[k] += int(kinds[k] > 0)
            n_done += 1
    assert all(v > 0 for v in seen.values()), seen


# ---------------------------------------------------------------------------------------------------------------------
# GPU: trees, needles, the checker
# ---------------------------------------------------------------------------------------------------------------------
KINDS = ("snp", "ins", "del", "rep_longer", "rep_shorter", "multi", "del_then_ins", "snp_snp")


def _make_tree(seed, n_ref, n_hap, max_len, n_sites, sigma=4, n_runs=0, extra=()):
    """Alleles of every kind on a grid, far enough apart never to overlap; `extra`: hand-made (pos, ref_len, alt, haplotypes)
    alleles spliced in by position.  Returns a dict with the host-side truth: haplotypes, journals, sites to plant on."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
    for _ in range(n_runs):                                   # dna5: runs of N
        at = int(rng.integers(0, n_ref - 40))
        ref[at:at + int(rng.integers(1, 30))] = 4
    cw = (n_hap + 63) // 64
    step = 2 * max_len + 8
    cells = np.arange(step, n_ref - 2 * step, step)
    keep = [c for c in cells if all(abs(int(c) - e[0]) > 2 * step + e[1] + len(e[2]) for e in extra)]
    cells = np.sort(rng.choice(keep, size=min(n_sites, len(keep)), replace=False)) if n_sites else []
    rows = []                                                 # (pos, ref_len, alt, coverage bits, kind)

    def bits():
        b = rng.random(n_hap) < 0.5
        b[int(rng.integers(0, n_hap))] = True
        return b

    def alt(n):
        return rng.integers(0, 4, n, dtype=np.uint8)

    for s, p in enumerate(int(c) for c in cells):
        kind, c = KINDS[s % len(KINDS)], bits()
        n1, n2 = int(rng.integers(1, max_len + 1)), int(rng.integers(1, max_len + 1))
        if kind == "snp":
            rows.append((p, 1, alt(1), c, kind))
        elif kind == "ins":
            rows.append((p, 0, alt(n1), c, kind))
        elif kind == "del":
            rows.append((p, n1, alt(0), c, kind))
        elif kind == "rep_longer":
            rows.append((p, min(n1, n2), alt(max(n1, n2) + 1), c, kind))
        elif kind == "rep_shorter":
            rows.append((p, max(n1, n2) + 1, alt(min(n1, n2)), c, kind))
        elif kind == "multi":
            c2 = bits() & ~c
            rows.append((p, 1, alt(1), c, kind))
            if c2.any():
                rows.append((p, 2, alt(3), c2, kind))
        elif kind == "del_then_ins":                          # an insertion directly behind a deletion, same haplotypes
            rows.append((p, n1, alt(0), c, kind))
            rows.append((p + n1, 0, alt(n2), c, kind))
        else:                                                 # back-to-back SNPs
            rows.append((p, 1, alt(1), c, kind))
            rows.append((p + 1, 1, alt(1), c, kind))
    for pos, rl, a, hs in extra:
        c = np.zeros(n_hap, bool)
        c[list(hs)] = True
        rows.append((pos, rl, np.asarray(a, np.uint8), c, "extra"))
    rows.sort(key=lambda r: r[0])                             # (stable: ties keep their order)
    al = np.zeros(len(rows), dtype=[("pos", "<u8"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("alt_off", "<u8")])
    cov = np.zeros((len(rows), cw), dtype=np.uint64)
    pool, off = [], 0
    for i, (pos, rl, a, c, _k) in enumerate(rows):
        al[i] = (pos, rl, len(a), off)
        pool.append(a)
        off += len(a)
        for h in np.nonzero(c)[0]:
            cov[i, h >> 6] |= np.uint64(1) << np.uint64(h & 63)
    pool = np.concatenate(pool).astype(np.uint8) if pool else np.zeros(0, np.uint8)
    t = {"ref": ref, "alleles": al, "pool": pool, "cov": cov, "n_hap": n_hap, "sigma": sigma, "journals": {}, "haps": {},
         "sites": [(k, pos, int(np.nonzero(c)[0][0])) for pos, _rl, _a, c, k in rows]}
    return t


def _hap(t, h):
    if h not in t["haps"]:
        t["haps"][h] = _apply(t["ref"], t["alleles"], t["pool"], t["cov"], h)
        t["journals"][h] = Journal(len(t["ref"]), t["alleles"], t["cov"], h)
        assert t["journals"][h].n == len(t["haps"][h])
    return t["haps"][h], t["journals"][h]


def _edit(rng, src, L, k):
    """src: L + k + 1 symbols; a needle of L symbols within k edits of a prefix of it (the recipe of test_jst_align._edited)"""
    nd = src.copy()
    if k == 0:
        return nd[:L]
    kind = int(rng.integers(0, 3)) if k >= 2 else int(rng.integers(0, 2))
    spent = 0
    if kind in (0, 2):
        nd = np.delete(nd, int(rng.integers(3, L - 3)))
        spent += 1
    if kind in (1, 2):
        at = int(rng.integers(3, L - 3))
        nd = np.insert(nd, at, (int(nd[at]) + 1 + int(rng.integers(0, 3))) & 3)
        spent += 1
    for _ in range(int(rng.integers(0, k - spent + 1))):
        at = int(rng.integers(0, L))
        nd[at] = (int(nd[at]) + 1 + int(rng.integers(0, 3))) & 3
    return nd[:L].astype(np.uint8)


def _plant(t, seed, L, k, per_kind=3, kinds=None):
    """needles cut from haplotypes ACROSS the alleles of every kind, then edited"""
    rng = np.random.default_rng(seed)
    out = []
    for kind in (kinds or sorted({s[0] for s in t["sites"]})):
        sites = [s for s in t["sites"] if s[0] == kind]
        for j in rng.permutation(len(sites))[:per_kind]:
            _k, pos, h = sites[int(j)]
            hp, J = _hap(t, h)
            x0 = int(np.searchsorted(J.org, pos))            # the first haplotype symbol at or behind the allele
            o = max(0, min(x0 - int(rng.integers(L // 4, 3 * L // 4)), len(hp) - (L + k + 1)))
            out.append(_edit(rng, hp[o:o + L + k + 1], L, k))
    return out


def _check(spm, ctx, t, needles, src, block=None, need=(), min_shared=True):
    """every record of src.project() against the NumPy reference and the replayer; sharing; the stats.  Returns the result
    rows keyed like the source: {(haplotype, pattern, end, score): (ref_begin, ref_end, ref_score, words)}"""
    sv, sops = src.view(), src.ops
    pr = src.project()
    try:
        rv, rops, st = pr.view(), pr.ops, pr.stats()
    finally:
        pr.close()
    assert len(rv) == len(sv) == st.n_alns and len(rops) == st.n_ops
    for f in ("haplotype", "pattern", "score"):
        assert np.array_equal(rv[f], sv[f]), f
    ref = t["ref"]
    seen = {"inside": 0, "gap_d": 0, "x_from_eq": 0, "i_from_ins": 0, "two_blocks": 0}
    cache, rows = {}, {}
    changed, inside = set(), set()
    for s, r in zip(sv, rv):
        h, p, b, e = int(s["haplotype"]), int(s["pattern"]), int(s["begin"]), int(s["end"])
        _hp, J = _hap(t, h)
        words = sops[int(s["cigar_off"]):int(s["cigar_off"]) + int(s["cigar_len"])]
        c0 = int(J.col_of[b]) if b < J.n else len(J.hx)
        c1 = int(J.col_of[e - 1]) + 1 if e > b else c0
        # the reference once per distinct (needle, transcript, journal stretch): it is a function of nothing else
        key = (p, words.tobytes(), (J.hx[c0:c1] >= 0).tobytes(), J.rp[c0:c1].tobytes(), int(J.anchor[b]) if b < J.n else -1)
        if key not in cache:
            cache[key] = np_project(J, ref, b, words, needles[p])
        rb, re, score, out, kinds = cache[key]
        got = rops[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])]
        assert (int(r["ref_begin"]), int(r["ref_end"]), int(r["ref_score"])) == (rb, re, score), (h, p, b, e, _cig(got), _cig(out))
        assert np.array_equal(got, out), (h, p, b, e, _cig(got), _cig(out))
        replay(needles[p], ref, rb, re, got, score)
        for k in kinds:
            seen[k] += int(kinds[k] > 0)
        if block and e > b:
            seen["two_blocks"] += int(J.org[b] // block < J.org[e - 1] // block)
        if not np.array_equal(got, words):
            changed.add(int(s["cigar_off"]))
        if kinds["inside"]:
            inside.add(int(s["cigar_off"]))
            assert rb == re
        rows[(h, p, e, int(s["score"]))] = (rb, re, score, got.tobytes())
    if len(sv) == 0:
        assert st.n_projected == 0 and st.n_ops == 0 and st.n_changed == 0 and st.n_inside_insertion == 0
        return rows
    # sharing: equal source slots <=> equal projected slots; one projection per distinct source slot, in pool order
    pairs = np.unique(np.stack([sv["cigar_off"].astype(np.int64), rv["cigar_off"].astype(np.int64)]), axis=1)
    assert len(np.unique(pairs[0])) == len(np.unique(pairs[1])) == pairs.shape[1]
    assert np.all(np.diff(pairs[1]) > 0), "the projected pool is not in source pool order"
    n_slots = pairs.shape[1]
    assert st.n_projected == n_slots
    if min_shared:
        assert n_slots < len(sv), "no transcript is shared: the row shows nothing about sharing"
    assert st.n_changed == len(changed) and st.n_inside_insertion == len(inside)
    if len(rv):
        last = int(np.argmax(rv["cigar_off"]))
        assert int(rv["cigar_off"][last]) + int(rv["cigar_len"][last]) == st.n_ops   # the pool holds nothing else
    for k in need:
        assert seen[k] > 0, (k, seen)
    print(f"records {len(sv)}, slots {n_slots}, words {st.n_ops}, changed {st.n_changed}, inside {st.n_inside_insertion}; "
          f"kinds {seen}; device ms rep {st.ms_representatives:.3f} count {st.ms_count:.3f} emit {st.ms_emit:.3f} "
          f"gather {st.ms_gather:.3f}, host {st.ms_host:.3f}")
    return rows


def _open(spm, ctx, t, needles, k, algo=None):
    ref_text = ctx.upload(t["ref"], sigma=t["sigma"])
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS if algo is None else algo, needles, k=k, sigma=t["sigma"])
    return ref_text, jst, ps


def _window(ps, n):
    return max(ps.window_size(p) for p in range(n))


def _run_row(spm, ctx, t, needles, k, block, need, algo=None, shard=None, min_shared=True):
    ref_text, jst, ps = _open(spm, ctx, t, needles, k, algo)
    try:
        jst.index(_window(ps, len(needles)), block, *(shard or ()))
        h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
        a = h.align()
        assert len(a) >= 1
        rows = _check(spm, ctx, t, needles, a, block, need, min_shared)
        a.close()
        h.close()
        return rows
    finally:
        jst.close()
        ps.close()
        ref_text.close()


_trees = {}


def _row1_tree():
    if 1 not in _trees:
        t = _make_tree(101, 16_000, 6, 8, 160)
        _trees[1] = (t, _plant(t, 102, 40, 2))
    return _trees[1]


ALL_KINDS = ("gap_d", "x_from_eq", "i_from_ins")


@pytest.mark.gpu
def test_row1_every_allele_kind(spm, ctx):
    t, needles = _row1_tree()
    _run_row(spm, ctx, t, needles, 2, 64, ALL_KINDS + ("two_blocks",))


@pytest.mark.gpu
def test_row2_alleles_longer_than_a_block_and_needles_inside_an_insertion(spm, ctx):
    rng = np.random.default_rng(7)
    big = rng.integers(0, 4, 80, dtype=np.uint8)
    # an 80-symbol insertion and a 40-symbol deletion that spans block borders (block 16)
    t = _make_tree(201, 16_000, 6, 40, 60, extra=[(5000, 0, big, (1, 3)), (9003, 40, [], (0, 2, 4))])
    needles = _plant(t, 202, 40, 2, per_kind=2)
    hp, J = _hap(t, 1)
    x0 = int(np.searchsorted(J.org, 5000))
    assert np.array_equal(hp[x0:x0 + 80], big)
    inside = [_edit(rng, hp[x0 + o:x0 + o + 26], 24, 1) for o in (3, 20, 41, 50)]
    hp0, J0 = _hap(t, 0)
    x1 = int(np.searchsorted(J0.org, 9003))
    needles.append(_edit(rng, hp0[x1 - 20:x1 + 23], 40, 2))            # across the long deletion
    ks = [2] * len(needles) + [1] * len(inside)
    _run_row(spm, ctx, t, needles + inside, ks, 16, ALL_KINDS + ("inside", "two_blocks"))


@pytest.mark.gpu
@pytest.mark.parametrize("n_hap,n_ref,n_needles", [(70, 16_000, 3), (1100, 4_000, 1)])
def test_row3_coverage_words_and_haplotype_groups(spm, ctx, n_hap, n_ref, n_needles):
    t = _make_tree(300 + n_hap, n_ref, n_hap, 8, 80 if n_hap == 70 else 24)
    needles = _plant(t, 301, 40, 2, per_kind=n_needles, kinds=("snp", "ins", "del", "rep_shorter"))
    _run_row(spm, ctx, t, needles, 2, 64, ALL_KINDS)


@pytest.mark.gpu
def test_row4_long_needles_wave_class_kernels(spm, ctx):
    t = _make_tree(401, 20_000, 8, 8, 200)
    needles = _plant(t, 402, 300, 12, per_kind=1)
    _run_row(spm, ctx, t, needles, 12, 64, ALL_KINDS)


@pytest.mark.gpu
def test_row5_exact_set(spm, ctx):
    t, _ = _row1_tree()
    needles = _plant(t, 502, 32, 0)
    rows = _run_row(spm, ctx, t, needles, 0, 64, ALL_KINDS, algo=spm.ALGO_SHIFTOR)
    assert any(v[2] > 0 for v in rows.values()), "every source transcript is |P|=: the projection must carry the alleles"


@pytest.mark.gpu
def test_row6_dna5_reference_with_n_runs(spm, ctx):
    t = _make_tree(601, 16_000, 6, 8, 160, sigma=5, n_runs=60)
    needles = _plant(t, 602, 40, 2)
    assert any(4 in nd for nd in needles), "no needle holds an N"
    _run_row(spm, ctx, t, needles, 2, 64, ALL_KINDS)


@pytest.mark.gpu
def test_row7_no_alleles_is_the_identity(spm, ctx):
    t = _make_tree(701, 8_000, 3, 8, 0)
    assert len(t["alleles"]) == 0
    rng = np.random.default_rng(702)
    hp, _J = _hap(t, 0)
    needles = [_edit(rng, hp[o:o + 43], 40, 2) for o in (100, 3000, 7900)]
    ref_text, jst, ps = _open(spm, ctx, t, needles, 2)
    jst.index(_window(ps, 3), 64)
    h = jst.search_device(ps, alignable=True)
    a = h.align()
    _check(spm, ctx, t, needles, a, 64)
    pr = a.project()
    sv, rv = a.view(), pr.view()
    assert np.array_equal(rv["ref_begin"], sv["begin"]) and np.array_equal(rv["ref_end"], sv["end"])
    assert np.array_equal(rv["ref_score"], sv["score"]) and pr.stats().n_changed == 0
    for s, r in zip(sv, rv):
        assert np.array_equal(a.ops[int(s["cigar_off"]):int(s["cigar_off"]) + int(s["cigar_len"])],
                              pr.ops[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])])
    for x in (pr, a, h, jst, ps, ref_text):
        x.close()


@pytest.mark.gpu
def test_row8_alleles_at_both_ends_of_the_reference(spm, ctx):
    n_ref = 8_010
    extra = [(0, 0, [1, 2, 3], (3,)), (1, 1, [0, 1], (1,)), (2, 3, [], (2,)),
             (n_ref - 6, 0, [3, 3, 0, 1], (3,)), (n_ref - 3, 3, [], (1,)), (n_ref - 1, 1, [2], (2,))]
    t = _make_tree(801, n_ref, 4, 8, 40, extra=extra)
    t["ref"][n_ref - 1] = 1                                   # (the SNP at the last position changes the symbol)
    rng = np.random.default_rng(802)
    needles = _plant(t, 803, 40, 2, per_kind=1)
    for h in range(4):
        hp, _J = _hap(t, h)
        for nd in (hp[:40].copy(), hp[-40:].copy()):          # the first and the last symbols of every haplotype
            nd[20] = (int(nd[20]) + 1) & 3
            needles.append(nd)
    rows = _run_row(spm, ctx, t, needles, 2, 64, ALL_KINDS)
    assert any(v[0] <= 1 for v in rows.values()) and any(v[1] >= n_ref - 1 for v in rows.values())


@pytest.mark.gpu
@pytest.mark.parametrize("across", [False, True])
def test_row9_selections_project_like_the_search(spm, ctx, across):
    t, needles = _row1_tree()
    ref_text, jst, ps = _open(spm, ctx, t, needles, 2)
    jst.index(_window(ps, len(needles)), 64)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    a = h.align()
    full = _check(spm, ctx, t, needles, a, 64, ALL_KINDS)
    sel = h.select(best=0 if across else 1, across=across)
    assert 0 < len(sel) < len(h)
    b = sel.align_selected()
    got = _check(spm, ctx, t, needles, b, 64, min_shared=False)
    assert len(got) == len(sel) and all(full[k] == v for k, v in got.items())
    for x in (b, sel, a, h, jst, ps, ref_text):
        x.close()


@pytest.mark.gpu
def test_row10_block_shard(spm, ctx):
    t, needles = _row1_tree()
    n_blocks = -(-len(t["ref"]) // 64)
    _run_row(spm, ctx, t, needles, 2, 64, (), shard=(n_blocks // 3, 2 * n_blocks // 3), min_shared=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 0])
def test_row11_slot_counts_around_a_workgroup(spm, ctx, n):
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
    _check(spm, ctx, t, needles, a, 64, min_shared=False)
    if n == 0:
        pr = a.project()
        assert len(pr) == 0 and len(pr.ops) == 0 and pr.device()[1] == 0 and pr.stats().n_projected == 0
        pr.close()
    for x in (a, h, jst, ps, ref_text):
        x.close()


@pytest.mark.gpu
def test_row12_refusals_repeatability_and_the_device_view(spm, ctx):
    t, needles = _row1_tree()
    ref_text, jst, ps = _open(spm, ctx, t, needles, 2)
    window = _window(ps, len(needles))
    jst.index(window, 64)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    a = h.align()
    # two calls: byte-identical host views
    p1, p2 = a.project(), a.project()
    assert p1.view().tobytes() == p2.view().tobytes() and p1.ops.tobytes() == p2.ops.tobytes() and len(p1) > 0
    assert p1.cigar(0) == _cig(p1.ops[int(p1.view()[0]["cigar_off"]):][:int(p1.view()[0]["cigar_len"])])
    # the device view: record i belongs to record i of the source's device view
    sp, sn, _so, _sno = a.device()
    rp, rn, ro, rno = p1.device()
    assert sn == rn == len(p1) and rno == len(p1.ops)
    sd, rd = download(ctx, sp, sn, spm.JST_ALN_DTYPE), download(ctx, rp, rn, spm.JST_REF_ALN_DTYPE)
    assert np.array_equal(download(ctx, ro, rno, np.dtype("<u4")), p1.ops)
    for f in ("haplotype", "pattern", "score"):
        assert np.array_equal(sd[f], rd[f]), f
    sv, rv = a.view(), p1.view()
    host = {(int(s["haplotype"]), int(s["pattern"]), int(s["end"]), int(s["score"])): r.tobytes() for s, r in zip(sv, rv)}
    assert len(host) == len(sv)
    for s, r in zip(sd, rd):
        assert host[(int(s["haplotype"]), int(s["pattern"]), int(s["end"]), int(s["score"]))] == r.tobytes()
    # begins only: no transcript to project
    b = h.align(begin_only=True)
    with pytest.raises(spm.SpmError, match="BEGIN_ONLY"):
        b.project()
    # unknown flag bits
    out = ctypes.c_void_p()
    assert spm.capi.lib().spm_hip_jst_alns_project(a._h, 2, ctypes.byref(out)) == -1 and not out.value
    # a destroyed source
    b.close()
    with pytest.raises(spm.SpmError):
        b.project()
    # the tree indexed again since the search
    jst.index(window, 128)
    with pytest.raises(spm.SpmError, match="indexed again"):
        a.project()
    # ... and the context still works: a fresh search projects, to the same answer (the rule reads no block length)
    h2 = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    a2 = h2.align()
    p3 = a2.project()
    v3 = p3.view()
    for f in ("ref_begin", "ref_end", "haplotype", "pattern", "score", "ref_score", "cigar_len"):
        assert np.array_equal(v3[f], rv[f]), f
    # a closed tree
    for x in (p1, p2, p3, h, h2):
        x.close()
    jst.close()
    with pytest.raises(spm.SpmError, match="closed"):
        a2.project()
    for x in (a, a2, ps, ref_text):
        x.close()
