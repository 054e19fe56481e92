"""Reads on both strands: stranded needle sets (spm_hip_patterns_create_stranded), the best stratum per READ
(SPM_SELECT_STRANDS) and the per-read summary of collapsed loci (spm_hip_jst_ref_loci_reads).

The expected answer never comes from the code under test: the complement tables, the selection rule and the read summary are
written again in NumPy here; occurrences come from the oracle's Myers scan of the NumPy reverse complement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cpp_programs import ROOT, build_cases, build_mirror, c_layout, download
from test_align import replay
from test_jst_project import _hap, _make_tree, _open, _plant, _window
from test_jst_select import device_order, host_order
from test_jst_select import device_view as jst_device_view
from test_jst_select import upload_records as jst_upload
from test_oracle_golden import GOLD, _fasta
from test_select import HIT, device_view, upload_records

gpu = pytest.mark.gpu
READ = np.dtype([("first_locus", "<u4"), ("n_loci", "<u4"), ("n_forward", "<u4"), ("primary", "<u4"), ("best", "<i4"),
                 ("best_ref_score", "<i4"), ("n_best", "<u4"), ("n_next", "<u4")])
COMP = {4: np.array([3, 2, 1, 0], np.uint8),                                       # ACGT
        5: np.array([4, 2, 1, 3, 0], np.uint8),                                    # ACGNT
        15: np.array([11, 12, 4, 5, 2, 3, 7, 6, 8, 14, 10, 0, 1, 13, 9], np.uint8)}  # ABCDGHKMNRSTVWY


def np_revcomp(r, sigma=4):
    out = np.asarray(r, np.uint8)[::-1].copy()
    m = out < sigma
    out[m] = COMP[sigma][out[m]]
    return out


def interleave(reads, sigma=4):
    out = []
    for r in reads:
        out += [np.asarray(r, np.uint8), np_revcomp(r, sigma)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the case programs, the layouts, the names
# ---------------------------------------------------------------------------------------------------------------------
CASES = [("strands_cases.cpp", 5000), ("jst_reads_core_cases.cpp", 2000), ("select_strands_plan_cases.cpp", 2000)]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
@pytest.mark.parametrize("source,min_checks", CASES, ids=[c[0][:-4] for c in CASES])
def test_case_programs(tmp_path, source, min_checks, sanitize):
    exe = build_cases(source, tmp_path, include=[os.path.join(ROOT, "include")], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= min_checks, r.stdout[-500:]


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define F(f) printf("%s %zu\n", #f, offsetof(spm_jst_read, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_jst_reads_stats, f))
int main(void)
{
    F(first_locus); F(n_loci); F(n_forward); F(primary); F(best); F(best_ref_score); F(n_best); F(n_next);
    S(ms_total); S(ms_host); S(n_reads); S(n_loci); S(n_mapped); S(n_unique); S(n_multi);
    printf("sizeof.read %zu\nsizeof.stats %zu\nflag.strands %u\n", sizeof(spm_jst_read), sizeof(spm_jst_reads_stats),
           SPM_SELECT_STRANDS);
    return 0;
}
"""
CALLS = ("spm_hip_patterns_create_stranded", "spm_hip_patterns_strands", "spm_hip_patterns_count", "spm_hip_patterns_needle",
         "spm_hip_jst_ref_loci_reads", "spm_hip_jst_reads_view", "spm_hip_jst_reads_device", "spm_hip_jst_reads_stats",
         "spm_hip_jst_reads_destroy")


def test_layouts_and_names(spm, tmp_path):
    import inspect
    assert ctypes.sizeof(spm.capi.JstRead) == 32 == spm.JST_READ_DTYPE.itemsize and spm.JST_READ_DTYPE == READ
    assert ctypes.sizeof(spm.capi.JstReadsStats) == 48
    want = c_layout(tmp_path, LAYOUT_C)
    assert int(want.pop("sizeof.read")) == 32 and int(want.pop("sizeof.stats")) == 48
    assert int(want.pop("flag.strands")) == spm.capi.SELECT_STRANDS == spm.SELECT_STRANDS == 8
    n_rec = n_st = 0
    for name, off in want.items():
        if name.startswith("stats."):
            assert getattr(spm.capi.JstReadsStats, name[6:]).offset == int(off), name
            n_st += 1
        else:
            assert getattr(spm.capi.JstRead, name).offset == int(off) == READ.fields[name][1], name
            n_rec += 1
    assert n_rec == len(spm.capi.JstRead._fields_) == 8 and n_st == len(spm.capi.JstReadsStats._fields_) == 7
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    for f in (spm.PatternSet.needle, spm.PatternSet.__len__, spm.JstRefLoci.reads, spm.JstReads.view, spm.JstReads.device,
              spm.JstReads.stats, spm.JstReads.close):
        assert callable(f)
    assert isinstance(spm.PatternSet.strands, property)
    assert "both_strands" in inspect.signature(spm.Context.patterns).parameters
    for f in (spm.Hits.select, spm.JstHits.select, spm.select_records, spm.select_jst_records):
        assert inspect.signature(f).parameters["strands"].default is False


def test_numpy_complement_tables_are_the_alphabets():
    for sigma, letters, comp in ((4, "ACGT", "TGCA"), (5, "ACGNT", "TGCNA"), (15, "ABCDGHKMNRSTVWY", "TVGHCDMKNYSABWR")):
        assert "".join(letters[c] for c in COMP[sigma]) == comp
        assert np.array_equal(COMP[sigma][COMP[sigma]], np.arange(sigma))
    assert np_revcomp([0, 0, 1, 9, 3], 4).tolist() == [0, 9, 2, 3, 3]


# ---------------------------------------------------------------------------------------------------------------------
# the rules again, in NumPy
# ---------------------------------------------------------------------------------------------------------------------
def np_select(a, w_of, best=None, loci=True, strands=False):
    """a: HIT records -> the records spm_hip_hits_select keeps, in (pattern, pos) order.  w_of: pattern -> window."""
    a = a[np.lexsort((a["pos"], a["pattern"]))]
    pos, pat, sc = a["pos"].astype(np.int64), a["pattern"].astype(np.int64), a["score"].astype(np.int64)
    keep = np.ones(len(a), bool)
    if loci:
        for i in range(len(a)):
            w = w_of(int(pat[i]))
            near = (pat == pat[i]) & (np.abs(pos - pos[i]) <= w)
            keep[i] = not np.any(near & ((sc < sc[i]) | ((sc == sc[i]) & (pos < pos[i]))))
    if best is not None:
        grp = pat >> 1 if strands else pat
        for g in np.unique(grp):
            m = grp == g
            keep[m] &= sc[m] <= sc[m].min() + best
    return a[keep]


def np_jselect(v, w_of, best=None, loci=True, across=False, strands=False):
    """v: spm_jst_hit records -> the records spm_hip_jst_hits_select keeps, in host order (haplotype, pos, pattern, score)"""
    pos, pat, sc, hap = (v[f].astype(np.int64) for f in ("pos", "pattern", "score", "haplotype"))
    keep = np.ones(len(v), bool)
    if loci:
        for i in range(len(v)):
            near = (hap == hap[i]) & (pat == pat[i]) & (np.abs(pos - pos[i]) <= w_of(int(pat[i])))
            keep[i] = not np.any(near & ((sc < sc[i]) | ((sc == sc[i]) & (pos < pos[i]))))
    if best is not None:
        unit = pat >> 1 if strands else pat
        grp = unit if across else hap * (int(unit.max()) + 1 if len(v) else 1) + unit
        for g in np.unique(grp):
            m = grp == g
            keep[m] &= sc[m] <= sc[m].min() + best
    return host_order(v[keep])


def np_reads(loci, n_reads, strands):
    """the read summary of a loci view"""
    out = np.zeros(n_reads, READ)
    pat, sc = loci["pattern"].astype(np.int64), loci["score"].astype(np.int64)
    for r in range(n_reads):
        mine = np.nonzero(pat // strands == r)[0]
        o = out[r]
        o["first_locus"] = int(np.count_nonzero(pat < strands * r))
        o["primary"], o["best"], o["best_ref_score"] = 0xFFFFFFFF, -1, -1
        if len(mine):
            assert mine[0] == o["first_locus"] and np.array_equal(mine, np.arange(mine[0], mine[0] + len(mine)))
            order = sorted((int(sc[i]), int(i)) for i in mine)
            o["n_loci"], o["n_forward"] = len(mine), int(np.count_nonzero(pat[mine] % strands == 0))
            o["primary"], o["best"] = order[0][1], order[0][0]
            o["best_ref_score"] = int(loci["ref_score"][order[0][1]])
            o["n_best"] = sum(1 for s, _ in order if s == order[0][0])
            o["n_next"] = sum(1 for s, _ in order if s == order[0][0] + 1)
    return out


def test_numpy_read_summary_on_a_hand_worked_list():
    loci = np.zeros(8, dtype=[("pattern", "<u4"), ("score", "<i4"), ("ref_score", "<i4")])
    loci["pattern"], loci["score"] = [2, 2, 2, 3, 3, 7, 7, 7], [1, 0, 0, 0, 1, 2, 1, 2]
    loci["ref_score"] = [4, 9, 3, 5, 6, 2, 8, 1]
    got = np_reads(loci, 5, 2)
    assert got.tolist() == [(0, 0, 0, 0xFFFFFFFF, -1, -1, 0, 0), (0, 5, 3, 1, 0, 9, 3, 2), (5, 0, 0, 0xFFFFFFFF, -1, -1, 0, 0),
                            (5, 3, 0, 6, 1, 8, 1, 2), (8, 0, 0, 0xFFFFFFFF, -1, -1, 0, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# GPU 1: a stranded set is the explicit set of 2n needles
# ---------------------------------------------------------------------------------------------------------------------
def _reads_from(rng, T, n, sigma, ks):
    """n reads of 24..40 symbols cut from T, every odd one reverse-complemented, read r with up to ks[r] substitutions"""
    reads = []
    for r in range(n):
        L = int(rng.integers(24, 41))
        at = int(rng.integers(0, len(T) - L))
        rd = T[at:at + L].copy()
        for _ in range(int(rng.integers(0, int(ks[r]) + 1))):
            j = int(rng.integers(0, L))
            rd[j] = (int(rd[j]) + 1 + int(rng.integers(0, sigma - 1))) % sigma
        reads.append(np_revcomp(rd, sigma) if r % 2 else rd)
    return reads


@gpu
@pytest.mark.parametrize("sigma,algo", [(4, "myers"), (5, "myers"), (15, "myers"), (4, "shiftor")])
def test_stranded_set_equals_the_explicit_set(spm, ctx, oracle, sigma, algo):
    rng = np.random.default_rng(100 + sigma + (algo == "shiftor"))
    T = rng.integers(0, sigma, 1 << 14, dtype=np.uint8)
    if sigma == 5:
        for at in rng.integers(0, len(T) - 8, 300):                # N runs: some reads hold N
            T[at:at + int(rng.integers(1, 4))] = 3
    myers = algo == "myers"
    n = 24
    ks = np.array([r % 3 for r in range(n)], np.uint16) if myers else np.zeros(n, np.uint16)
    reads = _reads_from(rng, T, n, sigma, ks)
    if sigma == 5:
        assert sum(1 for r in reads if np.any(r == 3)) >= 3
    A = spm.ALGO_MYERS if myers else spm.ALGO_SHIFTOR
    text = ctx.upload(T, sigma=sigma)
    ps = ctx.patterns(A, reads, k=ks, sigma=sigma, both_strands=True)
    ex = ctx.patterns(A, interleave(reads, sigma), k=np.repeat(ks, 2), sigma=sigma)
    plain = ctx.patterns(A, reads, k=ks, sigma=sigma)
    assert (ps.strands, len(ps), ps.n) == (2, 2 * n, 2 * n) and (ex.strands, len(ex)) == (1, 2 * n) and (plain.strands, len(plain)) == (1, n)
    for r in range(n):
        assert np.array_equal(ps.needle(2 * r), reads[r]) and np.array_equal(ps.needle(2 * r + 1), np_revcomp(reads[r], sigma))
        assert np.array_equal(plain.needle(r), reads[r])
        assert ps.window_size(2 * r) == ps.window_size(2 * r + 1) == ex.window_size(2 * r) == len(reads[r]) + (int(ks[r]) if myers else 0)
    with pytest.raises(spm.SpmError):
        ps.needle(2 * n)
    n_len = ctypes.c_uint32(77)                                    # cap < len: refused, len written
    assert spm.capi.lib().spm_hip_patterns_needle(ps._h, 1, None, 0, ctypes.byref(n_len)) == -1 and n_len.value == len(reads[0])
    assert ps.state_stride() == ex.state_stride() and ps.initial_state().tobytes() == ex.initial_state().tobytes()
    for engine in (spm.ENGINE_AUTO, spm.ENGINE_BRUTE):
        hs, he = spm.scan(ctx, text, ps, engine=engine), spm.scan(ctx, text, ex, engine=engine)
        vs = hs.view()
        assert vs.tobytes() == he.view().tobytes() and len(vs) >= n
        hs.close()
        he.close()
    if myers:
        n_rev = 0
        for r in range(n):
            want = oracle.myers(T, np_revcomp(reads[r], sigma), int(ks[r]), sigma=sigma)
            got = vs[vs["pattern"] == 2 * r + 1]
            assert np.array_equal(got["pos"], want["pos"]) and np.array_equal(got["score"], want["score"]), r
            n_rev += len(want) > 0
        assert n_rev >= n // 2                                      # the odd reads are found on the reverse strand
    for x in (ps, ex, plain, text):
        x.close()


@gpu
def test_stranded_create_refusals(spm, ctx):
    lib = spm.capi.lib()
    out = ctypes.c_void_p()
    r = np.arange(8, dtype=np.uint8) % 4
    off = np.array([0, 8], np.uint32)
    k = np.zeros(1, np.uint16)
    args = (r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 1,
            k.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    assert lib.spm_hip_patterns_create_stranded(ctx._h, spm.ALGO_MYERS, *args, 6, ctypes.byref(out)) == -4 and not out.value
    assert b"complement" in lib.spm_hip_last_error(ctx._h)
    big = np.array([0, 1 << 31], np.uint32)
    assert lib.spm_hip_patterns_create_stranded(ctx._h, spm.ALGO_MYERS, args[0], big.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                1, args[3], 4, ctypes.byref(out)) == -4 and not out.value
    assert lib.spm_hip_patterns_create_stranded(ctx._h, spm.ALGO_MYERS, args[0], args[1], 1 << 31, args[3], 4,
                                                ctypes.byref(out)) == -4 and not out.value
    assert lib.spm_hip_patterns_create_stranded(ctx._h, 9, *args, 4, ctypes.byref(out)) == -1
    for algo in (spm.ALGO_SHIFTOR, spm.ALGO_MYERS, spm.ALGO_MYERS_PREFIX, spm.ALGO_HORSPOOL):
        ps = ctx.patterns(algo, [r], k=0, both_strands=True)
        assert ps.strands == 2 and len(ps) == 2 and np.array_equal(ps.needle(1), np_revcomp(r))
        ps.close()
    empty = ctx.patterns(spm.ALGO_MYERS, [], k=0, both_strands=True)
    assert len(empty) == 0 and empty.strands == 2
    empty.close()
    assert lib.spm_hip_patterns_strands(None) == 0 and lib.spm_hip_patterns_count(None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU 2: the fixture, every odd read reverse-complemented
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_fixture_reads_on_both_strands(spm, ctx, oracle):
    refs = _fasta(os.path.join(GOLD, "sim_refx5.fasta"))
    T = np.concatenate([oracle.encode(s) for _n, s in refs])
    orig = [oracle.encode(s) for _n, s in _fasta(os.path.join(GOLD, "sim_reads_ref1x10.fa"))]
    reads = [np_revcomp(r) if i % 2 else r for i, r in enumerate(orig)]
    text = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, reads, k=0, both_strands=True)
    plain = ctx.patterns(spm.ALGO_MYERS, reads, k=0)
    v, vp = spm.scan(ctx, text, ps).view(), spm.scan(ctx, text, plain).view()
    for i, r in enumerate(orig):
        want = oracle.myers(T, r, 0)
        assert len(want) >= 1
        got = v[v["pattern"] == 2 * i + (i % 2)]
        assert np.array_equal(got["pos"], want["pos"]) and np.all(got["score"] == 0), i
    assert sorted(set(vp["pattern"].tolist())) == [i for i in range(len(orig)) if i % 2 == 0]   # the odd ones are missed
    assert sorted(set((v["pattern"] >> 1).tolist())) == list(range(len(orig)))
    for x in (ps, plain, text):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 3: the best stratum per read, linear.  A planted text whose sorted record list puts strand changes on a wave border
# and on a tile border.
# ---------------------------------------------------------------------------------------------------------------------
# per read: k, then copies planted of (read exact, read with 1 substitution, revcomp exact, revcomp with 1 substitution,
# read with 2 substitutions, revcomp with 2 substitutions).  An exact copy is 2k + 1 records (scores k..0..k), a copy with s
# substitutions 2 (k - s) + 1.
PLANTED = [
    (1, 20, 4, 0, 64, 0, 0),     # read 0: 64 forward records (min 0), then 64 reverse records of score 1: a wave border between
    (1, 0, 128, 22, 0, 0, 0),    # read 1: 128 forward records of score 1 end at index 256, a tile border; reverse exact: min 0
    (2, 10, 0, 10, 0, 0, 0),     # read 2: both strands, exact
    (1, 0, 0, 0, 0, 0, 0),       # read 3: neither strand
    (0, 30, 0, 0, 0, 0, 0),      # read 4: forward only
    (2, 0, 0, 20, 0, 0, 0),      # read 5: reverse only
    (1, 10, 0, 0, 0, 0, 0),      # read 6: a palindrome -- its own reverse complement
    (2, 10, 40, 0, 0, 0, 30),    # read 7: forward min 0, reverse min 2: the flag matters at best=1 too
    (2, 30, 0, 30, 0, 0, 0),     # read 8
    (2, 0, 0, 0, 0, 0, 0),       # read 9: neither
    (1, 0, 0, 6, 0, 0, 0),       # read 10: reverse only
    (1, 10, 0, 0, 0, 0, 0),      # read 11: forward only -- the largest pattern index is even
]
SEL_TILE = 256


def _planted_text(seed=20261019):
    rng = np.random.default_rng(seed)
    reads, ks = [], []
    for r, spec in enumerate(PLANTED):
        L = 24 + 2 * (r % 9)
        rd = rng.integers(0, 4, L, dtype=np.uint8)
        if r == 6:
            rd = np.concatenate([rd[:L // 2], np_revcomp(rd[:L // 2])])
            assert np.array_equal(rd, np_revcomp(rd))
        reads.append(rd)
        ks.append(spec[0])

    def subst(x, n_sub):
        x = x.copy()
        for j in ([len(x) // 2] if n_sub == 1 else [len(x) // 3, 2 * len(x) // 3])[:n_sub]:
            x[j] = (int(x[j]) + 1 + int(rng.integers(0, 3))) & 3
        return x

    pieces = []
    for r, spec in enumerate(PLANTED):
        fwd, rev = reads[r], np_revcomp(reads[r])
        for count, src, n_sub in ((spec[1], fwd, 0), (spec[2], fwd, 1), (spec[3], rev, 0), (spec[4], rev, 1), (spec[5], fwd, 2),
                                  (spec[6], rev, 2)):
            pieces += [subst(src, n_sub) for _ in range(count)]
    order = rng.permutation(len(pieces))
    parts = [rng.integers(0, 4, 40, dtype=np.uint8)]
    for j in order:
        parts += [pieces[int(j)], rng.integers(0, 4, int(rng.integers(12, 20)), dtype=np.uint8)]
    T = np.concatenate(parts)
    assert len(T) <= 1 << 16
    return T, reads, np.array(ks, np.uint16)


def _borders(a):
    """a: records in (pattern, pos) order -> for every read with records on both strands, the index its reverse records start at"""
    pat = a["pattern"].astype(np.int64)
    out = {}
    for r in np.unique(pat >> 1):
        f, v = np.count_nonzero(pat == 2 * r), np.count_nonzero(pat == 2 * r + 1)
        if f and v:
            out[int(r)] = int(np.count_nonzero(pat < 2 * r + 1))
    return out


def _check_planted(a, ks):
    """what the planted list must hold, asserted from the sorted records and the rule alone"""
    n = len(PLANTED)
    assert len(a) > 4 * SEL_TILE
    b = _borders(a)
    assert any(i % 64 == 0 and i % SEL_TILE for i in b.values()), b       # forward in one wave, reverse in the next
    assert any(i % SEL_TILE == 0 for i in b.values()), b                   # ... in one tile, reverse in the next
    has = [(bool(np.any(a["pattern"] == 2 * r)), bool(np.any(a["pattern"] == 2 * r + 1))) for r in range(n)]
    assert {(True, True), (True, False), (False, True), (False, False)} <= set(has)
    assert has[n - 1] == (True, False) and int(a["pattern"].max()) == 2 * (n - 1)
    w_of = lambda p: int(ks[p >> 1])
    fwd_best = rev_best = 0
    for best in (0, 1):
        w0, w1 = np_select(a, w_of, best=best), np_select(a, w_of, best=best, strands=True)
        assert 0 < len(w1) < len(w0) < len(a)
        lost = set(w0["pattern"].tolist()) - set(w1["pattern"].tolist())
        fwd_best += any(p & 1 for p in lost)                               # a reverse pattern lost everything: forward was best
        rev_best += any(not p & 1 for p in lost)
    assert fwd_best and rev_best
    assert len(np_select(a, w_of, best=0, strands=True)) < len(np_select(a, w_of, best=1, strands=True))


def test_planted_list_holds_its_cases_by_the_oracle_alone(oracle):
    T, reads, ks = _planted_text()
    needles = interleave(reads)
    rows = []
    for p, nd in enumerate(needles):
        h = oracle.myers(T, nd, int(ks[p >> 1]))
        h["pattern"] = p
        rows.append(h.astype(HIT))
    _check_planted(np.concatenate(rows), ks)


def _check_linear(ctx, sel, want):
    got = sel.view()
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    assert device_view(ctx, sel).tobytes() == want.tobytes()
    st = sel.select_stats()
    assert st.n_out == len(want)
    return st


@gpu
def test_linear_best_stratum_per_read(spm, ctx):
    T, reads, ks = _planted_text()
    text = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, reads, k=ks, both_strands=True)
    plain = ctx.patterns(spm.ALGO_MYERS, interleave(reads), k=np.repeat(ks, 2))
    h = spm.scan(ctx, text, ps, max_hits=1 << 20)
    a = h.view()
    _check_planted(a, ks)
    w_of = lambda p: int(ks[p >> 1])
    for kw in (dict(best=0), dict(best=1), dict(best=0, loci=False), dict(best=1, window=0)):
        rule_kw = dict(best=kw["best"], loci=kw.get("loci", True))
        wf = (lambda p: kw["window"]) if "window" in kw else w_of
        for strands in (True, False):
            sel = h.select(strands=strands, **kw)
            st = _check_linear(ctx, sel, np_select(a, wf, strands=strands, **rule_kw))
            assert st.n_in == len(a)
            if strands and kw == dict(best=0):                    # a selection of the selection; alignment as ever
                again = sel.select(best=0, strands=True)
                assert again.view().tobytes() == sel.view().tobytes()
                al = again.align()
                assert len(al) == again.device()[1] == len(sel.view())
                al.close()
                again.close()
            sel.close()
    # a raw buffer in arrival order, no needle set: the index convention
    rng = np.random.default_rng(5)
    shuffled = a[rng.permutation(len(a))]
    buf = upload_records(shuffled)
    for best in (0, 1):
        sel = spm.select_records(ctx, buf.data_ptr(), len(a), None, window=2, best=best, strands=True)
        _check_linear(ctx, sel, np_select(a, lambda p: 2, best=best, strands=True))
        sel.close()
    sel = spm.select_records(ctx, buf.data_ptr(), len(a), ps, best=0, strands=True)
    _check_linear(ctx, sel, np_select(a, w_of, best=0, strands=True))
    sel.close()
    odd = shuffled[shuffled["pattern"] <= 13]                      # the largest pattern index odd: (13 >> 1) + 1 minima
    buf2 = upload_records(odd)
    sel = spm.select_records(ctx, buf2.data_ptr(), len(odd), None, window=1, best=0, strands=True)
    _check_linear(ctx, sel, np_select(odd, lambda p: 1, best=0, strands=True))
    sel.close()
    # refusals: STRANDS without BEST; a set that is not stranded; bit 4 stays refused
    lib = spm.capi.lib()
    out = ctypes.c_void_p()
    for flags in (8, 8 | 1, 8 | 2 | 4):
        o = spm.capi.SelectOpts(flags=flags, window=1, strata=0, reserved=0)
        assert lib.spm_hip_hits_select(h._h, ctypes.byref(o), ctypes.byref(out)) == -1 and not out.value
        assert lib.spm_hip_records_select(ctx._h, ctypes.c_void_p(buf.data_ptr()), len(a), None, ctypes.byref(o), ctypes.byref(out)) == -1
    hp = spm.scan(ctx, text, plain, max_hits=1 << 20)
    assert hp.view().tobytes() == a.tobytes()
    with pytest.raises(spm.SpmError, match="stranded"):
        hp.select(best=0, strands=True)
    with pytest.raises(spm.SpmError, match="stranded"):
        spm.select_records(ctx, buf.data_ptr(), len(a), plain, best=0, strands=True)
    for x in (hp, h, ps, plain, text):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 4 / 5: the pan-genome.  A small tree; reads across its alleles, every odd one reverse-complemented; and pairs of places
# where a read fits one strand exactly and the other strand with one substitution.
# ---------------------------------------------------------------------------------------------------------------------
_pan = {}


def _pan_tree():
    if not _pan:
        t = _make_tree(3101, 12_000, 4, 6, 60)
        rng = np.random.default_rng(3102)
        ref, apos = t["ref"], t["alleles"]["pos"].astype(np.int64)
        free = [p for p in range(200, len(ref) - 200, 97) if np.all(np.abs(apos - p) > 120)]
        spots = [int(free[int(j)]) for j in rng.permutation(len(free))[:8]]
        twins = []
        for a, b in zip(spots[0::2], spots[1::2]):                 # ref[b, b + 36) = revcomp(ref[a, a + 36)) but for one symbol
            rc = np_revcomp(ref[a:a + 36])                         # (the last two twins: but for two)
            for at in (12, 24)[:1 if len(twins) < 2 else 2]:
                rc[at] = (int(rc[at]) + 1) & 3
            ref[b:b + 36] = rc
            twins.append((a, b))
        reads = [np_revcomp(r) if i % 2 else r for i, r in enumerate(_plant(t, 3103, 32, 2, per_kind=4))]
        n_cut = len(reads)
        for j, (a, b) in enumerate(twins):                         # forward best, then reverse best
            reads.append(ref[a:a + 36].copy() if j % 2 == 0 else np_revcomp(ref[a:a + 36]))
        reads.append(rng.integers(0, 4, 30, dtype=np.uint8))       # unmapped, between mapped ones
        reads.append(ref[spots[0] + 40:spots[0] + 70].copy())      # the last read: forward only
        _pan.update(t=t, reads=reads, n_cut=n_cut, k=2)
    return _pan["t"], _pan["reads"], _pan["k"]


def _pan_open(spm, ctx):
    t, reads, k = _pan_tree()
    ref_text = ctx.upload(t["ref"], sigma=4)
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS, reads, k=k, both_strands=True)
    jst.index(_window(ps, len(ps)), 64)
    return ref_text, jst, ps


def _jcheck(ctx, sel, want):
    got = sel.view()
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    assert jst_device_view(ctx, sel).tobytes() == device_order(want).tobytes()
    assert sel.select_stats().n_out == len(want) == len(sel)


@gpu
def test_pan_genome_best_stratum_per_read(spm, ctx):
    t, reads, k = _pan_tree()
    ref_text, jst, ps = _pan_open(spm, ctx)
    h = jst.search_device(ps, max_hits=1 << 21)
    src = h.view()
    assert len(src) > SEL_TILE
    w_of = lambda p: k
    differs = 0
    for kw in (dict(best=0), dict(best=1), dict(best=0, across=True), dict(best=1, across=True), dict(best=0, loci=False)):
        want = np_jselect(src, w_of, strands=True, **kw)
        plain_want = np_jselect(src, w_of, strands=False, **kw)
        differs += len(want) < len(plain_want)
        sel = h.select(strands=True, **kw)
        _jcheck(ctx, sel, want)
        sel.close()
        sel = h.select(**kw)
        _jcheck(ctx, sel, plain_want)
        sel.close()
    assert differs == 5
    both = set((src["pattern"][src["pattern"] % 2 == 0] >> 1).tolist()) & set((src["pattern"][src["pattern"] % 2 == 1] >> 1).tolist())
    assert len(both) >= 4                                          # the twins are found on both strands
    # without ACROSS: the records of haplotype h are the linear scan + select(strands=True) of the materialised haplotype
    want = np_jselect(src, w_of, best=0, strands=True)
    for hap in range(t["n_hap"]):
        hp, _J = _hap(t, hap)
        text = ctx.upload(hp)
        lin = spm.scan(ctx, text, ps, engine=spm.ENGINE_BRUTE, max_hits=1 << 20)
        sel = lin.select(best=0, strands=True)
        v = sel.view()
        mine = want[want["haplotype"] == hap]
        mine = mine[np.lexsort((mine["pos"], mine["pattern"]))]
        assert len(v) and np.array_equal(v["pos"], mine["pos"]) and np.array_equal(v["pattern"], mine["pattern"])
        assert np.array_equal(v["score"], mine["score"])
        for x in (sel, lin, text):
            x.close()
    # a raw buffer in arrival order without a set; with the stranded set; with a set that is not stranded
    rng = np.random.default_rng(9)
    buf = jst_upload(src[rng.permutation(len(src))])
    for kw in (dict(best=0), dict(best=1, across=True)):
        sel = spm.select_jst_records(ctx, buf.data_ptr(), len(src), None, window=k, strands=True, **kw)
        _jcheck(ctx, sel, np_jselect(src, w_of, strands=True, **kw))
        sel.close()
    sel = spm.select_jst_records(ctx, buf.data_ptr(), len(src), ps, best=0, strands=True)
    _jcheck(ctx, sel, want)
    sel.close()
    one = src[src["pattern"] == 2 * _pan["n_cut"]].copy()          # only pattern 0 occurs: haplotypes must not merge
    one["pattern"] = 0
    assert len(set(one["haplotype"].tolist())) >= 2
    buf1 = jst_upload(one)
    sel = spm.select_jst_records(ctx, buf1.data_ptr(), len(one), None, window=k, best=0, strands=True)
    _jcheck(ctx, sel, np_jselect(one, w_of, best=0, strands=True))
    sel.close()
    plain = ctx.patterns(spm.ALGO_MYERS, interleave(reads), k=k)
    with pytest.raises(spm.SpmError, match="stranded"):
        spm.select_jst_records(ctx, buf.data_ptr(), len(src), plain, best=0, strands=True)
    hp_ = jst.search_device(plain, max_hits=1 << 21)
    assert hp_.view().tobytes() == src.tobytes()
    with pytest.raises(spm.SpmError, match="stranded"):
        hp_.select(best=0, strands=True)
    with pytest.raises(spm.SpmError):
        h.select(loci=True, strands=True)                           # STRANDS without BEST
    for x in (hp_, h, plain, ps, jst, ref_text):
        x.close()


def _chain(h, **kw):
    sel = h.select(**kw)
    a = sel.align_selected()
    pr = a.project()
    nz = pr.normalize()
    lc = nz.collapse()
    for x in (nz, pr, a, sel):
        x.close()
    return lc


def _check_reads(ctx, lc, n_reads, strands):
    loci = lc.view()
    rd = lc.reads(n_reads, strands)
    want = np_reads(loci, n_reads, strands)
    got = rd.view()
    assert got.dtype == READ and got.tobytes() == want.tobytes(), (got.tolist(), want.tolist())
    p, n = rd.device()
    assert n == n_reads == len(rd) and download(ctx, p, n, READ).tobytes() == want.tobytes()
    st = rd.stats()
    assert (st.n_reads, st.n_loci, st.n_mapped) == (n_reads, len(loci), int(np.count_nonzero(want["n_loci"])))
    assert (st.n_unique, st.n_multi) == (int(np.count_nonzero(want["n_best"] == 1)), int(np.count_nonzero(want["n_best"] > 1)))
    assert st.ms_host > 0
    return rd, want, loci


@gpu
def test_end_to_end_reads_of_a_stranded_search(spm, ctx):
    t, reads, k = _pan_tree()
    ref_text, jst, ps = _pan_open(spm, ctx)
    h = jst.search_device(ps, max_hits=1 << 21)
    lc = _chain(h, best=0, across=True, strands=True)
    rd, want, loci = _check_reads(ctx, lc, len(reads), 2)
    ops = lc.ops
    assert np.count_nonzero(want["n_loci"] == 0) >= 1 and np.count_nonzero(want["n_loci"]) >= len(reads) - 2
    assert want["n_loci"][len(reads) - 2] == 0 and want["n_loci"][len(reads) - 1] == want["n_forward"][len(reads) - 1] >= 1
    n_rev = 0
    for L in loci:                                                 # every locus replays; a reverse one with the reverse complement
        p = int(L["pattern"])
        P = np_revcomp(reads[p >> 1]) if p & 1 else reads[p >> 1]
        assert np.array_equal(ps.needle(p), P)
        w = ops[int(L["cigar_off"]):int(L["cigar_off"]) + int(L["cigar_len"])]
        replay(P, t["ref"], int(L["ref_begin"]), int(L["ref_end"]), w, int(L["ref_score"]))
        n_rev += p & 1
    assert n_rev >= 4 and np.any(want["n_forward"] == 0) and np.any((want["n_forward"] > 0) & (want["n_loci"] > 0))
    rd2 = lc.reads(len(reads), 2)                                  # byte-identical across runs
    assert rd2.view().tobytes() == want.tobytes()
    # without the flag a twin keeps its worse strand too: more loci, the same primaries
    lc0 = _chain(h, best=0, across=True)
    rd0, want0, _l0 = _check_reads(ctx, lc0, len(reads), 2)
    assert int(want0["n_loci"].sum()) > int(want["n_loci"].sum()) and np.array_equal(want0["best"], want["best"])
    for x in (rd0, lc0, rd2, rd, lc, h, ps, jst, ref_text):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 6: the read summary's edges
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_read_summary_edges(spm, ctx):
    t = _make_tree(4101, 30_000, 1, 4, 6)
    rng = np.random.default_rng(4102)
    ref, apos = t["ref"], t["alleles"]["pos"].astype(np.int64)
    many, few = rng.integers(0, 4, 30, dtype=np.uint8), rng.integers(0, 4, 28, dtype=np.uint8)
    free = [p for p in range(100, len(ref) - 100, 48) if np.all(np.abs(apos - p) > 80)]
    assert len(free) >= 330
    for j, p in enumerate(free[:323]):
        ref[p:p + 30] = many
        if j % 40 == 0:
            ref[p + 15] = (int(many[15]) + 1) & 3                   # a few with one substitution: the next stratum
    for p in free[323:326]:
        ref[p:p + 28] = few
    absent = [rng.integers(0, 4, 26, dtype=np.uint8) for _ in range(3)]
    reads = [absent[0], many, absent[1], few, absent[2]]           # unmapped at 0, between two mapped ones, and at n - 1
    ref_text, jst, ps = _open(spm, ctx, t, reads, 1)
    jst.index(_window(ps, len(reads)), 64)
    h = jst.search_device(ps, max_hits=1 << 21)
    lc = _chain(h, best=1)
    rd, want, loci = _check_reads(ctx, lc, len(reads), 1)
    assert want["n_loci"].tolist()[0::2] == [0, 0, 0] and want["n_loci"][1] >= 300 and want["n_loci"][3] == 3
    assert want["n_best"][1] >= 300 and want["n_next"][1] >= 5 and want["first_locus"][1] == 0
    assert want["first_locus"].tolist()[2:] == [int(want["n_loci"][1])] * 2 + [len(loci)]
    assert np.array_equal(want["n_forward"], want["n_loci"])
    # more reads than the set has: unmapped tails; fewer: a locus out of range fails the call, no fault
    rd7, _w7, _l7 = _check_reads(ctx, lc, 7, 1)
    rd7.close()
    lib = spm.capi.lib()
    out = ctypes.c_void_p()
    with pytest.raises(spm.SpmError, match="-1"):
        lc.reads(3, 1)
    with pytest.raises(spm.SpmError, match="-1"):
        lc.reads(1, 2)
    assert b"outside" in lib.spm_hip_last_error(ctx._h)
    for strands in (0, 3):
        assert lib.spm_hip_jst_ref_loci_reads(lc._h, strands, 5, 0, ctypes.byref(out)) == -1 and not out.value
    assert lib.spm_hip_jst_ref_loci_reads(lc._h, 1, 5, 1, ctypes.byref(out)) == -1 and b"flag" in lib.spm_hip_last_error(ctx._h)
    assert lib.spm_hip_jst_ref_loci_reads(lc._h, 2, 1 << 31, 0, ctypes.byref(out)) == -1 and not out.value
    assert lib.spm_hip_jst_ref_loci_reads(None, 1, 5, 0, ctypes.byref(out)) == -1
    assert lib.spm_hip_jst_ref_loci_reads(lc._h, 1, 5, 0, None) == -1
    # the same loci read as a stranded set's: 5 patterns are 3 reads
    rd2, _w2, _l2 = _check_reads(ctx, lc, 3, 2)
    rd2.close()
    none = lc.reads(0, 1)
    assert len(none) == 0 and len(none.view()) == 0
    none.close()
    # no loci at all: every read unmapped
    nothing = ctx.patterns(spm.ALGO_MYERS, absent, k=1)
    h0 = jst.search_device(nothing, max_hits=1 << 21)
    assert len(h0) == 0
    lc0 = _chain(h0, best=0)
    rd0, want0, _l00 = _check_reads(ctx, lc0, 3, 1)
    assert want0.tolist() == [(0, 0, 0, 0xFFFFFFFF, -1, -1, 0, 0)] * 3
    # the result outlives the loci handle
    for x in (rd0, lc0, h0, nothing, lc, h, ps, jst, ref_text):
        x.close()
    assert rd.view().tobytes() == want.tobytes() and download(ctx, rd.device()[0], 5, READ).tobytes() == want.tobytes()
    rd.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 7: the C++ mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("strands_mirror_cases.cpp", tmp_path).exists()


@gpu
def test_mirror_routes_agree(spm, tmp_path):
    """locate_reads: device route == host route; batch_matcher{both_strands} == the explicit matcher of 2n needles"""
    import re
    r = subprocess.run([str(build_mirror("strands_mirror_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 300, r.stdout[-2000:]
    assert len(re.findall(r"reads mapped", r.stdout)) == 6 and "callbacks on both strands" in r.stdout
