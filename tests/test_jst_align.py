"""Begins and CIGAR transcripts of pan-genome hits (spm_hip_jst_hits_align, JstHits.align, journaled_sequence_tree::locate).

One alignment is computed per segment hit in the context buffer and fanned out to the haplotypes that share the context.
The expected answer never comes from that code alone:
  (a) every record is checked on the materialised haplotype (the NumPy allele walk of test_gpu_jst) with the NumPy DP
      and the replayer of test_align: begin is the largest begin at the hit's distance with lo = 0, the transcript
      consumes exactly P and hap[b, e), = / X agree with the symbols, runs are merged, cost = score;
  (b) all records are compared, bit for bit, with the route that needs no tree: upload the materialised haplotype,
      scan, Hits.align().
"""
import ctypes
import gc
import re
import subprocess

import numpy as np
import pytest

from cpp_programs import build_mirror, c_layout
from test_align import ref_begins, replay
from test_gpu_jst import _apply, _random_alleles

SEED_TEXT = 0x5EED0001
SEED_VAR = 0x5EED0003


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define F(f) printf("%s %zu\n", #f, offsetof(spm_jst_aln, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_jst_align_stats, f))
int main(void)
{
    F(begin); F(end); F(haplotype); F(pattern); F(score); F(cigar_off); F(cigar_len); F(reserved);
    S(ms_total); S(ms_begin); S(ms_cigar); S(ms_fanout); S(ms_host); S(ms_worklist); S(n_alns); S(n_segment_alns); S(n_ops);
    S(begin_lane); S(begin_wave); S(cigar_lane); S(cigar_wave); S(cigar_wave_global); S(reserved);
    printf("sizeof.aln %zu\nsizeof.stats %zu\nflag %u\n", sizeof(spm_jst_aln), sizeof(spm_jst_align_stats), SPM_SCAN_ALIGNABLE);
    return 0;
}
"""


def test_record_layout_matches_the_header(spm, tmp_path):
    assert ctypes.sizeof(spm.capi.JstAln) == 40 == spm.JST_ALN_DTYPE.itemsize
    assert ctypes.sizeof(spm.capi.JstAlignStats) == 80
    want = c_layout(tmp_path, LAYOUT_C)
    assert int(want.pop("sizeof.aln")) == 40 and int(want.pop("sizeof.stats")) == 80
    assert int(want.pop("flag")) == spm.capi.SCAN_ALIGNABLE == spm.SCAN_ALIGNABLE == 4
    n_rec = n_st = 0
    for name, off in want.items():
        if name.startswith("stats."):
            assert getattr(spm.capi.JstAlignStats, name[6:]).offset == int(off), name
            n_st += 1
        else:
            assert getattr(spm.capi.JstAln, name).offset == int(off), name
            assert spm.JST_ALN_DTYPE.fields[name][1] == int(off), name
            n_rec += 1
    assert n_rec == len(spm.capi.JstAln._fields_) == len(spm.JST_ALN_DTYPE.names) == 8
    assert n_st == len(spm.capi.JstAlignStats._fields_) == 15


def _build_locate_cases(out_dir):
    return build_mirror("jst_locate_cases.cpp", out_dir)


def test_locate_program_compiles_with_reference_flags(spm, tmp_path):
    assert _build_locate_cases(tmp_path).exists()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ---------------------------------------------------------------------------------------------------------------------
def _edited(rng, hp, L, k, myers=True):
    """A needle of L symbols cut from hp with at most k edits: one np.delete and / or one np.insert (as
    test_align.test_boundaries makes them), the rest of the budget substitutions."""
    o = int(rng.integers(0, len(hp) - L - k - 2))
    nd = hp[o:o + L + k + 1].copy()
    if not myers or k == 0:
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


def _jst_records(spm, jst, ps, **kw):
    """(hit view, alignment view, ops, align stats, jst stats) of one alignable search"""
    h = jst.search_device(ps, alignable=True, **kw)
    try:
        hv = h.view()
        a = h.align()
        try:
            return hv, a.view(), a.ops, a.stats(), jst.stats()
        finally:
            a.close()
    finally:
        h.close()


def _rows(rec, ops, hap_col=None):
    """records as sortable tuples (haplotype, begin, end, pattern, score, transcript words)"""
    hs = rec["haplotype"].tolist() if hap_col is None else [hap_col] * len(rec)
    out = []
    for h, b, e, p, s, o, n in zip(hs, rec["begin"].tolist(), rec["end"].tolist(), rec["pattern"].tolist(),
                                   rec["score"].tolist(), rec["cigar_off"].tolist(), rec["cigar_len"].tolist()):
        out.append((h, b, e, p, s, ops[o:o + n].tobytes()))
    return out


def _per_haplotype_route(spm, ctx, haps, ps, engine, sigma=4, only=None):
    """the route without the tree: upload every materialised haplotype, scan + Hits.align()"""
    out = []
    for h, hp in enumerate(haps):
        if only is not None and h not in only:
            continue
        t = ctx.upload(hp, sigma=sigma)
        r = spm.scan(ctx, t, ps, engine=engine, max_hits=1 << 21)
        a = r.align()
        out += _rows(a.view(), a.ops, hap_col=h)
        a.close()
        r.close()
        t.close()
    return sorted(out)


def _check_against_haplotypes(haps, needles, hv, rec, ops, myers=True):
    """(a): every record on its materialised haplotype -- columns equal the hit view's, NumPy DP begin (lo = 0), replay.
    The DP runs once per distinct (needle, distance, haplotype symbols it can see): records of haplotypes that are equal
    there have the same answer by definition, whatever the code under test shares."""
    assert len(rec) == len(hv)
    assert np.array_equal(rec["haplotype"], hv["haplotype"]) and np.array_equal(rec["pattern"], hv["pattern"])
    assert np.array_equal(rec["score"], hv["score"])
    if not myers:
        lens = np.array([len(needles[p]) for p in rec["pattern"]], dtype=np.uint64)
        assert np.array_equal(rec["begin"], hv["pos"]) and np.array_equal(rec["end"], hv["pos"] + lens)
        assert np.all(rec["cigar_len"] == 1) and np.array_equal(ops[rec["cigar_off"]], (lens.astype(np.uint32) << 4) | 7)
        for r in rec:
            hp = haps[int(r["haplotype"])]
            assert np.array_equal(hp[int(r["begin"]):int(r["end"])], needles[int(r["pattern"])])
        return
    assert np.array_equal(rec["end"], hv["pos"])
    assert np.all(rec["cigar_len"] <= 2 * rec["score"] + 1) and np.all(rec["cigar_len"] >= 1)
    uniq, pieces, off = {}, [], 0
    u_pat, u_end, u_d, u_lo, which = [], [], [], [], np.empty(len(rec), np.int64)
    for i, r in enumerate(rec):
        p, e, d = int(r["pattern"]), int(r["end"]), int(r["score"])
        hp = haps[int(r["haplotype"])]
        w = hp[max(0, e - (len(needles[p]) + d)):e]           # all an alignment of this hit can use (lo = 0 clips it)
        key = (p, d, w.tobytes())
        if key not in uniq:
            uniq[key] = len(u_pat)
            pieces.append(w)
            u_pat.append(p)
            u_d.append(d)
            u_lo.append(off)
            off += len(w)
            u_end.append(off)
        which[i] = uniq[key]
    T = np.concatenate(pieces)
    b = ref_begins(T, needles, np.array(u_pat), np.array(u_end), np.array(u_d), np.array(u_lo))
    span = (np.array(u_end) - b)[which]
    assert np.array_equal(rec["end"].astype(np.int64) - rec["begin"].astype(np.int64), span), "a begin is not the DP's"
    for r in rec:
        o = int(r["cigar_off"])
        replay(needles[int(r["pattern"])], haps[int(r["haplotype"])], int(r["begin"]), int(r["end"]),
               ops[o:o + int(r["cigar_len"])], int(r["score"]))


def _has_indel(ops):
    return bool(np.any(np.isin(ops & 15, [1, 2])))


def _sharing_asserts(rec, st, jst_st, k):
    n_off = len(np.unique(rec["cigar_off"]))
    print(f"records {len(rec)}, segment hits {jst_st.segment_hits}, segment alignments {st.n_segment_alns}, distinct "
          f"transcripts {n_off}, pool words {st.n_ops}; classes A {st.begin_lane}/{st.begin_wave} "
          f"B {st.cigar_lane}/{st.cigar_wave}/{st.cigar_wave_global}")
    assert st.n_alns == len(rec)
    assert n_off <= st.n_segment_alns <= jst_st.segment_hits
    assert st.n_ops <= (2 * k + 1) * st.n_segment_alns


# ---------------------------------------------------------------------------------------------------------------------
# GPU: tests
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [
    # n_ref, n_hap, n_var, max allele length, algo, |P|, k, block_len, sparse variants
    (60_000, 13, 300, 12, "myers", 40, 2, 256, True),
    (60_000, 100, 400, 40, "myers", 64, 3, 512, True),      # two coverage words, alleles longer than half a window
    (30_000, 64, 80, 300, "myers", 50, 2, 256, False),       # deletions / insertions longer than a block
    (40_000, 7, 1500, 3, "shiftor", 24, 0, 128, False),      # dense variants, exact matcher
    (50_000, 33, 200, 20, "myers", 200, 8, 0, True),         # default block length
    (12_000, 1500, 60, 8, "myers", 32, 1, 256, True),        # two haplotype groups
]
_counts = {}   # cfg -> (records, segment hits) of the rows that have run


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SHAPES)
def test_tree_shapes_equal_per_haplotype_alignments(spm, ctx, cfg):
    _run_shape(spm, ctx, cfg)


def _run_shape(spm, ctx, cfg):
    n_ref, n_hap, n_var, max_len, algo_name, L, k, block, sparse = cfg
    myers = algo_name == "myers"
    rng = np.random.default_rng(n_ref + 7 * n_hap + n_var)
    ref_text = ctx.generate(SEED_TEXT, 0, n_ref)
    ref = ref_text.download(0, n_ref)
    alleles, pool, cov = _random_alleles(rng, n_ref, n_hap, n_var, max_len)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov, n_hap)
    haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
    needles = [_edited(rng, haps[int(rng.integers(0, n_hap))], L, k, myers) for _ in range(24)]
    ps = ctx.patterns(spm.ALGO_MYERS if myers else spm.ALGO_SHIFTOR, needles, k=k)
    window = max(ps.window_size(p) for p in range(len(needles)))

    want = _per_haplotype_route(spm, ctx, haps, ps, spm.ENGINE_BRUTE)
    assert len(want) >= len(needles)

    jst.index(window, block)
    hv, rec, ops, st, jst_st = _jst_records(spm, jst, ps, engine=spm.ENGINE_AUTO, max_hits=1 << 20)
    _check_against_haplotypes(haps, needles, hv, rec, ops, myers)
    if myers:
        assert _has_indel(ops), "no transcript with an insertion or deletion: the row shows nothing"
    _sharing_asserts(rec, st, jst_st, k)
    got = sorted(_rows(rec, ops))
    assert got == want
    if sparse:
        assert len(rec) > jst_st.segment_hits, "no context with several members: transcripts are not shared"
    _counts[cfg] = (len(rec), int(jst_st.segment_hits))

    # the other engine, a larger window with another block length, blocks shorter than |P| (every alignment crosses a block
    # border and starts in a left context): the same records and transcripts
    small = 128 if L == 200 else L // 2
    for win, blk, engine in ((window, block, spm.ENGINE_BRUTE), (window + 37, 1000, spm.ENGINE_AUTO),
                             (window, small, spm.ENGINE_AUTO), (window, small, spm.ENGINE_BRUTE)):
        jst.index(win, blk)
        hv2, rec2, ops2, st2, jst_st2 = _jst_records(spm, jst, ps, engine=engine, max_hits=1 << 20)
        assert np.array_equal(hv2, hv)
        _sharing_asserts(rec2, st2, jst_st2, k)
        assert sorted(_rows(rec2, ops2)) == want, (win, blk, engine)
    jst.close()
    ps.close()
    ref_text.close()


@pytest.mark.gpu
def test_tree_shapes_share_transcripts_over_the_six_rows(spm, ctx):
    """over the six rows together there are more records than segment hits (rows that have not run yet run here)"""
    for cfg in SHAPES:
        if cfg not in _counts:
            _run_shape(spm, ctx, cfg)
    assert sum(c[0] for c in _counts.values()) > sum(c[1] for c in _counts.values()) > 0


@pytest.mark.gpu
def test_alignments_clipped_at_the_first_symbol_of_a_haplotype(spm, ctx):
    """lo = 0 of the haplotype: needles of two extra symbols followed by hap[0 : L - 2]"""
    rng = np.random.default_rng(41)
    n_ref, n_hap, L, k = 20_000, 8, 60, 2
    ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
    # haplotype 1: a replacement at reference position 1 that lengthens it; haplotype 2: a deletion at position 2;
    # the others start like the reference.  A few SNPs further right, shared by several haplotypes.
    rows = [(1, 1, 2, 0), (2, 3, 0, 2), (5000, 1, 1, 2), (9000, 1, 1, 3), (15000, 1, 1, 4)]
    pool = np.array([(int(ref[1]) + 1) & 3, (int(ref[1]) + 2) & 3, (int(ref[5000]) + 1) & 3, (int(ref[9000]) + 1) & 3,
                     (int(ref[15000]) + 2) & 3], dtype=np.uint8)
    cov = np.array([[1 << 1], [1 << 2], [0b10101010], [0b00001111], [0b11000011]], dtype=np.uint64)
    alleles = np.array(rows, dtype=spm.ALLELE_DTYPE)
    ref_text = ctx.upload(ref)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov, n_hap)
    haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
    assert len(haps[1]) == n_ref + 1 and len(haps[2]) == n_ref - 3
    assert not np.array_equal(haps[1][:L], haps[0][:L]) and not np.array_equal(haps[2][:L], haps[0][:L])
    needles = []
    for h in (0, 1, 2):
        hp = haps[h]
        x = (int(hp[0]) + 1) & 3   # two symbols that are not the haplotype's first: they can only be insertions
        needles.append(np.concatenate([[x, x], hp[:L - 2]]).astype(np.uint8))
    needles += [_edited(rng, haps[int(rng.integers(0, n_hap))], L, k) for _ in range(8)]
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    want = _per_haplotype_route(spm, ctx, haps, ps, spm.ENGINE_BRUTE)
    results = []
    for blk, engine in ((256, spm.ENGINE_AUTO), (256, spm.ENGINE_BRUTE), (16, spm.ENGINE_AUTO)):
        jst.index(L + k, blk)
        hv, rec, ops, st, jst_st = _jst_records(spm, jst, ps, engine=engine)
        _check_against_haplotypes(haps, needles, hv, rec, ops)
        for p, h in enumerate((0, 1, 2)):
            m = (rec["haplotype"] == h) & (rec["pattern"] == p) & (rec["end"] == L - 2)
            assert m.sum() == 1, (h, blk)
            r = rec[m][0]
            assert int(r["begin"]) == 0 and int(r["score"]) == 2
            o = int(r["cigar_off"])
            assert ops[o:o + int(r["cigar_len"])].tolist() == [2 << 4 | 1, (L - 2) << 4 | 7]     # 2I (L-2)=
        assert sorted(_rows(rec, ops)) == want
        results.append(hv)
    assert all(np.array_equal(results[0], x) for x in results[1:])
    jst.close()
    ps.close()
    ref_text.close()


@pytest.mark.gpu
def test_c5_shape_wave_classes_over_contexts(spm, ctx):
    """The C5 generator at test size: |P| = 1024, k = 64 over 64 haplotypes, the seed filter; stage A and stage B run
    their wave-per-hit classes over the context buffer.  The needles carry 52 ... 60 edits (insertions and deletions
    among them), so that only a handful of end positions per occurrence stay within k."""
    n_ref, n_hap, L, k = 400_000, 64, 1024, 64
    rng = np.random.default_rng(5)
    ref_text = ctx.generate(SEED_TEXT, 0, n_ref)
    ref = ref_text.download(0, n_ref)
    alleles, pool, cov = spm.synth_variants(SEED_TEXT, SEED_VAR, 0, n_ref, n_hap)
    cov2 = cov.reshape(-1, 1)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov2, n_hap)
    haps = [_apply(ref, alleles, pool, cov2, h) for h in range(n_hap)]
    needles = []
    for i in range(6):
        hp = haps[int(rng.integers(0, n_hap))]
        o = int(rng.integers(0, len(hp) - L - 8))
        nd = hp[o:o + L + 4].copy()
        at = np.sort(rng.choice(np.arange(8, L - 8), size=52 + i, replace=False))
        nd[at] = (nd[at] + 1 + rng.integers(0, 3, len(at))) & 3                 # real substitutions at distinct places
        nd = np.delete(nd, [100 + i, 500])
        nd = np.insert(nd, [300, 800 + i], [(int(nd[300]) + 1) & 3, (int(nd[800 + i]) + 2) & 3])
        needles.append(nd[:L].astype(np.uint8))
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    assert ps.filterable
    jst.index(L + k, 1024)
    hv, rec, ops, st, jst_st = _jst_records(spm, jst, ps, engine=spm.ENGINE_FILTER, max_hits=1 << 22)
    assert jst_st.engine_used == spm.ENGINE_FILTER
    assert len(rec) >= len(needles) and _has_indel(ops)
    assert st.begin_wave > 0 and st.cigar_wave + st.cigar_wave_global > 0
    assert st.n_segment_alns < st.n_alns
    _sharing_asserts(rec, st, jst_st, k)
    _check_against_haplotypes(haps, needles, hv, rec, ops)
    assert sorted(_rows(rec, ops)) == _per_haplotype_route(spm, ctx, haps, ps, spm.ENGINE_AUTO)
    jst.close()
    ps.close()
    ref_text.close()


@pytest.mark.gpu
def test_dna5_begin_only_and_block_shards(spm, ctx):
    rng = np.random.default_rng(17)
    n_ref, n_hap, L, k = 80_000, 20, 60, 2
    ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
    ref[ref == 3] = 4
    ref[rng.integers(0, n_ref, 60)] = 3
    ref_text = ctx.upload(ref, sigma=5)
    alleles, pool, cov = _random_alleles(rng, n_ref, n_hap, 300, 10)
    pool[pool == 3] = 4
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov, n_hap)
    haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
    needles = []
    while len(needles) < 16:
        hp = haps[int(rng.integers(0, n_hap))]
        o = int(rng.integers(0, len(hp) - L - 4))
        nd = hp[o:o + L + 1].copy()
        nd = np.delete(nd, 20) if len(needles) % 2 else np.insert(nd, 30, 0)[:L]
        nd[nd == 3] = 0
        needles.append(nd.astype(np.uint8))
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k, sigma=5)
    assert ps.filterable
    want = _per_haplotype_route(spm, ctx, haps, ps, spm.ENGINE_BRUTE, sigma=5)
    window = L + k
    n_blocks = jst.index(window, 256).n_blocks
    h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
    hv = h.view()
    a = h.align()
    rec, ops, st = a.view(), a.ops, a.stats()
    assert jst.stats().engine_used == spm.ENGINE_FILTER
    _check_against_haplotypes(haps, needles, hv, rec, ops)
    assert _has_indel(ops) and sorted(_rows(rec, ops)) == want and len(want) > 0
    # begins only
    ab = h.align(begin_only=True)
    rb, ob, sb = ab.view(), ab.ops, ab.stats()
    assert np.array_equal(rb["begin"], rec["begin"]) and np.array_equal(rb["end"], rec["end"])
    assert np.array_equal(rb["haplotype"], rec["haplotype"]) and np.array_equal(rb["pattern"], rec["pattern"])
    assert np.all(rb["cigar_len"] == 0) and len(ob) == 0 and sb.n_ops == 0 and sb.n_segment_alns == st.n_segment_alns
    assert ab.device()[3] == 0 and a.device()[1] == len(rec) and a.device()[3] == st.n_ops
    assert re.fullmatch(r"(\d+[=XID])+", a.cigar(0, rec, ops))
    ab.close()
    a.close()
    h.close()
    # block shards: the union of the shards' alignment records is the whole tree's
    cuts = [0, n_blocks // 3, n_blocks // 3 + 1, n_blocks]
    parts = []
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        assert jst.index(window, 256, b0, b1).n_blocks == b1 - b0
        _, r2, o2, _, _ = _jst_records(spm, jst, ps, max_hits=1 << 20)
        parts += _rows(r2, o2)
    assert sorted(parts) == want
    jst.close()
    ps.close()
    ref_text.close()


@pytest.mark.gpu
def test_refusals_and_lifetimes(spm, ctx):
    rng = np.random.default_rng(29)
    n_ref, n_hap, L, k = 40_000, 16, 80, 3

    def make():
        ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
        alleles, pool, cov = _random_alleles(rng, n_ref, n_hap, 120, 10)
        haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
        needles = [_edited(rng, haps[int(rng.integers(0, n_hap))], L, k) for _ in range(16)]
        return ref, alleles, pool, cov, haps, needles

    ref, alleles, pool, cov, haps, needles = make()
    ref_text = ctx.upload(ref)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov, n_hap)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    jst.index(L + k, 256)
    # without the flag: the same records, and a refusal that names the flag
    plain = jst.search_device(ps)
    flagged = jst.search_device(ps, alignable=True)
    assert plain.view().tobytes() == flagged.view().tobytes() and len(plain) > 0
    with pytest.raises(spm.SpmError, match=r"error -1: .*SPM_SCAN_ALIGNABLE"):
        plain.align()
    plain.close()
    # two calls: byte-identical host views
    a1, a2 = flagged.align(), flagged.align()
    assert a1.view().tobytes() == a2.view().tobytes() and a1.ops.tobytes() == a2.ops.tobytes() and len(a1) == len(flagged)
    a1.close()
    a2.close()
    # the tree indexed again after the search: an error, not a crash
    jst.index(L + k, 512)
    with pytest.raises(spm.SpmError, match=r"error -1: .*indexed again"):
        flagged.align()
    flagged.close()
    again = jst.search_device(ps, alignable=True)
    assert len(again.align()) == len(again)
    again.close()
    # a tree closed by its owner: refused, not read
    late = jst.search_device(ps, alignable=True)
    jst.close()
    with pytest.raises(spm.SpmError, match="closed"):
        late.align()
    late.close()
    ps.close()
    ref_text.close()

    # the hits keep tree, reference and needle set alive
    ref, alleles, pool, cov, haps, needles = make()

    def search():
        j = spm.Jst(ctx, ctx.upload(ref), alleles, pool, cov, n_hap)
        j.index(L + k, 256)
        return j.search_device(ctx.patterns(spm.ALGO_MYERS, needles, k=k), alignable=True)

    h = search()
    gc.collect()
    _ = [ctx.upload(rng.integers(0, 4, 1 << 18, dtype=np.uint8)) for _ in range(4)]  # (reuse of freed memory, were it freed)
    hv = h.view()
    a = h.align()
    rec, ops = a.view(), a.ops
    assert len(hv) >= 16
    _check_against_haplotypes(haps, needles, hv, rec, ops)
    a.close()
    h.close()


@pytest.mark.gpu
def test_scale_read_mapping_shape(spm, ctx):
    """2^22 reference bases x 64 haplotypes, 20 000 reads of 150 symbols with up to 3 edits (insertions and deletions
    among them).  The sample sizes below cap the test's time; nothing in a sample may fail."""
    n_ref, n_hap, L, k, n_needles = 1 << 22, 64, 150, 3, 20_000
    n_ref = n_ref // 10_000 * 10_000
    rng = np.random.default_rng(9)
    ref_text = ctx.generate(SEED_TEXT, 0, n_ref)
    ref = ref_text.download(0, n_ref)
    alleles, pool, cov = spm.synth_variants(SEED_TEXT, SEED_VAR, 0, n_ref, n_hap)
    cov2 = cov.reshape(-1, 1)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov2, n_hap)
    haps = [_apply(ref, alleles, pool, cov2, h) for h in range(n_hap)]
    mat = np.stack([_edited(rng, haps[int(rng.integers(0, n_hap))], L, k) for _ in range(n_needles)])
    ps = ctx.patterns(spm.ALGO_MYERS, mat, k=k)
    jst.index(L + k, 0)
    hv, rec, ops, st, jst_st = _jst_records(spm, jst, ps, max_hits=1 << 23)
    assert len(rec) >= n_needles and st.n_alns == len(rec) == len(hv)
    assert st.n_segment_alns < st.n_alns
    _sharing_asserts(rec, st, jst_st, k)
    assert np.array_equal(rec["end"], hv["pos"]) and np.array_equal(rec["score"], hv["score"])
    assert np.array_equal(rec["haplotype"], hv["haplotype"]) and np.array_equal(rec["pattern"], hv["pattern"])
    # every transcript: vectorised run-level checks (needle length consumed, end - begin consumed, cost = score)
    Lr = (ops >> 4).astype(np.int64)
    op = ops & 15
    lens = rec["cigar_len"].astype(np.int64)
    assert np.all(lens > 0)
    rid = np.repeat(np.arange(len(rec)), lens)
    sel = np.repeat(rec["cigar_off"].astype(np.int64), lens) + np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
    Ls, os_ = Lr[sel], op[sel]
    assert np.all(Ls > 0) and np.all(np.isin(os_, [1, 2, 7, 8]))
    q = np.bincount(rid, weights=Ls * np.isin(os_, [1, 7, 8]), minlength=len(rec))
    r = np.bincount(rid, weights=Ls * np.isin(os_, [2, 7, 8]), minlength=len(rec))
    c = np.bincount(rid, weights=Ls * np.isin(os_, [1, 2, 8]), minlength=len(rec))
    assert np.all(q == L)
    assert np.array_equal(r.astype(np.int64), (rec["end"] - rec["begin"]).astype(np.int64))
    assert np.array_equal(c.astype(np.int64), rec["score"].astype(np.int64))
    assert _has_indel(ops)
    # NumPy DP begins and symbol-level replay on a fixed-seed sample
    samp = np.sort(np.random.default_rng(1).choice(len(rec), size=min(20_000, len(rec)), replace=False))
    _check_against_haplotypes(haps, mat, hv[samp], rec[samp], ops)
    # full equality with the route without the tree on 4 of the 64 haplotypes
    only = (0, 21, 42, 63)
    m = np.isin(rec["haplotype"], only)
    assert sorted(_rows(rec[m], ops)) == _per_haplotype_route(spm, ctx, haps, ps, spm.ENGINE_AUTO, only=only)
    jst.close()
    ps.close()
    ref_text.close()


@pytest.mark.gpu
def test_cpp_locate_on_the_fixtures(spm, tmp_path):
    """tests/cpp/jst_locate_cases.cpp: locate through the device tree == locate_host == batch locate per fixture haplotype"""
    exe = _build_locate_cases(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 50, r.stdout[-2000:]
    moved = [int(x) for x in re.findall(r"(\d+) with begin != end - \|P\|", r.stdout)]
    assert len(moved) == 8 and sum(moved) > 0
