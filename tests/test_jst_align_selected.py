"""Begins and CIGAR transcripts of the records a pan-genome SELECTION kept (spm_hip_jst_selection_align,
JstHits.align_selected; contract in include/spm_hip.h, scheme in DESIGN.md 4.6).  The kept records are located in the tree's
index -- the search's fan-out inverted per record --, their distinct segment hits aligned once and gathered.

The yardsticks never come from the code under test:
  (a) `_check_against_haplotypes` of test_jst_align on the materialised haplotypes: NumPy DP begin with lo = 0, CIGAR replay,
      with the selection's host view as the hit view;
  (b) align() of an alignable search over the same tree and set (the existing entry point, itself pinned to (a)), matched by
      (haplotype, pattern, end, score): equal begins, equal transcript WORDS (never offsets).
The arithmetic of the inversion is checked first on the host alone, against a NumPy statement of the fan-out."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cpp_programs import download
from test_gpu_jst import _apply, _random_alleles
from test_jst_align import SEED_TEXT, SEED_VAR, SHAPES, _check_against_haplotypes, _edited, _rows
from test_jst_select import JH, ROWS, device_view, jrule, tree_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
MYERS_ROWS = [r for r in ROWS if r[6] == "myers"]

# ---------------------------------------------------------------------------------------------------------------------
# CPU: the prototype, the unchanged layout, the binding
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stdio.h>
#include "spm_hip.h"
int main(void)
{
    int (*f)(spm_jst_hits *, uint32_t, spm_jst_alns **) = spm_hip_jst_selection_align;
    printf("%u %u %u\n", (unsigned)sizeof(spm_jst_align_stats), (unsigned)sizeof(spm_jst_aln), SPM_ALIGN_BEGIN_ONLY);
    return f == 0;
}
"""


def test_prototype_layout_and_binding(spm, tmp_path):
    src, exe = tmp_path / "proto.c", tmp_path / "proto"
    src.write_text(LAYOUT_C)
    lib = os.path.join(ROOT, "libspm_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-L" + lib, "-l:libspm_hip.so", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.check_output([str(exe)], text=True).split() == ["80", "40", "1"]
    assert ctypes.sizeof(spm.capi.JstAlignStats) == 80 and ctypes.sizeof(spm.capi.JstAln) == 40
    assert "spm_hip_jst_selection_align" in spm.capi.EXPORTS and hasattr(spm.capi.lib(), "spm_hip_jst_selection_align")
    assert callable(spm.JstHits.align_selected)
    assert "selection" in spm.JstAlignments.device.__doc__       # documented as matched to the selection's device()


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the fan-out and its inverse, in NumPy alone
# ---------------------------------------------------------------------------------------------------------------------
GROUP = 1024          # haplotypes whose contexts are compared with each other
NONE = 0xFFFF


def _origins(n_ref, alleles, cov, h):
    """for every symbol of haplotype h the reference position it stems from (an alt symbol: its allele's position); the
    sibling of test_gpu_jst._apply"""
    out, r = [], 0
    for i, a in enumerate(alleles):
        if not (int(cov[i, h >> 6]) >> (h & 63)) & 1:
            continue
        p, rl, al = int(a["pos"]), int(a["ref_len"]), int(a["alt_len"])
        out.append(np.arange(r, p, dtype=np.int64))
        out.append(np.full(al, p, dtype=np.int64))
        r = min(n_ref, p + rl)
    out.append(np.arange(r, n_ref, dtype=np.int64))
    return np.concatenate(out)


class Model:
    """The index as the header states it: block j owns the haplotype symbols that stem from reference positions
    [jL, (j + 1)L); a context is what a (block, haplotype) owns plus window - 1 symbols of left context; equal contexts of one
    (block, haplotype group) cell are laid out once."""

    def __init__(self, t, block, window, jb=0, je=None):
        n_ref, self.n_hap, self.window = len(t["ref"]), t["n_hap"], window
        self.n_blocks = max(1, -(-n_ref // block))
        self.jb, self.je = jb, self.n_blocks if je is None else je
        self.n_groups = -(-self.n_hap // GROUP)
        self.hap_start = np.zeros((self.n_blocks + 1, self.n_hap), dtype=np.int64)
        for h in range(self.n_hap):
            org = _origins(n_ref, t["alleles"], t["cov"], h)
            assert len(org) == len(t["haps"][h])
            self.hap_start[:, h] = np.searchsorted(org, np.arange(self.n_blocks + 1) * block, side="left")
        nb = self.je - self.jb
        self.local_id = np.full((nb, self.n_hap), NONE, dtype=np.int64)
        self.ctx_base = np.zeros(nb * self.n_groups + 1, dtype=np.int64)
        off, owned, members = [0], [], []
        for jr in range(nb):
            j = self.jb + jr
            for g in range(self.n_groups):
                seen = {}
                for h in range(g * GROUP, min(self.n_hap, (g + 1) * GROUP)):
                    a, b = int(self.hap_start[j, h]), int(self.hap_start[j + 1, h])
                    if b <= a:
                        continue
                    lo = a - min(window - 1, a)
                    key = (a - lo, t["haps"][h][lo:b].tobytes())
                    if key not in seen:
                        seen[key] = len(seen)
                        off.append(off[-1] + b - lo)
                        owned.append(a - lo)
                        members.append([])
                    self.local_id[jr, h] = seen[key]
                    members[len(owned) - len(seen) + seen[key]].append(h)
                self.ctx_base[jr * self.n_groups + g + 1] = len(owned)
        self.ctx_off, self.ctx_owned, self.members = np.array(off, dtype=np.int64), np.array(owned, dtype=np.int64), members
        self.n_ctx = len(owned)

    def ctx_lo(self, j, h):
        a = self.hap_start[j, h]
        return a - np.minimum(self.window - 1, a)

    def fan_out(self, c, local, span_to_last):
        """the search's fan-out: the segment hit at buffer position ctx_off[c] + local, whose last symbol is
        local + span_to_last, for every member haplotype -> (haplotype, pos); nothing if it ends in the left context"""
        if local + span_to_last < self.ctx_owned[c]:
            return []
        cell = int(np.searchsorted(self.ctx_base, c, side="right")) - 1
        j = self.jb + cell // self.n_groups
        return [(h, int(self.ctx_lo(j, h)) + local) for h in self.members[c]]

    def locate(self, h, pos, span_to_last):
        """the inverse, vectorised over the records (h: one haplotype; pos: array): buffer positions, -1 where a record
        cannot be located.  span_to_last: -1 (Myers: pos is the exclusive end) or |P| - 1 (exact: pos is the begin)."""
        pos = np.asarray(pos, dtype=np.int64)
        last = pos + span_to_last
        col = self.hap_start[self.jb:self.je + 1, h]
        j = np.searchsorted(col, last, side="right") - 1          # the largest j with hap_start[j][h] <= last
        ok = (last >= 0) & (j >= 0) & (j < self.je - self.jb)
        jr = np.where(ok, j, 0)
        lid = self.local_id[jr, h]
        ok &= lid != NONE
        cell = jr * self.n_groups + h // GROUP
        c = np.where(ok, self.ctx_base[cell] + lid, 0)
        ok &= c < self.ctx_base[cell + 1]
        lo = self.ctx_lo(self.jb + jr, h)
        rel = last - lo
        ok &= (pos >= lo) & (rel >= self.ctx_owned[c]) & (rel < self.ctx_off[c + 1] - self.ctx_off[c])
        return np.where(ok, self.ctx_off[c] + pos - lo, -1), np.where(ok, c, -1)


@pytest.mark.parametrize("row", [ROWS[1], ROWS[2], ROWS[5]], ids=lambda r: r[0])
@pytest.mark.parametrize("shard", [False, True], ids=["whole", "shard"])
def test_inverse_of_the_fan_out_in_numpy(row, shard):
    """Every position of every context that the fan-out would report, for every member haplotype: the inverse gives back the
    context and the buffer position.  That covers a last symbol that is the last / the first owned symbol of a block, and a
    context that starts at the haplotype's first symbol.  Then the records that cannot be located."""
    t = tree_of(row)
    myers, L = t["myers"], t["L"]
    window = L + t["k"]
    span = -1 if myers else L - 1
    block = t["small_block"] if shard else 256
    probe = Model(t, block, window)
    jb, je = (probe.n_blocks // 3, probe.n_blocks // 3 * 2) if shard else (0, probe.n_blocks)
    M = probe if not shard else Model(t, block, window, jb, je)
    got = {h: ([], [], []) for h in range(M.n_hap)}
    n_first = n_last = n_start = 0
    for c in range(M.n_ctx):
        n = int(M.ctx_off[c + 1] - M.ctx_off[c])
        lo_local = max(int(M.ctx_owned[c]) - span, 0 if not myers else 1)
        locals_ = np.arange(lo_local, n - span)                  # every position whose last symbol is owned
        cell = int(np.searchsorted(M.ctx_base, c, side="right")) - 1
        j = M.jb + cell // M.n_groups
        for h in M.members[c]:
            base = int(M.ctx_lo(j, h))
            assert M.fan_out(c, int(locals_[0]), span)[M.members[c].index(h)] == (h, base + int(locals_[0]))
            got[h][0].append(base + locals_)
            got[h][1].append(M.ctx_off[c] + locals_)
            got[h][2].append(np.full(len(locals_), c))
            n_start += base == 0
    for h in range(M.n_hap):
        pos, want_at, want_c = (np.concatenate(x) for x in got[h])
        assert len(np.unique(pos)) == len(pos)                   # the fan-out is a bijection: no haplotype position twice
        a, b = int(M.hap_start[M.jb, h]), int(M.hap_start[M.je, h])
        # ... and every owned symbol is the last one of exactly one (the first |P| - 1 symbols of a haplotype end no exact hit)
        assert np.array_equal(np.sort(pos + span), np.arange(max(a, span), b))
        at, c = M.locate(h, pos, span)
        assert np.array_equal(at, want_at) and np.array_equal(c, want_c)
        # the named boundaries: the last symbol is the last owned symbol of a block / the first of the next
        edges = np.unique(M.hap_start[M.jb + 1:M.je, h])
        edges = edges[(edges > a) & (edges < b)]
        for e_last, counter in ((edges - 1, "last"), (edges, "first")):
            at, c = M.locate(h, e_last - span, span)
            assert np.all(at >= 0)
            own = M.ctx_owned[c] + M.ctx_off[c]
            if counter == "first":
                assert np.array_equal(at + span, own)            # the first owned symbol of its context
                n_first += len(at)
            else:
                assert np.array_equal(at + span + 1, M.ctx_off[c + 1])       # the last symbol of its context
                n_last += len(at)
        # records that cannot be located: beyond the indexed blocks on either side, no last symbol at all
        for bad in ([b - span, b - span + 5, b + 10 ** 6], [a - span - 1] if a else [], [0] if myers else []):
            if len(bad) and min(bad) >= 0:
                at, _ = M.locate(h, bad, span)
                assert np.all(at == -1), (h, bad)
    assert n_first > 0 and n_last > 0 and (shard or n_start >= M.n_hap)
    if not shard and myers:
        # a Myers hit that ends at |P| exactly: the context starts at the haplotype's first symbol, ctx_lo = 0
        at, c = M.locate(0, [L], span)
        assert at[0] == M.ctx_off[c[0]] + L and M.ctx_owned[c[0]] == 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ---------------------------------------------------------------------------------------------------------------------
ALN = np.dtype([("begin", "<u8"), ("end", "<u8"), ("haplotype", "<u4"), ("pattern", "<u4"), ("score", "<i4"),
                ("cigar_off", "<u4"), ("cigar_len", "<u4"), ("reserved", "<u4")])


def aln_device_view(ctx, a):
    """the records behind JstAlignments.device(), downloaded in their device order"""
    ptr, n, _, _ = a.device()
    return download(ctx, ptr, n, ALN)


def _open(spm, ctx, t):
    ref_text = ctx.upload(t["ref"], sigma=t["sigma"])
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS if t["myers"] else spm.ALGO_SHIFTOR, t["needles"], k=t["k"], sigma=t["sigma"])
    return ref_text, jst, ps


def _full_map(h):
    """yardstick (b): (haplotype, pattern, end, score) -> (begin, transcript words) of align() of an alignable search"""
    a = h.align()
    rec, ops, st = a.view(), a.ops, a.stats()
    a.close()
    out = {(hp, p, e, s): (b, w) for hp, b, e, p, s, w in _rows(rec, ops)}
    assert len(out) == len(rec)
    return out, st


def _check_b(rec, ops, full):
    for hp, b, e, p, s, w in _rows(rec, ops):
        assert full[(hp, p, e, s)] == (b, w), (hp, p, e, s)


def _check_all(spm, ctx, t, sel, full, full_st, sample=None, needles=None):
    """both yardsticks, the counts, the device view, the sharing of one align_selected(); returns (records, ops, stats)"""
    a = sel.align_selected()
    hv, rec, ops, st = sel.view(), a.view(), a.ops, a.stats()
    assert st.n_alns == len(rec) == len(sel) == len(hv) == len(a)
    pick = np.arange(len(rec)) if sample is None or len(rec) <= sample else \
        np.sort(np.random.default_rng(1).choice(len(rec), size=sample, replace=False))
    _check_against_haplotypes(t["haps"], t["needles"] if needles is None else needles, hv[pick], rec[pick], ops, t["myers"])
    assert np.array_equal(rec["haplotype"], hv["haplotype"]) and np.array_equal(rec["pattern"], hv["pattern"])
    assert np.array_equal(rec["score"], hv["score"])
    _check_b(rec, ops, full)
    # the device view: record i belongs to record i of the selection's device view
    dv, da = device_view(ctx, sel), aln_device_view(ctx, a)
    assert len(da) == len(dv)
    for f in ("haplotype", "pattern", "score"):
        assert np.array_equal(da[f], dv[f]), f
    assert np.array_equal(da["end"] if t["myers"] else da["begin"], dv["pos"])
    assert np.all(da["reserved"] == 0)
    assert sorted(_rows(da, ops)) == sorted(_rows(rec, ops))
    # the pool: one slot per distinct segment hit
    n_off = len(np.unique(rec["cigar_off"])) if len(rec) else 0
    assert n_off == st.n_segment_alns <= min(st.n_alns, full_st.n_segment_alns)
    assert st.n_ops == len(ops) == int(np.sum(2 * rec["score"][np.unique(rec["cigar_off"], return_index=True)[1]] + 1)
                                      if t["myers"] else n_off)
    a.close()
    return rec, ops, st


# ---------------------------------------------------------------------------------------------------------------------
# GPU: 1. tree rows
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_tree_rows_meet_both_yardsticks(spm, ctx, row):
    t = tree_of(row)
    ref_text, jst, ps = _open(spm, ctx, t)
    window = max(ps.window_size(p) for p in range(len(t["needles"])))
    modes = [dict(), dict(best=0)] + ([dict(best=0, across=True)] if t["myers"] else [dict(window=2)])
    for blk in (t["small_block"], 256):
        jst.index(window, blk)
        h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
        full, full_st = _full_map(h)
        for m in modes:
            sel = h.select(**m)
            assert 0 < len(sel) <= len(h)
            rec, ops, st = _check_all(spm, ctx, t, sel, full, full_st)
            if t["n_hap"] == 70 and not m:
                # records of different haplotypes share one transcript
                assert st.n_segment_alns < st.n_alns
                by_off = {}
                for r in rec:
                    by_off.setdefault(int(r["cigar_off"]), set()).add(int(r["haplotype"]))
                assert max(len(s) for s in by_off.values()) >= 2
            sel.close()
        h.close()
    jst.close()
    ps.close()
    ref_text.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: 2. block boundaries
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_hits_that_end_at_block_borders_and_at_the_needle_length(spm, ctx):
    """Haplotype 0 carries no variant left of reference position 6000: there its coordinates are the reference's, and with
    block 256 a hit that ends at 256 j has its last symbol on the last owned symbol of block j - 1, one that ends at 256 j + 1
    on the first owned symbol of block j.  Needles cut so that their occurrences end exactly there, and at |P|."""
    rng = np.random.default_rng(77)
    n_ref, n_hap, L, k = 16_000, 6, 64, 2
    ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
    alleles, pool, cov = _random_alleles(rng, n_ref, n_hap, 60, 8)
    for i, a in enumerate(alleles):
        if int(a["pos"]) < 6000:
            cov[i, 0] &= ~np.uint64(1)                       # haplotype 0: nothing left of 6000 (the others keep theirs)
            if cov[i, 0] == 0:
                cov[i, 0] = np.uint64(2)
    # ... and a deletion of 800 reference positions from 8000 on, carried by haplotypes 1 and 2: blocks 32 and 33 own nothing
    # there (equal consecutive block starts, cells without a context)
    keep = (alleles["pos"] < 7980) | (alleles["pos"] > 8810)
    alleles, cov = alleles[keep], cov[keep]
    at = int(np.searchsorted(alleles["pos"], 8000))
    alleles = np.insert(alleles, at, np.array([(8000, 800, 0, 0)], dtype=alleles.dtype))
    cov = np.insert(cov, at, np.array([[0b110]], dtype=np.uint64), axis=0)
    haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
    assert np.array_equal(haps[0][:6000], ref[:6000]) and any(len(hp) != n_ref for hp in haps)
    ends = [256 * 3, 256 * 3 + 1, 256 * 7, 256 * 7 + 1, 256 * 20, 256 * 20 + 1, L]
    needles = [ref[e - L:e].copy() for e in ends]
    x = (int(ref[0]) + 1) & 3
    needles.append(np.concatenate([[x, x], ref[:L - 2]]).astype(np.uint8))       # ends at L - 2, begin clipped at 0
    ends.append(L - 2)
    t = dict(ref=ref, alleles=alleles, pool=pool, cov=cov, haps=haps, myers=True, L=L, k=k, n_hap=n_hap, sigma=4)
    M = Model(t, 256, L + k)
    assert np.all(M.local_id[32:34, 1:3] == NONE) and np.all(M.local_id[32:34, 0] != NONE)
    assert M.hap_start[32, 1] == M.hap_start[33, 1] == M.hap_start[34, 1]
    joint = int(M.hap_start[34, 1])                          # haplotype 1: the first symbol right of the deletion
    across_gap = len(needles)
    needles.append(haps[1][joint - L // 2:joint + L // 2].copy())                # half on either side of the deletion
    needles += [_edited(rng, haps[int(rng.integers(0, n_hap))], L, k) for _ in range(6)]
    t["needles"] = needles
    ref_text, jst, ps = _open(spm, ctx, t)
    jst.index(L + k, 256)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
    full, full_st = _full_map(h)
    for m in (dict(), dict(best=0)):
        sel = h.select(**m)
        rec, ops, st = _check_all(spm, ctx, t, sel, full, full_st)
        for p, e in enumerate(ends):
            hit = rec[(rec["haplotype"] == 0) & (rec["pattern"] == p) & (rec["end"] == e)]
            assert len(hit) == 1, (p, e)                     # the planted occurrence is its locus' best record
            assert int(hit[0]["score"]) == (0 if p < 7 else 2)
            assert int(hit[0]["begin"]) == (e - L if p < 7 else 0)
        for hp in (1, 2):                                    # the locus whose last symbol lies behind two empty cells
            hit = rec[(rec["haplotype"] == hp) & (rec["pattern"] == across_gap) & (rec["score"] == 0)]
            want_end = int(M.hap_start[34, hp]) + L // 2
            assert len(hit) == 1 and int(hit[0]["end"]) == want_end and int(hit[0]["begin"]) == want_end - L
        sel.close()
    h.close()
    jst.close()
    ps.close()
    ref_text.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: 3. empty cells, two haplotype groups
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cfg", [SHAPES[2], SHAPES[5]], ids=["alleles longer than a block", "two haplotype groups"])
def test_empty_cells_and_haplotype_groups(spm, ctx, cfg):
    assert cfg in ((30_000, 64, 80, 300, "myers", 50, 2, 256, False), (12_000, 1500, 60, 8, "myers", 32, 1, 256, True))
    n_ref, n_hap, n_var, max_len, _, L, k, block, _ = cfg
    rng = np.random.default_rng(n_ref + 7 * n_hap + n_var)       # the tree of test_jst_align's row
    ref_text = ctx.generate(SEED_TEXT, 0, n_ref)
    ref = ref_text.download(0, n_ref)
    alleles, pool, cov = _random_alleles(rng, n_ref, n_hap, n_var, max_len)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov, n_hap)
    haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
    needles = [_edited(rng, haps[int(rng.integers(0, n_hap))], L, k) for _ in range(24)]
    t = dict(haps=haps, needles=needles, myers=True)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    # (alleles of up to 300 positions against blocks of 256: by the NumPy statement above none of them happens to empty a
    # whole cell of this tree; cells that own nothing are planted in the block-border test)
    jst.index(L + k, block)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 21)
    full, full_st = _full_map(h)
    for m in (dict(), dict(best=0, across=True)):
        sel = h.select(**m)
        assert len(sel) > 0
        rec, ops, st = _check_all(spm, ctx, t, sel, full, full_st, sample=2000)
        if n_hap > 1024 and not m:
            assert set((rec["haplotype"] >= 1024).tolist()) == {False, True}     # records in both haplotype groups
        sel.close()
    h.close()
    jst.close()
    ps.close()
    ref_text.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: 4. a block shard; 5. begins only
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_block_shard_and_reindexing(spm, ctx):
    t = tree_of(ROWS[1])
    ref_text, jst, ps = _open(spm, ctx, t)
    window = t["L"] + t["k"]
    n_blocks = jst.index(window, 256).n_blocks
    cut = n_blocks // 2
    assert jst.index(window, 256, cut, n_blocks).n_blocks == n_blocks - cut      # jb != 0
    h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
    full, full_st = _full_map(h)
    first = h.select()
    assert 0 < len(first) < len(h)
    _check_all(spm, ctx, t, first, full, full_st)
    h.close()
    assert jst.index(window, 256, 0, cut).n_blocks == cut                        # the other shard
    with pytest.raises(spm.SpmError, match=r"error -1: .*indexed again"):
        first.align_selected()
    h2 = jst.search_device(ps, alignable=True, max_hits=1 << 20)
    full2, full_st2 = _full_map(h2)
    fresh = h2.select()
    assert len(fresh) > 0
    _check_all(spm, ctx, t, fresh, full2, full_st2)
    jst.close()
    ps.close()


@gpu
def test_begins_only(spm, ctx):
    t = tree_of(ROWS[1])
    ref_text, jst, ps = _open(spm, ctx, t)
    jst.index(t["L"] + t["k"], 256)
    sel = jst.search_device(ps, max_hits=1 << 20).select()
    a, b = sel.align_selected(), sel.align_selected(begin_only=True)
    ra, rb = a.view(), b.view()
    for f in ("begin", "end", "haplotype", "pattern", "score"):
        assert np.array_equal(ra[f], rb[f]), f
    assert np.any(ra["begin"] != ra["end"] - t["L"])             # some begin is not end - |P|: the begins were computed
    assert np.all(rb["cigar_len"] == 0) and np.all(rb["cigar_off"] == 0) and len(b.ops) == 0
    sa, sb = a.stats(), b.stats()
    assert sb.n_ops == 0 and b.device()[3] == 0 and sb.n_segment_alns == sa.n_segment_alns and sa.n_ops == a.device()[3] > 0
    assert np.array_equal(aln_device_view(ctx, b)["begin"], aln_device_view(ctx, a)["begin"])
    jst.close()
    ps.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: 6. counts around a workgroup
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_counts_around_a_workgroup_and_an_empty_selection(spm, ctx):
    seen = []
    for row, m in ((ROWS[0], dict(best=0)), (ROWS[4], dict()), (ROWS[2], dict()), (ROWS[2], dict(loci=False))):
        t = tree_of(row)
        ref_text, jst, ps = _open(spm, ctx, t)
        jst.index(t["L"] + t["k"], 256)
        h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
        full, full_st = _full_map(h)
        sel = h.select(**m)
        seen.append(len(sel))
        _check_all(spm, ctx, t, sel, full, full_st, sample=1500)
        jst.close()
        ps.close()
    print("kept records:", seen)
    assert 0 < seen[0] < 64 and 0 < seen[1] < 64                 # less than one wave
    assert seen[2] > 256 and seen[2] % 256 != 0                  # several workgroups, the last one partly filled
    assert seen[3] > 1024 and seen[3] % 256 != 0
    # a needle that occurs nowhere: an empty selection gives an empty result
    t = tree_of(ROWS[0])
    ref_text = ctx.upload(t["ref"])
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS, [np.random.default_rng(404).integers(0, 4, 64, dtype=np.uint8)], k=1)
    jst.index(65, 256)
    sel = jst.search_device(ps).select()
    assert len(sel) == 0
    for begin_only in (False, True):
        a = sel.align_selected(begin_only=begin_only)
        st = a.stats()
        assert len(a) == 0 and len(a.view()) == 0 and len(a.ops) == 0 and st.n_alns == st.n_segment_alns == st.n_ops == 0
        assert a.device()[1] == 0
    jst.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: 7. object rules
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_object_rules_and_refusals(spm, ctx):
    t = tree_of(ROWS[1])
    ref_text, jst, ps = _open(spm, ctx, t)
    k = t["k"]
    jst.index(t["L"] + k, 256)
    h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
    full, full_st = _full_map(h)
    h.close()
    plain = jst.search_device(ps, max_hits=1 << 20)              # NOT alignable
    once = plain.select()
    twice = once.select(best=0)
    across = once.select(best=0, across=True)
    flagless = plain.select(loci=False)                          # a sorted copy of everything
    assert len(flagless) == len(plain) == len(full)
    with pytest.raises(spm.SpmError, match=r"error -1: .*spm_hip_jst_hits_align"):     # a search's own result
        plain.align_selected()
    plain.close()                                                # the source is gone before anything is aligned
    rec1, ops1, _ = _check_all(spm, ctx, t, once, full, full_st)
    rec2, ops2, _ = _check_all(spm, ctx, t, twice, full, full_st)
    recx, _, _ = _check_all(spm, ctx, t, across, full, full_st)
    recf, opsf, stf = _check_all(spm, ctx, t, flagless, full, full_st)
    assert stf.n_segment_alns == full_st.n_segment_alns          # everything kept: every segment alignment of the full route
    again = once.select()                                        # a selection of a selection: the same records
    rec3, ops3, _ = _check_all(spm, ctx, t, again, full, full_st)
    assert rec3.tobytes() == rec1.tobytes() and ops3.tobytes() == ops1.tobytes()
    assert len(rec2) == len(jrule(once.view(), k, best=0)) <= len(rec1)
    assert 0 < len(recx) == len(jrule(once.view(), k, best=0, across=True)) < len(rec1)
    # two calls: byte-identical host views
    a1, a2 = once.align_selected(), once.align_selected()
    assert a1.view().tobytes() == a2.view().tobytes() == rec1.tobytes() and a1.ops.tobytes() == a2.ops.tobytes()
    # the old entry point still refuses a selection, and says so
    with pytest.raises(spm.SpmError, match=r"error -1: .*selection"):
        once.align()
    # a selection out of a raw record buffer names no tree
    import torch
    buf = torch.from_numpy(np.ascontiguousarray(once.view()).view(np.int64).reshape(-1, 3).copy()).to("cuda")
    torch.cuda.synchronize()
    raw = spm.select_jst_records(ctx, buf.data_ptr(), len(once), ps)
    assert len(raw) == len(once)
    with pytest.raises(spm.SpmError, match=r"error -1: .*spm_hip_jst_records_select"):
        raw.align_selected()
    # unknown flag bits, NULL arguments
    L = spm.capi.lib()
    out = ctypes.c_void_p()
    assert L.spm_hip_jst_selection_align(once._h, 2, ctypes.byref(out)) == -1
    assert L.spm_hip_jst_selection_align(once._h, 0x80000001, ctypes.byref(out)) == -1
    assert L.spm_hip_jst_selection_align(None, 0, ctypes.byref(out)) == -1
    assert L.spm_hip_jst_selection_align(once._h, 0, None) == -1
    # a tree closed by its owner: refused, not read
    jst.close()
    with pytest.raises(spm.SpmError, match="closed"):
        once.align_selected()
    ps.close()
    ref_text.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: 9. one scale case
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_scale_read_mapping_shape(spm, ctx):
    """The read-mapping shape of test_jst_align at its size: 2^22 reference bases x 64 haplotypes, 20 000 reads of 150 symbols
    with up to 3 edits.  select() + align_selected(); yardstick (b) on all records, (a) on a sample of 500."""
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
    h = jst.search_device(ps, alignable=True, max_hits=1 << 23)
    fa = h.align()
    frec, fops, full_st = fa.view(), fa.ops, fa.stats()
    fa.close()
    sel = h.select()
    a = sel.align_selected()
    hv, rec, ops, st = sel.view(), a.view(), a.ops, a.stats()
    print(f"records in {len(frec)}, kept {len(rec)}; n_alns {st.n_alns}, n_segment_alns {st.n_segment_alns} (all records: "
          f"{full_st.n_segment_alns}), pool words {st.n_ops}; ms locate+order+gather {st.ms_fanout:.3f}, begins "
          f"{st.ms_begin:.3f}, transcripts {st.ms_cigar:.3f}, device total {st.ms_total:.3f}, host {st.ms_host:.3f} "
          f"(work list {st.ms_worklist:.3f}); all records: device {full_st.ms_total:.3f}, host {full_st.ms_host:.3f}")
    assert n_needles <= st.n_alns == len(rec) == len(hv) == len(sel) < len(frec)
    assert st.n_segment_alns <= full_st.n_segment_alns and st.n_segment_alns < st.n_alns
    assert len(np.unique(rec["cigar_off"])) == st.n_segment_alns
    for f in ("haplotype", "pattern", "score"):
        assert np.array_equal(rec[f], hv[f]), f
    assert np.array_equal(rec["end"], hv["pos"])
    # (b) on all records, vectorised: the same record of the full route, by (haplotype, pattern, end, score)
    def key(r):
        return np.lexsort((r["score"], r["end"], r["pattern"], r["haplotype"]))
    cols = lambda r: np.stack([r["haplotype"].astype(np.int64), r["pattern"].astype(np.int64), r["end"].astype(np.int64),
                               r["score"].astype(np.int64)], axis=1)
    fo = key(frec)
    fs = frec[fo]
    fk, sk = cols(fs), cols(rec)
    pack = lambda c: (c[:, 0] << 48) | (c[:, 1] << 26) | c[:, 2]     # 64 haplotypes, 20 000 needles, ends below 2^26
    assert len(np.unique(pack(fk))) == len(fk)
    at = np.searchsorted(pack(fk), pack(sk))
    assert np.array_equal(fk[at], sk)
    m = fs[at]
    assert np.array_equal(m["begin"], rec["begin"]) and np.array_equal(m["cigar_len"], rec["cigar_len"])
    width = int(rec["cigar_len"].max())
    for w in range(width):
        on = rec["cigar_len"] > w
        assert np.array_equal(ops[rec["cigar_off"][on] + w], fops[m["cigar_off"][on] + w])
    # (a) on a sample of 500
    samp = np.sort(np.random.default_rng(1).choice(len(rec), size=500, replace=False))
    _check_against_haplotypes(haps, mat, hv[samp], rec[samp], ops)
    da, dv = aln_device_view(ctx, a), device_view(ctx, sel)
    assert np.array_equal(da["end"], dv["pos"]) and np.array_equal(da["haplotype"], dv["haplotype"])
    assert np.array_equal(da["pattern"], dv["pattern"])
    jst.close()
    ps.close()
    ref_text.close()
