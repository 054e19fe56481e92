"""Mate rescue: spm_hip_jst_pairs_rescue behind the chain ... -> collapse -> reads -> pairs, and its Python binding.

The expected answer never comes from the code under test.  The rule is written again here: the jobs of a pair record, the
window and the admissible ends in a few lines, the distance of every end from oracle.sellers over the window, the begin
from the reference DP of test_align.py (ref_begins), concordance, tlen and flag from the lines of the header.  Transcripts
are checked with the replayer of test_align.py: the rule has no traceback of its own, so of a record everything but the number
of CIGAR words is compared byte for byte, and the words are replayed against needle and reference."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cpp_programs import ROOT, build_cases, build_mirror, c_layout, download
from test_align import ref_begins, replay
from test_jst_project import _hap, _make_tree, _window
from test_pairs import _chain, _free_stretches
from test_strands import np_revcomp

gpu = pytest.mark.gpu
RESCUE = np.dtype([("ref_begin", "<u8"), ("ref_end", "<u8"), ("pair", "<u4"), ("pattern", "<u4"), ("anchor", "<u4"),
                   ("score", "<i4"), ("cigar_off", "<u4"), ("cigar_len", "<u4"), ("tlen", "<i4"), ("flag", "<u2"), ("status", "<u2")])
RESCUED, NOTHING, NOT_CONCORDANT = 0, 1, 2
NONE = 0xFFFFFFFF
COUNTS = ("n_jobs", "n_rescued", "n_none", "n_not_concordant", "n_short", "max_window")
MIN_TLEN, MAX_TLEN, K_SEARCH, K = 100, 180, 2, 6


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the case program, the layouts, the names
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_case_program(tmp_path, sanitize):
    exe = build_cases("jst_rescue_core_cases.cpp", tmp_path, include=[os.path.join(ROOT, "include")], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 1000, r.stdout[-500:]


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_jst_rescue_opts, f))
#define F(f) printf("rescue.%s %zu\n", #f, offsetof(spm_jst_rescue, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_jst_rescues_stats, f))
int main(void)
{
    O(min_tlen); O(max_tlen); O(k); O(flags); O(reserved);
    F(ref_begin); F(ref_end); F(pair); F(pattern); F(anchor); F(score); F(cigar_off); F(cigar_len); F(tlen); F(flag); F(status);
    S(ms_total); S(ms_jobs); S(ms_search); S(ms_align); S(ms_emit); S(ms_host); S(n_pairs); S(n_jobs); S(n_rescued); S(n_none);
    S(n_not_concordant); S(n_short); S(max_window);
    printf("sizeof.opts %zu\nsizeof.rescue %zu\nsizeof.stats %zu\n", sizeof(spm_jst_rescue_opts), sizeof(spm_jst_rescue),
           sizeof(spm_jst_rescues_stats));
    printf("status.values %d\n", SPM_RESCUE_RESCUED + 10 * SPM_RESCUE_NONE + 100 * SPM_RESCUE_NOT_CONCORDANT);
    return 0;
}
"""
CALLS = ("spm_hip_jst_pairs_rescue", "spm_hip_jst_rescues_view", "spm_hip_jst_rescues_device", "spm_hip_jst_rescues_stats",
         "spm_hip_jst_rescues_destroy")


def test_layouts_and_names(spm, tmp_path):
    import inspect
    assert ctypes.sizeof(spm.capi.JstRescueOpts) == 20 and ctypes.sizeof(spm.capi.JstRescuesStats) == 80
    assert ctypes.sizeof(spm.capi.JstRescue) == 48 == spm.JST_RESCUE_DTYPE.itemsize and spm.JST_RESCUE_DTYPE == RESCUE
    assert np.dtype(spm.capi.JstRescue) == RESCUE
    want = c_layout(tmp_path, LAYOUT_C)
    assert (int(want.pop("sizeof.opts")), int(want.pop("sizeof.rescue")), int(want.pop("sizeof.stats"))) == (20, 48, 80)
    assert int(want.pop("status.values")) == 210 == RESCUED + 10 * NOTHING + 100 * NOT_CONCORDANT
    assert (spm.capi.RESCUE_RESCUED, spm.capi.RESCUE_NONE, spm.capi.RESCUE_NOT_CONCORDANT) == (RESCUED, NOTHING, NOT_CONCORDANT)
    seen = {"opts": 0, "rescue": 0, "stats": 0}
    for name, off in want.items():
        kind, field = name.split(".")
        ctype = {"opts": spm.capi.JstRescueOpts, "rescue": spm.capi.JstRescue, "stats": spm.capi.JstRescuesStats}[kind]
        assert getattr(ctype, field).offset == int(off), name
        if kind == "rescue":
            assert RESCUE.fields[field][1] == int(off) and RESCUE.fields[field][0].itemsize == getattr(ctype, field).size, name
        seen[kind] += 1
    assert seen == {"opts": len(spm.capi.JstRescueOpts._fields_), "rescue": len(spm.capi.JstRescue._fields_),
                    "stats": len(spm.capi.JstRescuesStats._fields_)} == {"opts": 5, "rescue": 11, "stats": 13}
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    for f in (spm.JstPairs.rescue, spm.JstRescues.view, spm.JstRescues.device, spm.JstRescues.stats, spm.JstRescues.close):
        assert callable(f)
    assert list(inspect.signature(spm.JstPairs.rescue).parameters)[1:] == ["loci", "reads", "reference", "patterns", "k", "min_tlen",
                                                                          "max_tlen"]


# ---------------------------------------------------------------------------------------------------------------------
# the rule again
# ---------------------------------------------------------------------------------------------------------------------
def stranded(reads, sigma=4):
    """needle q of the both_strands set: 2r the read, 2r + 1 its reverse complement"""
    out = []
    for r in reads:
        out += [np.asarray(r, np.uint8), np_revcomp(r, sigma)]
    return out


def np_window(a_begin, a_end, a_reverse, min_tlen, max_tlen, N):
    """(lo, hi, first admissible end, last admissible end), ends exclusive; first > last: nothing"""
    if not a_reverse:
        lo = a_begin
        hi = min(lo + max_tlen, N)
        return lo, hi, max(lo + min_tlen, a_end), hi
    lo = max(0, a_end - max_tlen)
    return lo, a_end, lo + 1, a_end


def np_rescue(oracle, ref, needles, loci, pairs, k, min_tlen, max_tlen):
    """-> (records with cigar_len 0, statistics, [(job, needle, lo)] of the found jobs)"""
    N = len(ref)
    jobs = []
    for p, R in enumerate(pairs):
        if R["flag1"] & 2:
            continue
        for x in (1, 0):                                           # anchored at mate 2: rescues mate 1, the first job
            a = int(R["locus2"] if x else R["locus1"])
            if a != NONE:
                jobs.append((p, x, a))
    out = np.zeros(len(jobs), RESCUE)
    st = dict.fromkeys(COUNTS, 0)
    st["n_jobs"] = len(jobs)
    found = []
    for j, (p, x, a) in enumerate(jobs):
        A = loci[a]
        a_begin, a_end, a_rev = int(A["ref_begin"]), int(A["ref_end"]), int(A["pattern"]) & 1
        assert int(A["pattern"]) >> 1 == 2 * p + x
        q = 4 * p + 2 * (1 - x) + (1 - a_rev)
        P = needles[q]
        lo, hi, e0, e1 = np_window(a_begin, a_end, a_rev, min_tlen, max_tlen, N)
        st["max_window"] = max(st["max_window"], hi - lo)
        o = out[j]
        o["pair"], o["pattern"], o["anchor"], o["score"], o["status"] = p, q, a, -1, NOTHING
        cand = None
        if len(P) <= k:
            st["n_short"] += 1
        elif e0 <= e1:
            h = oracle.sellers(ref[lo:hi], P, k)
            ends, d = h["pos"].astype(np.int64) + lo, h["score"].astype(np.int64)
            ok = (ends >= e0) & (ends <= e1) & (d <= k)
            if ok.any():
                cand = min(zip(d[ok].tolist(), ends[ok].tolist()))
        mate2 = x == 0                                             # the rescued mate
        if cand is None:
            o["flag"] = 0x1 | 0x4 | (0x20 if a_rev else 0) | (0x80 if mate2 else 0x40)
            st["n_none"] += 1
            continue
        o["score"], o["ref_end"] = cand
        found.append((j, q, lo))
    if found:
        js = np.array([f[0] for f in found])
        begins = ref_begins(ref, needles, np.array([f[1] for f in found]), out["ref_end"][js].astype(np.int64),
                            out["score"][js].astype(np.int64), np.array([f[2] for f in found], dtype=np.int64))
        off = 0
        for (j, q, lo), b in zip(found, begins.tolist()):
            o = out[j]
            A = loci[int(o["anchor"])]
            a_begin, a_end, a_rev = int(A["ref_begin"]), int(A["ref_end"]), int(A["pattern"]) & 1
            e = int(o["ref_end"])
            x = (int(A["pattern"]) >> 1) & 1
            o["ref_begin"], o["cigar_off"] = b, off
            off += 2 * int(o["score"]) + 1
            fb, fe, vb, ve = (b, e, a_begin, a_end) if a_rev else (a_begin, a_end, b, e)      # forward locus, reverse locus
            ok = fb <= vb and fe <= ve and min_tlen <= ve - fb <= max_tlen
            o["status"] = RESCUED if ok else NOT_CONCORDANT
            mate1_forward = (x == 1) if a_rev else (x == 0)
            o["tlen"] = ((ve - fb) if mate1_forward else -(ve - fb)) if ok else 0
            o["flag"] = 0x1 | (0x2 if ok else 0) | (0 if a_rev else 0x10) | (0x20 if a_rev else 0) | (0x80 if x == 0 else 0x40)
            st["n_rescued" if ok else "n_not_concordant"] += 1
    return out, st, found


class _Sellers:
    """oracle.sellers written out for the hand-worked list: a plain DP, every end with its distance"""
    @staticmethod
    def sellers(text, pat, k):
        m = len(pat)
        col = np.arange(m + 1)
        out = []
        for t, c in enumerate(text):
            new = np.empty_like(col)
            new[0] = 0
            for i in range(1, m + 1):
                new[i] = min(col[i - 1] + (pat[i - 1] != c), col[i] + 1, new[i - 1] + 1)
            col = new
            if col[m] <= k:
                out.append((t + 1, col[m]))
        return np.array(out, dtype=[("pos", "<u8"), ("score", "<i4")])


def test_rule_on_a_hand_worked_list(oracle):
    # the windows of the header's worked cases
    assert np_window(1000, 1030, 0, 100, 300, 10000) == (1000, 1300, 1100, 1300)
    assert np_window(720, 750, 1, 100, 300, 10000) == (450, 750, 451, 750)
    assert np_window(9800, 9830, 0, 100, 300, 10000) == (9800, 10000, 9900, 10000)
    lo, hi, e0, e1 = np_window(9950, 9980, 0, 100, 300, 10000)
    assert e0 > e1
    assert np_window(170, 200, 1, 100, 300, 10000) == (0, 200, 1, 200)
    # a reference of 400, reads of 20, min_tlen 50, max_tlen 120, k 3.  pair 0: mate 1 forward at [100,120), mate 2 (reverse
    # needle) lies at [180,200) with 2 substitutions: case 1.  pair 1: mate 2 reverse at [300,320), mate 1 lies at [290,310)
    # exactly: begins right of ... no, left of 300 but the fragment is 30 < 50: NOT_CONCORDANT.  pair 2: proper, no job.
    # pair 3: mate 1 forward at [350,370): ends 400 .. 400, nothing there.  pair 4: discordant, two jobs, both NONE.
    rng = np.random.default_rng(7)
    ref = rng.integers(0, 4, 400, dtype=np.uint8)
    m2 = ref[180:200].copy()
    m2[[4, 13]] ^= 1
    reads = [ref[100:120], np_revcomp(m2), ref[290:310], np_revcomp(ref[300:320]), ref[10:30], np_revcomp(ref[70:90]),
             ref[350:370], rng.integers(0, 4, 20, dtype=np.uint8), ref[40:60], ref[240:260]]
    needles = stranded(reads)
    loci = np.zeros(7, dtype=[("pattern", "<u4"), ("ref_begin", "<u8"), ("ref_end", "<u8")])
    loci["pattern"] = [0, 7, 8, 11, 12, 16, 18]
    loci["ref_begin"] = [100, 300, 10, 70, 350, 40, 240]
    loci["ref_end"] = [120, 320, 30, 90, 370, 60, 260]
    pairs = np.zeros(5, dtype=[("locus1", "<u4"), ("locus2", "<u4"), ("flag1", "<u2")])
    pairs["locus1"] = [0, NONE, 2, 4, 5]
    pairs["locus2"] = [NONE, 1, 3, NONE, 6]
    pairs["flag1"] = [0x49, 0x65, 0x63, 0x49, 0x41]
    for sellers in (_Sellers, oracle):                             # the plain DP above and the oracle agree
        got, st, found = np_rescue(sellers, ref, needles, loci, pairs, 3, 50, 120)
        assert got["pair"].tolist() == [0, 1, 3, 4, 4] and got["pattern"].tolist() == [3, 4, 15, 17, 19]
        assert got["anchor"].tolist() == [0, 1, 4, 6, 5]
        assert got[0].tolist() == (180, 200, 0, 3, 0, 2, 0, 0, 100, 0x93, RESCUED)
        assert got[1].tolist() == (290, 310, 1, 4, 1, 0, 5, 0, 0, 0x61, NOT_CONCORDANT)
        assert got[2].tolist() == (0, 0, 3, 15, 4, -1, 0, 0, 0, 0x85, NOTHING)
        assert got[3].tolist() == (0, 0, 4, 17, 6, -1, 0, 0, 0, 0x45, NOTHING)
        assert got[4].tolist() == (0, 0, 4, 19, 5, -1, 0, 0, 0, 0x85, NOTHING)
        assert st == dict(n_jobs=5, n_rescued=1, n_none=3, n_not_concordant=1, n_short=0, max_window=120)
        assert [f[0] for f in found] == [0, 1]
    got, st, _f = np_rescue(oracle, ref, needles, loci, pairs, 3, 20, 120)   # pair 1 with min_tlen 20: the fragment is 30
    assert got[1].tolist() == (290, 310, 1, 4, 1, 0, 5, 0, 30, 0x63, RESCUED)
    got, st, _f = np_rescue(oracle, ref, needles, loci, pairs, 1, 50, 120)   # k 1: two substitutions are too many
    assert got[0]["status"] == NOTHING and st["n_none"] == 4
    got, st, _f = np_rescue(oracle, ref, needles, loci, pairs, 20, 50, 120)  # needles of m <= k are not searched
    assert st["n_short"] == 5 == st["n_none"]


# ---------------------------------------------------------------------------------------------------------------------
# the chain and the check
# ---------------------------------------------------------------------------------------------------------------------
def _open(spm, ctx, t, reads, k, sigma=4):
    ref_text = ctx.upload(t["ref"], sigma=sigma)
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS, reads, k=k, sigma=sigma, both_strands=True)
    jst.index(_window(ps, len(ps)), 64)
    return ref_text, jst, ps


def _chain_of(spm, ctx, t, reads, k_search=K_SEARCH, sigma=4):
    """-> (loci, read summary, reference text, needle set, the handles to close last)"""
    ref_text, jst, ps = _open(spm, ctx, t, reads, k_search, sigma)
    h = jst.search_device(ps, max_hits=1 << 21)
    lc = _chain(h, best=1, across=True, strands=True)
    rd = lc.reads(len(reads), 2)
    return lc, rd, ref_text, ps, (h, jst)


def _check_rescue(ctx, oracle, ref, needles, lc, rd, pr, ref_text, ps, k, min_tlen, max_tlen):
    """one call against the rule: records, pool, device view, statistics.  -> (the result, the rule's records)"""
    loci, pairs = lc.view(), pr.view()
    want, counts, found = np_rescue(oracle, ref, needles, loci, pairs, k, min_tlen, max_tlen)
    rs = pr.rescue(lc, rd, ref_text, ps, k, min_tlen, max_tlen)
    got, ops = rs.view()
    assert got.dtype == RESCUE and len(got) == len(want) == len(rs)
    bare = got.copy()
    bare["cigar_len"] = 0
    assert bare.tobytes() == want.tobytes(), [(j, g, w) for j, (g, w) in enumerate(zip(bare.tolist(), want.tolist())) if g != w][:6]
    assert len(ops) == sum(2 * int(want["score"][j]) + 1 for j, _q, _lo in found)
    for j, q, _lo in found:
        r = got[j]
        n_words = int(r["cigar_len"])
        assert 1 <= n_words <= 2 * int(r["score"]) + 1
        replay(needles[q], ref, int(r["ref_begin"]), int(r["ref_end"]), ops[int(r["cigar_off"]):int(r["cigar_off"]) + n_words],
               int(r["score"]))
    assert np.all(got["cigar_len"][got["status"] == NOTHING] == 0)
    d_rec, n, d_ops, n_ops = rs.device()
    assert n == len(want) and n_ops == len(ops)
    assert download(ctx, d_rec, n, RESCUE).tobytes() == got.tobytes()
    assert download(ctx, d_ops, n_ops, np.uint32).tobytes() == ops.tobytes()
    st = rs.stats()
    assert st.n_pairs == len(pairs) and {c: int(getattr(st, c)) for c in COUNTS} == counts
    assert st.n_jobs == st.n_rescued + st.n_none + st.n_not_concordant and st.ms_host > 0
    return rs, want


# ---------------------------------------------------------------------------------------------------------------------
# GPU 1: every class, planted by hand
# ---------------------------------------------------------------------------------------------------------------------
_planted = {}


def _diverge(rng, x, n_sub=4):
    """n_sub substitutions, spread over the read"""
    x = x.copy()
    for at in np.linspace(3, len(x) - 4, n_sub).astype(int):
        x[at] = (int(x[at]) + 1 + int(rng.integers(0, 3))) & 3
    return x


def _planted_rescue():
    """the tree, the reads (2 per pair) and {class: [(pair, mate rescued, planted begin, planted end, edits), ...]}"""
    if _planted:
        return _planted["t"], _planted["reads"], _planted["classes"]
    t = _make_tree(6101, 12_000, 4, 6, 8)
    rng = np.random.default_rng(8102)
    ref = t["ref"]
    N = len(ref)
    apos = t["alleles"]["pos"].astype(np.int64)
    assert np.all(apos > 300) and np.all(apos < N - 300)          # the two ends of the reference are free of alleles
    spots = iter(_free_stretches(t, 240, 30, first=400))
    lens = iter(np.tile(np.arange(30, 37), 30).tolist())           # reads of 30 to 36 symbols
    noise = lambda: rng.integers(0, 4, next(lens), dtype=np.uint8)
    reads, classes = [], {}

    def pair(cls, mate1, mate2, rescued=None, begin=0, end=0, edits=0):
        classes.setdefault(cls, []).append((len(reads) // 2, rescued, begin, end, edits))
        reads.extend([mate1, mate2])

    def fragment(cls, tlen, anchor_forward=True, anchor_mate1=True, x=None, edit=_diverge, edits=4):
        """an exact anchor and a diverged mate, tlen apart: forward anchor at x, or reverse anchor ending at x + tlen"""
        x = next(spots) + 20 if x is None else x
        la, ly = next(lens), next(lens)
        if anchor_forward:
            anchor, yb = ref[x:x + la].copy(), x + tlen - ly
            mate = np_revcomp(edit(rng, ref[yb:yb + ly]))
        else:
            anchor, yb = np_revcomp(ref[x + tlen - la:x + tlen]), x
            mate = edit(rng, ref[yb:yb + ly])
        pair(cls, *((anchor, mate) if anchor_mate1 else (mate, anchor)), rescued=1 if anchor_mate1 else 0, begin=yb, end=yb + ly,
             edits=edits)
        return x

    def mixed(rng, src):                                           # one insertion, one deletion, two substitutions
        y = _diverge(rng, src, 2)
        y = np.delete(y, len(y) // 2)
        return np.insert(y, len(y) // 4, (int(y[len(y) // 4]) + 1) & 3).astype(np.uint8)

    pair("unmapped", noise(), noise())
    fragment("substitutions", 140)
    fragment("substitutions", 163, anchor_mate1=False)
    fragment("substitutions", 120, anchor_forward=False)
    fragment("substitutions", 177, anchor_forward=False, anchor_mate1=False)
    fragment("mixed", 150, edit=mixed)
    fragment("mixed", 131, anchor_forward=False, edit=mixed)
    x, la = next(spots) + 20, next(lens)
    pair("noise", ref[x:x + la].copy(), noise(), rescued=1)
    x, la = next(spots) + 20, next(lens)
    pair("noise", noise(), np_revcomp(ref[x:x + la]), rescued=0)
    # discordant: mate 1 forward here, mate 2 exactly (reverse) in another stretch, and a diverged copy of mate 2 beside mate 1
    x, far, la, ly = next(spots) + 20, next(spots) + 60, next(lens), next(lens)
    ref[x + 150 - ly:x + 150] = _diverge(rng, ref[far:far + ly])
    pair("discordant", ref[x:x + la].copy(), np_revcomp(ref[far:far + ly]), rescued=1, begin=x + 150 - ly, end=x + 150, edits=4)
    for tlen in (MIN_TLEN, MAX_TLEN):
        fragment("at_bound", tlen)
        fragment("at_bound", tlen, anchor_forward=False)
    for tlen in (MIN_TLEN - 1, MAX_TLEN + 1):
        fragment("outside", tlen)
        fragment("outside", tlen, anchor_forward=False)
    fragment("clipped_at_0", 130, anchor_forward=False, x=25)      # a reverse anchor that ends at 155 < max_tlen
    fragment("clipped_at_N", 140, x=N - 150)                       # a forward anchor whose window ends at N
    # a reverse anchor [x + 100, x + 100 + la); the mate lies inside it and begins right of its begin
    x, la = next(spots) + 20, 36
    inner = _diverge(rng, ref[x + 105:x + 100 + la])
    pair("dovetail", inner, np_revcomp(ref[x + 100:x + 100 + la]), rescued=0, begin=x + 105, end=x + 100 + la, edits=4)
    # the same stretch at two places, the mate is 4 substitutions away from both: the smaller end wins
    x, la, ly = next(spots) + 20, next(lens), next(lens)
    ref[x + 170 - ly:x + 170] = ref[x + 120 - ly:x + 120]
    pair("twice", ref[x:x + la].copy(), np_revcomp(_diverge(rng, ref[x + 120 - ly:x + 120])), rescued=1, begin=x + 120 - ly, end=x + 120,
         edits=4)
    for tlen in (140, 151):                                        # proper pairs
        x, la, ly = next(spots) + 20, next(lens), next(lens)
        pair("proper", ref[x:x + la].copy(), np_revcomp(ref[x + tlen - ly:x + tlen]))
    pair("unmapped", noise(), noise())
    reads = [np.ascontiguousarray(r, np.uint8) for r in reads]
    assert all(29 <= len(r) <= 36 for r in reads)
    _planted.update(t=t, reads=reads, classes=classes)
    return t, reads, classes


def _assert_planted_classes(want, pairs, classes):
    """every class exists, judged from the rule's answer"""
    by_pair = {}
    for r in want:
        by_pair.setdefault(int(r["pair"]), []).append(r)
    mate_of = lambda r: (int(r["pattern"]) >> 1) & 1

    def only(p, rescued):
        (r,) = [r for r in by_pair[p] if mate_of(r) == rescued]
        return r

    assert {c: len(v) for c, v in classes.items()} == dict(unmapped=2, substitutions=4, mixed=2, noise=2, discordant=1, at_bound=4,
                                                          outside=4, clipped_at_0=1, clipped_at_N=1, dovetail=1, twice=1, proper=2)
    for p, *_ in classes["unmapped"] + classes["proper"]:
        assert p not in by_pair
    assert all(pairs[p]["flag1"] & 2 for p, *_ in classes["proper"]) and all(pairs[p]["flag1"] & 0xC == 0xC for p, *_ in classes["unmapped"])
    tlens = []
    for cls in ("substitutions", "mixed", "at_bound", "clipped_at_0", "clipped_at_N", "twice"):
        for p, rescued, b, e, edits in classes[cls]:
            assert len(by_pair[p]) == 1 and pairs[p]["flag1"] & 0xC in (4, 8)          # one mate mapped, one job
            r = only(p, rescued)
            assert (int(r["status"]), int(r["ref_end"]), int(r["score"])) == (RESCUED, e, edits), (cls, p, r)
            assert int(r["ref_begin"]) == b or cls == "mixed"
            tlens.append((cls, int(r["tlen"])))
    assert [v for c, v in tlens if c == "substitutions"] == [140, -163, -120, 177]
    assert sorted(abs(v) for c, v in tlens if c == "at_bound") == [MIN_TLEN] * 2 + [MAX_TLEN] * 2
    assert [v for c, v in tlens if c in ("clipped_at_0", "clipped_at_N", "twice")] == [-130, 140, 120]
    for p, rescued, *_ in classes["noise"]:
        r = only(p, rescued)
        assert len(by_pair[p]) == 1 and (int(r["status"]), int(r["score"]), int(r["cigar_len"])) == (NOTHING, -1, 0)
    ((p, rescued, b, e, edits),) = classes["discordant"]
    assert len(by_pair[p]) == 2 and pairs[p]["flag1"] & 0xE == 0 and [mate_of(r) for r in by_pair[p]] == [0, 1]
    r = only(p, 1)
    assert (int(r["status"]), int(r["ref_begin"]), int(r["ref_end"]), int(r["score"]), int(r["tlen"])) == (RESCUED, b, e, 4, 150)
    assert int(only(p, 0)["status"]) == NOTHING
    for p, rescued, b, e, edits in classes["outside"]:             # not rescued at the planted place
        r = only(p, rescued)
        assert not (int(r["status"]) == RESCUED and int(r["ref_begin"]) == b and int(r["ref_end"]) == e)
    assert sum(int(only(p, rs)["status"]) == NOT_CONCORDANT for p, rs, *_ in classes["outside"]) >= 1   # min_tlen - 1, reverse anchor
    ((p, rescued, b, e, edits),) = classes["dovetail"]
    r = only(p, rescued)
    assert (int(r["status"]), int(r["ref_begin"]), int(r["ref_end"]), int(r["score"]), int(r["tlen"])) == (NOT_CONCORDANT, b, e, 4, 0)
    assert int(r["cigar_len"]) == 0 and r["flag"] == 0x61          # (the rule's records carry no word count)


@gpu
def test_hand_planted_classes(spm, ctx, oracle):
    t, reads, classes = _planted_rescue()
    needles = stranded(reads)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs, want = _check_rescue(ctx, oracle, t["ref"], needles, lc, rd, pr, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    _assert_planted_classes(want, pr.view(), classes)
    got, ops = rs.view()
    ((p, *_),) = classes["dovetail"]
    assert got[got["pair"] == p]["cigar_len"][0] >= 1              # NOT_CONCORDANT keeps its alignment
    st = rs.stats()
    assert st.max_window == MAX_TLEN and st.n_short == 0 and st.n_not_concordant >= 2 and st.n_none >= 3
    # k = 3: four edits are too many; k = 40: every needle is short
    for k, check in ((3, lambda s: s.n_rescued == 0), (40, lambda s: s.n_short == s.n_jobs == s.n_none)):
        other, _w = _check_rescue(ctx, oracle, t["ref"], needles, lc, rd, pr, ref_text, ps, k, MIN_TLEN, MAX_TLEN)
        assert check(other.stats())
        other.close()
    for x in (rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 2: word and lane borders
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_end_ranges_and_short_windows(spm, ctx, oracle):
    """the planted reads again under bounds that make end ranges of 1, 63, 64 and 65 ends, and windows shorter than m + k"""
    t, reads, _classes = _planted_rescue()
    needles = stranded(reads)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    seen = set()
    for min_tlen, max_tlen in ((150, 150), (100, 162), (100, 163), (100, 164), (20, 30), (1, 36), (1, 1000), (177, 20_000)):
        pr = lc.pairs(rd, min_tlen, max_tlen)
        rs, want = _check_rescue(ctx, oracle, t["ref"], needles, lc, rd, pr, ref_text, ps, K, min_tlen, max_tlen)
        loci = lc.view()
        for r in want:
            A = loci[int(r["anchor"])]
            lo, hi, e0, e1 = np_window(int(A["ref_begin"]), int(A["ref_end"]), int(A["pattern"]) & 1, min_tlen, max_tlen, len(t["ref"]))
            seen.add(e1 - e0 + 1)
            if hi - lo < len(needles[int(r["pattern"])]) + K:
                seen.add("short window")
            if hi - lo < max_tlen:
                seen.add("clipped")
        if (min_tlen, max_tlen) == (1, 1000):
            assert np.count_nonzero(want["status"] == RESCUED) >= 12
        rs.close()
        pr.close()
    assert {1, 63, 64, 65, "short window", "clipped"} <= seen, sorted(map(str, seen))
    for x in (rd, lc, ps, ref_text) + rest:
        x.close()


def _long_pairs(t, rng, lengths, sigma=4):
    """per length m: a forward-anchored and a reverse-anchored pair of two reads of m symbols, the mate 5 substitutions away"""
    ref = t["ref"]
    spots = iter(_free_stretches(t, 760, 2 * len(lengths), first=200))
    reads, planted = [], []
    for m in lengths:
        for anchor_forward in (True, False):
            x, tlen = next(spots) + 20, 2 * m + 40 + int(rng.integers(0, 60))
            if anchor_forward:
                anchor, yb = ref[x:x + m].copy(), x + tlen - m
                mate = np_revcomp(_diverge(rng, ref[yb:yb + m], 5), sigma)
            else:
                anchor, yb = np_revcomp(ref[x + tlen - m:x + tlen], sigma), x
                mate = _diverge(rng, ref[yb:yb + m], 5)
            planted.append((len(reads) // 2, yb, yb + m))
            reads += [anchor, mate] if len(planted) % 3 else [mate, anchor]
    return [np.ascontiguousarray(r, np.uint8) for r in reads], planted


@gpu
def test_word_borders(spm, ctx, oracle):
    """needles of 63 .. 256 symbols: every word count, and the launches that skip the jobs of the other word counts"""
    t = _make_tree(9101, 24_000, 2, 4, 4)
    rng = np.random.default_rng(9102)
    lengths = (63, 64, 65, 128, 129, 192, 256)
    reads, planted = _long_pairs(t, rng, lengths)
    needles = stranded(reads)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, 100, 700)
    rs, want = _check_rescue(ctx, oracle, t["ref"], needles, lc, rd, pr, ref_text, ps, K, 100, 700)
    assert len(want) == 2 * len(lengths)
    for (p, b, e), r in zip(planted, want):
        # the planted place is a candidate with 5 edits: the minimum of (d, e) is that or smaller (a tie one end to the left)
        assert (int(r["pair"]), int(r["status"])) == (p, RESCUED) and (int(r["score"]), int(r["ref_end"])) <= (5, e)
        assert abs(int(r["ref_begin"]) - b) <= 5 and abs(int(r["ref_end"]) - e) <= 5
    assert sorted({(len(needles[int(q)]) + 63) // 64 for q in want["pattern"]}) == [1, 2, 3, 4]
    tight, _w = _check_rescue(ctx, oracle, t["ref"], needles, lc, rd, pr, ref_text, ps, 4, 100, 700)    # five edits are too many
    assert tight.stats().n_rescued == 0
    for x in (tight, rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_dna5_needle_with_an_n(spm, ctx, oracle):
    t = _make_tree(9201, 12_000, 2, 4, 4, sigma=5, n_runs=3)
    rng = np.random.default_rng(9202)
    ref = t["ref"]
    free = [s for s in _free_stretches(t, 240, 40, first=200) if not np.any(ref[s:s + 240] == 4)][:4]
    assert len(free) == 4
    reads = []
    for j, s in enumerate(free):
        x, tlen = s + 20, 130 + 10 * j
        mate = _diverge(rng, ref[x + tlen - 34:x + tlen], 3)
        mate[17] = 4                                               # an N in the needle: one more edit
        if j == 3:
            ref[x + tlen - 34 + 17] = 4                            # ... unless the reference has an N there: ranks are compared
        reads += [ref[x:x + 33].copy(), np_revcomp(mate, 5)]
    needles = stranded(reads, 5)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads, sigma=5)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs, want = _check_rescue(ctx, oracle, ref, needles, lc, rd, pr, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    assert want["status"].tolist() == [RESCUED] * 4 and want["score"].tolist() == [4, 4, 4, 3]
    assert want["tlen"].tolist() == [130, 140, 150, 160]
    for x in (rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 3: random pairs cut from the haplotypes
# ---------------------------------------------------------------------------------------------------------------------
def _edits(rng, src, L, n):
    """a read of L symbols exactly n edit operations away from a prefix of src (len(src) >= L + n)"""
    nd = src.copy()
    for _ in range(n):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(2, L - 2))
        if kind == 0:
            nd[at] = (int(nd[at]) + 1 + int(rng.integers(0, 3))) & 3
        elif kind == 1:
            nd = np.delete(nd, at)
        else:
            nd = np.insert(nd, at, int(rng.integers(0, 4)))
    return nd[:L].astype(np.uint8)


def _random_pairs(t, seed, n_pairs):
    """fragments of 110 .. 170 haplotype symbols, both mates where the haplotype is the reference (the fragment between them
    may cross alleles), kept when the fragment is 100 .. 180 reference symbols; one mate gets 3 .. 6 edits"""
    rng = np.random.default_rng(seed)
    ref = t["ref"]
    reads, planted = [], []
    while len(planted) < n_pairs:
        h = int(rng.integers(0, t["n_hap"]))
        hp, J = _hap(t, h)
        L1, L2, frag = int(rng.integers(30, 37)), int(rng.integers(30, 37)), int(rng.integers(110, 171))
        o = int(rng.integers(10, len(hp) - frag - 20))
        o2 = o + frag - L2
        r1, r2 = int(J.anchor[o]), int(J.anchor[o2])
        if not (np.array_equal(hp[o:o + L1], ref[r1:r1 + L1]) and np.array_equal(hp[o2 - 8:o2 + L2 + 8], ref[r2 - 8:r2 + L2 + 8])):
            continue
        if not (np.array_equal(J.anchor[o:o + L1], np.arange(r1, r1 + L1)) and np.array_equal(J.anchor[o2:o2 + L2], np.arange(r2, r2 + L2))):
            continue
        if not MIN_TLEN + 8 <= r2 + L2 - r1 <= MAX_TLEN - 8:
            continue
        n_edits = int(rng.integers(3, 7))
        left_edited = bool(rng.integers(0, 2))
        fwd, rev = hp[o:o + L1].copy(), hp[o2:o2 + L2].copy()
        if left_edited:
            fwd = _edits(rng, hp[o:o + L1 + 8], L1, n_edits)
        else:                                                      # the reverse mate's last symbol bounds the fragment: edit its mirror
            rev = _edits(rng, hp[o2 - 8:o2 + L2][::-1].copy(), L2, n_edits)[::-1].copy()
        mates = [fwd, np_revcomp(rev)]
        rescued = 0 if left_edited else 1
        if rng.integers(0, 2):
            mates, rescued = mates[::-1], 1 - rescued
        planted.append((len(reads) // 2, rescued))
        reads += mates
    return [np.ascontiguousarray(r, np.uint8) for r in reads], planted


@gpu
def test_random_pairs_from_the_haplotypes(spm, ctx, oracle):
    t = _make_tree(6101, 12_000, 4, 6, 8)
    reads, planted = _random_pairs(t, 8301, 200)
    needles = stranded(reads)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs, want = _check_rescue(ctx, oracle, t["ref"], needles, lc, rd, pr, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    pairs = pr.view()
    jobs = {(int(r["pair"]), (int(r["pattern"]) >> 1) & 1): r for r in want}
    unmapped = [(p, y) for p, y in planted if pairs[p]["flag1"] & 0xC in (4, 8) and (p, y) in jobs]
    assert len(unmapped) >= 150                                    # (a mate of 3 edits can still be found by the search at k = 2)
    status = np.array([int(jobs[key]["status"]) for key in unmapped])
    assert np.all(status != NOTHING)                               # every planted mate has a candidate within k
    assert np.count_nonzero(status == RESCUED) >= 0.9 * len(unmapped), np.bincount(status)
    for x in (rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 4: determinism and lifetimes
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_determinism_and_lifetimes(spm, ctx):
    t, reads, _classes = _planted_rescue()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    a = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    b = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    (ra, oa), (rb, ob) = a.view(), b.view()
    assert len(ra) > 20 and len(oa) > 100 and ra.tobytes() == rb.tobytes() and oa.tobytes() == ob.tobytes()
    b.close()
    for x in (pr, rd, lc, ps, ref_text) + rest:                    # all five inputs, and what made them
        x.close()
    (rc, oc), (d_rec, n, d_ops, n_ops) = a.view(), a.device()
    assert rc.tobytes() == ra.tobytes() and oc.tobytes() == oa.tobytes()
    assert download(ctx, d_rec, n, RESCUE).tobytes() == ra.tobytes() and download(ctx, d_ops, n_ops, np.uint32).tobytes() == oa.tobytes()
    a.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 5: what is refused
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(spm, ctx):
    t, reads, _classes = _planted_rescue()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    lib = spm.capi.lib()
    err = lambda: lib.spm_hip_last_error(ctx._h)
    O = spm.capi.JstRescueOpts
    ok = O(MIN_TLEN, MAX_TLEN, K, 0, 0)
    good_rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    good = good_rs.view()

    def refused(word, code=-1, l=lc, r=rd, p=pr, ref=ref_text, pats=ps, opts=ok):
        out = ctypes.c_void_p()
        h = lambda x: x._h if x is not None else None
        o = ctypes.byref(opts) if opts is not None else None
        assert lib.spm_hip_jst_pairs_rescue(h(l), h(r), h(p), h(ref), h(pats), o, ctypes.byref(out)) == code and not out.value
        assert word in err(), err()

    unsupported = -4                                               # SPM_E_UNSUPPORTED
    refused(b"NULL", r=None)
    refused(b"NULL", p=None)
    refused(b"NULL", ref=None)
    refused(b"NULL", pats=None)
    refused(b"NULL", opts=None)
    out = ctypes.c_void_p()
    assert lib.spm_hip_jst_pairs_rescue(None, rd._h, pr._h, ref_text._h, ps._h, ctypes.byref(ok), ctypes.byref(out)) == -1
    assert lib.spm_hip_jst_pairs_rescue(lc._h, rd._h, pr._h, ref_text._h, ps._h, ctypes.byref(ok), None) == -1
    for bad, word in ((O(100, 180, K, 1, 0), b"flag"), (O(100, 180, K, 0, 7), b"reserved"), (O(0, 180, K, 0, 0), b"min_tlen"),
                      (O(181, 180, K, 0, 0), b"min_tlen"), (O(1, 1 << 31, K, 0, 0), b"max_tlen")):
        refused(word, opts=bad)
    other = spm.Context(0)                                         # handles of another context
    other_ref = other.upload(t["ref"], sigma=4)
    other_ps = other.patterns(spm.ALGO_MYERS, reads, k=K_SEARCH, both_strands=True)
    refused(b"context", ref=other_ref)
    refused(b"context", pats=other_ps)
    other_ps.close()
    other_ref.close()
    other.close()
    plain = lc.reads(2 * len(reads), 1)
    refused(b"strands", r=plain)
    fewer = lc.reads(len(reads) - 2, 2)
    refused(b"pairs", r=fewer)
    few = [r for c in ("proper", "unmapped") for p, *_ in _classes[c] for r in reads[2 * p:2 * p + 2]]
    lc4, rd4, ref4, ps4, rest4 = _chain_of(spm, ctx, t, few)       # another collapse with fewer loci
    assert 0 < len(lc4.view()) < len(lc.view())
    refused(b"loci", l=lc4)
    single = ctx.patterns(spm.ALGO_MYERS, stranded(reads), k=K_SEARCH)          # the same 2n needles, not a stranded set
    refused(b"stranded", pats=single)
    half = ctx.patterns(spm.ALGO_MYERS, reads[:-2], k=K_SEARCH, both_strands=True)
    refused(b"needles", pats=half)
    prefix = ctx.patterns(spm.ALGO_MYERS_PREFIX, reads, k=K_SEARCH, both_strands=True)
    refused(b"MYERS_PREFIX", code=unsupported, pats=prefix)
    long_reads = list(reads)
    long_reads[3] = np.random.default_rng(5).integers(0, 4, 300, dtype=np.uint8)
    long_ps = ctx.patterns(spm.ALGO_MYERS, long_reads, k=K_SEARCH, both_strands=True)
    refused(b"300", code=unsupported, pats=long_ps)
    ref5 = ctx.upload(t["ref"], sigma=5)
    refused(b"sigma", ref=ref5)
    # a pair record corrupted in the device buffer: locus1 beyond the loci.  Counted, not followed
    d_pairs, n_pairs = pr.device()
    PAIR = spm.JST_PAIR_DTYPE
    host = download(ctx, d_pairs, n_pairs, PAIR)
    victim = int(np.nonzero((host["flag1"] & 2 == 0) & (host["locus1"] != NONE))[0][0])
    broken = host.copy()
    broken["locus1"][victim] = len(lc.view()) + 5
    hip = ctypes.CDLL("libamdhip64.so")
    ctx.synchronize()
    assert hip.hipMemcpy(ctypes.c_void_p(d_pairs), broken.ctypes.data_as(ctypes.c_void_p), broken.nbytes, 1) == 0
    refused(b"disagree")
    assert hip.hipMemcpy(ctypes.c_void_p(d_pairs), host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1) == 0
    # accessors on NULL, and after all of this the call still answers as before
    assert lib.spm_hip_jst_rescues_view(None, None, None, None, None) == -1
    assert lib.spm_hip_jst_rescues_device(None, None, None, None, None) == -1 and lib.spm_hip_jst_rescues_stats(None, None) == -1
    lib.spm_hip_jst_rescues_destroy(None)
    with pytest.raises(spm.SpmError, match="-1"):
        pr.rescue(lc, rd, ref_text, ps, K, 0, 5)
    after = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    assert after.view()[0].tobytes() == good[0].tobytes() and after.view()[1].tobytes() == good[1].tobytes()
    # zero jobs (proper and unmapped pairs only), zero pairs: empty results
    pr4 = lc4.pairs(rd4, MIN_TLEN, MAX_TLEN)
    no_jobs = pr4.rescue(lc4, rd4, ref4, ps4, K, MIN_TLEN, MAX_TLEN)
    assert len(no_jobs) == 0 and no_jobs.stats().n_pairs == 4 and no_jobs.stats().n_jobs == 0 and pr4.stats().n_proper == 2
    for x in (no_jobs, pr4, rd4, lc4, ps4, ref4) + rest4:
        x.close()
    rd0 = lc.reads(0, 2)
    pr0 = lc.pairs(rd0, MIN_TLEN, MAX_TLEN)
    ps0 = ctx.patterns(spm.ALGO_MYERS, [], k=K_SEARCH, both_strands=True)
    empty = pr0.rescue(lc, rd0, ref_text, ps0, K, MIN_TLEN, MAX_TLEN)
    assert len(empty) == 0 and len(empty.view()[0]) == 0 and len(empty.view()[1]) == 0 and empty.stats().n_jobs == 0
    for x in (empty, ps0, pr0, rd0, after, good_rs, ref5, long_ps, prefix, half, single, fewer, plain, pr, rd, lc, ps,
              ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 6: the C++ mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("rescue_mirror_cases.cpp", tmp_path).exists()


@gpu
def test_mirror_rescues_agree_with_the_rule(spm, tmp_path):
    """locate_pairs_rescued on pairs cut from the fixture haplotypes: locate_pairs plus records that follow the rule"""
    r = subprocess.run([str(build_mirror("rescue_mirror_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 200, r.stdout[-2000:]
    assert len(re.findall(r"jobs: \d+ rescued", r.stdout)) == 2
