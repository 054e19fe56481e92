"""The mates of paired-end reads: spm_hip_jst_ref_loci_pairs behind the chain select -> align_selected -> project -> normalize
-> collapse -> reads, its Python binding and the C++ mirror's locate_pairs.

The expected answer never comes from the code under test: the rule -- every forward locus of one mate against every reverse
locus of the other, FR orientation, min_tlen <= fragment <= max_tlen, the minimum of (score sum, a, b) -- is written again in
NumPy here over the downloaded loci, as all combinations per pair."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cpp_programs import ROOT, build_cases, build_mirror, c_layout, download
from test_jst_project import _make_tree, _plant, _window
from test_strands import np_revcomp

gpu = pytest.mark.gpu
PAIR = np.dtype([("locus1", "<u4"), ("locus2", "<u4"), ("tlen", "<i4"), ("best", "<i4"), ("n_pairs", "<u4"), ("n_best", "<u4"),
                 ("n_next", "<u4"), ("flag1", "<u2"), ("flag2", "<u2")])
NONE = 0xFFFFFFFF
COUNTS = ("n_proper", "n_unique", "n_multi", "n_discordant", "n_one_mate", "n_unmapped", "max_window")


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the case program, the layouts, the names
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_case_program(tmp_path, sanitize):
    exe = build_cases("jst_pairs_core_cases.cpp", tmp_path, include=[os.path.join(ROOT, "include")], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 2000, r.stdout[-500:]


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_jst_pair_opts, f))
#define F(f) printf("pair.%s %zu\n", #f, offsetof(spm_jst_pair, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_jst_pairs_stats, f))
int main(void)
{
    O(min_tlen); O(max_tlen); O(flags); O(reserved);
    F(locus1); F(locus2); F(tlen); F(best); F(n_pairs); F(n_best); F(n_next); F(flag1); F(flag2);
    S(ms_total); S(ms_host); S(n_pairs); S(n_proper); S(n_unique); S(n_multi); S(n_discordant); S(n_one_mate); S(n_unmapped);
    S(max_window);
    printf("sizeof.opts %zu\nsizeof.pair %zu\nsizeof.stats %zu\n", sizeof(spm_jst_pair_opts), sizeof(spm_jst_pair),
           sizeof(spm_jst_pairs_stats));
    return 0;
}
"""
CALLS = ("spm_hip_jst_ref_loci_pairs", "spm_hip_jst_pairs_view", "spm_hip_jst_pairs_device", "spm_hip_jst_pairs_stats",
         "spm_hip_jst_pairs_destroy")


def test_layouts_and_names(spm, tmp_path):
    import inspect
    assert ctypes.sizeof(spm.capi.JstPairOpts) == 16 and ctypes.sizeof(spm.capi.JstPairsStats) == 72
    assert ctypes.sizeof(spm.capi.JstPair) == 32 == spm.JST_PAIR_DTYPE.itemsize and spm.JST_PAIR_DTYPE == PAIR
    want = c_layout(tmp_path, LAYOUT_C)
    assert (int(want.pop("sizeof.opts")), int(want.pop("sizeof.pair")), int(want.pop("sizeof.stats"))) == (16, 32, 72)
    seen = {"opts": 0, "pair": 0, "stats": 0}
    for name, off in want.items():
        kind, field = name.split(".")
        ctype = {"opts": spm.capi.JstPairOpts, "pair": spm.capi.JstPair, "stats": spm.capi.JstPairsStats}[kind]
        assert getattr(ctype, field).offset == int(off), name
        if kind == "pair":
            assert PAIR.fields[field][1] == int(off) and PAIR.fields[field][0].itemsize == getattr(ctype, field).size, name
        seen[kind] += 1
    assert seen == {"opts": len(spm.capi.JstPairOpts._fields_), "pair": len(spm.capi.JstPair._fields_),
                    "stats": len(spm.capi.JstPairsStats._fields_)} == {"opts": 4, "pair": 9, "stats": 10}
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    for f in (spm.JstRefLoci.pairs, spm.JstPairs.view, spm.JstPairs.device, spm.JstPairs.stats, spm.JstPairs.close):
        assert callable(f)
    assert list(inspect.signature(spm.JstRefLoci.pairs).parameters)[1:] == ["reads", "min_tlen", "max_tlen"]


# ---------------------------------------------------------------------------------------------------------------------
# the rule again, in NumPy: all combinations per pair
# ---------------------------------------------------------------------------------------------------------------------
def np_pairs(loci, n_reads, min_tlen, max_tlen):
    """loci: a loci view in its order -> (the pair records, the statistics)"""
    out = np.zeros(n_reads // 2, PAIR)
    st = dict.fromkeys(COUNTS, 0)
    pat, sc = loci["pattern"].astype(np.int64), loci["score"].astype(np.int64)
    rb, re_ = loci["ref_begin"].astype(np.int64), loci["ref_end"].astype(np.int64)
    idx = np.arange(len(loci))

    def primary(r):
        mine = idx[pat >> 1 == r]
        return min((int(sc[i]), int(i)) for i in mine)[1] if len(mine) else NONE

    for p in range(n_reads // 2):
        combos = []
        for m in (0, 1):
            A, B = idx[pat == 4 * p + 2 * m], idx[pat == 4 * p + 2 * (1 - m) + 1]
            if len(A) and len(B):
                ab, ae, bb, be = rb[A][:, None], re_[A][:, None], rb[B][None, :], re_[B][None, :]
                ok = (ab <= bb) & (ae <= be) & (be - ab >= min_tlen) & (be - ab <= max_tlen)
                st["max_window"] = max(st["max_window"], int(((bb >= ab) & (bb <= ab + max_tlen)).sum(axis=1).max()))
                i, j = np.nonzero(ok)
                combos += zip((sc[A][i] + sc[B][j]).tolist(), A[i].tolist(), B[j].tolist())
        o = out[p]
        if combos:
            combos.sort()
            s, a, b = combos[0]
            m1f = not pat[a] & 2
            l1, l2 = (a, b) if m1f else (b, a)
            t = int(re_[b] - rb[a])
            o["tlen"], o["best"], o["n_pairs"] = (t if m1f else -t), s, min(len(combos), NONE)
            o["n_best"] = sum(1 for c in combos if c[0] == s)
            o["n_next"] = sum(1 for c in combos if c[0] == s + 1)
        else:
            l1, l2 = primary(2 * p), primary(2 * p + 1)
            o["best"] = -1
        o["locus1"], o["locus2"] = l1, l2
        un1, un2 = l1 == NONE, l2 == NONE
        r1, r2 = (not un1) and bool(pat[l1] & 1), (not un2) and bool(pat[l2] & 1)
        proper = 2 if combos else 0
        o["flag1"] = 1 | proper | 4 * un1 | 8 * un2 | 16 * r1 | 32 * r2 | 0x40
        o["flag2"] = 1 | proper | 4 * un2 | 8 * un1 | 16 * r2 | 32 * r1 | 0x80
        st["n_proper"] += bool(combos)
        st["n_unique"] += bool(combos) and o["n_best"] == 1
        st["n_multi"] += bool(combos) and o["n_best"] > 1
        st["n_discordant"] += not combos and not un1 and not un2
        st["n_one_mate"] += un1 != un2
        st["n_unmapped"] += un1 and un2
    return out, {k: int(v) for k, v in st.items()}


def test_numpy_rule_on_a_hand_worked_list():
    loci = np.zeros(7, dtype=[("pattern", "<u4"), ("score", "<i4"), ("ref_begin", "<u8"), ("ref_end", "<u8")])
    # pair 0: case 1 of spm_hip.h; pair 1: mate 1 reverse; pair 2: one mate; pair 3: unmapped
    loci["pattern"] = [0, 3, 3, 5, 6, 6, 10]
    loci["score"] = [0, 1, 0, 0, 0, 0, 2]
    loci["ref_begin"] = [1000, 1170, 7000, 720, 500, 671, 40]
    loci["ref_end"] = [1030, 1200, 7030, 750, 530, 701, 70]
    got, st = np_pairs(loci, 8, 100, 300)
    assert got.tolist() == [(0, 1, 200, 1, 1, 1, 0, 0x63, 0x93), (3, 4, -250, 0, 1, 1, 0, 0x53, 0xA3),
                            (NONE, 6, 0, -1, 0, 0, 0, 0x45, 0x89), (NONE, NONE, 0, -1, 0, 0, 0, 0x4D, 0x8D)]
    assert st == dict(n_proper=2, n_unique=2, n_multi=0, n_discordant=0, n_one_mate=1, n_unmapped=1, max_window=1)
    got, st = np_pairs(loci, 8, 100, 249)                          # pair 1: 250 is now too long, 79 too short
    assert got[1].tolist() == (3, 4, 0, -1, 0, 0, 0, 0x51, 0xA1) and st["n_discordant"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# the chain and the check
# ---------------------------------------------------------------------------------------------------------------------
def _open(spm, ctx, t, reads, k):
    ref_text = ctx.upload(t["ref"], sigma=4)
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS, reads, k=k, both_strands=True)
    jst.index(_window(ps, len(ps)), 64)
    return ref_text, jst, ps


def _chain(h, **kw):
    sel = h.select(**kw)
    a = sel.align_selected()
    pr = a.project()
    nz = pr.normalize()
    lc = nz.collapse()
    for x in (nz, pr, a, sel):
        x.close()
    return lc


def _check_pairs(ctx, lc, rd, min_tlen, max_tlen):
    loci = lc.view()
    n_reads = len(rd)
    pr = lc.pairs(rd, min_tlen, max_tlen)
    want, counts = np_pairs(loci, n_reads, min_tlen, max_tlen)
    got = pr.view()
    assert got.dtype == PAIR and len(got) == n_reads // 2
    assert got.tobytes() == want.tobytes(), [(p, g, w) for p, (g, w) in enumerate(zip(got.tolist(), want.tolist())) if g != w][:8]
    p, n = pr.device()
    assert n == n_reads // 2 == len(pr) and download(ctx, p, n, PAIR).tobytes() == want.tobytes()
    st = pr.stats()
    assert st.n_pairs == n_reads // 2
    assert {k: int(getattr(st, k)) for k in COUNTS} == counts
    assert st.ms_host > 0
    return pr, want, loci


# ---------------------------------------------------------------------------------------------------------------------
# GPU 1: every class, planted by hand
# ---------------------------------------------------------------------------------------------------------------------
MIN_TLEN, MAX_TLEN = 100, 180
_planted = {}


def _free_stretches(t, width, n, first=100):
    """n starts s of stretches [s, s + width) with no allele within 60 bases"""
    apos = t["alleles"]["pos"].astype(np.int64)
    out, s = [], first
    while len(out) < n and s + width < len(t["ref"]) - 100:
        if np.all((apos < s - 60) | (apos > s + width + 60)):
            out.append(s)
            s += width
        else:
            s += 20
    assert len(out) == n, (len(out), n)
    return out


def _planted_pairs():
    """the tree, the reads (2 per pair) and {class: [(pair, planted tlen), ...]}"""
    if not _planted:
        t = _make_tree(6101, 12_000, 4, 6, 8)
        rng = np.random.default_rng(6102)
        ref = t["ref"]
        spots = iter(_free_stretches(t, 240, 26))
        lens = iter(np.tile(np.arange(30, 37), 20).tolist())       # reads of 30 to 36 symbols
        noise = lambda: rng.integers(0, 4, next(lens), dtype=np.uint8)
        reads, classes = [], {}
        later = []                                                 # reads are cut once the reference has its final content

        def pair(cls, tlen, mate1, mate2):
            """mate1 / mate2: functions of nothing that cut the read from the final reference"""
            classes.setdefault(cls, []).append((len(later), tlen))
            later.append((mate1, mate2))

        def fragment(cls, tlen, mate1_forward=True, both_forward=False):
            x, l1, l2 = next(spots) + 20, next(lens), next(lens)
            fwd = lambda: ref[x:x + l1].copy()
            rev = (lambda: ref[x + tlen - l2:x + tlen].copy()) if both_forward else (lambda: np_revcomp(ref[x + tlen - l2:x + tlen]))
            pair(cls, tlen, *((fwd, rev) if mate1_forward else (rev, fwd)))
            return x, l1, l2

        pair("unmapped", 0, noise, noise)                          # pair 0
        fragment("proper_forward", 140)
        fragment("proper_forward", 163)
        fragment("proper_reverse", 120, mate1_forward=False)
        fragment("proper_reverse", 177, mate1_forward=False)
        for j in range(2):                                         # an exact copy far away, a one-substitution copy beside the partner
            x, l1, l2 = next(spots) + 20, next(lens), next(lens)
            far = next(spots) + 50
            near = ref[far:far + l2].copy()
            near[l2 // 2] = (int(near[l2 // 2]) + 1) & 3
            ref[x + 150 - l2:x + 150] = near
            unique = lambda x=x, l1=l1: ref[x:x + l1].copy()
            repeated = lambda far=far, l2=l2: np_revcomp(ref[far:far + l2])
            pair("rescued", 150, *((unique, repeated) if j == 0 else (repeated, unique)))
        for tlen in (MIN_TLEN, MAX_TLEN):
            fragment("at_bound", tlen)
            fragment("at_bound", tlen, mate1_forward=False)
        for tlen in (MIN_TLEN - 1, MAX_TLEN + 1):
            fragment("outside", tlen)
            fragment("outside", tlen, mate1_forward=False)
        fragment("same_strand", 140, both_forward=True)
        fragment("same_strand", 150, both_forward=True, mate1_forward=False)
        x, l1, _l2 = next(spots) + 20, next(lens), next(lens)
        pair("one_mate", 0, (lambda x=x, l1=l1: ref[x:x + l1].copy()), noise)                   # mate 1 mapped
        x, l1, _l2 = next(spots) + 20, next(lens), next(lens)
        pair("one_mate", 0, noise, (lambda x=x, l1=l1: np_revcomp(ref[x:x + l1])))              # mate 2 mapped
        for j in range(2):                                         # the partner twice, at 110 and at 170: two equally good pairs
            x, l1, l2 = fragment("two_best", 110, mate1_forward=j == 0)
            ref[x + 170 - l2:x + 170] = ref[x + 110 - l2:x + 110]
        n_by_hand = len(later)
        for mate1, mate2 in later:
            reads += [mate1(), mate2()]
        cut = _plant(t, 6103, 32, 2, per_kind=1)                   # across the alleles of every kind; mates as they come
        cut = [np_revcomp(r) if i % 2 else r for i, r in enumerate(cut)]
        reads += cut[:len(cut) & ~1]
        classes["unmapped"].append((len(reads) // 2, 0))           # the last pair
        reads += [noise(), noise()]
        assert all(30 <= len(r) <= 36 for r in reads[:2 * n_by_hand])
        _planted.update(t=t, reads=reads, classes=classes)
    return _planted["t"], _planted["reads"], _planted["classes"]


def _planted_chain(spm, ctx, reads=None):
    t, planted, _c = _planted_pairs()
    reads = planted if reads is None else reads
    ref_text, jst, ps = _open(spm, ctx, t, reads, 2)
    h = jst.search_device(ps, max_hits=1 << 21)
    lc = _chain(h, best=1, across=True, strands=True)
    rd = lc.reads(len(reads), 2)
    return lc, rd, (h, ps, jst, ref_text)


@gpu
def test_hand_planted_classes(spm, ctx):
    t, reads, classes = _planted_pairs()
    lc, rd, rest = _planted_chain(spm, ctx)
    pr, want, loci = _check_pairs(ctx, lc, rd, MIN_TLEN, MAX_TLEN)
    summary = rd.view()
    pat = loci["pattern"].astype(np.int64)
    n_pairs = len(reads) // 2
    assert len(want) == n_pairs and {c: len(v) for c, v in classes.items()} == dict(
        unmapped=2, proper_forward=2, proper_reverse=2, rescued=2, at_bound=4, outside=4, same_strand=2, one_mate=2, two_best=2)
    for p, tlen in classes["proper_forward"]:                      # tlen is the fragment length
        assert want[p]["tlen"] == tlen > 0 and (want[p]["flag1"], want[p]["flag2"]) == (0x63, 0x93) and want[p]["best"] == 0
        assert int(loci["ref_end"][want[p]["locus2"]]) - int(loci["ref_begin"][want[p]["locus1"]]) == tlen
    for p, tlen in classes["proper_reverse"]:
        assert want[p]["tlen"] == -tlen and (want[p]["flag1"], want[p]["flag2"]) == (0x53, 0xA3) and want[p]["best"] == 0
    for (p, tlen), mate in zip(classes["rescued"], (1, 0)):        # the reported locus is not the read summary's primary
        own = int(summary["primary"][2 * p + mate])
        got = int(want[p][("locus1", "locus2")[mate]])
        assert got != own and pat[got] == pat[own] and loci["score"][own] == 0 and loci["score"][got] == 1
        assert abs(int(loci["ref_begin"][own]) - int(loci["ref_begin"][got])) > 100
        assert want[p]["best"] == 1 and abs(int(want[p]["tlen"])) == tlen and want[p]["n_pairs"] == 1 and want[p]["flag1"] & 2
        assert int(want[p][("locus2", "locus1")[mate]]) == int(summary["primary"][2 * p + 1 - mate])
    assert sorted(abs(int(want[p]["tlen"])) for p, _t in classes["at_bound"]) == [MIN_TLEN] * 2 + [MAX_TLEN] * 2
    assert sorted(int(want[p]["tlen"]) for p, _t in classes["at_bound"]) == [-MAX_TLEN, -MIN_TLEN, MIN_TLEN, MAX_TLEN]
    for p, tlen in classes["outside"]:                             # one base outside either bound: discordant
        assert want[p]["best"] == -1 and want[p]["tlen"] == 0 and want[p]["flag1"] & 0xE == 0 and want[p]["n_pairs"] == 0
        l1, l2 = int(want[p]["locus1"]), int(want[p]["locus2"])
        f, v = (l1, l2) if not pat[l1] & 1 else (l2, l1)
        assert int(loci["ref_end"][v]) - int(loci["ref_begin"][f]) == tlen and (pat[f] & 1, pat[v] & 1) == (0, 1)
    for p, _t in classes["same_strand"]:
        assert want[p]["best"] == -1 and want[p]["flag1"] & 0x3E == 0 and want[p]["flag2"] & 0x3E == 0
        assert NONE not in (want[p]["locus1"], want[p]["locus2"])
    (p1, _), (p2, _) = classes["one_mate"]
    assert (want[p1]["flag1"], want[p1]["flag2"]) == (0x49, 0x85) and want[p1]["locus2"] == NONE != want[p1]["locus1"]
    assert (want[p2]["flag1"], want[p2]["flag2"]) == (0x45 | 0x20, 0x89 | 0x10) and want[p2]["locus1"] == NONE != want[p2]["locus2"]
    assert [p for p, _t in classes["unmapped"]] == [0, n_pairs - 1]
    for p, _t in classes["unmapped"]:
        assert want[p].tolist() == (NONE, NONE, 0, -1, 0, 0, 0, 0x4D, 0x8D)
    for (p, tlen), sign in zip(classes["two_best"], (1, -1)):
        assert want[p]["n_best"] == 2 == want[p]["n_pairs"] and want[p]["best"] == 0 and want[p]["tlen"] == sign * tlen
    # a second call returns the same bytes; other bounds give another answer, still the rule's
    again = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    assert again.view().tobytes() == want.tobytes()
    again.close()
    wide, want_wide, _l = _check_pairs(ctx, lc, rd, 1, 100_000)
    assert np.count_nonzero(want_wide["flag1"] & 2) > np.count_nonzero(want["flag1"] & 2)
    for p, _t in classes["rescued"]:                               # with room for the far copy the exact pair wins
        assert want_wide[p]["best"] == 0 and want_wide[p]["n_pairs"] == 2 and want_wide[p]["n_next"] == 1
    wide.close()
    # the result outlives the loci and the reads handle
    for x in (rd, lc) + rest:
        x.close()
    assert pr.view().tobytes() == want.tobytes() and download(ctx, pr.device()[0], n_pairs, PAIR).tobytes() == want.tobytes()
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 2: runs across wave and block edges
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_runs_across_wave_and_block_edges(spm, ctx):
    t = _make_tree(7101, 30_000, 1, 4, 6)
    rng = np.random.default_rng(7102)
    ref, apos = t["ref"], t["alleles"]["pos"].astype(np.int64)
    motif = lambda: rng.integers(0, 4, 30, dtype=np.uint8)
    many, many_mate, few, few_mate, other, other_mate = (motif() for _ in range(6))
    free = [p for p in range(100, len(ref) - 200, 80) if np.all((apos < p - 60) | (apos > p + 140))]
    assert len(free) >= 330

    def plant(p, left, right, left_sub=False, right_sub=False):    # left at [p, p + 30), right at [p + 40, p + 70): fragment 70
        ref[p:p + 30] = left
        if left_sub:
            ref[p + 15] = (int(left[15]) + 1) & 3
        if right is not None:
            ref[p + 40:p + 70] = right
            if right_sub:
                ref[p + 55] = (int(right[15]) + 1) & 3

    for p in free[:3]:
        plant(p, few, few_mate)
    big = free[3:326]
    for j, p in enumerate(big):                                    # no partner behind the first ten; one behind the last
        has = (j >= 10 and j % 3 == 0) or j == len(big) - 1
        plant(p, many, many_mate if has else None, left_sub=j % 40 == 7, right_sub=j % 30 == 0)
    for p in free[326:329]:
        plant(p, other, other_mate, right_sub=True)
    absent = [rng.integers(0, 4, 30, dtype=np.uint8) for _ in range(2)]
    reads = [few, np_revcomp(few_mate), many, np_revcomp(many_mate), np_revcomp(other_mate), other, absent[0], absent[1]]
    ref_text, jst, ps = _open(spm, ctx, t, reads, 1)
    h = jst.search_device(ps, max_hits=1 << 21)
    lc = _chain(h, best=1, across=True, strands=True)
    rd = lc.reads(len(reads), 2)
    min_tlen, max_tlen = 60, 400
    pr, want, loci = _check_pairs(ctx, lc, rd, min_tlen, max_tlen)
    s = rd.view()
    lo, n_fwd = int(s["first_locus"][2]), int(s["n_forward"][2])
    hi = int(s["first_locus"][3]) + int(s["n_loci"][3])
    assert n_fwd > 256 and s["n_loci"][2] == n_fwd and s["n_forward"][3] == 0 and s["n_loci"][3] >= 100
    assert lo + 64 < 256 < hi - 64 and lo % 64 and hi % 64 and len(loci) % 256 and len(loci) > hi   # block edge inside; runs in mid-wave
    assert s["n_loci"][0] and s["n_loci"][5]
    fb, vb = loci["ref_begin"][lo:lo + n_fwd].astype(np.int64), loci["ref_begin"][lo + n_fwd:hi].astype(np.int64)
    window = lambda a: np.nonzero((vb >= fb[a]) & (vb <= fb[a] + max_tlen))[0]
    assert len(window(0)) == 0 and len(window(1)) == 0              # empty at the run's start
    assert len(vb) - 1 in window(n_fwd - 1)                         # ... and touching the run's last element
    assert want[1]["n_pairs"] > 256 and want[1]["n_best"] > 64 and want[1]["n_next"] > 8 and want[1]["best"] == 0
    assert want[0]["n_pairs"] >= 3 and want[2]["tlen"] < 0 and want[2]["best"] == 1 and want[3]["flag1"] == 0x4D
    assert pr.stats().max_window >= 3
    pr.close()
    tight, want_tight, _l = _check_pairs(ctx, lc, rd, 70, 70)       # only the partner of the same place
    assert want_tight[1]["n_pairs"] == s["n_loci"][3] and want_tight[1]["tlen"] == 70
    tight.close()
    # zero reads: an empty result; no loci: every pair unmapped
    nothing = ctx.patterns(spm.ALGO_MYERS, absent, k=1, both_strands=True)
    h0 = jst.search_device(nothing, max_hits=1 << 21)
    assert len(h0) == 0
    lc0 = _chain(h0, best=1, across=True, strands=True)
    rd0, rd6 = lc0.reads(0, 2), lc0.reads(6, 2)
    none = lc0.pairs(rd0, 1, 10)
    assert len(none) == 0 and len(none.view()) == 0 and none.stats().n_pairs == 0
    none.close()
    pr6, want6, _l6 = _check_pairs(ctx, lc0, rd6, 1, 10)
    assert want6.tolist() == [(NONE, NONE, 0, -1, 0, 0, 0, 0x4D, 0x8D)] * 3 and pr6.stats().n_unmapped == 3
    for x in (pr6, rd6, rd0, lc0, h0, nothing, rd, lc, h, ps, jst, ref_text):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 3: what is refused
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(spm, ctx):
    t, reads, _classes = _planted_pairs()
    lc, rd, rest = _planted_chain(spm, ctx)
    h = rest[0]
    lib = spm.capi.lib()
    n = len(lc.view())
    err = lambda: lib.spm_hip_last_error(ctx._h)
    good = lc.pairs(rd, MIN_TLEN, MAX_TLEN).view()

    def refused(loci_h, reads_h, opts, word):
        out = ctypes.c_void_p()
        o = ctypes.byref(opts) if opts is not None else None
        assert lib.spm_hip_jst_ref_loci_pairs(loci_h, reads_h, o, ctypes.byref(out)) == -1 and not out.value
        assert word in err(), err()

    O = spm.capi.JstPairOpts
    plain = lc.reads(2 * len(reads), 1)                            # the same loci as 2n reads on one strand
    refused(lc._h, plain._h, O(100, 180, 0, 0), b"strands")
    odd = lc.reads(len(reads) + 1, 2)
    refused(lc._h, odd._h, O(100, 180, 0, 0), b"odd")
    lc_best = _chain(h, best=0, across=True, strands=True)          # another collapse with fewer loci
    assert len(lc_best.view()) < n
    rd_best = lc_best.reads(len(reads), 2)
    refused(lc._h, rd_best._h, O(100, 180, 0, 0), b"loci")
    refused(lc_best._h, rd._h, O(100, 180, 0, 0), b"loci")
    # the same number of loci, but other loci: the pairs in another order.  Only the device can tell
    moved = reads[2:] + reads[:2]
    lc_moved, rd_moved, rest_moved = _planted_chain(spm, ctx, moved)
    assert len(lc_moved.view()) == n and lc_moved.view().tobytes() != lc.view().tobytes()
    refused(lc._h, rd_moved._h, O(100, 180, 0, 0), b"disagree")
    refused(lc_moved._h, rd._h, O(100, 180, 0, 0), b"disagree")
    for bad, word in ((O(0, 180, 0, 0), b"min_tlen"), (O(181, 180, 0, 0), b"min_tlen"), (O(1, 1 << 31, 0, 0), b"max_tlen"),
                      (O(100, 180, 1, 0), b"flag"), (O(100, 180, 0, 7), b"reserved")):
        refused(lc._h, rd._h, bad, word)
    refused(lc._h, None, O(100, 180, 0, 0), b"NULL")
    refused(lc._h, rd._h, None, b"NULL")
    out = ctypes.c_void_p()
    ok = O(100, 180, 0, 0)
    assert lib.spm_hip_jst_ref_loci_pairs(None, rd._h, ctypes.byref(ok), ctypes.byref(out)) == -1 and not out.value
    assert lib.spm_hip_jst_ref_loci_pairs(lc._h, rd._h, ctypes.byref(ok), None) == -1
    assert lib.spm_hip_jst_pairs_view(None, None, None) == -1 and lib.spm_hip_jst_pairs_device(None, None, None) == -1
    assert lib.spm_hip_jst_pairs_stats(None, None) == -1
    lib.spm_hip_jst_pairs_destroy(None)
    with pytest.raises(spm.SpmError, match="-1"):
        lc.pairs(rd, 0, 5)
    # the largest bounds are taken, and after all of this the call still answers as before
    big = lc.pairs(rd, 1, (1 << 31) - 1)
    big.close()
    after = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    assert after.view().tobytes() == good.tobytes()
    for x in (after, rd_moved, lc_moved) + rest_moved + (rd_best, lc_best, odd, plain, rd, lc) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 4: the C++ mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("pairs_mirror_cases.cpp", tmp_path).exists()


@gpu
def test_mirror_routes_agree(spm, tmp_path):
    """locate_pairs: device route == host route, on pairs cut from the fixture haplotypes"""
    r = subprocess.run([str(build_mirror("pairs_mirror_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 100, r.stdout[-2000:]
    assert len(re.findall(r"pairs proper", r.stdout)) == 6
