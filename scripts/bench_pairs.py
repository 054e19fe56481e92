"""Time the pairing of paired-end mates on the device beside the same rule in NumPy on the downloaded loci: one JSON line.

The tree is the `pan_reads` tree of scripts/bench_jst_project.py (64 haplotypes over --pan-log2 reference bases); the reads
are --pan-reads / 2 PAIRS cut from its haplotypes: fragments of 300 .. 500 symbols, mates of 150 symbols with up to 3 edits,
every odd pair with mate 1 on the reverse strand, one pair in 16 with its mates on the same strand.  The chain is search ->
select(best=1, across, strands) -> align_selected -> project -> normalize -> collapse -> reads; timed are
JstRefLoci.pairs() -- device time (HIP events) and the host clock of the call -- and the vectorised NumPy rule on the loci
view.  Every figure is the MEDIAN of --runs calls behind one warm-up call.  Nothing is asserted but that NumPy's records
equal the device's.  The row runs in a child process of its own under a time limit.

    python scripts/bench_pairs.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600]
                                  [--row-timeout 420] [--out profiles/r12/pairs.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import libspm_amd as S  # noqa: E402

sys.dont_write_bytecode = True  # (scripts/ holds programs, not a package: leave no cache directory beside them)
from bench_align import SEED_PAT, SEED_TEXT, SEED_VAR, edit_needle  # noqa: E402

COMP4 = np.array([3, 2, 1, 0], dtype=np.uint8)
NONE = 0xFFFFFFFF


def med(xs):
    return round(float(np.median(xs)), 4)


def build(ctx, log2_bases, n_reads):
    """the pan_reads tree and n_reads / 2 pairs cut from its haplotypes"""
    n_hap, L, kmax = 64, 150, 3
    ref_len = max(640000, (1 << log2_bases) // 640000 * 640000)
    ref = ctx.generate(SEED_TEXT, 0, ref_len)
    alleles, pool, cov = S.synth_variants(SEED_TEXT, SEED_VAR, 0, ref_len, n_hap)
    jst = S.Jst(ctx, ref, alleles, pool, cov.reshape(-1, 1), n_hap)
    rng = np.random.default_rng(12)
    chunk = min(1 << 20, ref_len // 2)
    n_pairs = n_reads // 2
    reads = np.empty((2 * n_pairs, L), dtype=np.uint8)
    per = (n_pairs + n_hap - 1) // n_hap
    for h in range(n_hap):   # the pairs of haplotype h come from one stretch of it
        piece = jst.extract(h, int(rng.integers(0, jst.haplotype_length(h) - chunk)), chunk)
        for p in range(h * per, min(n_pairs, (h + 1) * per)):
            frag = int(rng.integers(300, 501))
            o = int(rng.integers(0, chunk - frag - kmax - 1))
            left = edit_needle(piece[o:o + L + kmax], L, p % (kmax + 1), SEED_PAT ^ (p << 20))
            right = edit_needle(piece[o + frag - L:o + frag + kmax], L, (p // 4) % (kmax + 1), SEED_PAT ^ (p << 20) ^ 1)
            if p % 16 != 15:
                right = COMP4[right[::-1]]
            reads[2 * p], reads[2 * p + 1] = (right, left) if p % 2 else (left, right)
    ps = ctx.patterns(S.ALGO_MYERS, reads, k=kmax, both_strands=True)
    st = jst.index(L + kmax, 0)
    info = {"pairs": n_pairs, "read_len": L, "k": kmax, "reference_bases": ref_len, "haplotypes": n_hap,
            "context_symbols": int(st.context_symbols)}
    return ref, jst, ps, reads, info


def numpy_pairs(loci, summary, min_tlen, max_tlen):
    """the rule of spm_hip_jst_ref_loci_pairs, vectorised: the loci are in (pattern, ref_begin) order, so the window of a
    forward locus in the other mate's reverse run is two binary searches over a composite key; all combinations inside the
    windows are laid out flat"""
    n_pairs = len(summary) // 2
    out = np.zeros(n_pairs, dtype=S.JST_PAIR_DTYPE)
    pat, sc = loci["pattern"].astype(np.int64), loci["score"].astype(np.int64)
    rb, re_ = loci["ref_begin"].astype(np.int64), loci["ref_end"].astype(np.int64)
    key = (pat << 40) | rb                                           # ascending: the loci order
    a = np.nonzero(pat % 2 == 0)[0]
    q = (pat[a] ^ 2) | 1                                             # the other mate's reverse pattern
    lo = np.searchsorted(key, (q << 40) | rb[a], side="left")
    hi = np.searchsorted(key, (q << 40) | (rb[a] + max_tlen), side="right")
    cnt = hi - lo
    A = np.repeat(a, cnt)
    B = np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    t = re_[B] - rb[A]
    ok = (re_[A] <= re_[B]) & (t >= min_tlen) & (t <= max_tlen)     # (rb[A] <= rb[B]: the window)
    A, B, t = A[ok], B[ok], t[ok]
    pair, total = pat[A] >> 2, sc[A] + sc[B]
    k1 = np.full(n_pairs, np.iinfo(np.int64).max)
    np.minimum.at(k1, pair, (total << 32) | A)
    first = ((total << 32) | A) == k1[pair]                          # the combinations of the best a: the smallest b wins
    b_best = np.full(n_pairs, np.iinfo(np.int64).max)
    np.minimum.at(b_best, pair[first], B[first])
    proper = k1 != np.iinfo(np.int64).max
    pa, pb = np.where(proper, k1 & 0xFFFFFFFF, 0), np.where(proper, b_best, 0)
    best = np.where(proper, k1 >> 32, -1)
    m1f = (pat[pa] & 2) == 0 if len(loci) else np.zeros(n_pairs, bool)
    p1, p2 = summary["primary"][0::2].astype(np.int64), summary["primary"][1::2].astype(np.int64)
    l1 = np.where(proper, np.where(m1f, pa, pb), p1)
    l2 = np.where(proper, np.where(m1f, pb, pa), p2)
    tl = (re_[pb] - rb[pa]) if len(loci) else np.zeros(n_pairs, np.int64)
    out["locus1"], out["locus2"] = l1, l2
    out["tlen"] = np.where(proper, np.where(m1f, tl, -tl), 0)
    out["best"] = best
    out["n_pairs"] = np.minimum(np.bincount(pair, minlength=n_pairs), NONE)
    d = total - best[pair]
    out["n_best"] = np.minimum(np.bincount(pair[d == 0], minlength=n_pairs), NONE)
    out["n_next"] = np.minimum(np.bincount(pair[d == 1], minlength=n_pairs), NONE)
    un1, un2 = l1 == NONE, l2 == NONE
    r1 = ~un1 & ((pat[np.where(un1, 0, l1)] & 1) == 1) if len(loci) else np.zeros(n_pairs, bool)
    r2 = ~un2 & ((pat[np.where(un2, 0, l2)] & 1) == 1) if len(loci) else np.zeros(n_pairs, bool)
    base = 1 | np.where(proper, 2, 0)
    out["flag1"] = base | 4 * un1 | 8 * un2 | 16 * r1 | 32 * r2 | 0x40
    out["flag2"] = base | 4 * un2 | 8 * un1 | 16 * r2 | 32 * r1 | 0x80
    return out


def row(pan_log2, pan_reads, runs, min_tlen, max_tlen):
    ctx = S.Context(0)
    ref, jst, ps, reads, out = build(ctx, pan_log2, pan_reads)
    h = jst.search_device(ps, max_hits=1 << 26)
    sel = h.select(best=1, across=True, strands=True)
    a = sel.align_selected()
    pr = a.project()
    nz = pr.normalize()
    lc = nz.collapse()
    rd = lc.reads(len(reads), 2)
    out.update({"records": len(h), "selected": len(sel), "loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen})
    dev, host = [], []
    pairs = None
    for _ in range(runs + 1):
        if pairs is not None:
            pairs.close()
        t0 = time.perf_counter()
        pairs = lc.pairs(rd, min_tlen, max_tlen)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(pairs.stats().ms_total)
    st = pairs.stats()
    t0 = time.perf_counter()
    loci, summary = lc.view(), rd.view()
    t_view = (time.perf_counter() - t0) * 1e3
    t_np = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        want = numpy_pairs(loci, summary, min_tlen, max_tlen)
        t_np.append((time.perf_counter() - t0) * 1e3)
    equal = pairs.view().tobytes() == want.tobytes()
    out["pairs_call"] = {"ms_device": med(dev[1:]), "ms_call_host": med(host[1:]), "ms_first_call_host": round(host[0], 3),
                         "n_pairs": int(st.n_pairs), "n_proper": int(st.n_proper), "n_unique": int(st.n_unique),
                         "n_multi": int(st.n_multi), "n_discordant": int(st.n_discordant), "n_one_mate": int(st.n_one_mate),
                         "n_unmapped": int(st.n_unmapped), "max_window": int(st.max_window)}
    out["numpy_host_route"] = {"ms_views": round(t_view, 3), "ms_rule": med(t_np[1:]), "equal_to_device": bool(equal)}
    assert equal, "the NumPy rule and the device disagree"
    for x in (pairs, rd, lc, nz, pr, a, sel, h, ps, jst, ref):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-tlen", type=int, default=200)
    ap.add_argument("--max-tlen", type=int, default=600)
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds the row's child process may take")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", action="store_true", help=argparse.SUPPRESS)   # the child's mode: the row's JSON on stdout
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: a median of at least 5 runs")
    if a.row:
        print(json.dumps(row(a.pan_log2, a.pan_reads, a.runs, a.min_tlen, a.max_tlen)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--row", "--pan-log2", str(a.pan_log2), "--pan-reads", str(a.pan_reads),
           "--runs", str(a.runs), "--min-tlen", str(a.min_tlen), "--max-tlen", str(a.max_tlen)]
    r = subprocess.run(["timeout", "-k", "10", str(a.row_timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(json.dumps({"failed_row": "pairs", "returncode": r.returncode}))
        return 1
    res = {"metric": "paired-end mates: spm_hip_jst_ref_loci_pairs beside the vectorised NumPy rule on the downloaded loci; "
                     "medians of runs behind a warm-up, device times are HIP events", "runs": a.runs,
           "pairs": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
