"""Time mate rescue on the device beside the host route (the views downloaded, oracle.sellers per job): one JSON line.

The tree and the pairs are those of scripts/bench_pairs.py (the `pan_reads` tree, fragments of 300 .. 500 symbols, mates of
150 symbols with up to 3 edits), but in one pair in 16 a mate gets 8 substitutions more -- more than the search's k = 3 finds.
The chain is search -> select(best=1, across, strands) -> align_selected -> project -> normalize -> collapse -> reads -> pairs;
timed are JstPairs.rescue() -- the device time of each stage (HIP events) and the host clock of the call -- and, for
comparison, what a caller without it would do: download loci, read summary and pairs, then one oracle.sellers call per job
over the job's window (the search alone: no begin, no transcript).  Every figure is the MEDIAN of --runs calls behind one
warm-up call.  Nothing is asserted but that the host route finds the same (distance, end) for every job.  The row runs in a
child process of its own under a time limit.

    python scripts/bench_rescue.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600] [--k 12]
                                   [--row-timeout 420] [--out profiles/r13/rescue.jsonl]
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
from bench_pairs import COMP4, NONE, med  # noqa: E402


def build(ctx, log2_bases, n_reads):
    """the pan_reads tree and n_reads / 2 pairs cut from its haplotypes, as bench_pairs.build; pair p with p % 16 == 7 has 8
    substitutions more in its right mate"""
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
    for h in range(n_hap):
        piece = jst.extract(h, int(rng.integers(0, jst.haplotype_length(h) - chunk)), chunk)
        for p in range(h * per, min(n_pairs, (h + 1) * per)):
            frag = int(rng.integers(300, 501))
            o = int(rng.integers(0, chunk - frag - kmax - 1))
            left = edit_needle(piece[o:o + L + kmax], L, p % (kmax + 1), SEED_PAT ^ (p << 20))
            right = edit_needle(piece[o + frag - L:o + frag + kmax], L, (p // 4) % (kmax + 1), SEED_PAT ^ (p << 20) ^ 1)
            if p % 16 == 7:
                at = np.arange(9, L, 18)
                right[at] = (right[at] + 1) & 3
            right = COMP4[right[::-1]]
            reads[2 * p], reads[2 * p + 1] = (right, left) if p % 2 else (left, right)
    ps = ctx.patterns(S.ALGO_MYERS, reads, k=kmax, both_strands=True)
    st = jst.index(L + kmax, 0)
    info = {"pairs": n_pairs, "read_len": L, "k_search": kmax, "reference_bases": ref_len, "haplotypes": n_hap,
            "context_symbols": int(st.context_symbols)}
    return ref, jst, ps, reads, info


def host_route(oracle, T, reads, loci, pairs, k, min_tlen, max_tlen):
    """(distance, end) of every job, -1 / 0 for none: the search of the rule, one oracle.sellers call per job"""
    N = len(T)
    out = []
    for p in np.nonzero((pairs["flag1"] & 2) == 0)[0].tolist():
        for x in (1, 0):
            a = int(pairs["locus2" if x else "locus1"][p])
            if a == NONE:
                continue
            ab, ae, rev = int(loci["ref_begin"][a]), int(loci["ref_end"][a]), int(loci["pattern"][a]) & 1
            needle = reads[2 * p + 1 - x]
            if not rev:
                lo, needle = ab, COMP4[needle[::-1]]
                hi = min(lo + max_tlen, N)
                e0, e1 = max(lo + min_tlen, ae), hi
            else:
                lo, hi = max(0, ae - max_tlen), ae
                e0, e1 = lo + 1, ae
            best = (-1, 0)
            if e0 <= e1 and len(needle) > k:
                h = oracle.sellers(T[lo:hi], needle, k)
                ends, d = h["pos"].astype(np.int64) + lo, h["score"].astype(np.int64)
                ok = (ends >= e0) & (ends <= e1)
                if ok.any():
                    best = min(zip(d[ok].tolist(), ends[ok].tolist()))
            out.append(best)
    return out


def row(pan_log2, pan_reads, runs, min_tlen, max_tlen, k):
    from oracle import oracle
    oracle.build()
    ctx = S.Context(0)
    ref, jst, ps, reads, out = build(ctx, pan_log2, pan_reads)
    h = jst.search_device(ps, max_hits=1 << 26)
    sel = h.select(best=1, across=True, strands=True)
    a = sel.align_selected()
    pr = a.project()
    nz = pr.normalize()
    lc = nz.collapse()
    rd = lc.reads(len(reads), 2)
    pairs = lc.pairs(rd, min_tlen, max_tlen)
    out.update({"loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen, "k": k})
    stages = ("ms_total", "ms_jobs", "ms_search", "ms_align", "ms_emit")
    dev, host = {s: [] for s in stages}, []
    rs = None
    for _ in range(runs + 1):
        if rs is not None:
            rs.close()
        t0 = time.perf_counter()
        rs = pairs.rescue(lc, rd, ref, ps, k, min_tlen, max_tlen)
        host.append((time.perf_counter() - t0) * 1e3)
        st = rs.stats()
        for s in stages:
            dev[s].append(getattr(st, s))
    st = rs.stats()
    out["rescue_call"] = {**{s: med(v[1:]) for s, v in dev.items()}, "ms_call_host": med(host[1:]),
                          "ms_first_call_host": round(host[0], 3), "n_pairs": int(st.n_pairs), "n_jobs": int(st.n_jobs),
                          "n_rescued": int(st.n_rescued), "n_none": int(st.n_none), "n_not_concordant": int(st.n_not_concordant),
                          "n_short": int(st.n_short), "max_window": int(st.max_window)}
    t0 = time.perf_counter()
    loci, pv, T = lc.view(), pairs.view(), ref.download(0, len(ref))
    rd.view()
    t_view = (time.perf_counter() - t0) * 1e3
    t_host = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        want = host_route(oracle, T, reads, loci, pv, k, min_tlen, max_tlen)
        t_host.append((time.perf_counter() - t0) * 1e3)
    got = rs.view()[0]
    mine = [(int(s), int(e)) if s >= 0 else (-1, 0) for s, e in zip(got["score"].tolist(), got["ref_end"].tolist())]
    equal = mine == want
    out["host_route"] = {"ms_views": round(t_view, 3), "ms_sellers_per_job": med(t_host[1:]), "equal_to_device": bool(equal)}
    assert equal, "the host route and the device disagree"
    for x in (rs, pairs, rd, lc, nz, pr, a, sel, h, ps, jst, ref):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-tlen", type=int, default=200)
    ap.add_argument("--max-tlen", type=int, default=600)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds the row's child process may take")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", action="store_true", help=argparse.SUPPRESS)   # the child's mode: the row's JSON on stdout
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: a median of at least 5 runs")
    if a.row:
        print(json.dumps(row(a.pan_log2, a.pan_reads, a.runs, a.min_tlen, a.max_tlen, a.k)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--row", "--pan-log2", str(a.pan_log2), "--pan-reads", str(a.pan_reads),
           "--runs", str(a.runs), "--min-tlen", str(a.min_tlen), "--max-tlen", str(a.max_tlen), "--k", str(a.k)]
    r = subprocess.run(["timeout", "-k", "10", str(a.row_timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(json.dumps({"failed_row": "rescue", "returncode": r.returncode}))
        return 1
    res = {"metric": "mate rescue: spm_hip_jst_pairs_rescue beside the host route (views downloaded, oracle.sellers per job: the "
                     "search alone); medians of runs behind a warm-up, device times are HIP events", "runs": a.runs,
           "rescue": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
