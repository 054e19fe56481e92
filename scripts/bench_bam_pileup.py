"""Time the pileup of a sorted, duplicate-marked BAM handle on the device: one JSON line.

The inputs and the chain are those of scripts/bench_bam_markdup.py (the `pan_reads` tree, pairs and rescues, every tenth pair a
copy of the pair before it, base qualities), followed by Bam.sort() and Bam.markdup().  Timed, in ONE process: Bam.pileup() over
the whole reference -- the device time of each of its four stages (HIP events), the host clock of the call, what the tiles
stage reads in GB/s (the record bytes once) and n_tile_visits / n_taking_part, the redundancy of the tile scheme; beside it
ms_keys of the markdup call, the other stage that reads the bulk of the stream exactly once; the download of the record stream
and its line records; spm_hip_bam_pileup_host over the downloaded stream, by the host clock, whose counts must equal the
device's; and Pileup.sites() against the resident reference.  Every figure is the MEDIAN of --runs calls behind one warm-up call
(the host builder, which writes 32 bytes per reference position, runs --host-runs times).  Nothing is asserted but that two calls
return the same bytes and that host and device agree.  The row runs in a child process of its own under a time limit.

    python scripts/bench_bam_pileup.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--host-runs 3] [--min-tlen 200]
                                       [--max-tlen 600] [--k 12] [--row-timeout 420] [--out profiles/r24/bam_pileup.jsonl]
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
from bench_pairs import med  # noqa: E402
from bench_rescue import build  # noqa: E402

STAGES = ("ms_total", "ms_records", "ms_scan", "ms_tiles", "ms_summary")
COUNTS = ("n_records", "n_taking_part", "n_evidence", "n_covered", "sum_depth", "max_depth", "n_tile_visits", "tile_positions")


def row(pan_log2, pan_reads, runs, host_runs, min_tlen, max_tlen, k):
    ctx = S.Context(0)
    ref, jst, ps, reads, out = build(ctx, pan_log2, pan_reads)
    ps.close()
    for p in range(9, len(reads) // 2, 10):                         # every tenth pair repeats the pair before it
        reads[2 * p], reads[2 * p + 1] = reads[2 * p - 2], reads[2 * p - 1]
    ps = ctx.patterns(S.ALGO_MYERS, reads, k=out["k_search"], both_strands=True)
    h = jst.search_device(ps, max_hits=1 << 26)
    sel = h.select(best=1, across=True, strands=True)
    a = sel.align_selected()
    pr = a.project()
    nz = pr.normalize()
    lc = nz.collapse()
    rd = lc.reads(len(reads), 2)
    pairs = lc.pairs(rd, min_tlen, max_tlen)
    rs = pairs.rescue(lc, rd, ref, ps, k, min_tlen, max_tlen)
    ref_len = len(ref)
    quals = np.random.default_rng(23).integers(2, 42, reads.shape, dtype=np.uint8)
    b = lc.bam_ex(rd, ps, "pan_ref", ref_len, qualities=quals, pairs=pairs, rescues=rs)
    s = b.sort()
    keys = []
    for _ in range(runs + 1):
        m = s.markdup()
        keys.append(m.markdup_stats().ms_keys)
        if len(keys) <= runs:
            m.close()
    out.update({"loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen, "k": k, "ref_len": ref_len, "markdup_ms_keys": med(keys[1:])})
    stages = {x: [] for x in STAGES}
    clock = {x: [] for x in ("pileup_call", "download_stream", "pileup_host", "sites_call")}
    counts, first, n_sites = {}, None, 0
    for i in range(runs + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        p = m.pileup()
        clock["pileup_call"].append((time.perf_counter() - t0) * 1e3)
        st = p.stats()
        for x in STAGES:
            stages[x].append(getattr(st, x))
        counts = {c: int(getattr(st, c)) for c in COUNTS}
        t0 = time.perf_counter()
        n_sites = len(p.sites(ref))
        clock["sites_call"].append((time.perf_counter() - t0) * 1e3)
        if i in (0, runs):                                          # the first and the last call return the same bytes
            got = p.counts()
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), "two calls returned different bytes"
        p.close()
    m2 = s.markdup()                                                # a handle that has not been downloaded yet
    t0 = time.perf_counter()
    stream, lines = m2.records(), m2.lines()
    clock["download_stream"].append((time.perf_counter() - t0) * 1e3)
    m2.close()
    for i in range(host_runs + 1):
        t0 = time.perf_counter()
        host = S.bam_pileup_host(stream, lines, ref_len)
        clock["pileup_host"].append((time.perf_counter() - t0) * 1e3)
        if i == 0:
            assert np.array_equal(host, first), "the host builder and the device disagree"
        del host
    m_ = lambda d: {x: med(v[1:] if len(v) > 1 else v) for x, v in d.items()}
    tiles = med(stages["ms_tiles"][1:])
    out["pileup"] = {"stages": m_(stages), "ms_host_clock": m_(clock), **counts, "n_record_bytes": len(stream), "n_sites": n_sites,
                     "count_bytes": int(first.nbytes), "tile_visits_per_record": round(counts["n_tile_visits"] / max(counts["n_taking_part"], 1), 3),
                     "tiles_gb_per_s_record_bytes": round(len(stream) / max(tiles, 1e-6) / 1e6, 1),
                     "tiles_gb_per_s_count_bytes": round(int(first.nbytes) / max(tiles, 1e-6) / 1e6, 1)}
    for x in (m, s, b, rs, pairs, rd, lc, nz, pr, a, sel, h, ps, jst, ref):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
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
        print(json.dumps(row(a.pan_log2, a.pan_reads, a.runs, a.host_runs, a.min_tlen, a.max_tlen, a.k)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--row", "--pan-log2", str(a.pan_log2), "--pan-reads", str(a.pan_reads),
           "--runs", str(a.runs), "--host-runs", str(a.host_runs), "--min-tlen", str(a.min_tlen), "--max-tlen", str(a.max_tlen), "--k", str(a.k)]
    r = subprocess.run(["timeout", "-k", "10", str(a.row_timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(json.dumps({"failed_row": "bam_pileup", "returncode": r.returncode}))
        return 1
    res = {"metric": "pileup of a sorted, duplicate-marked BAM handle over the whole reference: spm_hip_bam_pileup behind sort and markdup "
                     "of the same run, ms_keys of that markdup beside it, the download of the record stream, spm_hip_bam_pileup_host over "
                     "the downloaded stream, and spm_hip_pileup_sites; medians of runs behind a warm-up, device times are HIP events",
           "runs": a.runs, "host_runs": a.host_runs, "bam_pileup": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
