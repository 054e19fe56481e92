"""Time duplicate marking of a BAM handle on the device: one JSON line.

The inputs and the chain are those of scripts/bench_bam_sort.py (the `pan_reads` tree, pairs and rescues), with every tenth pair
replaced by a copy of the pair before it: about 10 % planted duplicates.  Timed, in ONE process, without and with base
qualities: Bam.markdup() -- the device time of each of its five stages (HIP events), the host clock of the call, and what the
keys stage reads in GB/s (the record bytes once); next to it Bam.sort() of the same handle -- its device total and the host
clock of the call; the download of the marked file (file, record stream and line records); and spm_hip_bam_markdup_host over the
downloaded stream, by the host clock, whose marks must equal the device's.  Every figure is the MEDIAN of --runs calls behind
one warm-up call.  Nothing is asserted but that two calls return the same bytes and that host and device agree.  The row runs in
a child process of its own under a time limit.

    python scripts/bench_bam_markdup.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600] [--k 12]
                                        [--row-timeout 420] [--out profiles/r23/bam_markdup.jsonl]
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

STAGES = ("ms_total", "ms_keys", "ms_sort", "ms_mark", "ms_write", "ms_frame")
COUNTS = ("n_records", "n_pairs", "n_fragments", "n_dup_pairs", "n_dup_fragments", "n_dup_records", "n_fragments_beside_pairs")


def row(pan_log2, pan_reads, runs, min_tlen, max_tlen, k):
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
    out.update({"loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen, "k": k, "ref_len": ref_len, "planted_duplicate_pairs": len(reads) // 20})
    quals = np.random.default_rng(23).integers(2, 42, reads.shape, dtype=np.uint8)
    for label, q in (("no_qualities", None), ("qualities", quals)):
        stages = {s: [] for s in STAGES}
        clock = {x: [] for x in ("markdup_call", "sort_call", "download_marked", "markdup_host")}
        sort_total, first, counts = [], None, {}
        for i in range(runs + 1):
            b = lc.bam_ex(rd, ps, "pan_ref", ref_len, qualities=q, pairs=pairs, rescues=rs)
            ctx.synchronize()
            t0 = time.perf_counter()
            m = b.markdup()
            clock["markdup_call"].append((time.perf_counter() - t0) * 1e3)
            ms = m.markdup_stats()
            for x in STAGES:
                stages[x].append(getattr(ms, x))
            t0 = time.perf_counter()
            s = b.sort()
            clock["sort_call"].append((time.perf_counter() - t0) * 1e3)
            sort_total.append(s.sort_stats().ms_total)
            t0 = time.perf_counter()
            raw, stream, lines = m.bytes(), m.records(), m.lines()
            clock["download_marked"].append((time.perf_counter() - t0) * 1e3)
            first = (raw, lines.tobytes()) if first is None else first
            assert (raw, lines.tobytes()) == first, "two calls returned different bytes"
            in_stream, in_lines = b.records(), b.lines()
            t0 = time.perf_counter()
            dup = S.bam_markdup_host(in_stream, in_lines, ref_len)
            clock["markdup_host"].append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(dup, (lines["flag"] >> 10) & 1), "the host builder and the device disagree"
            counts = {c: int(getattr(ms, c)) for c in COUNTS}
            counts.update(n_record_bytes=len(stream), n_file_bytes=len(raw))
            for x in (s, m, b):
                x.close()
        m_ = lambda d: {x: med(v[1:]) for x, v in d.items()}
        keys = med(stages["ms_keys"][1:])
        out[label] = {"markdup": m_(stages), "sort_ms_total": med(sort_total[1:]), "ms_host_clock": m_(clock), **counts,
                      "keys_gb_per_s_record_bytes": round(counts["n_record_bytes"] / max(keys, 1e-6) / 1e6, 1)}
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
        print(json.dumps({"failed_row": "bam_markdup", "returncode": r.returncode}))
        return 1
    res = {"metric": "duplicate marking of a BAM handle: spm_hip_bam_markdup behind the BAM call of the same run, the sort call beside "
                     "it, the download of the marked file, and spm_hip_bam_markdup_host over the downloaded stream; medians of runs "
                     "behind a warm-up, device times are HIP events", "runs": a.runs, "bam_markdup": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
