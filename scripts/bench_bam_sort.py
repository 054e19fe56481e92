"""Time the coordinate sort of a BAM handle and the BAI index of the sorted file on the device: one JSON line.

The inputs and the chain are those of scripts/bench_bam.py (the `pan_reads` tree, pairs and rescues).  Timed, in ONE process and
per flag combination: JstRefLoci.bam() -- its own stages, what the sort is compared with; Bam.sort() -- the device time of each of
its five stages (HIP events), the host clock of the call, and what the gather kernel moves in GB/s (the record bytes once, read
and written); Bam.index() of the stored file and Bam.index(deflated) of the deflated one -- their four stages; the downloads of
the sorted file and of the index; and a HOST ROUTE over the downloaded unsorted file as the baseline: the keys out of the record
stream, a stable argsort, the records moved, spm_hip_bgzf_frame_host and spm_hip_bai_build_host, by the host clock (NumPy and the
library's serial host code; its file and index must equal the device's).  Every figure is the MEDIAN of --runs calls behind one
warm-up call.  Nothing is asserted but that two calls return the same bytes and that host route and device agree.  The row runs
in a child process of its own under a time limit.

    python scripts/bench_bam_sort.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600] [--k 12]
                                     [--row-timeout 420] [--out profiles/r19/bam_sort.jsonl]
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

BAM_STAGES = ("ms_total", "ms_lines", "ms_measure", "ms_write", "ms_frame", "ms_stats")
SORT_STAGES = ("ms_total", "ms_keys", "ms_sort", "ms_place", "ms_gather", "ms_frame")
BAI_STAGES = ("ms_total", "ms_records", "ms_chunks", "ms_bins", "ms_write")
BAI_COUNTS = ("n_bins", "n_chunks", "n_intv", "n_mapped", "n_unmapped", "n_no_coor", "n_bytes")


def host_route(raw_records, lines, rname, ref_len):
    """the unsorted record stream and its line records -> (the sorted file, its index, the milliseconds of each step)"""
    ms = {}
    t0 = time.perf_counter()
    stream = np.frombuffer(raw_records, np.uint8)
    off = lines["offset"].astype(np.int64)
    field = lambda at: (stream[off + at].astype(np.uint32) | stream[off + at + 1].astype(np.uint32) << 8 |
                        stream[off + at + 2].astype(np.uint32) << 16 | stream[off + at + 3].astype(np.uint32) << 24)
    ref_id, pos, flag = field(4), field(8), field(16) >> 16
    key = (ref_id != 0).astype(np.uint64) << np.uint64(33) | (pos + np.uint32(1)).astype(np.uint64) << np.uint64(1) | ((flag >> 4) & 1).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    ms["ms_keys_and_stable_sort"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    out_lines = lines[order].copy()
    lens = out_lines["len"].astype(np.int64)
    new_off = np.cumsum(lens) - lens
    out_lines["offset"] = new_off
    src = np.repeat(off[order] - new_off, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    sorted_stream = stream[src].tobytes()
    ms["ms_move_records"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    header = S.bam_header(rname, ref_len, sorted=True)
    file = header + S.bgzf_frame_host(sorted_stream)
    ms["ms_frame_host"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    D = 65280
    nb = (len(sorted_stream) + D - 1) // D
    offsets = np.array([len(header) + b * (D + 31) for b in range(nb)] + [len(header) + len(sorted_stream) + 31 * nb], np.uint64)
    bai = S.bai_build_host(sorted_stream, out_lines, offsets)
    ms["ms_bai_build_host"] = (time.perf_counter() - t0) * 1e3
    ms["ms_total"] = sum(ms.values())
    return file, bai, ms


def row(pan_log2, pan_reads, runs, min_tlen, max_tlen, k):
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
    rs = pairs.rescue(lc, rd, ref, ps, k, min_tlen, max_tlen)
    ref_len = len(ref)
    out.update({"loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen, "k": k, "ref_len": ref_len})
    names = [f"pair.{p}/frag" for p in range(len(reads) // 2)]
    for label, kw in (("plain", {}), ("cigar_m_secondary_names", {"cigar_m": True, "secondary": True, "names": names})):
        stages = {"bam": {s: [] for s in BAM_STAGES}, "sort": {s: [] for s in SORT_STAGES}, "index": {s: [] for s in BAI_STAGES},
                  "index_deflated": {s: [] for s in BAI_STAGES}}
        clock = {x: [] for x in ("sort_call", "index_call", "index_deflated_call", "download_unsorted", "download_sorted", "download_bai")}
        host = {}
        first = None
        for i in range(runs + 1):
            b = lc.bam(rd, ps, "pan_ref", ref_len, pairs=pairs, rescues=rs, **kw)
            st = b.stats()
            for x in BAM_STAGES:
                stages["bam"][x].append(getattr(st, x))
            t0 = time.perf_counter()
            s = b.sort()
            clock["sort_call"].append((time.perf_counter() - t0) * 1e3)
            ss = s.sort_stats()
            for x in SORT_STAGES:
                stages["sort"][x].append(getattr(ss, x))
            t0 = time.perf_counter()
            z = s.index()
            clock["index_call"].append((time.perf_counter() - t0) * 1e3)
            zs = z.stats()
            for x in BAI_STAGES:
                stages["index"][x].append(getattr(zs, x))
            f = s.deflate()
            t0 = time.perf_counter()
            zf = s.index(f)
            clock["index_deflated_call"].append((time.perf_counter() - t0) * 1e3)
            for x in BAI_STAGES:
                stages["index_deflated"][x].append(getattr(zf.stats(), x))
            t0 = time.perf_counter()
            raw = s.bytes()
            clock["download_sorted"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            bai = z.bytes()
            clock["download_bai"].append((time.perf_counter() - t0) * 1e3)
            first = (raw, bai, zf.bytes()) if first is None else first
            assert (raw, bai, zf.bytes()) == first, "two calls returned different bytes"
            t0 = time.perf_counter()
            unsorted_records, unsorted_lines = b.records(), b.lines()
            b.bytes()
            clock["download_unsorted"].append((time.perf_counter() - t0) * 1e3)
            want_file, want_bai, ms = host_route(unsorted_records, unsorted_lines, "pan_ref", ref_len)
            assert want_file == raw and want_bai == bai, "the host route and the device disagree"
            for x, v in ms.items():
                host.setdefault(x, []).append(v)
            counts = {c: int(getattr(zs, c)) for c in BAI_COUNTS}
            counts.update(n_records=int(ss.n_records), n_record_bytes=int(ss.n_record_bytes), n_file_bytes=int(s.stats().n_file_bytes),
                          n_deflated_file_bytes=int(f.stats().n_out), key_bits=int(ss.key_bits))
            for x in (zf, f, z, s, b):
                x.close()
        m = lambda d: {x: med(v[1:]) for x, v in d.items()}
        gather = med(stages["sort"]["ms_gather"][1:])
        out[label] = {**{name: m(d) for name, d in stages.items()}, "ms_host_clock": m(clock), "host_route": m(host), **counts,
                      "gather_gb_per_s_read_plus_written": round(2 * counts["n_record_bytes"] / max(gather, 1e-6) / 1e6, 1),
                      "gather_gb_per_s_record_bytes": round(counts["n_record_bytes"] / max(gather, 1e-6) / 1e6, 1)}
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
        print(json.dumps({"failed_row": "bam_sort", "returncode": r.returncode}))
        return 1
    res = {"metric": "coordinate-sorted BAM and BAI: spm_hip_bam_sort and spm_hip_bam_index behind the BAM call of the same run, the "
                     "index of the deflated file, the downloads, and a host route over the downloaded file; medians of runs behind a "
                     "warm-up, device times are HIP events", "runs": a.runs, "bam_sort": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
