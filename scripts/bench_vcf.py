"""Time the genotype calls and the VCF text of a pileup's sites on the device: one JSON line.

The inputs and the chain are those of scripts/bench_bam_pileup.py (the `pan_reads` tree, pairs and rescues, every tenth pair a
copy of the pair before it, base qualities), followed by Bam.sort(), Bam.markdup(), Bam.pileup() and Pileup.site_records().
Timed, in ONE process, per set of sites: PileupSites.vcf() -- the device time of each of its three stages (HIP events) and the
host clock of the call; beside it the download of the site records and spm_hip_pileup_sites_vcf_host over them, by the host
clock, whose bytes must equal the device's; the pileup's own ms_total, for scale; and a bare device-to-device copy of
n_text_bytes between two buffers (HIP events), with the ratio of the write stage to it -- written down, no threshold.  Two sets
of sites: the default thresholds of Pileup.sites(), and every covered column with at least one read against the reference
(min_alt 1, no share), which is some thousand times as many sites and mostly ref/ref calls.  Every figure is the MEDIAN of --runs
calls behind one warm-up call.  Nothing is asserted but that two calls return the same bytes and that host and device agree.
The row runs in a child process of its own under a time limit.

    python scripts/bench_vcf.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600] [--k 12]
                                [--row-timeout 420] [--out profiles/r25/vcf.jsonl]
"""
import argparse
import ctypes
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

STAGES = ("ms_total", "ms_call", "ms_scan", "ms_write")
COUNTS = ("n_sites", "n_variant", "n_ref", "n_ref_n", "n_low_qual", "n_header_bytes", "n_text_bytes", "group_sites")


def bare_copy_ms(ctx, n_bytes, runs):
    """a device-to-device copy of n_bytes between two buffers of their own, by HIP events: the median of `runs` behind a warm-up"""
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipFree.argtypes = [vp]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipMemset.argtypes = [vp, ctypes.c_int, ctypes.c_size_t]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    ctx.synchronize()
    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    assert hip.hipMalloc(ctypes.byref(src), max(n_bytes, 1)) == 0 and hip.hipMalloc(ctypes.byref(dst), max(n_bytes, 1)) == 0
    assert hip.hipMemset(src, 0x41, max(n_bytes, 1)) == 0
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    ms = []
    for _ in range(runs + 1):
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(dst, src, n_bytes, 3, None) == 0   # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        t = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
        ms.append(t.value)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    for p in (src, dst):
        hip.hipFree(p)
    return med(ms[1:])


def vcf_rows(ctx, p, ref, ref_len, runs, **site_kw):
    sr = p.site_records(ref, **site_kw)
    stages = {x: [] for x in STAGES}
    clock = {x: [] for x in ("vcf_call", "download_sites", "vcf_host")}
    counts, first = {}, None
    for i in range(runs + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        v = sr.vcf("pan_ref", "sample", ref_len)
        clock["vcf_call"].append((time.perf_counter() - t0) * 1e3)
        st = v.stats()
        for x in STAGES:
            stages[x].append(getattr(st, x))
        counts = {c: int(getattr(st, c)) for c in COUNTS}
        if i in (0, runs):                                          # the first and the last call return the same bytes
            got = v.text()
            first = got if first is None else first
            assert got == first, "two calls returned different bytes"
        v.close()
    for i in range(runs + 1):
        fresh = p.site_records(ref, **site_kw)                      # a handle that has not been downloaded yet
        ctx.synchronize()
        t0 = time.perf_counter()
        sites = fresh.view()
        clock["download_sites"].append((time.perf_counter() - t0) * 1e3)
        fresh.close()
        t0 = time.perf_counter()
        host = S.pileup_sites_vcf_host(sites, "pan_ref", "sample", ref_len)
        clock["vcf_host"].append((time.perf_counter() - t0) * 1e3)
        if i == 0:
            assert host == first, "the host builder and the device disagree"
        del host
    sr.close()
    m_ = lambda d: {x: med(v[1:]) for x, v in d.items()}
    copy = bare_copy_ms(ctx, counts["n_text_bytes"], runs)
    write = med(stages["ms_write"][1:])
    return {"site_opts": site_kw, "stages": m_(stages), "ms_host_clock": m_(clock), **counts, "site_bytes": 32 * counts["n_sites"],
            "ms_bare_copy_of_text": copy, "write_over_bare_copy": round(write / max(copy, 1e-6), 2)}


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
    quals = np.random.default_rng(23).integers(2, 42, reads.shape, dtype=np.uint8)
    b = lc.bam_ex(rd, ps, "pan_ref", ref_len, qualities=quals, pairs=pairs, rescues=rs)
    s = b.sort()
    m = s.markdup()
    totals = []
    for _ in range(runs + 1):
        p = m.pileup()
        totals.append(p.stats().ms_total)
        if len(totals) <= runs:
            p.close()
    out.update({"loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen, "k": k, "ref_len": ref_len, "pileup_ms_total": med(totals[1:])})
    out["vcf"] = [vcf_rows(ctx, p, ref, ref_len, runs), vcf_rows(ctx, p, ref, ref_len, runs, min_depth=1, min_alt=1, min_alt_permille=0)]
    for x in (p, m, s, b, rs, pairs, rd, lc, nz, pr, a, sel, h, ps, jst, ref):
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
        print(json.dumps({"failed_row": "vcf", "returncode": r.returncode}))
        return 1
    res = {"metric": "genotype calls and VCF text of a pileup's sites: spm_hip_pileup_sites_vcf behind sort, markdup, pileup and sites of the "
                     "same run, at the default site thresholds and at min_alt 1; the download of the site records and "
                     "spm_hip_pileup_sites_vcf_host over them; the pileup's ms_total; a bare device copy of n_text_bytes; medians of runs "
                     "behind a warm-up, device times are HIP events",
           "runs": a.runs, "vcf": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
