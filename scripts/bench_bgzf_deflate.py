"""Time the deflated BGZF container on the device: one JSON line.

The inputs and the chain are those of scripts/bench_bam.py (the `pan_reads` tree, pairs and rescues).  Timed, in ONE process and
per flag combination of the BAM call: Bam.deflate() -- the device time of each of its three stages (HIP events), the host clock
of the call and the download of the deflated file; the frame kernel (Context.bgzf, the stored container) over the same record
stream in the same run, its host clock and the download of the stored blocks; the size zlib level 1 gives for the same blocks
on the host (zlib.compressobj(1, DEFLATED, -15) per block, plus the 26 bytes of the member around it), the reference the ratio
is stated against.  Then, once, both calls over raw device buffers (RAW_SHAPES): pseudo-random bytes, which stay stored, and
synthetic records.  Every time is the MEDIAN of --runs calls behind one warm-up call.  Nothing is asserted but that two calls
return the same bytes, that gzip reads the deflated file back as the stored one, and (up to 25 MB) that the bytes are the host
deflater's.  The row runs in a child process of its own under a time limit.

--dynamic adds, per row and in the same loop of the same run, the call with SPM_BGZF_DYNAMIC: its file bytes, its three block-type
counts and its stage times beside those without the flag ("dynamic": {...}); and one more BAM row, "qualities", whose records
carry Phred-like base qualities (values 2 .. 41, skewed) where the other rows have the ff fill.

    python scripts/bench_bgzf_deflate.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600]
                                         [--k 12] [--row-timeout 900] [--dynamic] [--out profiles/r17/bgzf_deflate.jsonl]
"""
import argparse
import ctypes
import gzip
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import libspm_amd as S  # noqa: E402

sys.dont_write_bytecode = True  # (scripts/ holds programs, not a package: leave no cache directory beside them)
from bench_pairs import med  # noqa: E402
from bench_rescue import build  # noqa: E402

STAGES = ("ms_parse", "ms_scan", "ms_place")
COUNTS = ("n_in", "n_out", "n_blocks", "n_stored_blocks", "n_matches", "n_literals", "n_prefix_bytes")
RAW_SHAPES = [(kind, n) for kind in ("random", "records") for n in (1 << 20, 25_000_000, 200_000_000)]


def zlib1_size(data, D=65280):
    """the file zlib level 1 makes of the same blocks (without an EOF block)"""
    total = 0
    for at in range(0, len(data), D):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(data[at:at + D])) + len(c.flush()) + 26
    return total


def compare(ctx, ptr, n, runs, deflate, stored_bytes=None, check=None, dynamic=None):
    """deflate() and the frame kernel over the same n bytes at ptr -> the figures of one row.  dynamic: the same call with the flag"""
    st = {s: [] for s in STAGES}
    dyn_st, dyn_first, dyn_types = {s: [] for s in STAGES}, None, None
    call, down, frame, frame_call, frame_down = [], [], [], [], []
    first, counts = None, {}
    for i in range(runs + 1):
        t0 = time.perf_counter()
        z = deflate()
        call.append((time.perf_counter() - t0) * 1e3)
        ds = z.deflate_stats()
        for s in STAGES:
            st[s].append(getattr(ds, s))
        t0 = time.perf_counter()
        raw = z.bytes()
        down.append((time.perf_counter() - t0) * 1e3)
        first = raw if first is None else first
        assert raw == first, "two calls returned different bytes"
        counts = {c: int(getattr(ds, c)) for c in COUNTS}
        z.close()
        if dynamic is not None:
            z = dynamic()
            ds = z.deflate_stats()
            for s in STAGES:
                dyn_st[s].append(getattr(ds, s))
            dyn_types = z.block_types()
            if dyn_first is None:
                dyn_first = z.bytes()
                assert gzip.decompress(dyn_first) == gzip.decompress(raw), "the flagged file inflates to other bytes"
            z.close()
        t0 = time.perf_counter()
        f = ctx.bgzf(ptr, n)
        frame_call.append((time.perf_counter() - t0) * 1e3)
        frame.append(f.stats().ms_frame)
        t0 = time.perf_counter()
        stored = f.bytes()
        frame_down.append((time.perf_counter() - t0) * 1e3)
        f.close()
    if check is not None:
        check(first, stored)
    ms_device = round(sum(med(st[s][1:]) for s in STAGES), 4)
    out = {"deflate": {s: med(v[1:]) for s, v in st.items()}, "ms_deflate_device": ms_device, "ms_deflate_call_host": med(call[1:]),
           "ms_download_deflated": med(down[1:]), "ms_frame_kernel": med(frame[1:]), "ms_frame_call_host": med(frame_call[1:]),
           "ms_download_stored": med(frame_down[1:]), "stored_file_bytes": len(stored) + counts["n_prefix_bytes"] if stored_bytes is None else stored_bytes,
           "deflated_file_bytes": len(first), **counts}
    out["ms_deflate_plus_download_host"] = round(out["ms_deflate_call_host"] + out["ms_download_deflated"], 3)
    out["ms_frame_plus_download_host"] = round(out["ms_frame_call_host"] + out["ms_download_stored"], 3)
    out["claim_holds"] = out["ms_deflate_plus_download_host"] < out["ms_frame_plus_download_host"]
    out["deflate_gb_per_s"] = round(n / max(ms_device, 1e-6) / 1e6, 3)
    if dynamic is not None:
        out["dynamic"] = {"file_bytes": len(dyn_first), "n_stored": dyn_types[0], "n_fixed": dyn_types[1], "n_dynamic": dyn_types[2],
                          **{s: med(v[1:]) for s, v in dyn_st.items()}}
    return out


def raw_rows(ctx, runs, dynamic=False):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_bgzf_deflate import records
    n_max = max(n for _k, n in RAW_SHAPES)
    unit = np.frombuffer(records(4000, 17), np.uint8)
    hosts = {"random": np.random.default_rng(1).integers(0, 256, n_max, dtype=np.uint8), "records": np.resize(unit, n_max)}
    out = []
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), n_max) == 0
    for kind, n in RAW_SHAPES:
        host = hosts[kind]
        assert hip.hipMemcpy(p, host.ctypes.data, n, 1) == 0
        data = host[:n].tobytes()

        def check(raw, stored, data=data, n=n):
            assert gzip.decompress(raw) == data
            if n <= 25_000_000:
                assert raw == S.bgzf_deflate_host(data)

        r = compare(ctx, p.value, n, runs, lambda: ctx.bgzf_deflate(p.value, n), check=check,
                    dynamic=(lambda: ctx.bgzf_deflate(p.value, n, dynamic=True)) if dynamic else None)
        r.update({"kind": kind, "bytes": n, "zlib_level1_file_bytes": zlib1_size(data) + 28})
        out.append(r)
    ctx.synchronize()
    assert hip.hipFree(p) == 0
    return out


def row(pan_log2, pan_reads, runs, min_tlen, max_tlen, k, dynamic=False):
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
    out.update({"loci": len(lc), "ref_len": ref_len})
    names = [f"pair.{p}/frag" for p in range(len(reads) // 2)]
    rows = [("plain", {}), ("cigar_m_secondary_names", {"cigar_m": True, "secondary": True, "names": names})]
    if dynamic:
        read_len = len(reads[0])
        qual = 41 - np.minimum(np.random.default_rng(21).geometric(0.25, (len(reads), read_len)) - 1, 39)
        rows.append(("qualities", {"qualities": qual.astype(np.uint8)}))
    for label, kw in rows:
        b = lc.bam_ex(rd, ps, "pan_ref", ref_len, pairs=pairs, rescues=rs, **kw)
        stored_file = b.bytes()
        stream = b.records()
        d_rec, n_rec = b.device()[2:4]

        def check(raw, _stored, stored_file=stored_file):
            assert gzip.decompress(raw) == gzip.decompress(stored_file)

        r = compare(ctx, d_rec, n_rec, runs, b.deflate, stored_bytes=len(stored_file), check=check,
                    dynamic=(lambda b=b: b.deflate(dynamic=True)) if dynamic else None)
        r.update({"n_records": int(b.stats().n_records), "n_record_bytes": n_rec, "zlib_level1_file_bytes":
                  zlib1_size(gzip.decompress(S.bam_header("pan_ref", ref_len))) + zlib1_size(stream) + 28})
        out[label] = r
        b.close()
    for x in (rs, pairs, rd, lc, nz, pr, a, sel, h, ps, jst, ref):
        x.close()
    out["raw_buffers"] = raw_rows(ctx, runs, dynamic)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-tlen", type=int, default=200)
    ap.add_argument("--max-tlen", type=int, default=600)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--row-timeout", type=int, default=900, help="seconds the row's child process may take")
    ap.add_argument("--dynamic", action="store_true", help="also time every call with SPM_BGZF_DYNAMIC, and a row with base qualities")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", action="store_true", help=argparse.SUPPRESS)   # the child's mode: the row's JSON on stdout
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: a median of at least 5 runs")
    if a.row:
        print(json.dumps(row(a.pan_log2, a.pan_reads, a.runs, a.min_tlen, a.max_tlen, a.k, a.dynamic)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--row", "--pan-log2", str(a.pan_log2), "--pan-reads", str(a.pan_reads),
           "--runs", str(a.runs), "--min-tlen", str(a.min_tlen), "--max-tlen", str(a.max_tlen), "--k", str(a.k)] + (["--dynamic"] if a.dynamic else [])
    r = subprocess.run(["timeout", "-k", "10", str(a.row_timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(json.dumps({"failed_row": "bgzf_deflate", "returncode": r.returncode}))
        return 1
    res = {"metric": "deflated BGZF: Bam.deflate and Context.bgzf_deflate beside the frame kernel on the same bytes in the same run, the "
                     "downloads of both files, zlib level 1 on the same blocks; medians of runs behind a warm-up, device times are HIP "
                     "events", "runs": a.runs, "bgzf_deflate": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
