"""Time the BAM writer on the device: one JSON line.

The inputs and the chain are those of scripts/bench_sam.py (the `pan_reads` tree, pairs and rescues).  Timed, in ONE process and
per flag combination: JstRefLoci.bam() -- the device time of each of its five stages (HIP events) and the host clock of the
call; JstRefLoci.sam() on the same inputs in the same run -- its four stages, what the BAM call is compared with; the frame
kernel alone over that SAM text (Sam.bgzf), in GB/s of input; the download of the file; the C++ mirror's host route on the same
inputs (sam_host, then bam_of_sam with its framing: scripts/bench_bam_host.cpp, compiled here; its file must equal the
device's); and, once, the frame kernel alone over raw buffers of pseudo-random bytes (Context.bgzf: sizes, source offsets and
block sizes in RAW_SHAPES).  Every figure is the MEDIAN of --runs calls behind one warm-up call.  Nothing is asserted but that
two calls return the same bytes, that the file's size is what its statistics say, that gzip reads the framed SAM text back and
that the framed raw buffers equal the host framer's.  The row runs in a child process of its own under a time limit.
With --qual and / or --md the calls are spm_hip_jst_ref_loci_bam_ex / _sam_ex with the qualities of bench_sam.phred_profile and /
or the MD tag; the host route's timer knows neither, so its figure is left out then.

    python scripts/bench_bam.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600] [--k 12]
                                [--qual] [--md] [--row-timeout 420] [--out profiles/r15/bam.jsonl]
"""
import argparse
import ctypes
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import libspm_amd as S  # noqa: E402

sys.dont_write_bytecode = True  # (scripts/ holds programs, not a package: leave no cache directory beside them)
from bench_pairs import COMP4, med  # noqa: E402
from bench_rescue import build  # noqa: E402
from bench_sam import phred_profile  # noqa: E402

BAM_STAGES = ("ms_total", "ms_lines", "ms_measure", "ms_write", "ms_frame", "ms_stats")
SAM_STAGES = ("ms_total", "ms_lines", "ms_measure", "ms_write", "ms_stats")
# the frame kernel alone: (bytes, offset of the source from a 16-byte border, block_data)
RAW_SHAPES = [(n, off, D) for n in (1 << 20, 25_000_000, 200_000_000) for off in (0, 3) for D in (0, 4096)]
COUNTS = ("n_records", "n_record_bytes", "n_file_bytes", "header_file_bytes", "n_record_blocks", "n_reported", "n_secondary",
          "n_unmapped", "n_rescue_lines")


def raw_rows(ctx, runs):
    """Context.bgzf over pseudo-random bytes in a device allocation of their own"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    out, n_max = [], max(n for n, _o, _d in RAW_SHAPES)
    host = np.random.default_rng(1).integers(0, 256, n_max + 16, dtype=np.uint8)
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), n_max + 16) == 0 and hip.hipMemcpy(p, host.ctypes.data, n_max + 16, 1) == 0
    for n, off, D in RAW_SHAPES:
        ms = []
        for i in range(runs + 1):
            z = ctx.bgzf(p.value + off, n, block_data=D)
            ms.append(z.stats().ms_frame)
            if i == 0 and n <= 25_000_000:
                assert z.bytes() == S.bgzf_frame_host(host[off:off + n].tobytes(), D)
            z.close()
        out.append({"bytes": n, "source_offset": off, "block_data": D or 65280, "ms_frame": med(ms[1:]),
                    "gb_per_s": round(n / max(med(ms[1:]), 1e-6) / 1e6, 1)})
    ctx.synchronize()
    assert hip.hipFree(p) == 0
    return out


def row(pan_log2, pan_reads, runs, min_tlen, max_tlen, k, qual=False, md=False):
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
    out.update({"loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen, "k": k, "rescue_jobs": len(rs), "ref_len": ref_len})
    names = [f"pair.{p}/frag" for p in range(len(reads) // 2)]
    extras = {"qualities": phred_profile(len(reads), reads.shape[1]) if qual else None, "md": md, "reference": ref if md else None}
    out.update({"qual": qual, "md": md})
    # the views the C++ mirror's host route converts, downloaded once and written where its timer (bench_bam_host.cpp) reads them
    tmp = tempfile.mkdtemp(prefix="bench_bam_")
    t0 = time.perf_counter()
    views = {"loci": lc.view(), "ops": lc.ops, "members": lc.members, "member_scores": lc.member_scores, "reads": rd.view(),
             "pairs": pairs.view(), "rescues": rs.view()[0], "rescue_ops": rs.view()[1]}
    out["ms_input_views"] = round((time.perf_counter() - t0) * 1e3, 3)
    for name, v in views.items():
        v.tofile(os.path.join(tmp, name + ".bin"))
    both = np.empty((2 * len(reads), reads.shape[1]), dtype=np.uint8)
    both[0::2], both[1::2] = reads, COMP4[reads[:, ::-1]]
    both.tofile(os.path.join(tmp, "needles.bin"))
    exe = os.path.join(tmp, "bench_bam_host")
    lib = os.path.join(ROOT, "libspm_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "scripts", "bench_bam_host.cpp"), "-L" + lib, "-l:libspm_hip.so", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-lz"])
    for label, kw in (("plain", {}), ("cigar_m_secondary_names", {"cigar_m": True, "secondary": True, "names": names})):
        bam, sam, call, view, frame = {s: [] for s in BAM_STAGES}, {s: [] for s in SAM_STAGES}, [], [], []
        first = None
        for i in range(runs + 1):
            t0 = time.perf_counter()
            b = lc.bam_ex(rd, ps, "pan_ref", ref_len, pairs=pairs, rescues=rs, **extras, **kw)
            call.append((time.perf_counter() - t0) * 1e3)
            st = b.stats()
            for x in BAM_STAGES:
                bam[x].append(getattr(st, x))
            t0 = time.perf_counter()
            raw = b.bytes()
            view.append((time.perf_counter() - t0) * 1e3)
            assert len(raw) == st.n_file_bytes == st.header_file_bytes + st.n_record_bytes + 31 * st.n_record_blocks + 28
            first = raw if first is None else first
            assert raw == first, "two calls returned different bytes"
            counts = {c: int(getattr(st, c)) for c in COUNTS}
            b.close()
            s = lc.sam_ex(rd, ps, "pan_ref", pairs=pairs, rescues=rs, **extras, **kw)
            ss = s.stats()
            for x in SAM_STAGES:
                sam[x].append(getattr(ss, x))
            z = s.bgzf()
            frame.append(z.stats().ms_frame)
            if i == 0:
                assert gzip.decompress(z.bytes()) == s.text()
            sam_bytes = int(ss.n_bytes)
            z.close()
            s.close()
        ms_frame_text = med(frame[1:])
        bits = "".join("1" if kw.get(x) else "0" for x in ("cigar_m", "secondary", "names"))
        with open(os.path.join(tmp, f"bam_{bits}.bin"), "wb") as f:
            f.write(first)
        host_route = None
        if not qual and not md:
            r = subprocess.run([exe, tmp, str(reads.shape[1]), str(runs)] + list(bits) + [str(ref_len)], capture_output=True, text=True)
            assert r.returncode == 0, "the host route and the device disagree: " + r.stdout[-500:] + r.stderr[-500:]
            host_route = json.loads(r.stdout.strip().splitlines()[-1])
        out[label] = {"bam": {x: med(v[1:]) for x, v in bam.items()}, "sam_same_run": {x: med(v[1:]) for x, v in sam.items()},
                      "ms_call_host": med(call[1:]), "ms_first_call_host": round(call[0], 3), "ms_download_file": med(view[1:]), **counts,
                      "write_gb_per_s": round(counts["n_record_bytes"] / max(med(bam["ms_write"][1:]), 1e-6) / 1e6, 3),
                      "frame_gb_per_s": round(counts["n_record_bytes"] / max(med(bam["ms_frame"][1:]), 1e-6) / 1e6, 3),
                      "sam_text_bytes": sam_bytes, "ms_frame_sam_text": ms_frame_text,
                      "frame_sam_text_gb_per_s": round(sam_bytes / max(ms_frame_text, 1e-6) / 1e6, 3),
                      "host_route": host_route}
    shutil.rmtree(tmp, ignore_errors=True)
    for x in (rs, pairs, rd, lc, nz, pr, a, sel, h, ps, jst, ref):
        x.close()
    out["frame_raw_buffers"] = raw_rows(ctx, runs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-tlen", type=int, default=200)
    ap.add_argument("--max-tlen", type=int, default=600)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--qual", action="store_true", help="with base qualities (bench_sam.phred_profile)")
    ap.add_argument("--md", action="store_true", help="with the MD tag")
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds the row's child process may take")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", action="store_true", help=argparse.SUPPRESS)   # the child's mode: the row's JSON on stdout
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: a median of at least 5 runs")
    if a.row:
        print(json.dumps(row(a.pan_log2, a.pan_reads, a.runs, a.min_tlen, a.max_tlen, a.k, a.qual, a.md)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--row", "--pan-log2", str(a.pan_log2), "--pan-reads", str(a.pan_reads),
           "--runs", str(a.runs), "--min-tlen", str(a.min_tlen), "--max-tlen", str(a.max_tlen), "--k", str(a.k)]
    cmd += (["--qual"] if a.qual else []) + (["--md"] if a.md else [])
    r = subprocess.run(["timeout", "-k", "10", str(a.row_timeout)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(json.dumps({"failed_row": "bam", "returncode": r.returncode}))
        return 1
    res = {"metric": "BAM file: spm_hip_jst_ref_loci_bam behind pairs and rescues, the SAM call on the same inputs in the same run, the "
                     "frame kernel over the SAM text, the download of the file; medians of runs behind a warm-up, device times are "
                     "HIP events", "runs": a.runs, "bam": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
