"""Time the SAM writer on the device: one JSON line.

The tree, the pairs and the rescues are those of scripts/bench_rescue.py (the `pan_reads` tree, fragments of 300 .. 500
symbols, mates of 150 symbols with up to 3 edits, in one pair in 16 a mate with 8 substitutions more).  The chain is search ->
select(best=1, across, strands) -> align_selected -> project -> normalize -> collapse -> reads -> pairs -> rescue; timed are
JstRefLoci.sam() -- the device time of each of its four stages (HIP events) and the host clock of the call -- the download
of the two views (text and line records), each call followed by its download, so that the two alternate, and the C++
mirror's host route on the same inputs: journaled_sequence_tree::sam_host over the downloaded loci, reads, pairs and rescues
(scripts/bench_sam_host.cpp, compiled here; its text must equal the device's).  Every figure is the
MEDIAN of --runs calls behind one warm-up call, per flag combination.  Nothing is asserted but that two calls return the same
bytes and that the text has one line feed per line record.  The row runs in a child process of its own under a time limit.
With --qual and / or --md the call is spm_hip_jst_ref_loci_sam_ex with the qualities of phred_profile below and / or the MD tag;
the host route's timer knows neither, so its figure is left out then.

    python scripts/bench_sam.py [--pan-log2 27] [--pan-reads 100000] [--runs 5] [--min-tlen 200] [--max-tlen 600] [--k 12]
                                [--qual] [--md] [--row-timeout 420] [--out profiles/r14/sam.jsonl]
"""
import argparse
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

STAGES = ("ms_total", "ms_lines", "ms_measure", "ms_write", "ms_stats")
COUNTS = ("n_lines", "n_bytes", "n_reported", "n_secondary", "n_unmapped", "n_rescue_lines")


def phred_profile(n_reads, m, seed=0x51A1):
    """Base qualities for n_reads reads of m symbols, (n_reads, m) uint8: what a short-read instrument's look like.  Position i
    of a read has the mean 37 - 9 (i / m)^2 -- high at the start, sagging towards the end -- with normal noise of 3 around it,
    rounded and held to 2 .. 41; one read in ten loses its tail: from a point in its second half on, every value is 2."""
    rng = np.random.default_rng(seed)
    mean = 37.0 - 9.0 * (np.arange(m) / m) ** 2
    q = np.clip(np.rint(mean[None, :] + rng.normal(0.0, 3.0, (n_reads, m))), 2, 41).astype(np.uint8)
    cut = rng.integers(m // 2, m, n_reads)
    bad = rng.random(n_reads) < 0.1
    q[bad[:, None] & (np.arange(m)[None, :] >= cut[:, None])] = 2
    return q


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
    out.update({"loci": len(lc), "min_tlen": min_tlen, "max_tlen": max_tlen, "k": k, "rescue_jobs": len(rs)})
    names = [f"pair.{p}/frag" for p in range(len(reads) // 2)]
    extras = {"qualities": phred_profile(len(reads), reads.shape[1]) if qual else None, "md": md, "reference": ref if md else None}
    out.update({"qual": qual, "md": md})
    # the views the C++ mirror's host route formats, downloaded once and written where its timer (bench_sam_host.cpp) reads them
    tmp = tempfile.mkdtemp(prefix="bench_sam_")
    t0 = time.perf_counter()
    views = {"loci": lc.view(), "ops": lc.ops, "members": lc.members, "member_scores": lc.member_scores, "reads": rd.view(),
             "pairs": pairs.view(), "rescues": rs.view()[0], "rescue_ops": rs.view()[1]}
    out["ms_input_views"] = round((time.perf_counter() - t0) * 1e3, 3)
    for name, v in views.items():
        v.tofile(os.path.join(tmp, name + ".bin"))
    both = np.empty((2 * len(reads), reads.shape[1]), dtype=np.uint8)
    both[0::2], both[1::2] = reads, COMP4[reads[:, ::-1]]
    both.tofile(os.path.join(tmp, "needles.bin"))
    exe = os.path.join(tmp, "bench_sam_host")
    lib = os.path.join(ROOT, "libspm_amd")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "scripts", "bench_sam_host.cpp"), "-L" + lib, "-l:libspm_hip.so", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-lz"])
    for label, kw in (("plain", {}), ("cigar_m_secondary_names", {"cigar_m": True, "secondary": True, "names": names})):
        dev, call, view = {s: [] for s in STAGES}, [], []
        first = None
        for _ in range(runs + 1):
            t0 = time.perf_counter()
            s = lc.sam_ex(rd, ps, "pan_ref", pairs=pairs, rescues=rs, **extras, **kw)
            call.append((time.perf_counter() - t0) * 1e3)
            st = s.stats()
            for x in STAGES:
                dev[x].append(getattr(st, x))
            t0 = time.perf_counter()
            text, lines = s.text(), s.lines()
            view.append((time.perf_counter() - t0) * 1e3)
            assert text.count(b"\n") == len(lines) == st.n_lines and len(text) == st.n_bytes
            first = text if first is None else first
            assert text == first, "two calls returned different bytes"
            counts = {c: int(getattr(st, c)) for c in COUNTS}
            s.close()
        bits = "".join("1" if kw.get(x) else "0" for x in ("cigar_m", "secondary", "names"))
        with open(os.path.join(tmp, f"text_{bits}.bin"), "wb") as f:
            f.write(first)
        host_route = None
        if not qual and not md:
            r = subprocess.run([exe, tmp, str(reads.shape[1]), str(runs)] + list(bits), capture_output=True, text=True)
            assert r.returncode == 0, "the host route and the device disagree: " + r.stdout[-500:] + r.stderr[-500:]
            host_route = json.loads(r.stdout.strip().splitlines()[-1])
        out[label] = {**{x: med(v[1:]) for x, v in dev.items()}, "ms_call_host": med(call[1:]), "ms_first_call_host": round(call[0], 3),
                      "ms_views": med(view[1:]), **counts,
                      "write_gb_per_s": round(counts["n_bytes"] / max(med(dev["ms_write"][1:]), 1e-6) / 1e6, 3),
                      "host_route": host_route}
    shutil.rmtree(tmp, ignore_errors=True)
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
    ap.add_argument("--qual", action="store_true", help="with base qualities (phred_profile)")
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
        print(json.dumps({"failed_row": "sam", "returncode": r.returncode}))
        return 1
    res = {"metric": "SAM lines: spm_hip_jst_ref_loci_sam behind pairs and rescues, and the download of its two views; medians of "
                     "runs behind a warm-up, device times are HIP events", "runs": a.runs,
           "sam": json.loads(r.stdout.strip().splitlines()[-1])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
