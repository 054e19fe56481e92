"""What base qualities and the MD tag cost the SAM and the BAM writer, and what they do to the file: JSON lines.

The inputs and the chain are those of scripts/bench_sam.py (the `pan_reads` tree, pairs and rescues); the qualities are
bench_sam.phred_profile's.  One child process per row, under a time limit, rows of two kinds in alternating order:

  this tree    spm_hip_jst_ref_loci_sam_ex / _bam_ex with neither field (extras NULL), with qualities, with MD, with both: the
               device time of the measure and the write stage (HIP events) and the bytes written; and per combination the size
               of the stored BAM file and of the deflated one (spm_hip_bam_deflate) -- "neither" is the ff fill;
  parent       with --parent-lib, a libspm_hip.so built from the parent commit: spm_hip_jst_ref_loci_sam / _bam, the same stages.

Both kinds make the old calls through the same Python statements (old_call below), so "this tree, old call" against "parent" is
the cost of the feature to callers that do not use it.  Every figure is the MEDIAN of --runs calls behind one warm-up call.
Nothing is asserted but that two calls return the same counts.

    python scripts/bench_sam_qual_md.py [--parent-lib PATH] [--pairs-of-rows 3] [--pan-log2 27] [--pan-reads 100000] [--runs 5]
                                        [--row-timeout 420] [--out profiles/r20/sam_qual_md.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import libspm_amd as S  # noqa: E402

sys.dont_write_bytecode = True  # (scripts/ holds programs, not a package: leave no cache directory beside them)

NEW_EXPORTS = ("spm_hip_jst_ref_loci_sam_ex", "spm_hip_jst_ref_loci_bam_ex", "spm_hip_sam_md")
FLAGS = (("plain", {}), ("cigar_m_secondary", {"cigar_m": True, "secondary": True}))
FIELDS = (("neither", False, False), ("qual", True, False), ("md", False, True), ("both", True, True))


def old_call(kind, lc, rd, ps, pairs, rs, ref_len, cigar_m=False, secondary=False):
    """spm_hip_jst_ref_loci_sam / _bam as the parent's binding makes them: the calls a library of either tree exports"""
    opts = S.sam_opts("pan_ref", cigar_m=cigar_m, secondary=secondary)
    if kind == "sam":
        return S.Sam(lc.ctx, lc._new("sam", rd._h, pairs._h, rs._h, ps._h, C.byref(opts)), "pan_ref")
    bopts = S.capi.BamOpts(sam=opts, ref_len=int(ref_len), block_data=0, reserved=0)
    return S.Bam(lc.ctx, lc._new("bam", rd._h, pairs._h, rs._h, ps._h, C.byref(bopts)), S.capi.BGZF_BLOCK_DATA)


def row(lib, pan_log2, pan_reads, runs):
    if lib:                                                        # the parent's library knows nothing of the new calls
        S.capi.SO_PATH = os.path.abspath(lib)
        for name in NEW_EXPORTS:
            S.capi.SIGNATURES.pop(name)
    from bench_pairs import med
    from bench_rescue import build
    from bench_sam import phred_profile
    ctx = S.Context(0)
    ref, jst, ps, reads, out = build(ctx, pan_log2, pan_reads)
    h = jst.search_device(ps, max_hits=1 << 26)
    sel = h.select(best=1, across=True, strands=True)
    a = sel.align_selected()
    pr = a.project()
    nz = pr.normalize()
    lc = nz.collapse()
    rd = lc.reads(len(reads), 2)
    pairs = lc.pairs(rd, 200, 600)
    rs = pairs.rescue(lc, rd, ref, ps, 12, 200, 600)
    ref_len = len(ref)
    out.update({"tree": "parent" if lib else "this", "loci": len(lc), "rescue_jobs": len(rs)})
    quals = phred_profile(len(reads), reads.shape[1])

    def timed(make, size_of, sizes=False):
        ms, first, extra = {"ms_measure": [], "ms_write": []}, None, {}
        for i in range(runs + 1):
            x = make()
            st = x.stats()
            for k in ms:
                ms[k].append(getattr(st, k))
            n = size_of(st)
            first = n if first is None else first
            assert n == first, "two calls wrote different numbers of bytes"
            if sizes and i == 0:                                   # the file: stored, and deflated
                z = x.deflate()
                extra = {"stored_file_bytes": int(st.n_file_bytes), "deflated_file_bytes": int(z.device()[1])}
                z.close()
            x.close()
        return {**{k: med(v[1:]) for k, v in ms.items()}, "bytes": int(first), **extra}

    for label, kw in FLAGS:
        res = {"sam_old_call": timed(lambda: old_call("sam", lc, rd, ps, pairs, rs, ref_len, **kw), lambda st: st.n_bytes),
               "bam_old_call": timed(lambda: old_call("bam", lc, rd, ps, pairs, rs, ref_len, **kw), lambda st: st.n_record_bytes)}
        for name, with_q, with_md in (() if lib else FIELDS):
            ex = dict(qualities=quals if with_q else None, md=with_md, reference=ref if with_md else None, pairs=pairs, rescues=rs, **kw)
            res["sam_" + name] = timed(lambda: lc.sam_ex(rd, ps, "pan_ref", **ex), lambda st: st.n_bytes)
            res["bam_" + name] = timed(lambda: lc.bam_ex(rd, ps, "pan_ref", ref_len, **ex), lambda st: st.n_record_bytes, sizes=True)
        out[label] = res
    for x in (rs, pairs, rd, lc, nz, pr, a, sel, h, ps, jst, ref):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a libspm_hip.so built from the parent commit: rows of it alternate with this tree's")
    ap.add_argument("--pairs-of-rows", type=int, default=3, help="how often the two kinds of row alternate")
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds a row's child process may take")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--row", action="store_true", help=argparse.SUPPRESS)   # the child's mode: the row's JSON on stdout
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: a median of at least 5 runs")
    if a.row:
        print(json.dumps(row(a.lib, a.pan_log2, a.pan_reads, a.runs)))
        return 0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    order = []
    for i in range(a.pairs_of_rows):                               # parent first, then this tree first, ...
        order += ([a.parent_lib, ""] if i % 2 == 0 else ["", a.parent_lib]) if a.parent_lib else [""]
    for n, lib in enumerate(order):
        cmd = [sys.executable, os.path.abspath(__file__), "--row", "--lib", lib, "--pan-log2", str(a.pan_log2), "--pan-reads",
               str(a.pan_reads), "--runs", str(a.runs)]
        r = subprocess.run(["timeout", "-k", "10", str(a.row_timeout)] + cmd, capture_output=True, text=True)
        if r.returncode != 0:                                      # (nothing more is started on the device behind a row that failed)
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_row": n, "returncode": r.returncode}))
            return 1
        line = json.dumps({"metric": "SAM and BAM writers with and without base qualities and MD: medians of runs behind a warm-up, device "
                                     "times are HIP events", "runs": a.runs, "row": n, "result": json.loads(r.stdout.strip().splitlines()[-1])})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
