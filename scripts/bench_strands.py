"""Time what searching reads on both strands costs: one JSON line.

  * sets     patterns_create and one scan step of a STRANDED set of n reads beside a PLAIN set of the same n reads, for the C3
             shape (1024 reads |P| = 100, k <= 3) and the reads100 shape (100 000 reads |P| = 100, k <= 3) over --text-log2
             bases of synthetic dna4 text (bench.py's seeds and needles): host clock of the create call, build_stats (passes,
             dense, keys), device time of the scan.  Every odd read is reverse-complemented, so both strands have hits.
  * select   device time of select(best=0) with and without SPM_SELECT_STRANDS on the same records (the reads100 scan).
  * reads    device time of JstRefLoci.reads() beside the summary in NumPy on the same loci: the `pan_reads` tree of
             scripts/bench_jst_project.py, its reads compiled on both strands, best stratum per read across haplotypes.
Every figure is the MEDIAN of --runs calls behind one warm-up call; device times are HIP events.  Nothing is asserted but
that the NumPy summary equals the device's.  Every row runs in a child process of its own under a time limit.

    python scripts/bench_strands.py [--text-log2 30] [--pan-log2 27] [--pan-reads 100000] [--runs 5]
                                    [--only sets,select,reads] [--row-timeout 420] [--out profiles/r11/strands.jsonl]
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

SEED_TEXT, SEED_PAT = 0x5EED0001, 0x5EED0002
COMP4 = np.array([3, 2, 1, 0], dtype=np.uint8)


def med(xs):
    return round(float(np.median(xs)), 4)


def reads_of(n_text, n, L, k):
    """n reads of the benchmark's generator, every odd one reverse-complemented"""
    r = np.stack([S.synth_pattern(SEED_TEXT, SEED_PAT, n_text, p, L, k)[0] for p in range(n)])
    r[1::2] = COMP4[r[1::2, ::-1]]
    return r


def set_and_scan(ctx, text, reads, k, both, runs, max_hits):
    create, scan_ms = [], []
    ps = None
    for _ in range(runs + 1):
        if ps is not None:
            ps.close()
        t0 = time.perf_counter()
        ps = ctx.patterns(S.ALGO_MYERS, reads, k=k, both_strands=both)
        create.append((time.perf_counter() - t0) * 1e3)
    b = ps.build_stats()
    n_hits = 0
    for _ in range(runs + 1):
        h = S.scan(ctx, text, ps, max_hits=max_hits)
        st = h.stats()
        scan_ms.append(st.ms_total)
        n_hits, engine = int(st.n_hits), int(st.engine_used)
        h.close()
    out = {"needles": len(ps), "ms_create_host": med(create[1:]), "ms_tables": round(b.ms_tables, 3), "ms_index": round(b.ms_index, 3),
           "ms_upload": round(b.ms_upload, 3), "passes": int(b.passes), "dense": int(b.dense), "keys": int(b.keys),
           "filterable": bool(ps.filterable), "engine_used": engine, "ms_scan_device": med(scan_ms[1:]), "hits": n_hits}
    return ps, out


def row_sets(text_log2, runs):
    ctx = S.Context(0)
    n_text = 1 << text_log2
    text = ctx.generate(SEED_TEXT, 0, n_text)
    out = {"text_bases": n_text}
    for name, n in (("c3", 1024), ("reads100", 100_000)):
        reads = reads_of(n_text, n, 100, 3)
        row = {"reads": n, "read_len": 100, "k": 3}
        for both in (False, True):
            ps, row["stranded" if both else "plain"] = set_and_scan(ctx, text, reads, 3, both, runs, 1 << 24)
            ps.close()
        p, s = row["plain"], row["stranded"]
        row["stranded_over_plain"] = {"ms_create_host": round(s["ms_create_host"] / max(p["ms_create_host"], 1e-9), 3),
                                      "ms_scan_device": round(s["ms_scan_device"] / max(p["ms_scan_device"], 1e-9), 3),
                                      "keys": round(s["keys"] / max(p["keys"], 1), 3)}
        row["stranded_loses_filter"] = bool(p["filterable"] and not s["filterable"])
        row["stranded_loses_dense_pass"] = bool(p["dense"] and not s["dense"])
        out[name] = row
    text.close()
    return out


def row_select(text_log2, runs):
    ctx = S.Context(0)
    n_text = 1 << text_log2
    text = ctx.generate(SEED_TEXT, 0, n_text)
    reads = reads_of(n_text, 100_000, 100, 3)
    ps = ctx.patterns(S.ALGO_MYERS, reads, k=3, both_strands=True)
    h = S.scan(ctx, text, ps, max_hits=1 << 24)
    out = {"text_bases": n_text, "reads": 100_000, "records": int(h.stats().n_hits)}
    for strands in (False, True):
        dev, kept = [], 0
        for _ in range(runs + 1):
            s = h.select(best=0, strands=strands)
            st = s.select_stats()
            dev.append((st.ms_total, st.ms_order, st.ms_select))
            kept = int(st.n_out)
            s.close()
        out["strands" if strands else "plain"] = {"ms_device": med([d[0] for d in dev[1:]]), "ms_order": med([d[1] for d in dev[1:]]),
                                                  "ms_select": med([d[2] for d in dev[1:]]), "n_out": kept}
    for x in (h, ps, text):
        x.close()
    return out


def numpy_reads(loci, n_reads, strands):
    """the summary of spm_hip_jst_ref_loci_reads, vectorised: the loci are in pattern order"""
    out = np.zeros(n_reads, dtype=S.JST_READ_DTYPE)
    read = (loci["pattern"] // strands).astype(np.int64)
    out["first_locus"] = np.searchsorted(read, np.arange(n_reads), side="left")
    out["n_loci"] = np.bincount(read, minlength=n_reads)
    out["n_forward"] = np.bincount(read[loci["pattern"] % strands == 0], minlength=n_reads)
    key = (loci["score"].astype(np.uint64) << np.uint64(32)) | np.arange(len(loci), dtype=np.uint64)
    best = np.full(n_reads, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(best, read, key)
    mapped = out["n_loci"] > 0
    primary = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out["primary"] = np.where(mapped, primary, 0xFFFFFFFF)
    out["best"] = np.where(mapped, (best >> np.uint64(32)).astype(np.int64), -1)
    out["best_ref_score"] = np.where(mapped, loci["ref_score"][np.where(mapped, primary, 0)] if len(loci) else -1, -1)
    d = loci["score"].astype(np.int64) - out["best"][read]
    out["n_best"] = np.bincount(read[d == 0], minlength=n_reads)
    out["n_next"] = np.bincount(read[d == 1], minlength=n_reads)
    return out


def row_reads(pan_log2, pan_reads, runs):
    from bench_jst_project import build
    ctx = S.Context(0)
    ref, jst, plain, needles, _tables, max_hits, out = build(ctx, "reads", pan_log2, pan_reads)
    plain.close()
    reads = needles.copy()
    reads[1::2] = COMP4[reads[1::2, ::-1]]
    ps = ctx.patterns(S.ALGO_MYERS, reads, k=out["k"], both_strands=True)
    h = jst.search_device(ps, max_hits=max_hits)
    sel = h.select(best=0, across=True, strands=True)
    a = sel.align_selected()
    pr = a.project()
    nz = pr.normalize()
    lc = nz.collapse()
    out.update({"records": len(h), "selected": len(sel), "loci": len(lc)})
    dev, host = [], []
    rd = None
    for _ in range(runs + 1):
        if rd is not None:
            rd.close()
        t0 = time.perf_counter()
        rd = lc.reads(len(reads), 2)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(rd.stats().ms_total)
    st = rd.stats()
    t0 = time.perf_counter()
    loci = lc.view()
    t_view = (time.perf_counter() - t0) * 1e3
    t_np = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        want = numpy_reads(loci, len(reads), 2)
        t_np.append((time.perf_counter() - t0) * 1e3)
    equal = rd.view().tobytes() == want.tobytes()
    out["reads"] = {"ms_device": med(dev[1:]), "ms_call_host": med(host[1:]), "ms_first_call_host": round(host[0], 3),
                    "n_reads": int(st.n_reads), "n_mapped": int(st.n_mapped), "n_unique": int(st.n_unique), "n_multi": int(st.n_multi)}
    out["numpy_host_route"] = {"ms_loci_view": round(t_view, 3), "ms_summary": med(t_np[1:]), "equal_to_device": bool(equal)}
    assert equal, "the NumPy summary and the device disagree"
    for x in (rd, lc, nz, pr, a, sel, h, ps, jst, ref):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=30)
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default="sets,select,reads")
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds one row's child process may take")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", default=None, help=argparse.SUPPRESS)   # the child's mode: one row, its JSON on stdout
    a = ap.parse_args()
    if a.row:
        r = {"sets": lambda: row_sets(a.text_log2, a.runs), "select": lambda: row_select(a.text_log2, a.runs),
             "reads": lambda: row_reads(a.pan_log2, a.pan_reads, a.runs)}[a.row]()
        print(json.dumps(r))
        return 0
    res = {"metric": "reads on both strands: a stranded needle set beside the plain set of the same reads (create, scan), "
                     "select with and without SPM_SELECT_STRANDS, spm_hip_jst_ref_loci_reads beside NumPy; medians of runs "
                     "behind a warm-up, device times are HIP events", "runs": a.runs}
    for name in ("sets", "select", "reads"):
        if name not in a.only.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--text-log2", str(a.text_log2), "--pan-log2",
               str(a.pan_log2), "--pan-reads", str(a.pan_reads), "--runs", str(a.runs)]
        r = subprocess.run(["timeout", "-k", "10", str(a.row_timeout)] + cmd, capture_output=True, text=True)
        if r.returncode != 0:               # a row that failed or ran out of time ends the run: nothing more is started
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_row": name, "returncode": r.returncode}))
            return 1
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
