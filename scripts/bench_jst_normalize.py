"""Time the left-normalisation of projected pan-genome alignments (spm_hip_jst_ref_alns_normalize) beside the projection whose
output it reads, and beside the host route a caller needs without it: one JSON line.

The trees and needle sets are those of scripts/bench_jst_project.py and scripts/bench_jst_collapse.py (`pan_c5`: 256 needles
|P| = 1024, k <= 64; `pan_reads`: --pan-reads reads |P| = 150, k <= 3).  Per row and for both routes -- align() of an alignable
search, and select() + align_selected() -- behind one warm-up call, --runs normalize() calls: the MEDIAN device time per stage
(slots, normalise, offsets, gather, compact: HIP events) and host clock; slots, words in and out, changed slots, steps, joins
and pinned runs; the loci of collapse() with and without normalisation; in the same run the device time of the project() call
whose output is normalised; and the host clock of the host route: download of the projected records and pool, the rule in
column form in NumPy / Python on a fixed sample of --sample records (checked against the device's words), scaled to all
records.  There is no threshold: the line says which route is faster on each shape.

Every row runs in a child process of its own under a time limit.

    python scripts/bench_jst_normalize.py [--pan-log2 27] [--pan-reads 100000] [--runs 3] [--sample 10000]
                                          [--only pan_c5,pan_reads] [--row-timeout 420] [--out profiles/r10/jst_normalize.jsonl]
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
from bench_jst_project import build  # noqa: E402

INS, DEL, EQ = 1, 2, 7


def host_walk(P, ref, ref_begin, words):
    """The rule of the header on one transcript, one op per column; i and r follow the run as it moves."""
    col = np.repeat(words & 15, words >> 4).tolist()
    n = len(col)
    i, r = 0, ref_begin                                             # consumed by the columns before `at`
    at = 0
    while at < n:
        op = col[at]
        if op != INS and op != DEL:
            i += 1
            r += 1
            at += 1
            continue
        c, L = at, 0
        while c + L < n and col[c + L] == op:
            L += 1
        ci, cr = i, r
        while c >= 2 and col[c - 1] == EQ and (P[ci - 1] == P[ci + L - 1] if op == INS else ref[cr - 1] == ref[cr + L - 1]):
            col[c - 1], col[c - 1 + L] = op, EQ
            c -= 1
            ci -= 1
            cr -= 1
            while c >= 1 and col[c - 1] == op:                      # a run of the same op on the left: one run from now on
                c -= 1
                L += 1
                if op == INS:
                    ci -= 1
                else:
                    cr -= 1
        i, r = (ci + L, cr) if op == INS else (ci, cr + L)
        at = c + L
        # the = columns the run passed lie behind it now: they are counted as they are walked over
    col = np.array(col, dtype=np.uint32)
    cut = np.concatenate([[0], np.nonzero(np.diff(col))[0] + 1, [n]])
    return ((np.diff(cut).astype(np.uint32) << 4) | col[cut[:-1]]).astype(np.uint32)


def measure(ctx, make, runs, ref_host, needles, sample):
    a, closers = make()
    pr = a.project()
    ps = pr.stats()
    out = {"project": {"ms_device": round(ps.ms_total, 4), "ms_call_host": round(ps.ms_host, 3), "records": int(ps.n_alns),
                       "slots": int(ps.n_projected), "pool_words": int(ps.n_ops)}}
    if ps.n_alns == 0:
        out["empty"] = True
        return out
    stats, host = [], []
    nz = None
    for _r in range(runs + 1):
        if nz is not None:
            nz.close()
        ctx.synchronize()
        t0 = time.perf_counter()
        nz = pr.normalize()
        ctx.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        stats.append(nz.normalize_stats())
    med = lambda f: round(float(np.median([getattr(s, f) for s in stats[1:]])), 4)
    st = stats[-1]
    out["normalize"] = {"ms_device": med("ms_total"), "ms_slots": med("ms_slots"), "ms_normalize": med("ms_normalize"),
                        "ms_offsets": med("ms_offsets"), "ms_gather": med("ms_gather"), "ms_compact": med("ms_compact"),
                        "ms_call_host": round(float(np.median(host[1:])), 3), "ms_first_call_host": round(host[0], 3),
                        "records": int(st.n_alns), "slots": int(st.n_slots), "words_in": int(st.n_ops_in),
                        "words_out": int(st.n_ops), "changed_slots": int(st.n_changed), "steps": int(st.n_steps),
                        "joined": int(st.n_joined), "pinned": int(st.n_pinned)}
    plain, merged = pr.collapse(), nz.collapse()
    out["loci"] = {"plain": len(plain), "normalized": len(merged)}
    plain.close()
    merged.close()
    # the host route: the download, then the walk on a fixed sample, scaled
    t0 = time.perf_counter()
    rv, rops = pr.view(), pr.ops
    t_download = (time.perf_counter() - t0) * 1e3
    gv, gops = nz.view(), nz.ops
    pick = np.sort(np.random.default_rng(10).choice(len(rv), size=min(sample, len(rv)), replace=False))
    equal = True
    t0 = time.perf_counter()
    got = []
    for j in pick.tolist():
        s = rv[j]
        o = int(s["cigar_off"])
        got.append(host_walk(needles[int(s["pattern"])], ref_host, int(s["ref_begin"]), rops[o:o + int(s["cigar_len"])]))
    t_walk = (time.perf_counter() - t0) * 1e3
    for j, w in zip(pick.tolist(), got):
        g = gv[j]
        equal = equal and w.tobytes() == gops[int(g["cigar_off"]):int(g["cigar_off"]) + int(g["cigar_len"])].tobytes()
    scaled = t_download + t_walk * len(rv) / len(pick)
    out["numpy_host_route"] = {"ms_download": round(t_download, 2), "sample": int(len(pick)), "ms_walk_sample": round(t_walk, 2),
                               "ms_scaled_to_all_records": round(scaled, 2), "equal_to_device": bool(equal)}
    out["normalize_call_below_host_route"] = bool(np.median(host[1:]) < scaled)
    out["normalize_device_below_project_device"] = bool(med("ms_total") < ps.ms_total)
    assert equal, "the host route and the device disagree"
    for x in [nz, pr, a] + closers:
        x.close()
    return out


def row(shape, log2_bases, n_reads, runs, sample):
    ctx = S.Context(0)
    ref, jst, ps, needles, _tables, max_hits, out = build(ctx, shape, log2_bases, n_reads)
    ref_host = ref.download(0, len(ref))

    def all_records():
        h = jst.search_device(ps, max_hits=max_hits, alignable=True)
        return h.align(), [h]

    def selected():
        h = jst.search_device(ps, max_hits=max_hits)
        s = h.select()
        return s.align_selected(), [s, h]

    out["align_all"] = measure(ctx, all_records, runs, ref_host, needles, sample)
    out["align_selected"] = measure(ctx, selected, runs, ref_host, needles, sample)
    for x in (jst, ps, ref):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sample", type=int, default=10_000)
    ap.add_argument("--only", default="pan_c5,pan_reads")
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds one row's child process may take")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", default=None, help=argparse.SUPPRESS)   # the child's mode: one row, its JSON on stdout
    a = ap.parse_args()
    if a.row:
        print(json.dumps(row("c5" if a.row == "pan_c5" else "reads", a.pan_log2, a.pan_reads, a.runs, a.sample)))
        return 0
    res = {"metric": "spm_hip_jst_ref_alns_normalize: median device ms per stage (HIP events) and host clock of runs behind a "
                     "warm-up, beside the project call whose output it normalises and the NumPy host route (download, the "
                     "column-form walk on a sample, scaled)", "runs": a.runs}
    for name in ("pan_c5", "pan_reads"):
        if name not in a.only.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--pan-log2", str(a.pan_log2), "--pan-reads",
               str(a.pan_reads), "--runs", str(a.runs), "--sample", str(a.sample)]
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
