"""Time the collapse of projected pan-genome alignments to one record per locus (spm_hip_jst_ref_alns_collapse) beside the
projection whose output it collapses, and beside the host route a caller needs without it: one JSON line.

The trees and needle sets are those of scripts/bench_jst_project.py (`pan_c5`: 256 needles |P| = 1024, k <= 64; `pan_reads`:
--pan-reads reads |P| = 150, k <= 3).  Per row and for both routes -- align() of an alignable search, and select() +
align_selected() -- behind one warm-up call, --runs collapse() calls: the MEDIAN device time per stage (slots, order, records,
emit: HIP events) and host clock; loci / members / slots per record and max_run; in the same run the device time of the
project() call whose output is collapsed; and the median host clock of the host route in NumPy -- download of the projected
records and pool, sort by the tuple, comparison of the transcript words, fold of the haplotypes -- whose loci, pools and map
are checked against the device's.  There is no threshold: the line says which route is faster on each shape.

Every row runs in a child process of its own under a time limit.

    python scripts/bench_jst_collapse.py [--pan-log2 27] [--pan-reads 100000] [--runs 3] [--only pan_c5,pan_reads]
                                         [--row-timeout 420] [--out profiles/r07/jst_collapse.json]
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


def host_route(pr):
    """What a caller does today: download, sort, compare, fold.  Returns (loci, ops, members, member_scores, locus_of)."""
    rv, rops = pr.view(), pr.ops                                   # the download
    n = len(rv)
    slots, slot_of = np.unique(rv["cigar_off"], return_inverse=True)
    first = np.zeros(len(slots), dtype=np.int64)
    first[slot_of[::-1]] = np.arange(n - 1, -1, -1)                # a record of every slot
    s = rv[first]
    width = int(s["cigar_len"].max())
    words = np.zeros((len(slots), width), dtype=np.int64)          # transcripts padded with 0 behind cigar_len words
    col = np.arange(width)
    mask = col[None, :] < s["cigar_len"][:, None]
    words[mask] = rops[(s["cigar_off"].astype(np.int64)[:, None] + col[None, :])[mask]]
    table = np.concatenate([np.stack([s["pattern"].astype(np.int64), s["ref_begin"].astype(np.int64), s["ref_end"].astype(np.int64),
                                      s["ref_score"].astype(np.int64), s["cigar_len"].astype(np.int64)], axis=1), words], axis=1)
    uniq, slot_locus = np.unique(table, axis=0, return_inverse=True)   # sort by the tuple, then compare the words
    slot_locus = slot_locus.reshape(-1)
    locus_of = slot_locus[slot_of].astype(np.uint32)
    order = np.lexsort((rv["score"], rv["haplotype"], locus_of))    # the fold: (locus, haplotype, score)
    lo, ho, so = locus_of[order], rv["haplotype"][order], rv["score"][order]
    head = np.ones(n, dtype=bool)
    head[1:] = (lo[1:] != lo[:-1]) | (ho[1:] != ho[:-1])
    members, member_scores = ho[head].astype(np.uint32), so[head].astype(np.int32)
    loci = np.zeros(len(uniq), dtype=S.JST_REF_LOCUS_DTYPE)
    loci["pattern"], loci["ref_begin"], loci["ref_end"], loci["ref_score"], loci["cigar_len"] = uniq[:, :5].T
    loci["n_records"] = np.bincount(locus_of, minlength=len(uniq))
    loci["n_haplotypes"] = np.bincount(lo[head], minlength=len(uniq))
    loci["cigar_off"] = np.cumsum(loci["cigar_len"], dtype=np.int64) - loci["cigar_len"]
    loci["member_off"] = np.cumsum(loci["n_haplotypes"], dtype=np.int64) - loci["n_haplotypes"]
    loci["score"] = np.minimum.reduceat(member_scores, loci["member_off"].astype(np.int64))
    ops = uniq[:, 5:][np.arange(width)[None, :] < uniq[:, 4][:, None]].astype(np.uint32)
    return loci, ops, members, member_scores, locus_of


def measure(ctx, make, runs):
    a, closers = make()
    pr = a.project()
    ps = pr.stats()
    out = {"project": {"ms_device": round(ps.ms_total, 4), "ms_call_host": round(ps.ms_host, 3), "records": int(ps.n_alns),
                       "slots": int(ps.n_projected), "pool_words": int(ps.n_ops)}}
    if ps.n_alns == 0:
        out["empty"] = True
        return out
    stats, host = [], []
    lc = None
    for r in range(runs + 1):
        if lc is not None:
            lc.close()
        ctx.synchronize()
        t0 = time.perf_counter()
        lc = pr.collapse()
        ctx.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        stats.append(lc.stats())
    med = lambda f: round(float(np.median([getattr(s, f) for s in stats[1:]])), 4)
    st = stats[-1]
    out["collapse"] = {"ms_device": med("ms_total"), "ms_slots": med("ms_slots"), "ms_order": med("ms_order"),
                       "ms_records": med("ms_records"), "ms_emit": med("ms_emit"),
                       "ms_call_host": round(float(np.median(host[1:])), 3), "ms_first_call_host": round(host[0], 3),
                       "records": int(st.n_alns), "slots": int(st.n_slots), "loci": int(st.n_loci), "members": int(st.n_members),
                       "pool_words": int(st.n_ops), "multi_slot_loci": int(st.n_multi_slot), "max_run": int(st.max_run),
                       "loci_per_record": round(st.n_loci / st.n_alns, 5)}
    t_host = []
    for _r in range(runs):
        t0 = time.perf_counter()
        got = host_route(pr)
        t_host.append((time.perf_counter() - t0) * 1e3)
    want = (lc.view(), lc.ops, lc.members, lc.member_scores, lc.locus_of)
    equal = all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
    out["numpy_host_route"] = {"ms_median": round(float(np.median(t_host)), 2), "equal_to_device": bool(equal)}
    out["collapse_call_below_host_route"] = bool(np.median(host[1:]) < np.median(t_host))
    assert equal, "the host route and the device disagree"
    for x in [lc, pr, a] + closers:
        x.close()
    return out


def row(shape, log2_bases, n_reads, runs):
    ctx = S.Context(0)
    ref, jst, ps, _needles, _tables, max_hits, out = build(ctx, shape, log2_bases, n_reads)

    def all_records():
        h = jst.search_device(ps, max_hits=max_hits, alignable=True)
        return h.align(), [h]

    def selected():
        h = jst.search_device(ps, max_hits=max_hits)
        s = h.select()
        return s.align_selected(), [s, h]

    out["align_all"] = measure(ctx, all_records, runs)
    out["align_selected"] = measure(ctx, selected, runs)
    for x in (jst, ps, ref):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="pan_c5,pan_reads")
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds one row's child process may take")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", default=None, help=argparse.SUPPRESS)   # the child's mode: one row, its JSON on stdout
    a = ap.parse_args()
    if a.row:
        print(json.dumps(row("c5" if a.row == "pan_c5" else "reads", a.pan_log2, a.pan_reads, a.runs)))
        return 0
    res = {"metric": "spm_hip_jst_ref_alns_collapse: median device ms per stage (HIP events) and host clock of runs behind a "
                     "warm-up, beside the project call whose output it collapses and the NumPy host route (download, sort, "
                     "compare, fold)", "runs": a.runs}
    for name in ("pan_c5", "pan_reads"):
        if name not in a.only.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--pan-log2", str(a.pan_log2), "--pan-reads",
               str(a.pan_reads), "--runs", str(a.runs)]
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
