"""Time the alignment of the SELECTED loci of a pan-genome search (spm_hip_jst_selection_align) beside the alignment of all
records (spm_hip_jst_hits_align): one JSON line.

The shapes are those of scripts/bench_jst_select.py, built by its needle builders: pan_c5 (bench.py's C5 tree and needles) and
pan_reads (the read-mapping shape of tests/test_jst_align.py).  Per shape, behind one warm-up round, --reps rounds that
alternate the two routes in one process, best round with the median in brackets:
  (i)  search(alignable) -> align() of everything;
  (ii) search -> select() -> align_selected().
Reported: records in, loci kept, segment alignments of both routes, device time by HIP events of locate + order + gather
(route (ii)) / the alignment fan-out (route (i)), of stage A and of stage B, and the host clock of each call.  The claim to
check: route (ii) is below route (i) in device time and in host clock (align calls, and whole routes), and computes no more
segment alignments.

    python scripts/bench_jst_locate.py [--c5-log2 27] [--reads-log2 22] [--reads 20000] [--reps 5] [--only pan_c5,pan_reads]
                                       [--out profiles/r04/jst_locate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import libspm_amd as S  # noqa: E402

sys.dont_write_bytecode = True  # (scripts/ holds programs, not a package: leave no cache directory beside them)
from bench_jst_select import SEED_PAT, SEED_TEXT, SEED_VAR, edit_needle, edited  # noqa: E402


def build(ctx, shape, log2_bases, n_reads):
    """tree, needle set and index of bench_jst_select.pan"""
    n_hap = 64
    ref_len = max(640000, (1 << log2_bases) // 640000 * 640000) if shape == "c5" else (1 << log2_bases) // 10_000 * 10_000
    ref = ctx.generate(SEED_TEXT, 0, ref_len)
    alleles, pool, cov = S.synth_variants(SEED_TEXT, SEED_VAR, 0, ref_len, n_hap)
    jst = S.Jst(ctx, ref, alleles, pool, cov.reshape(-1, 1), n_hap)
    mix = S.capi.lib().spm_hip_mix64
    if shape == "c5":
        L, kmax, n_pat, block = 1024, 64, 256, 1024
        needles = []
        for p in range(n_pat):
            r = mix(SEED_PAT + 7919 * p)
            h = r % n_hap
            o = (r >> 8) % (jst.haplotype_length(h) - 2 * (L + kmax))
            needles.append(edit_needle(jst.extract(h, o, L + kmax), L, p % (kmax + 1), SEED_PAT ^ (p << 20)))
    else:
        L, kmax, n_pat, block = 150, 3, n_reads, 0
        rng = np.random.default_rng(9)
        haps = [jst.extract(h, 0, jst.haplotype_length(h)) for h in range(n_hap)]
        needles = np.stack([edited(rng, haps[int(rng.integers(0, n_hap))], L, kmax) for _ in range(n_pat)])
        del haps
    ps = ctx.patterns(S.ALGO_MYERS, needles, k=kmax)
    st = jst.index(L + kmax, block)
    info = {"needles": n_pat, "needle_len": L, "k": kmax, "reference_bases": ref_len, "haplotypes": n_hap,
            "context_symbols": int(st.context_symbols)}
    return ref, jst, ps, info


def summary(rounds):
    """best round and median of every column"""
    a = np.asarray(rounds, dtype=np.float64)
    return [round(float(x), 4) for x in a.min(axis=0)], [round(float(x), 4) for x in np.median(a, axis=0)]


def pan(ctx, shape, log2_bases, n_reads, reps):
    ref, jst, ps, out = build(ctx, shape, log2_bases, n_reads)
    max_hits = 1 << 23
    cols = ["ms_device", "ms_map", "ms_stage_a", "ms_stage_b", "ms_align_call_host", "ms_worklist_host", "ms_route_host"]
    all_rounds, sel_rounds = [], []
    counts = {}
    for r in range(reps + 1):
        # (i) everything
        ctx.synchronize()
        t0 = time.perf_counter()
        h = jst.search_device(ps, max_hits=max_hits, alignable=True)
        t1 = time.perf_counter()
        a = h.align()
        t2 = time.perf_counter()
        st = a.stats()
        all_rounds.append((st.ms_total, st.ms_fanout, st.ms_begin, st.ms_cigar, (t2 - t1) * 1e3, st.ms_worklist, (t2 - t0) * 1e3))
        counts["records"] = int(st.n_alns)
        counts["segment_alns_all"] = int(st.n_segment_alns)
        counts["pool_words_all"] = int(st.n_ops)
        a.close()
        h.close()
        # (ii) the selected loci
        ctx.synchronize()
        t0 = time.perf_counter()
        h = jst.search_device(ps, max_hits=max_hits)
        s = h.select()
        t1 = time.perf_counter()
        a = s.align_selected()
        t2 = time.perf_counter()
        st = a.stats()
        ss = s.select_stats()
        sel_rounds.append((st.ms_total, st.ms_fanout, st.ms_begin, st.ms_cigar, (t2 - t1) * 1e3, st.ms_worklist, (t2 - t0) * 1e3))
        counts["loci_kept"] = int(st.n_alns)
        counts["segment_alns_selected"] = int(st.n_segment_alns)
        counts["pool_words_selected"] = int(st.n_ops)
        counts["ms_select_device"] = round(float(ss.ms_total), 4)
        assert int(ss.n_in) == counts["records"]
        a.close()
        s.close()
        h.close()
    out.update(counts)
    for name, rounds in (("align_all", all_rounds), ("align_selected", sel_rounds)):
        best, med = summary(rounds[1:])
        out[name] = {c: b for c, b in zip(cols, best)}
        out[name + "_median"] = {c: m for c, m in zip(cols, med)}
    A, B = out["align_all"], out["align_selected"]
    out["selected_below_all_device"] = bool(B["ms_device"] < A["ms_device"])
    out["selected_below_all_host_call"] = bool(B["ms_align_call_host"] < A["ms_align_call_host"])
    out["selected_below_all_host_route"] = bool(B["ms_route_host"] < A["ms_route_host"])
    out["selected_no_more_segment_alns"] = bool(out["segment_alns_selected"] <= out["segment_alns_all"])
    jst.close()
    ps.close()
    ref.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c5-log2", type=int, default=27)
    ap.add_argument("--reads-log2", type=int, default=22)
    ap.add_argument("--reads", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="pan_c5,pan_reads")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    only = set(a.only.split(","))
    ctx = S.Context(0)
    res = {"metric": "spm_hip_jst_selection_align beside spm_hip_jst_hits_align: device ms (HIP events; ms_map = locate + order + "
                     "gather / the alignment fan-out), host clock of the align call and of the whole route; best of reps, "
                     "medians beside", "reps": a.reps}
    if "pan_c5" in only:
        res["pan_c5"] = pan(ctx, "c5", a.c5_log2, 0, a.reps)
    if "pan_reads" in only:
        res["pan_reads"] = pan(ctx, "reads", a.reads_log2, a.reads, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
