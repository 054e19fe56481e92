"""Time spm_hip_hits_align on the hit sets of the C4 and C5 shapes, and spm_hip_jst_hits_align on two pan-genome
trees: one JSON line.

C4: 100 000 needles |P| = 150, k <= 3 over --c4-gib of synthetic dna4 text (bench.py's seeds and needles).
C5: 256 needles |P| = 1024, k <= 64 over --c5-gib of plain synthetic text (the shape of config C5's needles; the
plain-text counterpart of the pan-genome row below).
Per set: the scan, then --reps align calls with and without SPM_ALIGN_BEGIN_ONLY; the device times of each stage
(best of the calls), the host wall clock of the call, and how the hits were split over the kernel classes.

Pan-genome rows (--pan-log2 bases of reference x 64 haplotypes, bench.py's C5 tree): `pan_c5` 256 needles |P| = 1024,
k <= 64 (bench.py's needles) and `pan_reads` --pan-reads reads |P| = 150, k <= 3 cut from the haplotypes with up to k
edits.  Per row: the alignable search, then --reps JstHits.align() calls behind a warm-up, full and BEGIN_ONLY: the
best call's device times (stage A, stage B, fan-out: HIP events), its host work-list time and the host clock around
the synchronised call; records, segment alignments, pool words.  Beside it the route without the tree for
--pan-route-haplotypes haplotypes (extract + upload + scan + align, each timed on the host clock), and that sum
scaled to 64 haplotypes -- labelled as scaled, it is not a measurement of 64.

    python scripts/bench_align.py [--c4-gib 8] [--c5-gib 0.125] [--reps 5] [--pan-log2 27] [--pan-reads 100000]
                                  [--only c4,c5,pan_c5,pan_reads]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libspm_amd as S  # noqa: E402

SEED_TEXT, SEED_PAT, SEED_VAR = 0x5EED0001, 0x5EED0002, 0x5EED0003


def one(ctx, name, L, kmax, n_pat, gib, reps):
    n = int(gib * 2**30) & ~1023
    text = ctx.generate(SEED_TEXT, 0, n)
    needles = np.stack([S.synth_pattern(SEED_TEXT, SEED_PAT, n, p, L, kmax)[0] for p in range(n_pat)])
    ps = ctx.patterns(S.ALGO_MYERS, needles, k=kmax)
    h = S.scan(ctx, text, ps, max_hits=1 << 23)
    scan = h.stats()
    out = {"needles": n_pat, "needle_len": L, "k": kmax, "text_bytes": n, "hits": int(scan.n_hits),
           "scan_ms": round(scan.ms_total, 3)}
    for label, begin_only in (("full", False), ("begin_only", True)):
        best, host = None, []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            a = h.align(begin_only=begin_only)
            host.append((time.perf_counter() - t0) * 1e3)
            st = a.stats()
            a.close()
            if r == 0:
                continue  # (the first call builds the set's alignment tables)
            if best is None or st.ms_total < best.ms_total:
                best = st
        out[label] = {"ms_device": round(best.ms_total, 4), "ms_begin": round(best.ms_begin, 4),
                      "ms_cigar": round(best.ms_cigar, 4), "ms_call_host": round(float(np.median(host[1:])), 3),
                      "ms_first_call_host": round(host[0], 3), "ops": int(best.n_ops),
                      "begin_lane": int(best.begin_lane), "begin_wave": int(best.begin_wave),
                      "cigar_lane": int(best.cigar_lane), "cigar_wave": int(best.cigar_wave),
                      "cigar_wave_global": int(best.cigar_wave_global)}
    h.close()
    ps.close()
    text.close()
    return out


def edit_needle(src, L, e, seed):
    """bench.py's needle: e edits at pseudo-random places (substitute / delete / insert), trimmed back to L"""
    mix = S.capi.lib().spm_hip_mix64
    out = [int(x) for x in src[:L + e]]
    for j in range(e):
        r = mix(seed + j + 1)
        at = r % L
        kind = (r >> 32) % 3
        if kind == 0:
            out[at] = (out[at] + 1 + (r >> 40) % 3) & 3
        elif kind == 1:
            del out[at]
        else:
            out.insert(at, (r >> 40) & 3)
    return np.array(out[:L], dtype=np.uint8)


def pan(ctx, shape, log2_bases, n_reads, reps, route_haps):
    n_hap = 64
    ref_len = max(640000, (1 << log2_bases) // 640000 * 640000)
    ref = ctx.generate(SEED_TEXT, 0, ref_len)
    alleles, pool, cov = S.synth_variants(SEED_TEXT, SEED_VAR, 0, ref_len, n_hap)
    jst = S.Jst(ctx, ref, alleles, pool, cov.reshape(-1, 1), n_hap)
    mix = S.capi.lib().spm_hip_mix64
    if shape == "c5":
        L, kmax, n_pat, block, max_hits = 1024, 64, 256, 1024, 1 << 23
        needles = []
        for p in range(n_pat):
            r = mix(SEED_PAT + 7919 * p)
            h = r % n_hap
            o = (r >> 8) % (jst.haplotype_length(h) - 2 * (L + kmax))
            needles.append(edit_needle(jst.extract(h, o, L + kmax), L, p % (kmax + 1), SEED_PAT ^ (p << 20)))
    else:
        L, kmax, n_pat, block, max_hits = 150, 3, n_reads, 0, 1 << 26
        rng = np.random.default_rng(9)
        chunk = min(1 << 20, ref_len // 2)
        needles = np.empty((n_pat, L), dtype=np.uint8)
        per = (n_pat + n_hap - 1) // n_hap
        for h in range(n_hap):   # the reads of haplotype h come from one stretch of it
            piece = jst.extract(h, int(rng.integers(0, jst.haplotype_length(h) - chunk)), chunk)
            for p in range(h * per, min(n_pat, (h + 1) * per)):
                o = int(rng.integers(0, chunk - L - kmax - 1))
                needles[p] = edit_needle(piece[o:o + L + kmax], L, p % (kmax + 1), SEED_PAT ^ (p << 20))
    ps = ctx.patterns(S.ALGO_MYERS, needles, k=kmax)
    st = jst.index(L + kmax, block)
    out = {"needles": n_pat, "needle_len": L, "k": kmax, "reference_bases": ref_len, "haplotypes": n_hap,
           "haplotype_symbols": int(st.haplotype_symbols), "context_symbols": int(st.context_symbols)}
    search, h = [], None
    for r in range(reps + 1):
        if h is not None:
            h.close()
        ctx.synchronize()
        t0 = time.perf_counter()
        h = jst.search_device(ps, max_hits=max_hits, alignable=True)
        ctx.synchronize()
        js = jst.stats()
        search.append(((time.perf_counter() - t0) * 1e3, js.ms_scan + js.ms_fanout))
    out["search"] = {"ms_call_host": round(min(x[0] for x in search[1:]), 3), "ms_device": round(min(x[1] for x in search[1:]), 4),
                     "records": len(h), "segment_hits": int(js.segment_hits)}
    for label, begin_only in (("full", False), ("begin_only", True)):
        best, host = None, []
        for r in range(reps + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            a = h.align(begin_only=begin_only)
            ctx.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            s = a.stats()
            a.close()
            if r and (best is None or s.ms_host < best.ms_host):
                best = s
        out[label] = {"ms_call_host": round(min(host[1:]), 3), "ms_first_call_host": round(host[0], 3),
                      "ms_worklist_host": round(best.ms_worklist, 3), "ms_begin": round(best.ms_begin, 4),
                      "ms_cigar": round(best.ms_cigar, 4), "ms_fanout": round(best.ms_fanout, 4),
                      "ms_device": round(best.ms_total, 4), "records": int(best.n_alns),
                      "segment_alns": int(best.n_segment_alns), "pool_words": int(best.n_ops),
                      "segment_alns_per_record": round(best.n_segment_alns / max(1, best.n_alns), 5),
                      "begin_lane": int(best.begin_lane), "begin_wave": int(best.begin_wave),
                      "cigar_lane": int(best.cigar_lane), "cigar_wave": int(best.cigar_wave),
                      "cigar_wave_global": int(best.cigar_wave_global)}
    h.close()
    # the route without the tree, per haplotype: materialise on the host, upload, scan, align
    parts = {"extract": 0.0, "upload": 0.0, "scan": 0.0, "align": 0.0}
    n_route = 0
    for hap in range(0, n_hap, max(1, n_hap // max(1, route_haps)))[:route_haps] if route_haps else []:
        t0 = time.perf_counter()
        hp = jst.extract(hap, 0, jst.haplotype_length(hap))
        t1 = time.perf_counter()
        tx = ctx.upload(hp)
        ctx.synchronize()
        t2 = time.perf_counter()
        hh = S.scan(ctx, tx, ps, max_hits=1 << 23)
        n_route += len(hh.view())
        ctx.synchronize()
        t3 = time.perf_counter()
        a = hh.align()
        ctx.synchronize()
        t4 = time.perf_counter()
        a.close()
        hh.close()
        tx.close()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[k] += v * 1e3
    if route_haps:
        total = sum(parts.values())
        out["per_haplotype_route"] = {"haplotypes": route_haps, "records": n_route,
                                      "ms": {k: round(v, 2) for k, v in parts.items()}, "ms_total": round(total, 2),
                                      "ms_total_scaled_to_64_haplotypes": round(total * n_hap / route_haps, 1)}
    jst.close()
    ps.close()
    ref.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c4-gib", type=float, default=8.0)
    ap.add_argument("--c5-gib", type=float, default=0.125)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pan-log2", type=int, default=27, help="pan-genome rows: log2 of the reference length")
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--pan-route-haplotypes", type=int, default=4)
    ap.add_argument("--only", default="c4,c5,pan_c5,pan_reads")
    a = ap.parse_args()
    only = set(a.only.split(","))
    ctx = S.Context(0)
    res = {"metric": "spm_hip_hits_align / spm_hip_jst_hits_align device ms per hit set (stage A begins, stage B "
                     "transcripts, fan-out)"}
    if "c4" in only:
        res["c4"] = one(ctx, "c4", 150, 3, 100_000, a.c4_gib, a.reps)
    if "c5" in only:
        res["c5"] = one(ctx, "c5", 1024, 64, 256, a.c5_gib, a.reps)
    if "pan_c5" in only:
        res["pan_c5"] = pan(ctx, "c5", a.pan_log2, 0, a.reps, a.pan_route_haplotypes)
    if "pan_reads" in only:
        res["pan_reads"] = pan(ctx, "reads", a.pan_log2, a.pan_reads, a.reps, a.pan_route_haplotypes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
