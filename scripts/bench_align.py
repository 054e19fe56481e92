"""Time spm_hip_hits_align on the hit sets of the C4 and C5 shapes: one JSON line.

C4: 100 000 needles |P| = 150, k <= 3 over --c4-gib of synthetic dna4 text (bench.py's seeds and needles).
C5: 256 needles |P| = 1024, k <= 64 over --c5-gib of plain synthetic text (the shape of config C5's needles; the
journaled-sequence search itself has no alignment step).
Per set: the scan, then --reps align calls with and without SPM_ALIGN_BEGIN_ONLY; the device times of each stage
(best of the calls), the host wall clock of the call, and how the hits were split over the kernel classes.

    python scripts/bench_align.py [--c4-gib 8] [--c5-gib 0.125] [--reps 5]
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

SEED_TEXT, SEED_PAT = 0x5EED0001, 0x5EED0002


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c4-gib", type=float, default=8.0)
    ap.add_argument("--c5-gib", type=float, default=0.125)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = S.Context(0)
    res = {"metric": "spm_hip_hits_align device ms per hit set (stage A begins, stage B transcripts)",
           "c4": one(ctx, "c4", 150, 3, 100_000, a.c4_gib, a.reps),
           "c5": one(ctx, "c5", 1024, 64, 256, a.c5_gib, a.reps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
