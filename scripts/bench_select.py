"""Time hit selection (spm_hip_hits_select) on the C4 shape and on the repeat-rich c3r shape: one JSON line.

C4:  100 000 needles |P| = 150, k <= 3 over --c4-gib of synthetic dna4 text (bench.py's seeds and needles).
c3r: 1024 needles |P| = 100, k <= 3 over --c3r-gib of the repeat-rich text at --repeat-ppm (bench.py's c3r generator).
Per shape, behind one warm-up call each, --reps rounds that alternate the routes on the same box in the same process:
  * select():                device time of its order and select steps (HIP events, best round), host clock of the call,
                             n_in / n_loci / n_out;
  * the route a user has without it: Hits.view() of a fresh scan (download + host sort) plus the rule in NumPy, host clock;
  * align() of all hits  against  select() + align() of the loci: device time and host clock of each.
The first select() of the process is reported on its own: it pays the load of the unit's code object.

    python scripts/bench_select.py [--c4-gib 8] [--c3r-gib 16] [--repeat-ppm 50000] [--reps 5] [--only c4,c3r]
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


def numpy_loci(h, w):
    """LOCI on the host: h sorted by (pattern, pos); one window for every needle"""
    pos, pat, sc = h["pos"].astype(np.int64), h["pattern"].astype(np.int64), h["score"].astype(np.int64)
    keep = np.ones(len(h), dtype=bool)
    for d in range(1, len(h)):
        near = (pat[d:] == pat[:-d]) & (pos[d:] - pos[:-d] <= w)
        if not near.any():
            break
        keep[d:] &= ~(near & (sc[:-d] <= sc[d:]))
        keep[:-d] &= ~(near & (sc[d:] < sc[:-d]))
    return h[keep]


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def one(ctx, text, ps, kmax, max_hits, reps, with_align):
    h = S.scan(ctx, text, ps, max_hits=max_hits)
    out = {"hits": int(h.stats().n_hits), "scan_ms": round(h.stats().ms_total, 3)}
    first, first_ms = clock(lambda: h.select())
    out["first_select_call_host_ms"] = round(first_ms, 3)
    first.close()
    sel_dev, sel_host, host_route, host_view, al_all, al_loci = [], [], [], [], [], []
    counts = None
    for r in range(reps + 1):
        s, ms = clock(lambda: h.select())
        st = s.select_stats()
        sel_dev.append((st.ms_total, st.ms_order, st.ms_select))
        sel_host.append(ms)
        counts = {"n_in": int(st.n_in), "n_loci": int(st.n_loci), "n_out": int(st.n_out), "key_bits": int(st.key_bits)}
        s.close()
        # today's route: a fresh result (view() keeps its sorted copy), downloaded, sorted and selected on the host
        fresh = S.scan(ctx, text, ps, max_hits=max_hits)
        fresh.stats()
        v, ms_view = clock(lambda: fresh.view())
        kept, ms_rule = clock(lambda: numpy_loci(v, kmax))
        host_view.append(ms_view)
        host_route.append(ms_view + ms_rule)
        assert len(kept) == counts["n_loci"]
        fresh.close()
        if with_align:
            a, ms_a = clock(lambda: h.align())
            al_all.append((a.stats().ms_total, ms_a))
            a.close()

            def route():
                s2 = h.select()
                a2 = s2.align()
                return s2, a2
            (s2, a2), ms_b = clock(route)
            al_loci.append((s2.select_stats().ms_total + a2.stats().ms_total, ms_b, s2.select_stats().ms_total, a2.stats().ms_total))
            a2.close()
            s2.close()
    best = min(sel_dev[1:])
    out.update(counts)
    out["select"] = {"ms_device": round(best[0], 4), "ms_order": round(best[1], 4), "ms_select": round(best[2], 4),
                     "ms_call_host": round(min(sel_host[1:]), 3), "ms_call_host_median": round(float(np.median(sel_host[1:])), 3)}
    out["host_route"] = {"ms_view": round(min(host_view[1:]), 3), "ms_view_plus_numpy_rule": round(min(host_route[1:]), 3),
                         "ms_view_plus_numpy_rule_median": round(float(np.median(host_route[1:])), 3)}
    if with_align:
        out["align_all"] = {"ms_device": round(min(x[0] for x in al_all[1:]), 4), "ms_call_host": round(min(x[1] for x in al_all[1:]), 3),
                            "ms_call_host_median": round(float(np.median([x[1] for x in al_all[1:]])), 3)}
        b = min(al_loci[1:])
        out["select_then_align_loci"] = {"ms_device": round(b[0], 4), "ms_device_select": round(b[2], 4), "ms_device_align": round(b[3], 4),
                                         "ms_call_host": round(min(x[1] for x in al_loci[1:]), 3),
                                         "ms_call_host_median": round(float(np.median([x[1] for x in al_loci[1:]])), 3)}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c4-gib", type=float, default=8.0)
    ap.add_argument("--c3r-gib", type=float, default=16.0)
    ap.add_argument("--repeat-ppm", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="c4,c3r")
    a = ap.parse_args()
    only = set(a.only.split(","))
    ctx = S.Context(0)
    res = {"metric": "spm_hip_hits_select device ms (order + select), beside view() + NumPy rule on the host and align() of "
                     "all hits against select() + align() of the loci", "reps": a.reps}
    if "c4" in only:
        n = int(a.c4_gib * 2**30) & ~1023
        text = ctx.generate(SEED_TEXT, 0, n)
        needles = np.stack([S.synth_pattern(SEED_TEXT, SEED_PAT, n, p, 150, 3)[0] for p in range(100_000)])
        ps = ctx.patterns(S.ALGO_MYERS, needles, k=3)
        res["c4"] = dict({"needles": 100_000, "needle_len": 150, "k": 3, "text_bytes": n}, **one(ctx, text, ps, 3, 1 << 23, a.reps, True))
        ps.close()
        text.close()
    if "c3r" in only:
        n = int(a.c3r_gib * 2**30) & ~1023
        text = ctx.generate_repeats(SEED_TEXT, 0, n, a.repeat_ppm)
        needles = np.stack([S.synth_repeat_pattern(SEED_TEXT, SEED_PAT, n, p, 100, 3, a.repeat_ppm)[0] for p in range(1024)])
        ps = ctx.patterns(S.ALGO_MYERS, needles, k=3)
        res["c3r"] = dict({"needles": 1024, "needle_len": 100, "k": 3, "text_bytes": n, "repeat_ppm": a.repeat_ppm},
                          **one(ctx, text, ps, 3, 1 << 27, a.reps, False))
        ps.close()
        text.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
