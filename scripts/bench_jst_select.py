"""Time the selection of pan-genome hits (spm_hip_jst_hits_select) on two shapes: one JSON line.

pan_c5:    bench.py's C5 tree and needles -- 256 needles |P| = 1024, k <= 64 over --c5-log2 reference bases x 64 haplotypes.
pan_reads: the read-mapping shape of tests/test_jst_align.py::test_scale_read_mapping_shape, built as the test builds it --
           2^--reads-log2 reference bases rounded down to whole 10 000, 64 haplotypes, --reads reads |P| = 150, k = 3, each
           cut from a random haplotype by the test's `_edited` (one deletion and / or one insertion, the rest of the budget
           substitutions) under the test's generator seed.
Per shape, behind one warm-up round, --reps rounds that alternate the two routes in one process:
  * select() + view() of the result: device time of the order and select steps (HIP events, best round), host clock of
    select() alone and of select() + view();
  * the route a user has without it: view() of all records of a fresh search (download + host sort) plus the rule in
    NumPy, host clock.
Both routes must keep the same number of records.  The claim to check: on pan_reads the selected route is below the host
route in wall clock, best round against best round (`selected_route_below_host_route`; the medians are printed beside).

    python scripts/bench_jst_select.py [--c5-log2 27] [--reads-log2 22] [--reads 20000] [--reps 5] [--only pan_c5,pan_reads]
                                       [--out profiles/r04/jst_select.json]
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


def edited(rng, hp, L, k):
    """tests/test_jst_align.py::_edited for a Myers needle: L symbols cut from hp with at most k edits"""
    o = int(rng.integers(0, len(hp) - L - k - 2))
    nd = hp[o:o + L + k + 1].copy()
    kind = int(rng.integers(0, 3)) if k >= 2 else int(rng.integers(0, 2))
    spent = 0
    if kind in (0, 2):
        nd = np.delete(nd, int(rng.integers(3, L - 3)))
        spent += 1
    if kind in (1, 2):
        at = int(rng.integers(3, L - 3))
        nd = np.insert(nd, at, (int(nd[at]) + 1 + int(rng.integers(0, 3))) & 3)
        spent += 1
    for _ in range(int(rng.integers(0, k - spent + 1))):
        at = int(rng.integers(0, L))
        nd[at] = (int(nd[at]) + 1 + int(rng.integers(0, 3))) & 3
    return nd[:L].astype(np.uint8)


def numpy_loci(v, w, n_pat):
    """LOCI on the host: the records of a view(), one window for every needle; the locus is (haplotype, pattern)"""
    v = v[np.lexsort((v["pos"], v["pattern"], v["haplotype"]))]
    grp = v["haplotype"].astype(np.int64) * n_pat + v["pattern"].astype(np.int64)
    pos, sc = v["pos"].astype(np.int64), v["score"].astype(np.int64)
    keep = np.ones(len(v), dtype=bool)
    for d in range(1, len(v)):
        near = (grp[d:] == grp[:-d]) & (pos[d:] - pos[:-d] <= w)
        if not near.any():
            break
        keep[d:] &= ~(near & (sc[:-d] <= sc[d:]))
        keep[:-d] &= ~(near & (sc[d:] < sc[:-d]))
    return v[keep]


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def pan(ctx, shape, log2_bases, n_reads, reps):
    n_hap = 64
    ref_len = max(640000, (1 << log2_bases) // 640000 * 640000) if shape == "c5" else (1 << log2_bases) // 10_000 * 10_000
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
        L, kmax, n_pat, block, max_hits = 150, 3, n_reads, 0, 1 << 23
        rng = np.random.default_rng(9)
        haps = [jst.extract(h, 0, jst.haplotype_length(h)) for h in range(n_hap)]
        needles = np.stack([edited(rng, haps[int(rng.integers(0, n_hap))], L, kmax) for _ in range(n_pat)])
        del haps
    ps = ctx.patterns(S.ALGO_MYERS, needles, k=kmax)
    st = jst.index(L + kmax, block)
    out = {"needles": n_pat, "needle_len": L, "k": kmax, "reference_bases": ref_len, "haplotypes": n_hap,
           "context_symbols": int(st.context_symbols)}
    h = jst.search_device(ps, max_hits=max_hits)
    out["records"] = len(h)
    first, first_ms = clock(lambda: h.select())
    out["first_select_call_host_ms"] = round(first_ms, 3)
    first.close()
    dev, sel_host, sel_view_host, host_view, host_route = [], [], [], [], []
    counts = None
    for r in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        s = h.select()
        t1 = time.perf_counter()
        kept = s.view()
        t2 = time.perf_counter()
        stt = s.select_stats()
        dev.append((stt.ms_total, stt.ms_order, stt.ms_select))
        sel_host.append((t1 - t0) * 1e3)
        sel_view_host.append((t2 - t0) * 1e3)
        counts = {"n_in": int(stt.n_in), "n_loci": int(stt.n_loci), "n_out": int(stt.n_out), "key_bits": int(stt.key_bits)}
        s.close()
        # the route without it: a fresh result (view() keeps its sorted copy), downloaded, sorted and selected on the host
        fresh = jst.search_device(ps, max_hits=max_hits)
        ctx.synchronize()
        v, ms_view = clock(lambda: fresh.view())
        loci, ms_rule = clock(lambda: numpy_loci(v, kmax, n_pat))
        host_view.append(ms_view)
        host_route.append(ms_view + ms_rule)
        assert len(loci) == len(kept) == counts["n_loci"], (len(loci), len(kept), counts)
        fresh.close()
    best = min(dev[1:])
    out.update(counts)
    out["select"] = {"ms_device": round(best[0], 4), "ms_order": round(best[1], 4), "ms_select": round(best[2], 4),
                     "ms_call_host": round(min(sel_host[1:]), 3), "ms_call_host_median": round(float(np.median(sel_host[1:])), 3),
                     "ms_select_plus_view_host": round(min(sel_view_host[1:]), 3),
                     "ms_select_plus_view_host_median": round(float(np.median(sel_view_host[1:])), 3)}
    out["host_route"] = {"ms_view": round(min(host_view[1:]), 3), "ms_view_plus_numpy_rule": round(min(host_route[1:]), 3),
                         "ms_view_plus_numpy_rule_median": round(float(np.median(host_route[1:])), 3)}
    out["selected_route_below_host_route"] = bool(min(sel_view_host[1:]) < min(host_route[1:]))
    h.close()
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
    res = {"metric": "spm_hip_jst_hits_select: device ms (order + select) and host clock of select() + view(), beside view() of "
                     "all records + the rule in NumPy on the host", "reps": a.reps}
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
