"""Time the projection of pan-genome alignments onto the reference (spm_hip_jst_alns_project) beside the alignment whose
output it projects: one JSON line.

The trees and needle sets are those of scripts/bench_align.py --only pan_c5,pan_reads: `pan_c5` 256 needles |P| = 1024,
k <= 64 (bench.py's C5 tree and needles) and `pan_reads` --pan-reads reads |P| = 150, k <= 3.  Per row and for both routes --
align() of an alignable search, and select() + align_selected() -- behind one warm-up call, --reps project() calls; the best
call's device time per stage (representatives, count, emit, gather: HIP events) and its host clock; n_projected / n_alns; in
the same run the device time of the align call whose output is projected (stage A, stage B, fan-out / locate + gather); and
the host clock of projecting a fixed sample of --sample records in NumPy (an event-table lookup per haplotype position, the
host-side walk a caller would write), checked against the device's records and scaled to all records -- labelled as scaled,
it is not a measurement of all of them.  The claim to report on: projecting once per slot costs less device time than
stages A + B of the same alignments, on both rows.

Every row runs in a child process of its own under a time limit.

    python scripts/bench_jst_project.py [--pan-log2 27] [--pan-reads 100000] [--reps 5] [--sample 10000]
                                        [--only pan_c5,pan_reads] [--row-timeout 420] [--out profiles/r05/jst_project.json]
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
from bench_align import SEED_PAT, SEED_TEXT, SEED_VAR, edit_needle  # noqa: E402

INS, DEL, EQ, X = 1, 2, 7, 8


def build(ctx, shape, log2_bases, n_reads):
    """tree, needle set and index of bench_align.pan"""
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
        needles = np.stack(needles)
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
    info = {"needles": n_pat, "needle_len": L, "k": kmax, "reference_bases": ref_len, "haplotypes": n_hap,
            "context_symbols": int(st.context_symbols)}
    return ref, jst, ps, needles, (alleles, cov), max_hits, info


class HostWalk:
    """The projection on the host in NumPy: every haplotype position of a record is looked up in the event table of its
    haplotype (the alleles it carries, where their alts start in the haplotype, the running shift)."""

    def __init__(self, ref, alleles, cov):
        self.ref, self.tables = ref, {}
        self.alleles, self.cov = alleles, np.asarray(cov, dtype=np.uint64).reshape(-1)

    def table(self, h):
        if h not in self.tables:
            a = self.alleles[((self.cov >> np.uint64(h)) & np.uint64(1)).astype(bool)]
            p, rl, al = a["pos"].astype(np.int64), a["ref_len"].astype(np.int64), a["alt_len"].astype(np.int64)
            cs = np.cumsum(al - rl)
            hs = p + np.concatenate([[0], cs[:-1]]) if len(p) else p
            self.tables[h] = (hs, p, rl, al, cs)
        return self.tables[h]

    def project(self, h, begin, words, P):
        hs, p, rl, al, cs = self.table(h)
        t_op = np.repeat(words & 15, words >> 4)
        on_h = t_op != INS
        xs = begin + np.arange(int(on_h.sum()), dtype=np.int64)
        n = np.searchsorted(hs, xs, side="right") - 1
        m = np.maximum(n, 0)
        k = xs - hs[m] if len(hs) else xs
        in_alt = (n >= 0) & (k < al[m]) if len(hs) else np.zeros(len(xs), bool)
        paired_h = ~in_alt | (k < rl[m]) if len(hs) else np.ones(len(xs), bool)
        if len(hs):
            rho_h = np.where(n < 0, xs, np.where(in_alt, p[m] + np.minimum(k, np.minimum(rl[m], al[m])), xs - cs[m]))
        else:
            rho_h = xs
        paired = np.zeros(len(t_op), bool)
        rho = np.zeros(len(t_op), np.int64)
        paired[on_h], rho[on_h] = paired_h, rho_h
        i = np.cumsum(t_op != DEL) - 1
        op = np.full(len(t_op), INS, np.int64)
        sym = (t_op != DEL) & paired
        op[sym] = np.where(P[i[sym]] == self.ref[rho[sym]], EQ, X)
        op[(t_op == DEL) & paired] = DEL
        op[(t_op == DEL) & ~paired] = 0
        gap = np.zeros(len(t_op), np.int64)
        cons = np.nonzero(paired)[0]
        if len(cons) > 1:
            gap[cons[1:]] = np.diff(rho[cons]) - 1
        out = np.repeat(np.stack([np.full(len(op), DEL), op], axis=1).reshape(-1),
                        np.stack([gap, (op != 0).astype(np.int64)], axis=1).reshape(-1))
        cut = np.concatenate([[0], np.nonzero(out[1:] != out[:-1])[0] + 1, [len(out)]])
        w = ((np.diff(cut) << 4) | out[cut[:-1]]).astype(np.uint32)
        if len(cons):
            return int(rho[cons[0]]), int(rho[cons[-1]]) + 1, int((out != EQ).sum()), w
        return int(rho_h[0]), int(rho_h[0]), int((out != EQ).sum()), w


def measure(ctx, make, reps, walk, needles, sample):
    """make() -> (JstAlignments, things to close).  The align call's device times, then reps + 1 project() calls."""
    a, closers = make()
    st = a.stats()
    out = {"align": {"ms_device": round(st.ms_total, 4), "ms_stage_a": round(st.ms_begin, 4), "ms_stage_b": round(st.ms_cigar, 4),
                     "ms_map": round(st.ms_fanout, 4), "ms_call_host": round(st.ms_host, 3), "records": int(st.n_alns),
                     "segment_alns": int(st.n_segment_alns), "pool_words": int(st.n_ops)}}
    best, host = None, []
    for r in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        pr = a.project()
        ctx.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        s = pr.stats()
        if r and (best is None or s.ms_total < best.ms_total):
            best = s
        if r < reps:
            pr.close()
    out["project"] = {"ms_device": round(best.ms_total, 4), "ms_representatives": round(best.ms_representatives, 4),
                      "ms_count": round(best.ms_count, 4), "ms_emit": round(best.ms_emit, 4),
                      "ms_gather": round(best.ms_gather, 4), "ms_call_host": round(min(host[1:]), 3),
                      "ms_first_call_host": round(host[0], 3), "records": int(best.n_alns), "projected": int(best.n_projected),
                      "projected_per_record": round(best.n_projected / max(1, best.n_alns), 5), "pool_words": int(best.n_ops),
                      "changed": int(best.n_changed), "inside_insertion": int(best.n_inside_insertion)}
    out["project_below_stages_a_b_device"] = bool(best.ms_total < st.ms_begin + st.ms_cigar)
    # the host walk on a fixed sample of the records, checked against the device's
    sv, sops, rv, rops = a.view(), a.ops, pr.view(), pr.ops
    n = len(sv)
    pick = np.random.default_rng(5).choice(n, size=min(sample, n), replace=False) if n else []
    for h in {int(x) for x in sv["haplotype"][pick]}:
        walk.table(h)                       # (the event tables are built once per tree: not part of the per-record clock)
    t0 = time.perf_counter()
    got = []
    for j in pick:
        s = sv[j]
        o = int(s["cigar_off"])
        got.append(walk.project(int(s["haplotype"]), int(s["begin"]), sops[o:o + int(s["cigar_len"])], needles[int(s["pattern"])]))
    dt = (time.perf_counter() - t0) * 1e3
    for j, (rb, re, sc, w) in zip(pick, got):
        r = rv[j]
        o = int(r["cigar_off"])
        assert (int(r["ref_begin"]), int(r["ref_end"]), int(r["ref_score"])) == (rb, re, sc), (j, r, rb, re, sc)
        assert np.array_equal(rops[o:o + int(r["cigar_len"])], w), j
    out["numpy_host_walk"] = {"sample": len(pick), "ms_sample": round(dt, 2),
                              "ms_scaled_to_all_records": round(dt * n / max(1, len(pick)), 1), "equal_to_device": True}
    pr.close()
    a.close()
    for c in closers:
        c.close()
    return out


def row(shape, log2_bases, n_reads, reps, sample):
    ctx = S.Context(0)
    ref, jst, ps, needles, (alleles, cov), max_hits, out = build(ctx, shape, log2_bases, n_reads)
    walk = HostWalk(ref.download(0, len(ref)), alleles, cov)

    def all_records():
        h = jst.search_device(ps, max_hits=max_hits, alignable=True)
        h.align().close()                   # (the first call builds the set's alignment tables)
        return h.align(), [h]

    def selected():
        h = jst.search_device(ps, max_hits=max_hits)
        s = h.select()
        return s.align_selected(), [s, h]

    out["align_all"] = measure(ctx, all_records, reps, walk, needles, sample)
    out["align_selected"] = measure(ctx, selected, reps, walk, needles, sample)
    jst.close()
    ps.close()
    ref.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-log2", type=int, default=27)
    ap.add_argument("--pan-reads", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=10_000)
    ap.add_argument("--only", default="pan_c5,pan_reads")
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds one row's child process may take")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--row", default=None, help=argparse.SUPPRESS)   # the child's mode: one row, its JSON on stdout
    a = ap.parse_args()
    if a.row:
        print(json.dumps(row("c5" if a.row == "pan_c5" else "reads", a.pan_log2, a.pan_reads, a.reps, a.sample)))
        return 0
    res = {"metric": "spm_hip_jst_alns_project: device ms per stage (HIP events) and host clock, best of reps behind a warm-up, "
                     "beside the device ms of the align call whose output it projects", "reps": a.reps}
    for name in ("pan_c5", "pan_reads"):
        if name not in a.only.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--pan-log2", str(a.pan_log2), "--pan-reads",
               str(a.pan_reads), "--reps", str(a.reps), "--sample", str(a.sample)]
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
