"""ms_order / ms_select of spm_hip_hits_select on the C4 and c3r shapes of scripts/bench_select.py and nothing else (no
host route, no align): one JSON line.  Cheap enough to run many times, e.g. alternating between two checkouts whose
libraries are to be compared; --tag names the checkout in the line.

    python scripts/bench_select_stages.py [--tag NAME] [--c4-gib 8] [--c3r-gib 16] [--reps 11]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libspm_amd as S  # noqa: E402

SEED_TEXT, SEED_PAT = 0x5EED0001, 0x5EED0002


def stages(h, reps):
    h.select().close()                      # the first call pays the module load
    rows = []
    for _ in range(reps):
        s = h.select()
        st = s.select_stats()
        rows.append((st.ms_order, st.ms_select, st.ms_total))
        n = (int(st.n_in), int(st.n_loci), int(st.n_out), int(st.key_bits))
        s.close()
    rows = rows[1:]
    return {"n_in": n[0], "n_loci": n[1], "n_out": n[2], "key_bits": n[3],
            "ms_order": round(min(r[0] for r in rows), 4), "ms_select": round(min(r[1] for r in rows), 4),
            "ms_order_median": round(float(np.median([r[0] for r in rows])), 4),
            "ms_select_median": round(float(np.median([r[1] for r in rows])), 4)}


ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="")
ap.add_argument("--c4-gib", type=float, default=8.0)
ap.add_argument("--c3r-gib", type=float, default=16.0)
ap.add_argument("--reps", type=int, default=11)
a = ap.parse_args()
ctx = S.Context(0)
res = {"lib": a.tag, "script": "bench_select_stages", "reps": a.reps}
n = int(a.c4_gib * 2**30) & ~1023
text = ctx.generate(SEED_TEXT, 0, n)
needles = np.stack([S.synth_pattern(SEED_TEXT, SEED_PAT, n, p, 150, 3)[0] for p in range(100_000)])
ps = ctx.patterns(S.ALGO_MYERS, needles, k=3)
h = S.scan(ctx, text, ps, max_hits=1 << 23)
res["c4"] = stages(h, a.reps)
h.close()
ps.close()
text.close()
n = int(a.c3r_gib * 2**30) & ~1023
text = ctx.generate_repeats(SEED_TEXT, 0, n, 50000)
needles = np.stack([S.synth_repeat_pattern(SEED_TEXT, SEED_PAT, n, p, 100, 3, 50000)[0] for p in range(1024)])
ps = ctx.patterns(S.ALGO_MYERS, needles, k=3)
h = S.scan(ctx, text, ps, max_hits=1 << 27)
res["c3r"] = stages(h, a.reps)
h.close()
ps.close()
text.close()
print(json.dumps(res))
