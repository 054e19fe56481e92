"""GPU: the dense pass (filter_dense.hpp seed_filter_dense_kernel: dense_group / dense_drain) with its presence bits, fingerprint
buckets and per-wave queue in every state, on key sets built for it (tests/dense_states.py; tests/test_dense_states.py
checks the builder against the product's tables on the CPU).

tests/test_gpu_dense.py forces the dense pass on 700 needles or fewer: 0.3 % of the presence bits, no full bucket,
bucket_shift 20, a queue that holds a handful of entries and is emptied once, at the span's end.  Here a 16-symbol exact
needle is its own key and a 64-symbol Myers needle (k = 3) is four keys, so the set has one overflowed bucket (its last five
keys are found ONLY through the accept-all marker), one full bucket, and the text carries windows that are no keys but pass
the presence bits -- in floods that fill the queue to exactly its capacity (three batches drained at once), in ragged floods
(drains of two batches, a remainder kept), sparsely (one partial batch at the span's end), and beside true occurrences.
Every true occurrence keeps ONE intact seed (Myers) or is one key (exact), so a queue entry that is lost, doubled or
given another entry's offset removes or moves a hit.  The reference is never the filter: the brute-force engine (whole list),
the construction (every planted occurrence, with its score) and the CPU oracle.  test_regime runs the sets the dense pass
is made for -- 100 000 reads, dense by themselves -- against the brute-force engine and the oracle."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dense_states as DS

pytestmark = pytest.mark.gpu

OFFSET = 1 << 40
N_TEXT = DS.N_TEXT
SETS = {"shiftor16": ("exact16", "SHIFTOR", 0), "horspool16": ("exact16", "HORSPOOL", 0), "myers64": ("myers64", "MYERS", 3)}
SEED_TEXT, SEED_PAT = 0x5EED0001, 0x5EED0002
_built, _cases = {}, {}


class Case:
    pass


def _hits(pattern, pos, score):
    h = np.zeros(len(pos), dtype=[("pattern", np.int64), ("pos", np.int64), ("score", np.int64)])
    h["pattern"], h["pos"], h["score"] = pattern, pos, score
    return np.sort(h, order=["pattern", "pos"])


def _rows(v):
    """a device list as plain columns (it comes sorted by pattern, pos)"""
    return _hits(v["pattern"], v["pos"], v["score"])


def _oracle_list(oracle, mode, T, needles):
    """exact sets: oracle.naive_exact per needle; myers64: oracle.scan_multi on the whole text"""
    if mode == "myers64":
        return _rows(oracle.scan_multi(oracle.MYERS, T, list(needles), k=3, threads=16))
    with ThreadPoolExecutor(16) as pool:
        found = list(pool.map(lambda nd: oracle.naive_exact(T, nd), needles))
    pat = np.repeat(np.arange(len(needles)), [len(f) for f in found])
    pos = np.concatenate(found).astype(np.int64)
    return _hits(pat, pos, np.zeros(len(pos), np.int64))


def _patterns(spm, ctx, algo, needles, k, n_keys):
    os.environ["SPM_HIP_FILTER_DENSE"] = "2"
    try:
        ps = ctx.patterns(getattr(spm, "ALGO_" + algo), needles, k=k)
    finally:
        del os.environ["SPM_HIP_FILTER_DENSE"]
    bs = ps.build_stats()
    assert ps.filterable and (int(bs.dense), int(bs.passes), int(bs.anchor_sixteenths), int(bs.keys)) == (1, 1, 16, n_keys)
    return ps


def _filter_scan(spm, ctx, text, ps, *args, fallback_spans=0, **kw):
    """conditions on every filter scan, not measurements: a brute-force re-scan would find what the filter lost"""
    h = spm.scan(ctx, text, ps, *args, engine=spm.ENGINE_FILTER, **kw)
    st = h.stats()
    assert (int(st.engine_used), int(st.fell_back), int(st.main_launches)) == (spm.ENGINE_FILTER, 0, 1)
    if fallback_spans is not None:
        assert int(st.fallback_spans) == fallback_spans
    return h.view().copy(), st


def _case(spm, ctx, oracle, which, shift):
    """The set, its text laid out on the scan's own span borders, the whole filter scan, and the references -- once."""
    if (which, shift) in _cases:
        return _cases[which, shift]
    mode, algo, k = SETS[which]
    if shift not in _built:
        _built[shift] = DS.built_set(shift)
    ks, D = _built[shift]
    c = Case()
    c.mode, c.k, c.ks = mode, k, ks
    c.needles = DS.exact16(ks) if mode == "exact16" else DS.myers64(ks)
    c.ps = _patterns(spm, ctx, algo, c.needles, k, ks.n)
    span = 8192
    for again in range(2):      # the span depends on the device and on the text's length: lay out, scan, read it, lay out again
        c.lay = DS.case_layout(ks, D, mode, span)
        c.T = c.lay.text
        c.text = ctx.upload(c.T)
        c.got, st = _filter_scan(spm, ctx, c.text, c.ps)
        if int(st.span_symbols) == span:
            break
        span = int(st.span_symbols)
    assert int(st.span_symbols) == span, "the layout's span borders are not the scan's"
    c.span = span
    c.brute = spm.scan(ctx, c.text, c.ps, engine=spm.ENGINE_BRUTE).view().copy()
    ref = _cases.get(("oracle", mode, shift, span))     # (Shift-Or and Horspool share the set, the text and the oracle's list)
    if ref is None:
        ref = _cases["oracle", mode, shift, span] = _oracle_list(oracle, mode, c.T, c.needles)
    c.oracle = ref
    _cases[which, shift] = c
    return c


def _sorted(h):
    return h[np.lexsort((h["pos"], h["pattern"]))]


@pytest.mark.parametrize("shift", [20, 18])
@pytest.mark.parametrize("which", list(SETS))
def test_states(spm, ctx, oracle, which, shift):
    c = _case(spm, ctx, oracle, which, shift)
    lay, got, exact = c.lay, c.got, c.mode == "exact16"
    # 1. the brute-force engine  2. the oracle  3. the construction
    assert np.array_equal(got, c.brute)
    assert np.array_equal(_rows(got), c.oracle)
    rows = {(int(p), int(x)): int(s) for p, x, s in zip(got["pattern"], got["pos"], got["score"])}
    assert len(lay.planted) >= 200
    for p, s, e, edits in lay.planted:
        assert rows.get((p, s if exact else e)) == edits, ("planted occurrence lost", p, s, e, edits)
    over = set(c.ks.groups["over"][7:].tolist()) if exact else {1, 2}      # keys that have no slot of their own in bucket B
    assert over <= {p for p, *_ in lay.planted}
    # a sub-range that begins and ends inside the aligned flood: cold, and with left context == that part of the whole scan
    a, b = lay.stretches[0], lay.stretches[1]
    assert a.kind == b.kind == "flood_aligned" and a.end == b.begin and a.end - a.begin >= 2 * c.span
    lo, hi = a.begin + c.span // 2 + 7, b.end - c.span // 2 - 5
    last = got["pos"].astype(np.int64) + (15 if exact else -1)      # the hit's last symbol
    part = got[(last >= lo) & (last < hi)].copy()
    part["pos"] += OFFSET
    assert len(part) >= 32
    for warm in (False, True):
        sub, _ = _filter_scan(spm, ctx, c.text, c.ps, lo, hi, left_context=warm, pos_offset=OFFSET)
        bsub = spm.scan(ctx, c.text, c.ps, lo, hi, engine=spm.ENGINE_BRUTE, left_context=warm, pos_offset=OFFSET).view()
        assert np.array_equal(sub, bsub), (which, shift, warm)
        if warm:
            assert np.array_equal(sub, part)
        else:
            assert len(sub) >= 32
    # independent haystacks with borders inside the ragged floods, one of them empty == per-segment brute-force scans
    r0, r1 = lay.stretches[2], lay.stretches[3]
    assert r0.kind == r1.kind == "flood_ragged"
    offs = np.array([0, r0.begin + 1003, r0.begin + 5009, r0.begin + 5009, r1.begin + 4444, r1.end - 77, N_TEXT[shift]], dtype=np.uint64)
    h = spm.scan_segments(ctx, c.text, c.ps, offs, engine=spm.ENGINE_FILTER)
    st = h.stats()
    assert (int(st.engine_used), int(st.fell_back), int(st.fallback_spans)) == (spm.ENGINE_FILTER, 0, 0)
    ref = [spm.scan(ctx, c.text, c.ps, int(x), int(y), engine=spm.ENGINE_BRUTE).view().copy()
           for x, y in zip(offs, offs[1:]) if y > x]
    ref = _sorted(np.concatenate(ref))
    assert len(ref) >= 200 and np.array_equal(h.view(), ref)


def _certain_survivors(c, lo, hi):
    """windows starting in [lo, hi) that reach resolve_kernel by construction: key windows of the plants, accept_all and
    fp_twin decoys"""
    at = [s + 16 * j for p, s, e, edits in c.lay.planted for j in range((e - s) // 16) if edits == 0]
    at += [s + 16 * j for p, s, e, edits in c.lay.planted if edits for j in range(4)
           if np.array_equal(c.T[s + 16 * j:s + 16 * j + 16], c.needles[p][16 * j:16 * j + 16])]
    at += [x for x, name in c.lay.decoy_at if name in ("accept_all", "fp_twin")]
    return np.sort(np.array([x for x in at if lo <= x < hi], dtype=np.int64))


@pytest.mark.parametrize("which", ["shiftor16", "myers64"])
@pytest.mark.parametrize("budget", [2, 64])
def test_spans_give_up_with_a_full_queue(spm, ctx, oracle, which, budget):
    """Spans whose survivors exceed a small budget give up while windows are still queued and are scanned again by the
    brute-force kernel: same hits, each once.  A budget of 64 is spent in the middle of the aligned flood's spans only."""
    c = _case(spm, ctx, oracle, which, 20)
    os.environ["SPM_HIP_FILTER_SPAN_BUDGET"] = str(budget)
    try:
        got, st = _filter_scan(spm, ctx, c.text, c.ps, fallback_spans=None)
    finally:
        del os.environ["SPM_HIP_FILTER_SPAN_BUDGET"]
    assert int(st.fallback_spans) > 0 and int(st.fell_back) == 0
    assert np.array_equal(got, c.brute)
    key = got["pattern"].astype(np.int64) << 40 | got["pos"].astype(np.int64)
    assert len(np.unique(key)) == len(key)
    if budget == 64:
        # by construction: a span gives up for certain with more than 64 survivors well inside it, and cannot with fewer
        # than 60 around it; the 65th of an aligned-flood span lies in its middle
        must = may = 0
        for b in range(0, N_TEXT[20], c.span):
            inner = _certain_survivors(c, b + 16, b + c.span - 32)
            must += len(inner) > budget
            may += len(_certain_survivors(c, b - 32, b + c.span + 16)) > budget - 4
            if len(inner) > budget:
                assert c.span // 4 < inner[budget] - b < c.span * 9 // 10
        flooded = sum((s.end - s.begin) // c.span for s in c.lay.stretches if s.kind == "flood_aligned")
        assert must == flooded >= 8 and must <= int(st.fallback_spans) <= may


def test_deferred_floods(spm, ctx, oracle):
    """SPM_SCAN_DEFER on the flooded text: three scans back to back, results from the device-side fused copy"""
    import torch
    c = _case(spm, ctx, oracle, "shiftor16", 20)
    want = c.brute
    cap = len(want) + 64
    bufs = [torch.zeros((cap + 1, 2), dtype=torch.int64, device="cuda") for _ in range(3)]
    hs = []
    for buf in bufs:
        h = spm.scan(ctx, c.text, c.ps, engine=spm.ENGINE_FILTER, flags=spm.SCAN_DEFER)
        h.copy_fused_device(buf.data_ptr(), cap)
        hs.append(h)
    ctx.synchronize()
    torch.cuda.current_stream().synchronize()
    for h, buf in zip(hs, bufs):
        assert buf[0].cpu().tolist() == [len(want), 0]
        rec = buf[1:1 + len(want)].cpu().numpy().view(np.uint8).reshape(-1, 16)
        got = np.sort(np.frombuffer(rec.tobytes(), dtype=spm.HIT_DTYPE), order=["pattern", "pos"])
        assert np.array_equal(got, want)
        st = h.stats()
        assert (int(st.engine_used), int(st.fell_back), int(st.fallback_spans), int(st.main_launches)) == (spm.ENGINE_FILTER, 0, 0, 1)
        h.close()


@pytest.mark.parametrize("L", [150, 100], ids=["c4", "reads100"])
def test_regime(spm, ctx, oracle, L):
    """100 000 reads of L symbols, k = 3, every one planted in the 8 Mi symbols that are scanned; no knob: the set takes the
    dense pass by itself, with 400 000 keys, bucket_shift 14 and an eighth of the presence bits set."""
    n, k, n_reads = 1 << 23, 3, 100_000
    made = [spm.synth_pattern(SEED_TEXT, SEED_PAT, n, p, L, k) for p in range(n_reads)]
    needles = np.stack([m[0] for m in made])
    origin = np.array([m[1] for m in made], dtype=np.int64)
    text = ctx.generate(SEED_TEXT, 0, n)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    bs = ps.build_stats()
    assert ps.filterable and (int(bs.dense), int(bs.passes)) == (1, 1) and int(bs.anchor_sixteenths) <= 8
    got, st = _filter_scan(spm, ctx, text, ps, max_hits=1 << 22)
    brute = spm.scan(ctx, text, ps, engine=spm.ENGINE_BRUTE, max_hits=1 << 22).view()
    assert len(brute) >= n_reads and np.array_equal(got, brute)
    # every read: a hit within k of origin + L with at most the p mod 4 edits it was given
    pat, pos, score = got["pattern"].astype(np.int64), got["pos"].astype(np.int64), got["score"]
    near = (np.abs(pos - (origin[pat] + L)) <= k) & (score <= pat % (k + 1))
    assert len(np.unique(pat[near])) == n_reads
    # the oracle with all reads on two windows of 64 Ki symbols, read with window - 1 symbols of left context
    T = text.download(0, n)
    w = L + k
    for lo in (int(origin[777]) // 1024 * 1024, 5 << 20):
        lo = max(lo, 65536)
        hi = lo + 65536
        o = oracle.scan_multi(oracle.MYERS, T[lo - (w - 1):hi], list(needles), k=k, threads=16)
        o = o[o["pos"] > w - 1]
        o["pos"] += lo - (w - 1)
        mine = got[(got["pos"] > lo) & (got["pos"] <= hi)]
        assert len(mine) >= 500 and np.array_equal(_rows(mine), _rows(o))
    # a shard with left context and a position offset == the same part of the whole scan
    lo, hi = (3 << 20) + 7, (4 << 20) + 3
    part, _ = _filter_scan(spm, ctx, text, ps, lo, hi, left_context=True, pos_offset=OFFSET, max_hits=1 << 22)
    sel = got[(got["pos"] > lo) & (got["pos"] <= hi)].copy()
    sel["pos"] += OFFSET
    assert len(sel) >= 10_000 and np.array_equal(part, sel)
