"""CPU: the builder of tests/dense_states.py against the product's own tables, and the regime the dense pass really runs in.

tests/cpp/dense_census (a host-only program over libspm_amd/csrc/index_build.hpp, explicit tuning, also under
AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program, run directly) builds a needle set and prints what its
filter_index holds: bucket_shift, the accept-all buckets, the full ones, the presence bits.  The builder predicts every one of
those numbers from the three hashes written again in NumPy; its decoy windows are checked class by class against a level-1b
look-up written from the rule; its texts against the CPU oracle.  The last test pins WHY the built sets are needed: the
needle sets the dense pass is made for (100 000 reads) have accept-all buckets, a bucket_shift far from 20 and a sixth of
the presence bits set -- a 700-needle set, which is what the other dense tests force, has none of that."""
import os
import subprocess

import numpy as np
import pytest

import dense_states as DS
from cpp_programs import LIB, build_cases

SEED_TEXT, SEED_PAT = 0x5EED0001, 0x5EED0002
N_KEYS = DS.N_KEYS
_sets = {}


def built(shift):
    """(KeySet, Decoys) of one shift: built once"""
    if shift not in _sets:
        _sets[shift] = DS.built_set(shift)
    return _sets[shift]


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    out = tmp_path_factory.mktemp("dense_census")
    exes = {}

    def run(needles, algo, k, dense, sanitize=False, threads=16):
        if sanitize not in exes:
            exes[sanitize] = build_cases("dense_census.cpp", out, std="c++17", include=[os.path.join(LIB, "csrc")],
                                         sanitize=sanitize, threads=True)
        needles = np.ascontiguousarray(needles, dtype=np.uint8)
        path = out / "set.bin"
        with open(path, "wb") as f:
            f.write(np.array([needles.shape[0], needles.shape[1], algo, k], dtype="<u4").tobytes())
            f.write(needles.tobytes())
        r = subprocess.run([str(exes[sanitize]), str(path), str(dense), str(threads)], capture_output=True, text=True, timeout=600)
        print(r.stdout, r.stderr)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        c = dict(line.split("=", 1) for line in r.stdout.splitlines())
        for name in ("accept_all", "full"):
            if name in c:
                c[name] = [int(x) for x in c[name].split(",") if x]
        return {a: b if isinstance(b, list) or "/" in b else int(b) for a, b in c.items()}

    return run


def _needles(spm, which, ks):
    return {"shiftor16": (spm.ALGO_SHIFTOR, DS.exact16(ks), 0), "horspool16": (spm.ALGO_HORSPOOL, DS.exact16(ks), 0),
            "myers64": (spm.ALGO_MYERS, DS.myers64(ks), 3)}[which]


def test_the_hashes_invert():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 32, 1000, dtype=np.uint64)
    assert np.array_equal(DS.key_of(DS.syms(keys)), keys)
    assert DS.syms(np.array([0x1B]))[0].tolist() == [3, 2, 1] + [0] * 13        # the first symbol lowest
    k = DS.with_bloom(DS.bloom(keys), keys >> 20)
    assert np.array_equal(k, keys)                                                # bits 20..31 and the presence bit fix the key
    for shift in (20, 18, 14):
        m = DS.bucket_members(0x5A5, shift)
        assert len(np.unique(m)) == 1 << shift and (DS.bucket(m, shift) == 0x5A5).all()
    assert [DS.shift_of(n) for n in (1, 8192, 8193, 16384, 16385, 32768, 400000)] == [20, 20, 19, 19, 18, 18, 14]
    assert int(DS.fp(0)) == 0x8000 and int(DS.fp(0xFFFFFFFF)) == 0x8000 | (0x7FFF ^ 0x7FFF ^ 0x1FF)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
@pytest.mark.parametrize("shift", [20, 18])
@pytest.mark.parametrize("which", ["shiftor16", "horspool16", "myers64"])
def test_the_rule_predicts_the_products_tables(spm, census, which, shift, sanitize):
    ks, _ = built(shift)
    algo, needles, k = _needles(spm, which, ks)
    c = census(needles, algo, k, dense=2, sanitize=sanitize, threads=1 if sanitize else 16)
    assert (c["rc"], c["passes"], c["dense"], c["hash_variant"]) == (0, 1, 1, 3)
    assert c["anchor_sixteenths"] == 16                 # every window is looked up
    assert c["keys"] == ks.n == N_KEYS[shift]           # one layout only: the needles' keys are the builder's
    assert c["bucket_shift"] == shift == DS.shift_of(ks.n) and c["buckets"] == 1 << (32 - shift)
    assert c["accept_all"] == [DS.BUCKET_OVER]          # exactly one bucket overflowed, and it is B
    assert c["full"] == [DS.BUCKET_FULL]                # B8: eight slots used, not overflowed
    assert c["largest_fill"] == DS.SLOTS
    assert c["presence_bits"] == len(np.unique(DS.bloom(ks.keys))) and c["presence_table"] == 1 << DS.BLOOM_BITS
    # the rule's own table says the same
    table = DS.bucket_table(ks.keys, shift)
    assert table[DS.BUCKET_OVER][-1] == DS.ACCEPT_ALL and DS.ACCEPT_ALL not in table[DS.BUCKET_FULL]
    assert table[DS.BUCKET_OVER][:7] == DS.fp(ks.keys[ks.groups["over"]][:7]).tolist()     # five `over` keys have no slot


def _level1b(table, shift, key):
    """what dense_drain decides for a queued window"""
    slots = table.get(int(DS.bucket(key, shift)), [])
    return int(DS.fp(key)) in slots or (len(slots) == DS.SLOTS and slots[-1] == DS.ACCEPT_ALL)


@pytest.mark.parametrize("shift", [20, 18])
def test_every_decoy_class_holds_its_property(shift):
    ks, D = built(shift)
    DS.check_decoys(ks, D)
    table = DS.bucket_table(ks.keys, shift)
    bits = set(DS.bloom(ks.keys).tolist())
    keys = set(ks.keys.tolist())
    assert all(_level1b(table, shift, k) for k in ks.keys)
    passes = {"bit_only": False, "accept_all": True, "fp_twin": True, "full_bucket_miss": False}
    for name, want in passes.items():
        d = getattr(D, name)
        assert len(d) >= DS.N_TWINS
        for x in d.tolist():
            assert x not in keys and int(DS.bloom(x)) in bits and _level1b(table, shift, x) == want, (name, hex(x))
    pairs = set(zip(DS.bucket(ks.keys, shift).tolist(), DS.fp(ks.keys).tolist()))
    for name in ("bit_only", "full_bucket_miss"):
        d = getattr(D, name)
        assert not (set(zip(DS.bucket(d, shift).tolist(), DS.fp(d).tolist())) & pairs)
    assert (DS.bucket(D.accept_all, shift) == DS.BUCKET_OVER).all() and (DS.bucket(D.full_bucket_miss, shift) == DS.BUCKET_FULL).all()
    assert len(set((ks.keys[ks.groups["fill"]] & 15).tolist())) == 16
    assert len(set(DS.fp(ks.keys[ks.groups["over"]]).tolist())) == 12 and len(set(DS.fp(ks.keys[ks.groups["full"]]).tolist())) == 8


@pytest.mark.parametrize("mode", ["exact16", "myers64"])
def test_lay_out(oracle, mode):
    ks, D = built(20)
    span = 8192
    lay = DS.lay_out(ks, D, mode, 1 << 18, span, seed=3)
    T = lay.text
    kinds = [(s.kind, s.f, s.exact_only) for s in lay.stretches]
    assert kinds[:6] == [("flood_aligned", 1.0, True), ("flood_aligned", 1.0, False), ("flood_ragged", 0.5, False),
                         ("flood_ragged", 0.125, False), ("sparse", 1 / 64, False), ("one_per_span", 0.0, False)]
    per = 1 if mode == "exact16" else 4
    for s in lay.stretches:
        assert s.begin % span == 0 and s.end % span == 0 and s.end - s.begin >= 2 * span
        n_dec = sum(s.decoys.values())
        surv = s.true_blocks + s.decoys["accept_all"] + s.decoys["fp_twin"]
        if s.kind == "one_per_span":
            assert s.trues == 2 and n_dec == 0
            continue
        assert s.trues * 64 >= s.blocks                                     # t >= 1/64
        assert abs(n_dec + (s.true_blocks if s.f == 1.0 else 0) - s.f * s.blocks) <= s.f * s.blocks / 8, (s.kind, n_dec)
        # survivors: far inside the default budget of a quarter of the SYMBOLS; the aligned flood carries more than an
        # eighth of its blocks so that a budget of 64 is spent in the middle of an 8 KiB span
        assert surv * 3 <= s.blocks if s.kind == "flood_aligned" else surv * 8 <= s.blocks, (s.kind, surv, s.blocks)
        if s.kind == "flood_aligned":
            assert s.end - s.begin >= 16384 and surv * span > 64 * 16 * s.blocks and s.decoys["bit_only"] * 2 > s.blocks
            assert all(s.decoys[c] > 0 for c in DS.DECOY_CLASSES)
    a, b = lay.stretches[0], lay.stretches[1]
    assert a.end == b.begin                                                  # one flood of four spans
    # what the stretches are for, by the kernel's rule: drains as (entries queued, batches, entries kept, at the span's end)
    for s in lay.stretches:
        for at in range(s.begin, s.end, span):
            drains = DS.queue_trace(T, ks, at, span)
            mid, end = [d for d in drains if not d[3]], [d for d in drains if d[3]]
            if s.kind == "flood_aligned" and s.exact_only:
                assert mid and mid[0][:3] == (DS.QUEUE_CAP, 3, 0)           # 64, 128, 192: three batches, nothing kept
                assert mode == "myers64" or all(d[:3] == (DS.QUEUE_CAP, 3, 0) for d in mid)
            elif s.kind == "flood_ragged" and s.f == 0.5:
                assert len(mid) >= 2 and all(d[1] == 2 and 0 < d[2] < 64 for d in mid)      # two batches, a remainder kept
            elif s.kind in ("sparse", "one_per_span"):
                assert not mid and len(end) == 1 and 0 < end[0][0] < 64      # emptied once, by a partial batch
            assert len(end) <= 1 and all(d[0] <= DS.QUEUE_CAP for d in drains)
    # a decoy block is no key
    keys = set(ks.keys.tolist())
    for at, name in lay.decoy_at:
        assert int(DS.key_of(T[at:at + 16])[0]) not in keys
    starts = {x[1] for x in lay.planted}
    beside = [name for at, name in lay.decoy_at if at + 16 in starts or any(at - 16 * per == x for x in starts)]
    assert {"accept_all", "fp_twin"} <= set(beside)
    # the planted occurrences, by the oracle on the text alone
    needles = DS.exact16(ks) if mode == "exact16" else DS.myers64(ks)
    special = 20 + DS.N_TWINS
    if mode == "exact16":
        assert {p for p, *_ in lay.planted} >= set(range(special))
        for p in sorted({p for p, *_ in lay.planted}):
            found = set(int(x) for x in oracle.naive_exact(T, needles[p]))
            assert found == {s for q, s, e, _ in lay.planted if q == p}
    else:
        hits = oracle.scan_multi(oracle.MYERS, T, list(needles), k=3, threads=16)
        rows = {(int(p), int(x)): int(s) for p, x, s in zip(hits["pattern"], hits["pos"], hits["score"])}
        for p, s, e, edits in lay.planted:
            assert rows.get((p, e), 99) == edits
        ends = {}
        for p, s, e, _ in lay.planted:
            ends.setdefault(p, []).append(e)
        extra = [(p, x) for (p, x) in rows if not any(abs(x - e) <= 3 for e in ends.get(p, []))]
        assert extra == []                                                   # nothing but the plants and their neighbourhood
        assert {p for p, *_ in lay.planted} >= set(range(special // 4))
        edited = [x for x in lay.planted if x[3] == 3]
        assert len(edited) * 2 > len(lay.planted)
    # the one_per_span plants touch the border from both sides
    s = next(s for s in lay.stretches if s.kind == "one_per_span")
    assert {(x[1], x[2]) for x in lay.planted if s.begin <= x[1] < s.end} == {(s.begin + span - 16 * per, s.begin + span),
                                                                             (s.begin + span, s.begin + span + 16 * per)}


@pytest.mark.parametrize("shift", [20, 18])
@pytest.mark.parametrize("mode", ["exact16", "myers64"])
def test_a_remainder_that_is_dropped_would_lose_a_hit(mode, shift):
    """The texts of tests/test_gpu_dense_states.py, by the kernel's rule: among the entries that a drain leaves in the queue
    are key windows of planted occurrences, in the ragged floods too -- a kernel that forgets the remainder loses their hits.
    (True occurrences come every 31 slots: with a period that divides a chunk they all sat in lanes the remainder never
    holds, and such a kernel passed.)"""
    ks, D = built(shift)
    lay = DS.case_layout(ks, D, mode, 8192)
    seeds = {s + 16 * j for p, s, e, edits in lay.planted for j in range((e - s) // 16)}
    keys = set(ks.keys.tolist())
    lost = {}
    for s in lay.stretches:
        kept = []
        for at in range(s.begin, s.end, 8192):
            DS.queue_trace(lay.text, ks, at, 8192, kept=kept)
        lost[s.kind] = lost.get(s.kind, 0) + sum(x in seeds and int(DS.key_of(lay.text[x:x + 16])[0]) in keys for x in set(kept))
    assert sum(lost.values()) >= 4 and (lost["flood_ragged"] >= 1 or mode == "exact16" and shift == 18), lost


def _reads(spm, n, L):
    """bench.py's C4 / reads100 needles: drawn from 8 Gi symbols of text, so no two reads overlap.  (Drawn from a text they
    cover twice over, 100 000 reads share keys: 12.5 % of the bits and no accept-all bucket.)"""
    return np.stack([spm.synth_pattern(SEED_TEXT, SEED_PAT, 1 << 33, p, L, 3)[0] for p in range(n)])


@pytest.mark.parametrize("L", [150, 100], ids=["c4", "reads100"])
def test_the_regime_of_real_read_sets(spm, census, L):
    """100 000 reads, k = 3, dense by itself: accept-all buckets, 14 .. 15 bits of bucket_shift, a sixth of the presence bits."""
    c = census(_reads(spm, 100000, L), spm.ALGO_MYERS, 3, dense=1)
    assert (c["rc"], c["passes"], c["dense"], c["hash_variant"]) == (0, 1, 1, 3)
    assert len(c["accept_all"]) >= 1 and c["bucket_shift"] <= 15 and c["presence_bits"] * 10 >= c["presence_table"]
    assert c["anchor_sixteenths"] <= 8 and c["largest_fill"] == DS.SLOTS


def test_a_small_forced_set_reaches_none_of_it(spm, census):
    c = census(_reads(spm, 700, 150), spm.ALGO_MYERS, 3, dense=2)
    assert (c["rc"], c["passes"], c["dense"], c["hash_variant"]) == (0, 1, 1, 3)
    assert c["accept_all"] == [] and c["bucket_shift"] == 20 and c["presence_bits"] * 100 < c["presence_table"]
