"""Key sets and texts that put the dense pass (libspm_amd/csrc/filter_dense.hpp: dense_group / dense_drain) into every state of
its presence bits, fingerprint buckets and per-wave queue (a helper module of tests/test_dense_states.py and
tests/test_gpu_dense_states.py, not a test file).

A needle of exactly 16 (k + 1) symbols has one seed layout only, so its keys are the test's to choose: a 16-symbol exact
needle is its own key, a 64-symbol Myers needle with k = 3 is four keys at offsets 0 / 16 / 32 / 48.  The three hashes of
filter_shared.hpp are written again here in NumPy and inverted: a key set with one overflowed ("accept-all") bucket B and
one full bucket B8, and 16-symbol windows that are NOT keys but pass level 1 (presence bit set) and then meet each state
of level 1b.  lay_out() plants them in a text in stretches that fill, half-fill and starve the queue.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

M32 = 0xFFFFFFFF
MUL = 0x9E3779B1                    # dense_bucket's multiplier (odd: invertible mod 2^32)
INV = pow(MUL, -1, 1 << 32)
BLOOM_BITS = 20                     # kDenseBloomBits
SLOTS = 8                           # kDenseSlots
ACCEPT_ALL = 0x7FFF                 # kDenseAcceptAll
QUEUE_CAP = 192                     # kDenseQueueCap
BUCKET_OVER, BUCKET_FULL = 0x5A5, 0x2C3     # B and B8
N_TWINS = 16
DECOY_CLASSES = ("bit_only", "accept_all", "fp_twin", "full_bucket_miss")
# the sets and texts of tests/test_gpu_dense_states.py (tests/test_dense_states.py checks the same ones on the CPU).  20 000
# needles: the oracle takes ~1.5 s on a quarter of a MiB and ~5 s on a whole one, so the text shrinks, not the set
N_KEYS = {20: 3000, 18: 20000}
N_TEXT = {20: 1 << 20, 18: 1 << 18}


# ---- the rule (filter_shared.hpp, index_tables.hpp build_bits_level1, index_types.hpp window_key) ----
def _u(key):
    return np.asarray(key, dtype=np.uint64) & M32


def bloom(key):
    """dense_bloom_index: the presence bit of a key"""
    k = _u(key)
    return (k ^ (k >> 13)) & ((1 << BLOOM_BITS) - 1)


def bucket(key, shift):
    """dense_bucket"""
    return ((_u(key) * MUL) & M32) >> shift


def fp(key):
    """dense_fp: 15 bits and the `used` bit"""
    k = _u(key)
    return 0x8000 | ((k ^ (k >> 15) ^ (k >> 23)) & 0x7FFF)


def shift_of(n_keys: int) -> int:
    """bucket_shift of a pass with n_keys keys: about two keys per bucket"""
    lg = 12
    while (1 << lg) * 2 < n_keys and lg < 24:
        lg += 1
    return 32 - lg


def bucket_members(b: int, shift: int):
    """all 2^shift keys of bucket b"""
    r = np.arange(1 << shift, dtype=np.uint64)
    return (((np.uint64(b) << np.uint64(shift)) | r) * INV) & M32


def with_bloom(h, high12):
    """the key whose presence bit is h and whose bits 20..31 are high12 (key ^ key >> 13 leaves bits 19..31 as they are)"""
    h32 = (_u(high12) << 20) | _u(h)
    k = h32
    for _ in range(3):
        k = h32 ^ (k >> 13)
    return k


def syms(keys):
    """keys -> rows of 16 symbols: symbol i at bits 2 i, the first symbol lowest"""
    k = _u(keys).reshape(-1, 1)
    return ((k >> (2 * np.arange(16, dtype=np.uint64))) & 3).astype(np.uint8)


def key_of(rows):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 16)
    return (rows << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1) & M32


def window_keys(T):
    """the keys of all 16-symbol windows of T: window t = T[t:t + 16]"""
    T = np.asarray(T, dtype=np.uint64)
    k = np.zeros(max(len(T) - 15, 0), dtype=np.uint64)
    for i in range(16):
        k |= T[i:len(T) - 15 + i] << np.uint64(2 * i)
    return k


def bucket_table(keys, shift):
    """build_bits_level1's buckets, written again: {bucket: [slots]}; a bucket that met a ninth fingerprint ends in
    ACCEPT_ALL.  Keys are inserted in list order, as the build inserts them in needle order."""
    table = {}
    for b, f in zip(bucket(keys, shift).tolist(), fp(keys).tolist()):
        s = table.setdefault(b, [])
        if f in s:
            continue
        if len(s) < SLOTS:
            s.append(f)
        else:
            s[SLOTS - 1] = ACCEPT_ALL
    return table


# ---- key sets ----
@dataclass
class KeySet:
    keys: np.ndarray                # uint64 values < 2^32, all distinct; order = needle order
    shift: int
    groups: dict                    # name -> indices into keys: over, full, twin, fill
    twins: list = field(default_factory=list)   # (decoy, K1, K2): presence bit of K1, bucket and fingerprint of K2

    @property
    def n(self):
        return len(self.keys)


def key_set(seed: int, n_fill: int, shift: int) -> KeySet:
    """12 keys with 12 fingerprints in bucket B (`over`: it overflows), 8 keys with 8 fingerprints in B8 (`full`), N_TWINS
    keys made to share (bucket, fingerprint) with a non-key window (`twin`), and n_fill random keys elsewhere (`fill`) that
    between them begin with all 16 dimers and leave every other bucket with fewer than 8 fingerprints."""
    rng = np.random.default_rng(seed)
    B, B8 = BUCKET_OVER, BUCKET_FULL

    def distinct_fp(b, n):
        m = rng.permutation(bucket_members(b, shift))
        _, first = np.unique(fp(m), return_index=True)
        return m[np.sort(first)[:n]]

    over, full = distinct_fp(B, 12), distinct_fp(B8, 8)
    cand = np.unique(rng.integers(0, 1 << 32, n_fill + n_fill // 8 + 64, dtype=np.uint64))
    cand = rng.permutation(cand)
    bk = bucket(cand, shift)
    cand = cand[(bk != B) & (bk != B8)]
    # no accident may fill a third bucket: drop what would put more than five keys into one (the twins add at most one each)
    bk = bucket(cand, shift)
    order = np.argsort(bk, kind="stable")
    rank = np.empty(len(cand), dtype=np.int64)
    sb = bk[order]
    starts = np.r_[0, np.flatnonzero(sb[1:] != sb[:-1]) + 1]
    rank[order] = np.arange(len(cand)) - np.repeat(starts, np.diff(np.r_[starts, len(cand)]))
    fill = cand[rank < 5][:n_fill]
    assert len(fill) == n_fill and len(set((fill & 15).tolist())) == 16
    taken = set(fill.tolist()) | set(over.tolist()) | set(full.tolist())
    twins = []
    while len(twins) < N_TWINS:
        k1 = int(fill[int(rng.integers(0, n_fill))])
        d = int(with_bloom(bloom(k1), rng.integers(0, 1 << 12)))
        b = int(bucket(d, shift))
        if d in taken or b in (B, B8) or any(b == int(bucket(t[2], shift)) for t in twins):
            continue
        m = bucket_members(b, shift)
        m = m[(fp(m) == fp(d)) & (m != d)]
        m = [int(x) for x in m if int(x) not in taken]
        if not m:
            continue
        k2 = m[int(rng.integers(0, len(m)))]
        taken.add(k2)
        twins.append((d, k1, k2))
    keys = np.concatenate([over, full, np.array([t[2] for t in twins], dtype=np.uint64), fill])
    assert len(np.unique(keys)) == len(keys) and shift_of(len(keys)) == shift, (len(keys), shift)
    edges = np.cumsum([0, 12, 8, N_TWINS, n_fill])
    groups = {name: np.arange(edges[i], edges[i + 1]) for i, name in enumerate(("over", "full", "twin", "fill"))}
    ks = KeySet(keys, shift, groups, twins)
    table = bucket_table(keys, shift)
    assert [b for b, s in table.items() if s[-1] == ACCEPT_ALL] == [B]
    assert [b for b, s in table.items() if len(s) == SLOTS and s[-1] != ACCEPT_ALL] == [B8]
    return ks


@dataclass
class Decoys:
    bit_only: np.ndarray
    accept_all: np.ndarray
    fp_twin: np.ndarray
    full_bucket_miss: np.ndarray


def decoys(ks: KeySet, seed: int = 1, n_each: int = 256) -> Decoys:
    """Four classes of 16-symbol windows that are not keys and whose presence bit IS set (each checked by the rule above):
    bit_only          bucket neither B nor B8, no key shares (bucket, fingerprint): rejected at level 1b
    accept_all        bucket B: passes level 1b through the overflow marker; absent from the directory
    fp_twin           (bucket, fingerprint) of a key K2: passes level 1b by collision; absent from the directory
    full_bucket_miss  bucket B8, fingerprint not among its eight: rejected although the bucket is full"""
    rng = np.random.default_rng(seed)
    keys, shift = ks.keys, ks.shift
    bits = np.zeros(1 << BLOOM_BITS, dtype=bool)
    bits[bloom(keys)] = True
    pair = np.unique((bucket(keys, shift) << 16) | fp(keys))

    def fresh(c):
        c = c[bits[bloom(c)] & ~np.isin(c, keys)]
        return rng.permutation(np.unique(c))[:n_each]

    m = bucket_members(BUCKET_OVER, shift)
    accept_all = fresh(m)
    m = bucket_members(BUCKET_FULL, shift)
    full_miss = fresh(m[~np.isin(fp(m), fp(keys[ks.groups["full"]]))])
    c = with_bloom(bloom(keys[rng.integers(0, len(keys), 4 * n_each)]), rng.integers(0, 1 << 12, 4 * n_each))
    b = bucket(c, shift)
    bit_only = fresh(c[(b != BUCKET_OVER) & (b != BUCKET_FULL) & ~np.isin((b << 16) | fp(c), pair)])
    D = Decoys(bit_only, accept_all, np.array([t[0] for t in ks.twins], dtype=np.uint64), full_miss)
    check_decoys(ks, D)
    return D


def check_decoys(ks: KeySet, D: Decoys):
    keys, shift = ks.keys, ks.shift
    key_bits = set(bloom(keys).tolist())
    key_set_ = set(keys.tolist())
    pair = set(((bucket(keys, shift) << 16) | fp(keys)).tolist())
    full_fp = set(fp(keys[ks.groups["full"]]).tolist())
    for name in DECOY_CLASSES:
        d = getattr(D, name)
        assert len(d) >= 8 and len(np.unique(d)) == len(d), name
        assert not (set(d.tolist()) & key_set_), name
        assert set(bloom(d).tolist()) <= key_bits, name
    b = bucket(D.bit_only, shift)
    assert not np.isin(b, (BUCKET_OVER, BUCKET_FULL)).any() and not (set(((b << 16) | fp(D.bit_only)).tolist()) & pair)
    assert (bucket(D.accept_all, shift) == BUCKET_OVER).all()
    assert (bucket(D.full_bucket_miss, shift) == BUCKET_FULL).all() and not (set(fp(D.full_bucket_miss).tolist()) & full_fp)
    for d, k1, k2 in ks.twins:
        assert d not in key_set_ and k1 in key_set_ and k2 in key_set_ and k1 != k2
        assert bloom(d) == bloom(k1) and bucket(d, shift) == bucket(k2, shift) and fp(d) == fp(k2)
        assert int(bucket(d, shift)) not in (BUCKET_OVER, BUCKET_FULL)


# ---- needle sets from one key list ----
def exact16(ks: KeySet):
    """Shift-Or / Horspool: one key per needle -> (n, 16) symbols"""
    return syms(ks.keys)


def myers64(ks: KeySet):
    """Myers, k = 3: four keys per needle, the groups kept together (three needles carry the 12 `over` keys)"""
    assert ks.n % 4 == 0
    return syms(ks.keys).reshape(-1, 64)


# ---- texts ----
# One stretch: (kind, spans, slot symbols, a decoy every .. slots, a true occurrence every .. slots, phase, exact copies
# only, one accept_all and one fp_twin decoy per .. decoys).  31 slots between true occurrences: a period that divided the
# 1024 symbols of a chunk would put every one of them into the same lanes, and into the same places of the queue.
PLAN = (
    ("flood_aligned", 2, 16, 1, 31, "zero", True, 16),      # every push round queues 64 entries: 64, 128, 192, drain 3
    ("flood_aligned", 2, 16, 1, 31, "zero", False, 16),     # ... and rounds of 61 .. 63 where an edited piece sits (myers64)
    ("flood_ragged", 2, 32, 1, 31, "random", False, 64),    # f = 1/2: rounds of 1 .. 63 lanes, drains with a remainder
    ("flood_ragged", 2, 32, 4, 31, "random", False, 64),    # f = 1/8
    ("sparse", 3, 32, 32, 31, "random", False, 64),         # f = 1/64: emptied at the span's end by a partial batch
    ("one_per_span", 3, 0, 0, 0, "zero", False, 0),         # one occurrence flush before a span border, one flush behind it
)
STRETCH_F = {("flood_aligned", 1): 1.0, ("flood_ragged", 1): 0.5, ("flood_ragged", 4): 0.125, ("sparse", 32): 1 / 64}


@dataclass
class Stretch:
    kind: str
    begin: int
    end: int
    f: float                        # the share of blocks that was to hold a decoy
    exact_only: bool
    decoys: dict                    # class -> count
    trues: int = 0
    true_blocks: int = 0

    @property
    def blocks(self):
        return (self.end - self.begin) // 16


@dataclass
class Layout:
    text: np.ndarray
    planted: list                   # (pattern, start, end, edits): the occurrence text[start:end) of needle `pattern`
    stretches: list
    decoy_at: list                  # (start, class)
    span: int


def lay_out(ks: KeySet, D: Decoys, mode: str, n_text: int, span: int, seed: int = 0, plan=PLAN) -> Layout:
    """A text of n_text random symbols with the stretches of `plan`, each beginning at a span border, repeated (with other
    decoys, keys and phases) while they fit.  mode: "exact16" | "myers64"."""
    assert mode in ("exact16", "myers64") and span % 1024 == 0
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 4, n_text, dtype=np.uint8)
    needles = exact16(ks) if mode == "exact16" else myers64(ks)
    per, L = (1, 16) if mode == "exact16" else (4, 64)
    n_needles = len(needles)
    # what is planted, in turn: every key of the three special groups as the intact seed, then some of the fill
    special = n_needles - len(ks.groups["fill"]) // per
    turn = [(p, j) for p in range(special) for j in range(per)]
    turn += [(int(p), int(j)) for p, j in zip(rng.integers(special, n_needles, 27), rng.integers(0, per, 27))]
    assert len(turn) % 8 == 7           # (every turn is in time the edited one: an exact copy comes every eighth time)
    planted, stretches, decoy_at = [], [], []
    state = {"true": 0, "decoy": 0, "beside": 0}
    dsyms = {name: syms(getattr(D, name)) for name in DECOY_CLASSES}
    bits = np.zeros(1 << BLOOM_BITS, dtype=bool)
    bits[bloom(ks.keys)] = True

    def put_true(at, exact_only, piece=None, clean=False):
        for _ in range(len(turn) if clean else 1):
            p, j = turn[state["true"] % len(turn)]
            j = j if piece is None else piece
            state["true"] += 1
            occ = needles[p].copy()
            T[at:at + L] = occ
            # (an aligned flood of exact copies: a needle whose own pieces straddle into the queue waits for its next turn)
            if not clean or not any(dirty(at + 16 * q + 1, at + 16 * q + 16) for q in range(per - 1)):
                break
        edits = 0
        if mode == "myers64" and not exact_only and state["true"] % 8 != 0:     # (an exact copy now and then)
            for q in range(4):
                if q != j:
                    i = 16 * q + int(rng.integers(0, 16))
                    occ[i] = (occ[i] + int(rng.integers(1, 4))) & 3
                    edits += 1
        T[at:at + L] = occ
        planted.append((p, at, at + L, edits))

    def dirty(lo, hi):
        """a window that starts in [lo, hi) has its presence bit set"""
        return bool(bits[bloom(window_keys(T[lo:hi + 15]))].any())

    def pick_decoy(at, name, until):
        """The class's next decoy at `at`.  In an aligned flood the windows that straddle two blocks must stay out of the
        queue, or no push round queues exactly 64: the next one that leaves the windows starting in (at - 16, until) without
        a presence bit (the blocks' own windows apart)."""
        rows = dsyms[name]
        for _ in range(len(rows) if until else 1):
            T[at:at + 16] = rows[state["decoy"] % len(rows)]
            state["decoy"] += 1
            if not until or not (dirty(at - 15, at) or dirty(at + 1, until)):
                break

    def put_decoy(at, st, name, clean=False):
        pick_decoy(at, name, at + 1 if clean else 0)
        st.decoys[name] += 1
        decoy_at.append((at, name))

    at_span = 1
    n_spans = n_text // span - 1            # (the first and the last span stay random)
    rep = 0
    while at_span + sum(s[1] for s in plan) <= n_spans:
        for kind, spans, slot, d_every, t_every, phase, exact_only, surv_every in plan:
            s0, s1 = at_span * span, (at_span + spans) * span
            at_span += spans
            st = Stretch(kind, s0, s1, STRETCH_F.get((kind, d_every), 0.0), exact_only, {c: 0 for c in DECOY_CLASSES})
            stretches.append(st)
            if kind == "one_per_span":
                put_true(s0 + span - L, False, piece=per - 1)       # its intact seed is the last block before the border
                put_true(s0 + span, False, piece=0)                 # ... the first block behind it
                st.trues, st.true_blocks = 2, 2 * per
                continue
            flood = kind.startswith("flood")
            busy, after_true, n_dec = s0, False, 0
            for j in range((s1 - s0) // slot):
                a = s0 + j * slot
                if a < busy:
                    continue
                ph = 0 if phase == "zero" else int(rng.integers(0, 16))
                if j % t_every == t_every // 2 + 1 and a + ph + L <= s1:
                    put_true(a + ph, exact_only, clean=exact_only and kind == "flood_aligned")
                    if kind == "flood_aligned" and decoy_at and decoy_at[-1][0] == a - 16 and dirty(a - 15, a):
                        pick_decoy(a - 16, decoy_at[-1][1], a)      # (the decoy in front of it: one that suits both sides)
                    st.trues += 1
                    st.true_blocks += per
                    busy = a + -(-(ph + L) // slot) * slot
                    after_true = True
                    continue
                if j % d_every != 0:
                    after_true = False
                    continue
                before_true = (j + 1) % t_every == t_every // 2 + 1
                if flood and (after_true or before_true):       # accept_all / fp_twin directly beside a true occurrence
                    name = ("accept_all", "fp_twin")[state["beside"] % 2]
                    state["beside"] += 1
                elif n_dec % surv_every == 3:
                    name = "accept_all"
                elif n_dec % surv_every == surv_every // 2 + 3:
                    name = "fp_twin"
                elif n_dec % 8 == 5:
                    name = "full_bucket_miss"
                else:
                    name = "bit_only"
                n_dec += 1
                after_true = False
                put_decoy(a + ph, st, name, clean=kind == "flood_aligned")
        rep += 1
    assert rep >= 1, "the text holds no whole plan"
    return Layout(T, planted, stretches, decoy_at, span)


# ---- the queue, by the kernel's rule ----
def queue_trace(T, ks: KeySet, begin: int, span: int, unroll: int = 4, kept=None):
    """What the per-wave queue of dense_group / dense_drain does over the span [begin, begin + span) of a set whose anchors
    are all 16 dimers: the drains as (entries queued, batches taken, entries kept, at the span's end).  A lane owns the 16
    windows that start in (L - 16, L], L its first symbol of a chunk; the chunks of a group are taken in pairs, a lane's
    positives of a pair one per push round (first chunk before second, window by window), the lanes of a round in lane
    order; after a round the wave takes the whole batches from the queue's top once more than QUEUE_CAP - 64 entries wait,
    and everything at the span's end.  kept: a list that receives the window starts of the entries such a drain leaves."""
    bits = np.zeros(1 << BLOOM_BITS, dtype=bool)
    bits[bloom(ks.keys)] = True
    assert begin >= 16 and span % (1024 * unroll) == 0 and begin + span <= len(T)
    pos = bits[bloom(window_keys(T[begin - 15:begin + span + 15]))][:span]      # pos[i]: the window starting at begin - 15 + i
    pairs = pos.reshape(-1, 2, 64, 16)                                           # [pair of chunks][chunk][lane][window]
    queue, drains = [], []
    for pi, pair in enumerate(pairs):
        lanes = []
        for lane in range(64):
            u, d = np.nonzero(pair[:, lane, :])
            order = np.argsort(2 * d + u, kind="stable")
            lanes.append((begin - 15 + (2 * pi + u[order]) * 1024 + lane * 16 + d[order]).tolist())
        for r in range(max(len(x) for x in lanes)):
            queue += [x[r] for x in lanes if len(x) > r]
            assert len(queue) <= QUEUE_CAP
            if len(queue) > QUEUE_CAP - 64:
                left = len(queue) & 63
                drains.append((len(queue), len(queue) >> 6, left, False))
                queue = queue[:left]
                if kept is not None:
                    kept += queue
    if queue:
        drains.append((len(queue), (len(queue) + 63) >> 6, 0, True))
    return drains


def built_set(shift: int):
    """(KeySet, Decoys) of N_KEYS[shift] keys"""
    ks = key_set(1000 + shift, N_KEYS[shift] - 20 - N_TWINS, shift)
    return ks, decoys(ks, seed=shift)


def case_layout(ks: KeySet, D: Decoys, mode: str, span: int) -> Layout:
    return lay_out(ks, D, mode, N_TEXT[ks.shift], span, seed=ks.shift + len(mode))
