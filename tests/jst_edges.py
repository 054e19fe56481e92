"""Hand-made pan-genome trees for the journaled-sequence search (a helper module of tests/test_jst_edges.py and
tests/test_gpu_jst_edges.py, not a test file).

The search's contract is the union over haplotypes of a linear scan of each materialised haplotype.  The random trees of
tests/test_gpu_jst.py keep their alleles on a grid: two never touch, none sits at either end of the reference or on a block
border, no block holds many.  The builders here put alleles exactly there -- at position 0, at the last position and behind
it (pos == n_ref), on a block border, inside and across one another on disjoint haplotypes, back to back on one haplotype,
320 in a row -- and cut needles that end at, just behind and across every one of them, so that a (block, haplotype) cell
that loses a symbol loses a record.  The builders call nothing of the library: trees, haplotypes and journals come from
_make_tree / _apply / Journal (tests/test_jst_project.py, tests/test_gpu_jst.py).  Only expected() and touching_case() at
the end take the library, for the per-haplotype scans and for the fuzz case that scripts/fuzz_jst.py shares with the tests.
"""
from __future__ import annotations

import numpy as np

from test_gpu_jst import _apply, _expected, _got, _needles_from
from test_jst_project import _edit, _hap, _make_tree

N_REF = 4096
BORDER = 1024        # a border of every block length the GPU tests index with, but 1000
CHAIN = 2600         # where the chain of touching alleles on one haplotype starts
STRETCH = (3092, 3412)   # 320 SNPs on consecutive positions: more alleles in one block than a signature's bit set holds
BLOCKS = (64, 256, 512, 1000, 4096, 0)
ALLELE_DTYPE = [("pos", "<u8"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("alt_off", "<u8")]


# ---------------------------------------------------------------------------------------------------------------------
# the rule of spm_hip.h
# ---------------------------------------------------------------------------------------------------------------------
def carriers(cov, i):
    """the haplotypes that carry allele i"""
    return [64 * w + b for w in range(cov.shape[1]) for b in range(64) if (int(cov[i, w]) >> b) & 1]


def legal(n_ref, alleles, cov):
    """The allele-table rule of spm_hip.h, transcribed: sorted by position, no position behind n_ref, and two alleles
    whose reference ranges overlap (after ref_len is clamped to the reference) share no haplotype; the table order
    breaks ties, so an allele that STARTS where an earlier one ends is free."""
    pos = alleles["pos"].astype(np.int64)
    if np.any(pos > n_ref) or np.any(np.diff(pos) < 0):
        return False
    end = pos + np.minimum(alleles["ref_len"].astype(np.int64), n_ref - pos)
    for i in range(len(pos)):
        j = i + 1
        while j < len(pos) and pos[j] < end[i]:
            if np.any(cov[i] & cov[j]):
                return False
            j += 1
    return True


def table(rows, n_hap):
    """(alleles, pool, cov) of rows (pos, ref_len, alt, haplotypes) in the order given"""
    cw = (n_hap + 63) // 64
    al = np.zeros(len(rows), dtype=ALLELE_DTYPE)
    cov = np.zeros((len(rows), cw), dtype=np.uint64)
    pool, off = [], 0
    for i, (pos, rl, alt, hs) in enumerate(rows):
        al[i] = (pos, rl, len(alt), off)
        pool.append(np.asarray(alt, np.uint8))
        off += len(alt)
        for h in hs:
            cov[i, h >> 6] |= np.uint64(1) << np.uint64(h & 63)
    return al, (np.concatenate(pool) if pool else np.zeros(0, np.uint8)), cov


# ---------------------------------------------------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------------------------------------------------
def _tree(seed, n_ref, n_hap, labelled):
    """labelled: (label, pos, ref_len, alt, haplotypes).  A dict of _make_tree, plus "labels" (one per table row) and "plant"
    (the rows needles are cut at).  An alt symbol that would equal the reference symbol it replaces is bumped."""
    ref = np.random.default_rng(seed).integers(0, 4, n_ref, dtype=np.uint8)      # (_make_tree's first draw)
    extra = []
    for _label, pos, rl, alt, hs in labelled:
        alt = np.array(alt, dtype=np.uint8)
        for x in range(min(rl, len(alt), n_ref - pos)):
            if alt[x] == ref[pos + x]:
                alt[x] = (int(alt[x]) + 1) & 3
        extra.append((pos, rl, alt, tuple(hs)))
    t = _make_tree(seed, n_ref, n_hap, 8, 0, extra=extra)
    assert np.array_equal(t["ref"], ref)
    order = sorted(range(len(extra)), key=lambda i: extra[i][0])                 # (stable, as _make_tree sorts)
    t["labels"] = [labelled[i][0] for i in order]
    for row, i in enumerate(order):
        assert int(t["alleles"][row]["pos"]) == extra[i][0] and carriers(t["cov"], row) == sorted(extra[i][3])
    t["plant"] = list(range(len(order)))
    return t


def edge_tree():
    """8 haplotypes over 4096 reference symbols; every entry is legal (test_jst_edges asserts it)"""
    rng = np.random.default_rng(4096)
    n, B, p = N_REF, BORDER, CHAIN

    def alt(k):
        return rng.integers(0, 4, k, dtype=np.uint8)

    rows = [
        # the ends of the reference
        ("insertion in front of the reference", 0, 0, alt(3), (0,)),
        ("deletion of the first 300", 0, 300, alt(0), (1,)),
        ("insertion behind the last symbol", n, 0, alt(5), (2,)),
        ("deletion to the end, ref_len beyond it", n - 40, 1000, alt(0), (3,)),
        ("SNP at the last position", n - 1, 1, alt(1), (4,)),
        # on the border B
        ("insertion on the border", B, 0, alt(4), (0,)),
        ("SNP before the border", B - 1, 1, alt(1), (1,)),
        ("SNP on the border", B, 1, alt(1), (2,)),
        ("deletion across the border", B - 3, 5, alt(0), (3,)),
        ("deletion ending on the border", B - 5, 5, alt(0), (4,)),
        ("deletion starting on the border", B, 5, alt(0), (5,)),
        # overlap on disjoint haplotypes
        ("deletion of 700", 1500, 700, alt(0), (0,)),
        ("SNP inside the deletion", 1600, 1, alt(1), (1,)),
        ("insertion inside the deletion", 1700, 0, alt(6), (2,)),
        ("deletion inside the deletion", 1650, 10, alt(0), (3,)),
        ("nested deletion of 600", 1550, 600, alt(0), (4,)),
        ("deletion overlapping the end of the 700", 2100, 200, alt(0), (5,)),
        # a chain on one haplotype: a left context passes through all of them
        ("chain: SNP", p, 1, alt(1), (6,)),
        ("chain: SNP behind the SNP", p + 1, 1, alt(1), (6,)),
        ("chain: deletion", p + 2, 4, alt(0), (6,)),
        ("chain: insertion, then SNP at its position", p + 6, 0, alt(3), (6,)),
        ("chain: SNP at the insertion's position", p + 6, 1, alt(1), (6,)),
        ("chain: first of two insertions at one position", p + 10, 0, alt(2), (6,)),
        ("chain: second of two insertions at one position", p + 10, 0, alt(2), (6,)),
        ("chain: replacement 3 -> 7", p + 12, 3, alt(7), (6,)),
        # an allele that changes nothing
        ("empty allele", p + 20, 0, alt(0), (7,)),
    ]
    n_hand = len(rows)
    for q in range(*STRETCH):
        bits = rng.random(8) < 0.5
        bits[int(rng.integers(0, 8))] = True
        # haplotypes 6 and 7 agree on the last 256 SNPs and differ on every one before: a signature that dropped the alleles
        # beyond its bit set, instead of refusing to share, would take their contexts of a 512 block for one
        bits[7] = bits[6] if q >= STRETCH[1] - 256 else not bits[6]
        if not bits.any():
            bits[0] = True
        rows.append((f"stretch SNP {q}", q, 1, alt(1), tuple(int(h) for h in np.nonzero(bits)[0])))
    t = _tree(4097, n, 8, rows)
    stretch = [i for i, lab in enumerate(t["labels"]) if lab.startswith("stretch")]
    assert len(stretch) == 320 and len(t["labels"]) == n_hand + 320
    t["plant"] = [i for i, lab in enumerate(t["labels"]) if not lab.startswith("stretch")] + stretch[::40]
    return t


DEG_REF = 2048


def degenerate_tree():
    """haplotype 0 has no symbol, haplotype 1 has 30 (fewer than any needle), haplotype 2 is the reference"""
    z = np.zeros(0, np.uint8)
    return _tree(2049, DEG_REF, 3, [("all deleted", 0, DEG_REF, z, (0,)),
                                    ("deletion of the first 1000", 0, 1000, z, (1,)),
                                    ("deletion of all but 20 of the rest", 1010, 1018, z, (1,))])


def deleted_tree():
    """one haplotype, wholly deleted: a tree without a single context"""
    return _tree(2050, DEG_REF, 1, [("all deleted", 0, DEG_REF, np.zeros(0, np.uint8), (0,))])


# The 96-symbol, 3-haplotype tree of tests/cpp/jst_walk_core_cases.cpp (edge_tree(96, 3)): the same formula for the reference
# and the same table, written out in both places.  WALK_STATS is what that program computes for block length 16 and window 8
# from the brute-force haplotypes and the host-side walk, and asserts; tests/test_gpu_jst_edges.py asserts it of the device.
WALK_REF, WALK_BLOCK, WALK_WINDOW = 96, 16, 8
WALK_ROWS = [(0, 0, [3, 2, 1], (0,)), (0, 3, [], (1,)), (10, 1, [2], (0,)), (15, 34, [], (2,)), (28, 8, [], (1,)),
             (30, 4, [], (0,)), (34, 1, [1], (0,)), (46, 0, [0, 1, 2, 3] * 3, (1,)), (60, 4, [], (1,)),
             (64, 0, [0, 1, 2, 3], (1,)), (64, 1, [2], (1,)), (64, 6, [], (2,)), (70, 0, [1, 1], (2,)), (78, 5, [], (2,)),
             (92, 14, [], (2,)), (95, 1, [0], (0, 1)), (96, 0, [2, 2, 0, 1, 3], (0, 1)), (96, 0, [3], (2,))]
WALK_STATS = {"contexts": 16, "unique_contexts": 15, "context_symbols": 315, "haplotype_symbols": 252}


def walk_tree():
    """(ref, alleles, pool, cov, n_hap) of the tree above"""
    ref = np.array([((i * 2654435761) & 0xFFFFFFFF) >> 30 for i in range(WALK_REF)], dtype=np.uint8)
    return (ref,) + table(WALK_ROWS, 3) + (3,)


WIDE_HAP = 1030
WIDE_SITE = 2200    # no other allele within 100 positions


def wide_tree():
    """1030 haplotypes = two haplotype groups, the second of 6; rows of 1030 context ids start on and off 16-byte
    boundaries.  The grid alleles draw their coverage from three random halves and their complements, so that the
    haplotypes fall into a few dozen distinct coverage columns (columns())."""
    rng = np.random.default_rng(1030)
    everyone = set(range(WIDE_HAP))
    halves = [set(int(h) for h in np.nonzero(rng.random(WIDE_HAP) < 0.5)[0]) for _ in range(3)]

    def alt(k):
        return rng.integers(0, 4, k, dtype=np.uint8)

    rows = [("site: first allele", WIDE_SITE, 1, [0], (63, 1023)),
            ("site: second allele", WIDE_SITE, 1, [0], (64, 1024)),
            ("carried by the last haplotype alone", 3000, 0, alt(4), (WIDE_HAP - 1,)),
            ("carried by all but one", 1000, 2, alt(0), sorted(everyone - {512}))]
    for j in range(12):
        half = halves[j % 3] if (j // 3) % 2 == 0 else everyone - halves[j % 3]
        rl, al = [(1, 1), (0, 5), (7, 0), (3, 6)][j % 4]
        rows.append((f"grid {j}", 150 + 310 * j, rl, alt(al), sorted(half)))
    t = _tree(1031, N_REF, WIDE_HAP, rows)
    # the two alleles of the site spell different symbols (both differ from the reference)
    a, b = [i for i, lab in enumerate(t["labels"]) if lab.startswith("site")]
    r = int(t["ref"][WIDE_SITE])
    t["pool"][int(t["alleles"][a]["alt_off"])] = (r + 1) & 3
    t["pool"][int(t["alleles"][b]["alt_off"])] = (r + 2) & 3
    return t


WIDE_SPECIAL = (0, 63, 64, 512, 1023, 1024, WIDE_HAP - 1)


def wide_who(_i, hs):
    """the carriers needles are cut at on the wide tree: the first, the last, and the haplotypes around the word and group
    borders (all carriers would be a thousand needles per allele)"""
    return sorted({hs[0], hs[-1]} | (set(hs) & set(WIDE_SPECIAL)))


def site_differences(t, needles, plants, k, records_of):
    """The two-allele site of the wide tree: a needle cut ACROSS the site on a carrier of one allele is found on the carrier
    of the other allele one error worse, or not at all.  records_of(h) -> {(pos, pattern): score}.  Returns how many
    needles were compared."""
    a, b = [i for i, lab in enumerate(t["labels"]) if lab.startswith("site")]
    n = 0
    for mine, other, i in ((63, 64, a), (64, 63, b), (1023, 1024, a), (1024, 1023, b)):
        x0, _x1 = allele_span(t, i, mine)
        for h, pos, p in planted_records(needles, plants, k):
            e = pos if k else pos + len(needles[p])
            if h == mine and e - len(needles[p]) + k < x0 < e - k:
                n += 1
                assert records_of(mine)[(pos, p)] <= k
                assert records_of(other).get((pos, p), k + 1) > records_of(mine)[(pos, p)], (mine, other, pos, p)
    return n


def columns(t):
    """{coverage column: its haplotypes}: haplotypes with equal columns are the same sequence"""
    n_hap = t["n_hap"]
    bits = np.zeros((len(t["alleles"]), n_hap), dtype=bool)
    for i in range(len(t["alleles"])):
        bits[i, carriers(t["cov"], i)] = True
    out = {}
    for h in range(n_hap):
        out.setdefault(bits[:, h].tobytes(), []).append(h)
    return out


def haplotypes(t, hs=None):
    return [_hap(t, h)[0] for h in (range(t["n_hap"]) if hs is None else hs)]


# ---------------------------------------------------------------------------------------------------------------------
# needles
# ---------------------------------------------------------------------------------------------------------------------
def allele_span(t, i, h):
    """(x0, x1) in haplotype h's coordinates: the first symbol at or behind allele i, and the end of its alt"""
    _hp, J = _hap(t, h)
    x0 = int(np.searchsorted(J.org, int(t["alleles"][i]["pos"])))
    return x0, x0 + int(t["alleles"][i]["alt_len"])


def plant_ends(t, i, h, L):
    """the exclusive ends needles are cut at for allele i on haplotype h: at the allele, one behind, at the end of the alt,
    one behind, and half a needle behind (the needle spans the allele), clamped to [L, len(hap)]"""
    x0, x1 = allele_span(t, i, h)
    n = len(_hap(t, h)[0])
    return [min(max(e, L), n) for e in (x0, x0 + 1, x1, x1 + 1, x0 + L // 2)]


def needles_at(t, L, k, who=None, seed=5):
    """(needles, plants): plants[p] = (haplotype, exclusive end) needle p was cut at.  who(i, carriers) -> the carriers
    to cut at (default: all of them).  k == 0: the needles are hap[e - L : e].  k > 0: one substitution at index 7; every
    third needle instead carries the edits of test_jst_project._edit -- an insertion and / or a deletion -- applied to the
    REVERSED stretch that ends at e, so that the needle stays within k edits of a suffix of hap[: e] and e stays an end."""
    rng = np.random.default_rng(seed)
    seen, cuts = set(), []

    def cut(h, e):
        if (h, e) not in seen and len(_hap(t, h)[0]) >= L:
            seen.add((h, e))
            cuts.append((h, e))

    for i in t["plant"]:
        hs = carriers(t["cov"], i)
        for h in (hs if who is None else who(i, hs)):
            if len(_hap(t, h)[0]) >= L:
                for e in plant_ends(t, i, h, L):
                    cut(h, e)
    for h in range(t["n_hap"]) if who is None else sorted({h for h, _e in cuts}):
        cut(h, L)
        cut(h, len(_hap(t, h)[0]))
    needles = []
    for p, (h, e) in enumerate(cuts):
        hp = _hap(t, h)[0]
        if k and p % 3 == 2 and e >= L + k + 1:
            nd = _edit(rng, hp[e - (L + k + 1):e][::-1].copy(), L, k)[::-1].copy()
        else:
            nd = hp[e - L:e].copy()
            if k:
                nd[7] = (int(nd[7]) + 1) & 3
        needles.append(nd.astype(np.uint8))
    return needles, cuts


def degenerate_needles(t):
    """the Myers set of the degenerate tree: what needles_at cuts (only the reference haplotype is long enough) and
    needles over the places where the 30-symbol haplotype's deletions start and end"""
    L, k = MYERS_LK
    needles, plants = needles_at(t, L, k)
    return needles + [t["ref"][o:o + L].copy() for o in (500, 985, 1005, 2000)], plants


def planted_records(needles, plants, k):
    """what a search must hold for the plants: Myers reports ends, the exact matcher begins"""
    if k:
        return [(h, e, p) for p, (h, e) in enumerate(plants)]
    return [(h, e - len(needles[p]), p) for p, (h, e) in enumerate(plants)]


MYERS_LK = (40, 2)
EXACT_LK = (24, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the per-haplotype routes, an empty haplotype left out (there is nothing to upload, and nothing to find)
# ---------------------------------------------------------------------------------------------------------------------
def expected(spm, ctx, haps, ps, engine, hs=None):
    """_expected of test_gpu_jst over the non-empty haplotypes; hs names them when `haps` is a selection"""
    out = []
    for i, hp in enumerate(haps):
        if len(hp):
            h = i if hs is None else hs[i]
            out += [(h,) + r[1:] for r in _expected(spm, ctx, [hp], ps, engine)]
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------
# random trees whose alleles touch
# ---------------------------------------------------------------------------------------------------------------------
def random_touching_alleles(rng, n_ref, n_hap, n_var, max_len):
    """Random alleles at positions drawn uniformly from [0, n_ref] WITH repeats: alleles touch, share positions, sit at
    both ends and behind the last symbol, and overlap on disjoint haplotypes.  An allele goes to those haplotypes of a
    random subset that are free at its position (free[h] <= pos; then free[h] = pos + ref_len, clamped), which is the rule
    of spm_hip.h; an allele nobody can carry is dropped."""
    cw = (n_hap + 63) // 64
    free = np.zeros(n_hap, dtype=np.int64)
    rows = []
    for p in np.sort(rng.integers(0, n_ref + 1, n_var)).tolist():
        kind = int(rng.integers(0, 4))
        rl = 1 if kind == 0 else 0 if kind == 1 else int(rng.integers(1, max_len + 1))
        al = 1 if kind == 0 else 0 if kind == 2 else int(rng.integers(1, max_len + 1))
        bits = rng.random(n_hap) < rng.choice([0.05, 0.3, 0.5, 0.9])
        bits[int(rng.integers(0, n_hap))] = True
        bits &= free <= p
        if not bits.any():
            continue
        free[bits] = min(p + rl, n_ref)
        rows.append((p, rl, rng.integers(0, 4, al, dtype=np.uint8), np.nonzero(bits)[0].tolist()))
    al, pool, cov = table(rows, n_hap)
    return al, pool, cov.reshape(len(rows), cw)


def touching_case(spm, ctx, seed):
    """The body of scripts/fuzz_jst.one_case over random_touching_alleles, without its skip of short haplotypes: an empty
    haplotype is left out of the expected side (it contributes nothing), needles are cut from the haplotypes long enough
    to hold one.  Returns ("ok" | "bad" | "skipped", records compared); skipped only if no haplotype can hold a needle."""
    rng = np.random.default_rng(seed)
    n_ref = int(rng.choice([600, 2_000, 6_000]))
    n_hap = int(rng.choice([1, 2, 7, 33, 64, 65, 130]))
    max_len = int(rng.choice([1, 3, 12, 40, 200]))
    n_var = int(rng.choice([0, 5, 60, 400, 1500]))
    algo_name = "myers" if rng.random() < 0.8 else "shiftor"
    L = int(rng.choice([24, 40, 64, 100]))
    k = 0 if algo_name == "shiftor" else int(min(rng.choice([0, 1, 2, 3, 8]), L // 12 - 1))
    block = int(rng.choice([0, 64, 128, 256, 1000]))
    ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
    alleles, pool, cov = random_touching_alleles(rng, n_ref, n_hap, n_var, max_len)
    haps = [_apply(ref, alleles, pool, cov, h) for h in range(n_hap)]
    long_enough = [hp for hp in haps if len(hp) > L + 8]
    if not long_enough:
        return "skipped", 0
    needles = _needles_from(rng, long_enough, int(rng.choice([1, 8, 40])), L, k)
    ref_text = ctx.upload(ref)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov, n_hap)
    ps = ctx.patterns(spm.ALGO_MYERS if algo_name == "myers" else spm.ALGO_SHIFTOR, needles, k=k)
    window = max(ps.window_size(p) for p in range(len(needles))) + int(rng.choice([0, 0, 5, 40]))
    exp = expected(spm, ctx, haps, ps, spm.ENGINE_BRUTE)
    st = jst.index(window, block)
    got = _got(jst.search(ps, engine=spm.ENGINE_AUTO, max_hits=1 << 22))
    ok = got == exp and st.haplotype_symbols == sum(len(hp) for hp in haps)
    if not ok:
        print(f"MISMATCH seed {seed}: {len(got)} vs {len(exp)} records, {st.haplotype_symbols} vs {sum(len(hp) for hp in haps)} "
              f"symbols; n_ref {n_ref} haplotypes {n_hap} alleles {len(alleles)} max_len {max_len} {algo_name} |P| {L} k {k} "
              f"window {window} block {block}", flush=True)
    jst.close()
    ps.close()
    ref_text.close()
    return ("ok" if ok else "bad"), len(exp)
