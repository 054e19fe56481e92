"""CPU: the hand-made trees of tests/jst_edges.py that tests/test_gpu_jst_edges.py runs the pan-genome search on.  Before a
GPU sees them: every tree is legal under the allele-table rule of spm_hip.h (and its three mirror images are not), the
journal of every haplotype has the length of its NumPy application, and -- by the oracle alone -- every planted needle is
found at its planted end on its haplotype, every allele has a record that ends at it, one that ends just behind it and one
that spans it, and the haplotypes too short for a needle have none.  The last is what keeps the GPU tests from passing on an
empty case."""
import numpy as np
import pytest

import jst_edges as E
from test_gpu_jst import _apply
from test_jst_project import Journal, _hap

TREES = {"edge": E.edge_tree, "degenerate": E.degenerate_tree, "deleted": E.deleted_tree, "wide": E.wide_tree}
_made = {}


def tree(name):
    if name not in _made:
        _made[name] = TREES[name]()
    return _made[name]


def test_the_rule_accepts_the_trees_and_refuses_their_mirror_images():
    for name in TREES:
        t = tree(name)
        assert E.legal(len(t["ref"]), t["alleles"], t["cov"]), name
    n = 1000
    snp, ins = (100, 1, [1], (0,)), (100, 0, [1, 2], (0,))
    assert E.legal(n, *E.table([ins, snp], 1)[::2])                  # the insertion stands in front of position 100
    assert not E.legal(n, *E.table([snp, ins], 1)[::2])              # ... but not behind a SNP that has consumed it
    dele = (100, 10, [], (0,))
    assert E.legal(n, *E.table([dele, (105, 0, [1], (1,))], 2)[::2])
    assert not E.legal(n, *E.table([dele, (105, 0, [1], (0,))], 2)[::2])         # an insertion inside a carried deletion
    assert E.legal(n, *E.table([dele, (110, 0, [1], (0,))], 2)[::2])             # directly behind it: free
    t = tree("edge")
    assert not E.legal(len(t["ref"]), t["alleles"][::-1], t["cov"][::-1])        # out of order
    assert E.legal(n, *E.table([(n, 0, [1], (0,))], 1)[::2]) and not E.legal(n, *E.table([(n + 1, 0, [1], (0,))], 1)[::2])
    # the clamp: a deletion to the end with ref_len beyond it overlaps nothing behind the reference
    assert E.legal(n, *E.table([(n - 5, 1000, [], (0,)), (n, 0, [1], (0,))], 1)[::2])


def test_the_edge_tree_is_the_one_described():
    t = tree("edge")
    n, B, p = E.N_REF, E.BORDER, E.CHAIN
    al = t["alleles"]
    assert len(al) == 26 + 320 and t["n_hap"] == 8 and len(t["ref"]) == n
    rows = {(int(a["pos"]), int(a["ref_len"]), int(a["alt_len"]), tuple(E.carriers(t["cov"], i))) for i, a in enumerate(al)}
    for r in [(0, 0, 3, (0,)), (0, 300, 0, (1,)), (n, 0, 5, (2,)), (n - 40, 1000, 0, (3,)), (n - 1, 1, 1, (4,)),
              (B, 0, 4, (0,)), (B - 1, 1, 1, (1,)), (B, 1, 1, (2,)), (B - 3, 5, 0, (3,)), (B - 5, 5, 0, (4,)), (B, 5, 0, (5,)),
              (1500, 700, 0, (0,)), (1600, 1, 1, (1,)), (1700, 0, 6, (2,)), (1650, 10, 0, (3,)), (1550, 600, 0, (4,)),
              (2100, 200, 0, (5,)), (p, 1, 1, (6,)), (p + 1, 1, 1, (6,)), (p + 2, 4, 0, (6,)), (p + 6, 0, 3, (6,)),
              (p + 6, 1, 1, (6,)), (p + 10, 0, 2, (6,)), (p + 12, 3, 7, (6,)), (p + 20, 0, 0, (7,))]:
        assert r in rows, r
    # the insertion at p + 6 stands in front of the SNP at p + 6; the two insertions at p + 10 are two table rows
    at = [i for i, a in enumerate(al) if int(a["pos"]) == p + 6]
    assert [int(al[i]["ref_len"]) for i in at] == [0, 1]
    assert sum(1 for a in al if int(a["pos"]) == p + 10) == 2
    # 320 SNPs in a row: one block of 512, 1000 or 4096 holds more table entries than the 256 bits of a signature
    q = al["pos"].astype(np.int64)
    for L in (512, 1000, 4096):
        assert max(int(np.count_nonzero(q // L == j)) for j in range(-(-n // L))) > 256
    assert max(int(np.count_nonzero(q // 256 == j)) for j in range(n // 256)) <= 256
    # haplotypes 6 and 7: alike on the last 256 SNPs of the stretch, unlike on the 64 before, equally long contexts in the
    # 512 block that holds the stretch -- only the "not shared" path keeps the two apart there
    st = [i for i, lab in enumerate(t["labels"]) if lab.startswith("stretch")]
    on6 = np.array([6 in E.carriers(t["cov"], i) for i in st])
    on7 = np.array([7 in E.carriers(t["cov"], i) for i in st])
    assert np.array_equal(on6[64:], on7[64:]) and np.array_equal(on6[:64], ~on7[:64])
    assert all(E.carriers(t["cov"], i) for i in st)
    h6, h7 = E.haplotypes(t, (6, 7))
    assert len(h6) - len(h7) == 7 and np.array_equal(h6[3156 + 7:3584 + 7], h7[3156:3584])
    assert int(np.count_nonzero(h6[3092 + 7:3156 + 7] != h7[3092:3156])) == 64
    # every SNP changes its symbol (an alt equal to the reference would make the allele invisible)
    for a in al:
        if int(a["ref_len"]) == 1 and int(a["alt_len"]) == 1:
            assert t["pool"][int(a["alt_off"])] != t["ref"][int(a["pos"])]
    haps = E.haplotypes(t)
    assert [len(h) for h in haps] == [n + 3 + 4 - 700, n - 300, n + 5 + 6, n - 40 - 5 - 10, n - 5 - 600, n - 5 - 200,
                                      n - 4 + 3 + 2 + 2 + 4, n]
    assert np.array_equal(haps[2][-5:], t["pool"][int(al[-1]["alt_off"]):][:5]) and int(al[-1]["pos"]) == n


@pytest.mark.parametrize("name", list(TREES))
def test_journal_length_equals_the_numpy_application(name):
    t = tree(name)
    for h in range(t["n_hap"]):
        hp = _apply(t["ref"], t["alleles"], t["pool"], t["cov"], h)
        assert Journal(len(t["ref"]), t["alleles"], t["cov"], h).n == len(hp)
    if name == "degenerate":
        assert [len(h) for h in E.haplotypes(t)] == [0, 30, E.DEG_REF]
    if name == "deleted":
        assert len(_hap(t, 0)[0]) == 0
    if name == "wide":
        cols = E.columns(t)
        assert len(cols) <= 16 and sum(len(v) for v in cols.values()) == E.WIDE_HAP
        alone = [v for v in cols.values() if len(v) == 1]
        assert [E.WIDE_HAP - 1] in alone and [512] in alone
        for a, b in ((63, 64), (1023, 1024)):                # the two alleles of the site spell different symbols
            site =[i for i, lab in enumerate(t["labels"]) if lab.startswith("site")]
            xa, xb = E.allele_span(t, site[0], a)[0], E.allele_span(t, site[1], b)[0]
            sa, sb = int(_hap(t, a)[0][xa]), int(_hap(t, b)[0][xb])
            assert len({sa, sb, int(t["ref"][E.WIDE_SITE])}) == 3


def _oracle_records(O, haps, needles, k, hs=None):
    """{haplotype: {(pos, pattern): score}} by the oracle alone; an empty haplotype has nothing to scan"""
    out = {}
    for i, hp in enumerate(haps):
        h = i if hs is None else hs[i]
        out[h] = {}
        if len(hp):
            r = O.scan_multi(O.MYERS if k else O.SHIFTOR, hp, needles, k=k, threads=4)
            out[h] = {(int(a), int(b)): int(c) for a, b, c in zip(r["pos"], r["pattern"], r["score"])}
    return out


@pytest.mark.parametrize("L,k", [E.MYERS_LK, E.EXACT_LK])
def test_every_edge_of_the_edge_tree_has_its_records(oracle, L, k):
    t = tree("edge")
    haps = E.haplotypes(t)
    needles, plants = E.needles_at(t, L, k)
    assert len(needles) >= 100 and all(len(nd) == L for nd in needles)
    rec = _oracle_records(oracle, haps, needles, k)
    n_rec = sum(len(v) for v in rec.values())
    print(f"|P| {L} k {k}: {len(needles)} needles, {n_rec} records over {len(haps)} haplotypes")
    assert n_rec >= len(needles)
    for h, pos, p in E.planted_records(needles, plants, k):
        assert rec[h].get((pos, p), k + 1) <= k, (h, pos, p)
    # every bullet: a record that ends at the allele, one that ends one behind its alt, one that spans it -- on every carrier
    shift = 0 if k else L                                   # the exact matcher reports begins
    ends = {h: {pos + shift for pos, _p in v} for h, v in rec.items()}
    for i in t["plant"]:
        for h in E.carriers(t["cov"], i):
            x0, x1 = E.allele_span(t, i, h)
            at, _b, _c, behind, across = E.plant_ends(t, i, h, L)
            assert {at, behind, across} <= ends[h], (t["labels"][i], h)
            assert across - L <= x0 and x1 <= across, (t["labels"][i], h)      # the needle cut there holds the whole alt
    if k:
        # the insertion behind the last reference symbol: records that end on each of its five symbols
        n2 = len(haps[2])
        assert {n2 - x for x in range(5)} & ends[2] >= {n2, n2 - 4}
    # the planted needles of one haplotype are found on the others only where the sequences agree: the sets differ
    assert len({frozenset(v) for v in rec.values()}) == len(haps)


def test_the_degenerate_trees_have_no_record_where_there_is_no_room(oracle):
    t = tree("degenerate")
    haps = E.haplotypes(t)
    L, k = E.MYERS_LK
    needles, plants = E.degenerate_needles(t)
    assert {h for h, _e in plants} == {2}                   # nothing can be cut from the empty and the 30-symbol haplotype
    rec = _oracle_records(oracle, haps, needles, k)
    assert rec[0] == {} and rec[1] == {} and len(rec[2]) >= len(needles)
    t1 = tree("deleted")
    assert len(E.haplotypes(t1)[0]) == 0 and len(t1["alleles"]) == 1


def test_the_wide_tree_differs_where_it_should(oracle):
    t = tree("wide")
    L, k = E.MYERS_LK
    needles, plants = E.needles_at(t, L, k, who=E.wide_who)
    cols = E.columns(t)
    reps = [v[0] for v in cols.values()]
    rec = _oracle_records(oracle, E.haplotypes(t, reps), needles, k, hs=reps)
    col_of = {h: v[0] for v in cols.values() for h in v}
    for h, pos, p in E.planted_records(needles, plants, k):
        assert rec[col_of[h]].get((pos, p), k + 1) <= k, (h, pos, p)
    assert E.site_differences(t, needles, plants, k, lambda h: rec[col_of[h]]) >= 4    # one per carrier
    last = rec[col_of[E.WIDE_HAP - 1]]
    others = set().union(*(set(v) for r, v in rec.items() if r != col_of[E.WIDE_HAP - 1]))
    assert set(last) - others, "the last haplotype has no record of its own"


def test_random_touching_alleles_are_legal_and_touch():
    seen = {"touching": 0, "overlap": 0, "at_0": 0, "at_n_ref": 0}
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n_ref = int(rng.choice([60, 300, 1000]))
        n_hap = int(rng.choice([1, 2, 5, 66]))
        alleles, pool, cov = E.random_touching_alleles(rng, n_ref, n_hap, int(rng.choice([3, 20, 80, 300])),
                                                       int(rng.choice([1, 3, 12, 40])))
        assert E.legal(n_ref, alleles, cov) and len(pool) == int(alleles["alt_len"].sum())
        assert all(E.carriers(cov, i) for i in range(len(alleles)))
        ref = rng.integers(0, 4, n_ref, dtype=np.uint8)
        for h in (range(n_hap) if n_hap <= 5 else (0, 1, 63, 64, 65)):
            hp = _apply(ref, alleles, pool, cov, h)
            assert Journal(n_ref, alleles, cov, h).n == len(hp)
        pos = alleles["pos"].astype(np.int64)
        end = pos + np.minimum(alleles["ref_len"].astype(np.int64), n_ref - pos)
        seen["at_0"] += bool(np.any(pos == 0))
        seen["at_n_ref"] += bool(np.any(pos == n_ref))
        for i in range(len(pos) - 1):
            j = i + 1
            while j < len(pos) and pos[j] <= end[i]:
                shared = bool(np.any(cov[i] & cov[j]))
                seen["touching"] += shared and pos[j] == end[i]
                seen["overlap"] += (not shared) and pos[j] < end[i]
                j += 1
    assert all(v > 0 for v in seen.values()), seen
