"""GPU: the pan-genome search (spm_hip_jst_index / _search / _hits_align) on the hand-made trees of tests/jst_edges.py,
against what it is defined to be: the union over haplotypes of a linear scan of each materialised haplotype.

Every comparison is exact.  The expected side never comes from the tree: the haplotypes are the NumPy application of the
alleles, the records the per-haplotype scans of test_gpu_jst._expected (one haplotype also through the oracle), the
alignments the per-haplotype route of test_jst_align, the projections the NumPy journal of test_jst_project.
tests/test_jst_edges.py shows, by the oracle alone, that every allele of every tree has records at it, behind it and across
it -- so a cell that loses a symbol fails a row here.

An insertion behind the last reference symbol (pos == n_ref) once belonged to no block where the block length divides
n_ref.  Before `a_lo[n_blocks] = n_alleles`, test_search_on_the_edge_tree failed on an MI355X in every row of block lengths
64, 256, 512, 4096 and the default (256), at both windows and on both engines: 1 339 of 1 346 Myers records (the seven that
end in the inserted symbols of haplotype 2 missing), 444 of 446 exact records, stats.haplotype_symbols 30 923 for 30 928;
every row of block length 1000 passed, and test_block_shards_on_the_edge_tree failed likewise.
"""
import numpy as np
import pytest

import jst_edges as E
from test_gpu_jst import _got
from test_jst_align import _check_against_haplotypes, _has_indel, _jst_records, _per_haplotype_route, _rows
from test_jst_project import ALL_KINDS, _check

pytestmark = pytest.mark.gpu

_trees, _sets, _wants = {}, {}, {}
BUILDERS = {"edge": E.edge_tree, "degenerate": E.degenerate_tree, "deleted": E.deleted_tree, "wide": E.wide_tree}


def _tree(name):
    if name not in _trees:
        _trees[name] = BUILDERS[name]()
    return _trees[name]


def _set(name, which):
    """(needles, plants, k, myers) of a tree's Myers or exact set, made once"""
    if (name, which) not in _sets:
        t = _tree(name)
        L, k = E.MYERS_LK if which == "myers" else E.EXACT_LK
        if name == "degenerate":
            needles, plants = E.degenerate_needles(t)
        else:
            needles, plants = E.needles_at(t, L, k, who=E.wide_who if name == "wide" else None)
        _sets[(name, which)] = (needles, plants, k, which == "myers")
    return _sets[(name, which)]


def _open(spm, ctx, name, which):
    t = _tree(name)
    needles, _plants, k, myers = _set(name, which)
    ref_text = ctx.upload(t["ref"])
    jst = spm.Jst(ctx, ref_text, t["alleles"], t["pool"], t["cov"], t["n_hap"])
    ps = ctx.patterns(spm.ALGO_MYERS if myers else spm.ALGO_SHIFTOR, needles, k=k)
    return t, ref_text, jst, ps, max(ps.window_size(p) for p in range(len(needles)))


def _want(spm, ctx, name, which, ps):
    """the per-haplotype scans (brute-force engine), once per tree and set; every plant must be among them"""
    key = (name, which, "records")
    if key not in _wants:
        t = _tree(name)
        needles, plants, k, _myers = _set(name, which)
        if name == "wide":                                   # once per distinct coverage column, replicated
            cols = list(E.columns(t).values())
            reps = [v[0] for v in cols]
            per = E.expected(spm, ctx, E.haplotypes(t, reps), ps, spm.ENGINE_BRUTE, hs=reps)
            members = {v[0]: v for v in cols}
            want = sorted((h,) + r[1:] for r in per for h in members[r[0]])
        else:
            want = E.expected(spm, ctx, E.haplotypes(t), ps, spm.ENGINE_BRUTE)
        found = {r[:3]: r[3] for r in want}
        for rec in E.planted_records(needles, plants, k):
            assert found.get(rec, k + 1) <= k, ("a planted needle is not found at its place", rec)
        _wants[key] = want
    return _wants[key]


def _want_rows(spm, ctx, name, which, ps):
    """the per-haplotype alignments: upload, scan, Hits.align() (the empty haplotype has nothing to upload)"""
    key = (name, which, "rows")
    if key not in _wants:
        haps = E.haplotypes(_tree(name))
        _wants[key] = _per_haplotype_route(spm, ctx, haps, ps, spm.ENGINE_BRUTE, only=[h for h, x in enumerate(haps) if len(x)])
    return _wants[key]


def _close(*xs):
    for x in xs:
        x.close()


def test_search_on_the_edge_tree(spm, ctx, oracle):
    haps = E.haplotypes(_tree("edge"))
    total = sum(len(h) for h in haps)
    bad = []
    for which in ("myers", "exact"):
        t, ref_text, jst, ps, window = _open(spm, ctx, "edge", which)
        needles, _plants, k, myers = _set("edge", which)
        if myers:
            for h, hp in enumerate(haps):
                assert jst.haplotype_length(h) == len(hp)
                assert np.array_equal(jst.extract(h, 0, len(hp)), hp)
            assert np.array_equal(jst.extract(2, len(haps[2]) - 10, 10), haps[2][-10:])
        want = _want(spm, ctx, "edge", which, ps)
        assert len(want) >= len(needles)
        O = oracle
        hits = O.scan_multi(O.MYERS if myers else O.SHIFTOR, haps[2], needles, k=k, threads=8)
        assert sorted((2, int(a), int(b), int(c)) for a, b, c in zip(hits["pos"], hits["pattern"], hits["score"])) \
            == [e for e in want if e[0] == 2]
        for block in E.BLOCKS:
            for win in (window, window + 37):
                st = jst.index(win, block)
                if st.haplotype_symbols != total:
                    bad.append((which, block, win, "haplotype_symbols", int(st.haplotype_symbols), total))
                for engine in (spm.ENGINE_AUTO, spm.ENGINE_BRUTE):
                    got = _got(jst.search(ps, engine=engine, max_hits=1 << 20))
                    if got != want:
                        missing = sorted(set(want) - set(got))
                        bad.append((which, block, win, engine, f"{len(got)} records for {len(want)}",
                                    "missing", missing[:4], "unexpected", sorted(set(got) - set(want))[:4]))
        _close(jst, ps, ref_text)
    for row in bad:
        print("MISMATCH", row)
    assert not bad, bad


def test_block_shards_on_the_edge_tree(spm, ctx):
    for which in ("myers", "exact"):
        t, ref_text, jst, ps, window = _open(spm, ctx, "edge", which)
        want = _want(spm, ctx, "edge", which, ps)
        n_blocks = jst.index(window, 256).n_blocks
        assert n_blocks == E.N_REF // 256
        b = E.BORDER // 256
        for cuts in ([0, b, b + 1, n_blocks], [0, n_blocks - 1, n_blocks]):      # the block of the border; the last block
            parts = []
            for b0, b1 in zip(cuts[:-1], cuts[1:]):
                assert jst.index(window, 256, b0, b1).n_blocks == b1 - b0
                parts += _got(jst.search(ps, max_hits=1 << 20))
            assert sorted(parts) == want, (which, cuts)
        _close(jst, ps, ref_text)


def test_alignments_on_the_edge_tree(spm, ctx):
    haps = E.haplotypes(_tree("edge"))
    for which in ("myers", "exact"):
        t, ref_text, jst, ps, window = _open(spm, ctx, "edge", which)
        needles, _plants, k, myers = _set("edge", which)
        want = _want_rows(spm, ctx, "edge", which, ps)
        assert len(want) == len(_want(spm, ctx, "edge", which, ps))
        for block in (64, 256):
            jst.index(window, block)
            h = jst.search_device(ps, alignable=True, max_hits=1 << 20)
            hv = h.view()
            a = h.align()
            rec, ops = a.view(), a.ops
            _check_against_haplotypes(haps, needles, hv, rec, ops, myers)
            assert not myers or _has_indel(ops)
            rows = sorted(_rows(rec, ops))
            assert rows == want, (which, block)
            # the inverse of the fan-out, over cells without a context: every record located again, the same alignments
            sel = h.select(loci=False)
            b = sel.align_selected()
            assert sorted(_rows(b.view(), b.ops)) == rows, (which, block)
            # in reference coordinates, against the NumPy journal (the insertion behind the last symbol included)
            got = _check(spm, ctx, t, needles, a, block, ALL_KINDS)
            assert len(got) == len(rows)
            _close(b, sel, a, h)
        _close(jst, ps, ref_text)


def test_haplotypes_without_room_for_a_needle(spm, ctx):
    t, ref_text, jst, ps, window = _open(spm, ctx, "degenerate", "myers")
    haps = E.haplotypes(t)
    needles, _plants, k, _myers = _set("degenerate", "myers")
    assert [jst.haplotype_length(h) for h in range(3)] == [0, 30, E.DEG_REF] == [len(h) for h in haps]
    want = _want(spm, ctx, "degenerate", "myers", ps)
    want_rows = _want_rows(spm, ctx, "degenerate", "myers", ps)
    assert len(want) >= len(needles) and {r[0] for r in want} == {2}
    for block in (64, 256, 0):
        st = jst.index(window, block)
        assert st.haplotype_symbols == 30 + E.DEG_REF
        for engine in (spm.ENGINE_AUTO, spm.ENGINE_BRUTE):
            assert _got(jst.search(ps, engine=engine)) == want, (block, engine)
        hv, rec, ops, _st, _jst_st = _jst_records(spm, jst, ps)
        _check_against_haplotypes(haps, needles, hv, rec, ops)
        assert sorted(_rows(rec, ops)) == want_rows and set(rec["haplotype"].tolist()) == {2}
    _close(jst, ps, ref_text)
    # one haplotype, wholly deleted: no context at all -- empty results, no error
    t1 = _tree("deleted")
    ref_text = ctx.upload(t1["ref"])
    jst = spm.Jst(ctx, ref_text, t1["alleles"], t1["pool"], t1["cov"], 1)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=k)
    assert jst.haplotype_length(0) == 0
    for block in (256, 0):
        st = jst.index(window, block)
        assert st.unique_contexts == 0 and st.contexts == 0 and st.haplotype_symbols == 0 and st.context_symbols == 0
        assert len(jst.search(ps)) == 0
        h = jst.search_device(ps, alignable=True)
        a = h.align()
        assert len(h) == 0 and len(a) == 0 and len(a.view()) == 0 and len(a.ops) == 0
        _close(a, h)
    _close(jst, ps, ref_text)


def test_index_statistics_equal_the_host_walk(spm, ctx):
    """The device index of the 96-symbol tree counts what tests/cpp/jst_walk_core_cases.cpp counts on the host, from the
    brute-force haplotypes and the same walk functions (tests/test_jst_walk_cpp.py runs that program): both sides assert
    jst_edges.WALK_STATS."""
    ref, alleles, pool, cov, n_hap = E.walk_tree()
    assert E.legal(len(ref), alleles, cov)
    ref_text = ctx.upload(ref)
    jst = spm.Jst(ctx, ref_text, alleles, pool, cov, n_hap)
    st = jst.index(E.WALK_WINDOW, E.WALK_BLOCK)
    got = {k: int(getattr(st, k)) for k in E.WALK_STATS}
    print(got)
    assert got == E.WALK_STATS and st.n_blocks == E.WALK_REF // E.WALK_BLOCK
    _close(jst, ref_text)


def test_search_on_the_wide_tree(spm, ctx):
    t, ref_text, jst, ps, window = _open(spm, ctx, "wide", "myers")
    needles, plants, k, _myers = _set("wide", "myers")
    want = _want(spm, ctx, "wide", "myers", ps)
    st = jst.index(window, 256)
    assert st.haplotype_symbols == sum(len(h) for h in E.haplotypes(t))
    for engine in (spm.ENGINE_AUTO, spm.ENGINE_BRUTE):
        got = _got(jst.search(ps, engine=engine, max_hits=1 << 22))
        assert got == want, engine
    by_hap = {}
    for h, pos, p, s in got:
        by_hap.setdefault(h, {})[(pos, p)] = s
    assert E.site_differences(t, needles, plants, k, lambda h: by_hap[h]) >= 4
    last = E.WIDE_HAP - 1
    assert set(by_hap[last]) - set().union(*(set(v) for h, v in by_hap.items() if h != last))
    _close(jst, ps, ref_text)


def test_random_trees_with_touching_alleles(spm, ctx):
    """30 seeds of jst_edges.touching_case (scripts/fuzz_jst.py --geometry touching runs the same cases for as long as asked)"""
    results = [E.touching_case(spm, ctx, seed) for seed in range(800000, 800030)]
    assert all(r[0] != "bad" for r in results), [i for i, r in enumerate(results) if r[0] == "bad"]
    assert sum(r[0] == "ok" for r in results) >= 25 and sum(r[1] for r in results) > 1000
