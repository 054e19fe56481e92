"""GPU: the pileup of a coordinate-sorted record stream (spm_hip_bam_pileup, spm_hip_bam_pileup_records) and its variant sites
(spm_hip_pileup_sites), byte for byte against the serial host builder and against the rule written again in
tests/pileup_rule.py: hand-built streams aimed at the tile borders the first call's stats report, contention on one column
across a wave and a workgroup, SEQ and QUAL at every alignment, every counted disagreement; end to end behind sort and markdup on
the planted tree of test_gpu_markdup.py; planted substitutions found as sites."""
import ctypes
import struct

import numpy as np
import pytest

from cpp_programs import download
from pileup_rule import make_stream, parse_records, py_pileup, py_sites, sites_as_tuples, words_of
from test_bam_pileup import REF_LEN as HAND_REF_LEN, WORKED_WANT, as_counts, disagreements, worked_table
from test_gpu_bai import _Device
from test_gpu_markdup import GROUPS, RNAME, _single_reads
from test_gpu_sam import _names
from test_gpu_sam_qual_md import decode_bam
from test_pairs import _free_stretches
from test_rescue import _chain_of
from test_sam import LINE

gpu = pytest.mark.gpu
INVALID = -1
A, C, G, T_, N, DEL, INS, LOWQ = range(8)
_tile = {}


def _raw(ctx, stream, lines, ref_len, shift=0, **kw):
    """Context.bam_pileup over an uploaded stream that starts `shift` bytes behind a 4-byte border -> (counts, the stats, the
    device view)"""
    dev = [_Device(b"\x5d" * shift + stream), _Device(np.ascontiguousarray(lines, LINE).tobytes())]
    try:
        p = ctx.bam_pileup(dev[0].ptr.value + shift, len(stream), dev[1].ptr.value, len(lines), ref_len, **kw)
        counts, st = p.counts(), p.stats()
        d, n = p.device()
        assert n == counts.shape[1] == len(p)
        view = download(ctx, d, 8 * n, np.uint32).reshape(8, n)
        p.close()
        return counts, st, view
    finally:
        ctx.synchronize()
        for d in dev:
            d.close()


def _three_ways(spm, ctx, stream, lines, ref_len, shift=0, **kw):
    """device == host builder == the Python rule, the stats equal NumPy's -> (counts, the stats)"""
    got, st, view = _raw(ctx, stream, lines, ref_len, shift, **kw)
    host = spm.bam_pileup_host(stream, lines, ref_len, **kw)
    want = py_pileup(stream, lines, ref_len, **kw)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), (kw, np.argwhere(got != want)[:8].tolist())
    assert got.tobytes() == host.tobytes() == view.tobytes()
    depth = got[:6].sum(axis=0, dtype=np.uint64)
    assert (st.n_records, st.n_evidence, st.sum_depth) == (len(lines), int(got.sum(dtype=np.uint64)), int(depth.sum()))
    assert (st.n_covered, st.max_depth) == (int(np.count_nonzero(depth)), int(depth.max()) if depth.size else 0)
    assert st.ms_host > 0 and st.ms_total >= 0 and st.tile_positions >= 1
    return got, st


def _tile_positions(ctx):
    if not _tile:
        stream, lines = make_stream(worked_table())
        _tile["T"] = int(_raw(ctx, stream, lines, HAND_REF_LEN)[1].tile_positions)
    return _tile["T"]


def _rec(rng, pos, cigar, **kw):
    q = sum(w >> 4 for w in words_of(cigar) if (w & 15) in (0, 1, 4, 7, 8))
    seq = "".join("ACGTN"[i] for i in rng.choice(5, q, p=[.24, .24, .24, .24, .04]))
    return dict(pos=pos, cigar=cigar, seq=seq, qual=rng.integers(0, 42, q).tolist(), **kw)


@gpu
def test_worked_table_and_tile_borders(spm, ctx):
    stream, lines = make_stream(worked_table())
    got, st = _three_ways(spm, ctx, stream, lines, HAND_REF_LEN)
    assert np.array_equal(got, as_counts(WORKED_WANT)) and st.n_taking_part == 10 and st.n_tile_visits >= 10
    T = _tile_positions(ctx)
    rng = np.random.default_rng(31)
    ref_len = 4 * T + 50
    recs = [_rec(rng, 0, "9M"), _rec(rng, ref_len - 9, "9M"), _rec(rng, 0, "1M"), _rec(rng, ref_len - 1, "1M")]   # pos = 0, end = ref_len
    for k in (1, 2, 3):
        for d in (-1, 0, 1):
            recs.append(_rec(rng, k * T + d, "5M1I3M"))                           # begins at k T - 1, k T, k T + 1
            recs.append(_rec(rng, k * T + d - 11, "2S4M2D5M"))                    # ends there
            recs.append(_rec(rng, k * T + d - 1, "1M1I1M"))                       # an I whose column is the tile's last or first
    recs.append(_rec(rng, T - 5, f"5M{2 * T}D5M"))                                # a D across three tiles
    recs.append(_rec(rng, T + 3, f"4M{2 * T + 10}N4M"))                           # an N across three tiles
    recs.append(_rec(rng, 7, f"3M{3 * T}D1M1I2M", flag=0x400))                    # excluded by default: a long record that is not walked
    recs.sort(key=lambda r: r["pos"])
    recs += [dict(pos=-1, ref_id=-1, flag=4, cigar="", seq="ACGT")] * 3           # unplaced records behind the placed ones
    stream, lines = make_stream(recs)
    whole, st = _three_ways(spm, ctx, stream, lines, ref_len)
    assert st.tile_positions == T and st.n_taking_part == len(recs) - 4 and st.n_tile_visits > st.n_taking_part
    assert whole[DEL, T:3 * T].min() >= 1 and whole[INS].sum() >= 18
    regions = [(T - 1, 3 * T + 1), (T + 1, 2 * T - 1), (17, T + 301), (T + 100, T + 200), (T, 2 * T), (2 * T - 1, 2 * T), (2 * T, 2 * T + 1),
               (0, 1), (ref_len - 1, ref_len), (5, 5), (ref_len, ref_len), (3 * T + 1, ref_len)]
    for begin, end in regions:                                      # begin and end at T +- 1 and off the multiples of T; inside one record
        for kw in (dict(), dict(min_baseq=20, exclude_flags=0x4)):
            got, _st = _three_ways(spm, ctx, stream, lines, ref_len, begin=begin, end=end, **kw)
            assert got.shape == (8, end - begin)
            if not kw:
                assert np.array_equal(got, whole[:, begin:end]), (begin, end)
    got, _st = _three_ways(spm, ctx, stream, lines, ref_len, begin=T + 100, end=T + 200)
    assert got[DEL].tolist() == [1] * 100 and got[:5].sum() == 0    # a region inside one record's deletion (and another's N)
    # zero records, and an empty region over zero records
    got, st = _three_ways(spm, ctx, b"", np.zeros(0, LINE), ref_len)
    assert got.shape == (8, ref_len) and not got.any() and st.n_tile_visits == 0
    assert _three_ways(spm, ctx, b"", np.zeros(0, LINE), 0)[0].shape == (8, 0)


@gpu
def test_contention_alignments_and_shifts(spm, ctx):
    T = _tile_positions(ctx)
    rng = np.random.default_rng(32)
    ref_len = 2 * T + 200
    recs, at = [], {}
    for g, pos in zip((1, 64, 65, 300), (40, T - 1, T, T + 77)):    # copies on one column: contention across a wave and a workgroup
        at[g] = pos
        recs += [dict(pos=pos, cigar="1M", seq="ACGT"[j % 4], qual=[j % 40]) for j in range(g)]
        recs += [dict(pos=pos + 3, cigar="2M1D1M", seq="GGG") for _ in range(g)]
    for name_len in range(1, 9):                                    # SEQ and QUAL through every alignment
        for l_seq in range(30, 38):
            recs.append(_rec(rng, int(rng.integers(100, T + 300)), f"{l_seq}M", name=b"n" * name_len))
    recs.sort(key=lambda r: r["pos"])
    recs += [dict(pos=-1, ref_id=-1, flag=4, cigar="", seq="ACGTAC", name=b"unplaced")] * 2
    stream, lines = make_stream(recs)
    offs = [(int(o) + 36 + stream[int(o) + 12] + 4 * struct.unpack_from("<H", stream, int(o) + 16)[0]) for o in lines["offset"]]
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    for shift in range(4):                                          # the stream at 0..3 bytes behind a 4-byte border
        for kw in (dict(), dict(min_baseq=20), dict(min_baseq=93, begin=T - 3, end=T + 90)):
            got, st = _three_ways(spm, ctx, stream, lines, ref_len, shift=shift, **kw)
            if not kw:
                for g, pos in at.items():
                    assert got[:4, pos].sum() >= g and got[G, pos + 3] >= g and got[DEL, pos + 5] >= g
                assert st.max_depth >= 300


@gpu
def test_counted_disagreements_and_refusals(spm, ctx):
    lib = spm.capi.lib()
    for name, (stream, lines, ref_len) in disagreements().items():
        dev = [_Device(stream), _Device(lines.tobytes())]
        h = ctypes.c_void_p(0x7777)
        rc = lib.spm_hip_bam_pileup_records(ctx._h, dev[0].ptr, len(stream), dev[1].ptr, len(lines), ref_len, None, ctypes.byref(h))
        assert rc == INVALID and not h.value, name
        assert b"disagree" in lib.spm_hip_last_error(ctx._h)
        ctx.synchronize()
        assert download(ctx, dev[0].ptr.value, len(stream), np.uint8).tobytes() == stream, name   # the caller's buffers are untouched
        assert download(ctx, dev[1].ptr.value, len(lines), LINE).tobytes() == lines.tobytes(), name
        for d in dev:
            d.close()
        with pytest.raises(spm.SpmError, match="-1.*disagree"):
            spm.bam_pileup_host(stream, lines, ref_len)             # the host builder refuses the same inputs
    stream, lines = make_stream(worked_table())
    for kw, why in ((dict(min_baseq=94), "min_baseq"), (dict(begin=9, end=8), "region"), (dict(end=HAND_REF_LEN + 1), "region")):
        with pytest.raises(spm.SpmError, match="-1.*" + why):
            _raw(ctx, stream, lines, HAND_REF_LEN, **kw)
    with pytest.raises(spm.SpmError, match="-4"):
        _raw(ctx, stream, lines, (1 << 31) + 1)
    got, _st = _three_ways(spm, ctx, stream, lines, HAND_REF_LEN)   # the context works on
    assert np.array_equal(got, as_counts(WORKED_WANT))


def _primary_span(stream, lines, read):
    """(pos, l_seq) of the primary record of a read"""
    for o, r, f in zip(lines["offset"].tolist(), lines["read"].tolist(), lines["flag"].tolist()):
        if r == read and not f & 0x900:
            return struct.unpack_from("<i", stream, o + 8)[0], struct.unpack_from("<I", stream, o + 20)[0]
    raise AssertionError(read)


@gpu
def test_end_to_end_behind_sort_and_markdup(spm, ctx):
    t, reads, at, quals = _single_reads()
    ref_len = len(t["ref"])
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    b = lc.bam_ex(rd, ps, RNAME, ref_len, qualities=quals, names=_names(len(reads)))
    s = b.sort()
    m = s.markdup()
    p, p_all = m.pileup(), m.pileup(exclude_flags=0x4)
    stream, lines = decode_bam(m.bytes())[1], m.lines()
    assert stream == m.records()
    m.close()                                                       # the results outlive their source
    got, got_all = p.counts(), p_all.counts()
    for counts, kw in ((got, dict()), (got_all, dict(exclude_flags=0x4))):
        assert counts.shape == (8, ref_len) and np.array_equal(counts, py_pileup(stream, lines, ref_len, **kw))
        assert counts.tobytes() == spm.bam_pileup_host(stream, lines, ref_len, **kw).tobytes()
    depth, depth_all = p.depth(), p_all.depth()
    assert depth.dtype == np.uint32 and np.array_equal(depth, got[:6].sum(axis=0))
    for g in GROUPS:                                                # a planted duplicate group adds depth 1, or g without the exclusion
        pos, m_len = _primary_span(stream, lines, at[f"group{g}"][0])
        assert depth[pos:pos + m_len].tolist() == [1] * m_len and depth_all[pos:pos + m_len].tolist() == [g] * m_len, g
    n_dup = int(((lines["flag"] & 0x400) != 0).sum())
    placed = int(((lines["flag"] & 0x4) == 0).sum())
    for x, counts, n_taking in ((p, got, placed - n_dup), (p_all, got_all, placed)):
        st, d = x.stats(), counts[:6].sum(axis=0, dtype=np.uint64)
        assert (st.sum_depth, st.n_covered, st.max_depth) == (int(d.sum()), int(np.count_nonzero(d)), int(d.max()))
        assert (st.n_records, st.n_taking_part, st.n_evidence) == (len(lines), n_taking, int(counts.sum(dtype=np.uint64)))
        assert st.n_tile_visits >= st.n_taking_part and st.ms_total >= 0 and st.ms_host > 0
    assert n_dup >= sum(g - 1 for g in GROUPS)
    assert p_all.stats().max_depth >= 300 and got[LOWQ].sum() == 0
    lowq = s.pileup(min_baseq=21, begin=1000, end=ref_len - 7)      # a region, a quality threshold, the sorted handle that is not marked
    want = py_pileup(stream, lines, ref_len, min_baseq=21, begin=1000, end=ref_len - 7, exclude_flags=0x304)   # (s carries no 0x400)
    assert np.array_equal(lowq.counts(), want) and want[LOWQ].sum() > 0
    again = s.markdup().pileup()                                    # two runs give identical bytes
    assert again.counts().tobytes() == got.tobytes()
    d_ptr, n = p.device()
    assert n == ref_len and download(ctx, d_ptr, 8 * n, np.uint32).tobytes() == got.tobytes()
    with pytest.raises(spm.SpmError, match="-1.*order"):
        b.pileup()                                                  # the records in read order: refused by the order test
    for x in (again, lowq, p_all, p, s, b, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_sites_of_planted_substitutions(spm, ctx):
    t = _single_reads()[0]
    ref = t["ref"]
    ref_len = len(ref)
    spots = _free_stretches(t, 300, 40, first=1000)
    reads, planted = [], []
    for spot, m_len, col in ((spots[-1], 50, 20), (spots[-2], 64, 31), (spots[-3], 37, 5)):   # 3 of 5 copies carry a substitution
        x = spot + 40
        base = (int(ref[x + col]) + 1 + len(planted)) % 4
        assert base != ref[x + col]
        for j in range(5):
            r = np.array(ref[x:x + m_len], np.uint8)
            if j < 3:
                r[col] = base
            reads.append(r)
        planted.append((x + col, base))
    reads += [np.array(ref[spots[-4] + 40:spots[-4] + 90], np.uint8)] * 2       # plain reads: no site
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    b = lc.bam_ex(rd, ps, RNAME, ref_len)
    s = b.sort()
    p = s.pileup()
    counts = p.counts()
    stream, lines = s.records(), s.lines()
    assert np.array_equal(counts, py_pileup(stream, lines, ref_len)) and len(parse_records(stream, lines)) == len(reads)
    got = p.sites(ref_text)
    assert got.dtype == spm.PILEUP_SITE_DTYPE
    assert sites_as_tuples(got) == py_sites(counts, 0, ref) == sites_as_tuples(spm.pileup_sites_host(counts, 0, ref))
    for pos, base in planted:
        (site,) = [x for x in got if x["pos"] == pos]
        assert (site["depth"], site["alt"], site["counts"][base], site["counts"][ref[pos]], site["ref"]) == (5, 3, 3, 2, ref[pos])
    assert len(got) == len(planted)
    for kw in (dict(min_alt=4), dict(min_alt=3, min_alt_permille=600), dict(min_alt_permille=601), dict(min_depth=0, min_alt=0, min_alt_permille=0),
               dict(min_depth=5, min_alt=0, min_alt_permille=0), dict(min_depth=6, min_alt=0, min_alt_permille=0)):
        assert sites_as_tuples(p.sites(ref_text, **kw)) == py_sites(counts, 0, ref, **kw), kw
    assert len(p.sites(ref_text, min_alt=4)) == 0 and len(p.sites(ref_text, min_depth=0, min_alt=0, min_alt_permille=0)) == ref_len
    # a reference one symbol short is refused; a pileup that ends where it ends is taken
    short = ctx.upload(ref[:-1])
    with pytest.raises(spm.SpmError, match="-1.*shorter"):
        p.sites(short)
    lo = planted[0][0] - 3
    part = s.pileup(begin=lo, end=ref_len - 1)
    assert sites_as_tuples(part.sites(short)) == py_sites(part.counts(), lo, ref) == [x for x in sites_as_tuples(got) if x[0] >= lo]
    dna5 = ctx.upload(ref, sigma=5)
    with pytest.raises(spm.SpmError, match="-1.*dna4"):
        p.sites(dna5)
    for x in (dna5, part, short, p, s, b, rd, lc, ps, ref_text) + rest:
        x.close()
