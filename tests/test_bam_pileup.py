"""CPU: the pileup by the serial host builder (spm_hip_bam_pileup_host) and its variant sites (spm_hip_pileup_sites_host) on
hand-built record streams: the worked table of spm_hip.h, against the table itself and against the rule written again in
tests/pileup_rule.py; quality, MAPQ and flag thresholds; regions; every refusal on the host, every counted disagreement; the
thresholds of the sites at their edges; layouts and exported names."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

from cpp_programs import c_layout
from pileup_rule import PLANES, make_stream, py_pileup, py_sites, sites_as_tuples
from test_sam import LINE

INVALID, UNSUPPORTED, OVERFLOW = -1, -4, -5
REF_LEN = 1000
A, C, G, T, N, DEL, INS, LOWQ = range(8)


def worked_table():
    """the table of spm_hip.h and bam_pileup_core.hpp"""
    R = lambda pos, cigar, seq, **kw: dict(pos=pos, cigar=cigar, seq=seq, **kw)
    return [R(10, "4M", "ACGT"), R(10, "2=1X1=", "ACNT"), R(11, "2M2D2M", "CGAA"), R(12, "2M3N2M", "GTCC"), R(12, "2I3M", "TTGTA"),
            R(12, "2S1I3M", "AATGTA"), R(13, "2M2I2M", "TAGGAC"), R(13, "3M2S", "TAACC"), R(14, "2H3M1P2M3H", "AACAC"),
            R(15, "3M", "ACG", qual=[0, 20, 255]), R(15, "3M", "AAA", flag=0x400),
            dict(pos=-1, ref_id=-1, flag=4, cigar="", seq="ACGTA")]


WORKED_WANT = {(A, 10): 2, (A, 14): 5, (A, 15): 5, (A, 16): 1, (A, 17): 1, (C, 11): 3, (C, 16): 3, (C, 17): 1, (C, 18): 2, (G, 12): 5,
               (G, 17): 1, (T, 13): 7, (N, 12): 1, (DEL, 13): 1, (DEL, 14): 1, (INS, 14): 1}


def as_counts(want, n=REF_LEN, begin=0):
    out = np.zeros((8, n), np.uint32)
    for (plane, pos), v in want.items():
        if begin <= pos < begin + n:
            out[plane, pos - begin] = v
    return out


def check(spm, stream, lines, ref_len=REF_LEN, **kw):
    """host builder == the Python rule -> the counts"""
    got = spm.bam_pileup_host(stream, lines, ref_len, **kw)
    want = py_pileup(stream, lines, ref_len, **kw)
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:8]
    return got


def test_worked_table_of_the_header(spm):
    stream, lines = make_stream(worked_table())
    got = check(spm, stream, lines)
    assert np.array_equal(got, as_counts(WORKED_WANT)), np.argwhere(got != as_counts(WORKED_WANT))
    assert spm.PILEUP_PLANES == PLANES and int(got.sum()) == sum(WORKED_WANT.values())
    # min_baseq at 0 / 1 / 93: quality 0 falls at 1, quality 20 at 93, ff never
    for min_baseq, low in ((0, []), (1, [15]), (20, [15]), (21, [15, 16]), (93, [15, 16])):
        got = check(spm, stream, lines, min_baseq=min_baseq)
        want = dict(WORKED_WANT)
        for col in low:
            want[(LOWQ, col)] = 1
            plane = {15: A, 16: C}[col]
            want[(plane, col)] -= 1
        assert np.array_equal(got, as_counts(want)), min_baseq
        assert got[G, 17] == 1 and got[LOWQ].sum() == len(low)      # every other record has ff qualities
    # the duplicate takes part once 0x400 is not excluded
    got = check(spm, stream, lines, exclude_flags=0x4)
    want = dict(WORKED_WANT)
    for col in (15, 16, 17):
        want[(A, col)] = want.get((A, col), 0) + 1
    assert np.array_equal(got, as_counts(want))


def test_mapq_and_every_exclude_bit(spm):
    recs = [dict(pos=5, cigar="3M", seq="AAA", mapq=0), dict(pos=5, cigar="3M", seq="CCC", mapq=29), dict(pos=5, cigar="3M", seq="GGG", mapq=30),
            dict(pos=6, cigar="3M", seq="TTT", mapq=255)]
    stream, lines = make_stream(recs)
    for min_mapq, planes in ((0, (A, C, G, T)), (1, (C, G, T)), (29, (C, G, T)), (30, (G, T)), (31, (T,)), (255, (T,))):
        got = check(spm, stream, lines, min_mapq=min_mapq)
        assert [p for p in range(8) if got[p].any()] == list(planes), min_mapq
    bits = (0x1, 0x2, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800)
    recs = [dict(pos=20 + 2 * i, cigar="2M", seq="CC", flag=bit) for i, bit in enumerate(bits)] + [dict(pos=50, cigar="2M", seq="CC", flag=4)]
    stream, lines = make_stream(recs)
    got = check(spm, stream, lines)                                 # the default: 0x100, 0x200, 0x400 and 0x4 stay out
    assert [int(got[C, 20 + 2 * i]) for i in range(len(bits))] == [int(not bit & 0x704) for bit in bits] and got[C, 50] == 0
    assert np.array_equal(got, check(spm, stream, lines, exclude_flags=0x704)) and np.array_equal(got, check(spm, stream, lines, exclude_flags=0x700))
    got = check(spm, stream, lines, exclude_flags=0x4)              # nothing but the unmapped record stays out
    assert [int(got[C, 20 + 2 * i]) for i in range(len(bits))] == [1] * len(bits) and got[C, 50] == 0
    for bit in bits:                                                # each bit on its own; 0x4 is always excluded
        got = check(spm, stream, lines, exclude_flags=bit)
        assert [int(got[C, 20 + 2 * i]) for i in range(len(bits))] == [int(b != bit) for b in bits] and got[C, 50] == 0


def test_regions_and_empty_inputs(spm):
    stream, lines = make_stream(worked_table())
    whole = as_counts(WORKED_WANT)
    for begin, end in ((0, REF_LEN), (10, 19), (11, 18), (12, 13), (13, 15), (14, 14), (0, 10), (19, REF_LEN), (16, 17), (999, 1000), (1000, 1000)):
        got = check(spm, stream, lines, begin=begin, end=end)
        assert got.shape == (8, end - begin) and np.array_equal(got, whole[:, begin:end]), (begin, end)
    assert np.array_equal(check(spm, stream, lines, begin=12), whole[:, 12:])   # end None: ref_len
    got = spm.bam_pileup_host(b"", np.zeros(0, LINE), REF_LEN)                  # zero records: all-zero counts
    assert got.shape == (8, REF_LEN) and not got.any()
    assert spm.bam_pileup_host(b"", np.zeros(0, LINE), 0).shape == (8, 0)
    # a record that ends at ref_len, one that begins at 0, and a long deletion across the region's borders
    recs = [dict(pos=0, cigar="3M", seq="GAT"), dict(pos=2, cigar="2M500D2M", seq="ACGT"), dict(pos=REF_LEN - 3, cigar="3M", seq="TTT")]
    stream, lines = make_stream(recs)
    got = check(spm, stream, lines)
    assert got[DEL, 4:504].tolist() == [1] * 500 and got[G, 0] == 1 and got[T, REF_LEN - 1] == 1 and got[:, 504:506].sum() == 2
    for begin, end in ((3, 5), (100, 200), (503, 505), (REF_LEN - 1, REF_LEN)):
        assert np.array_equal(check(spm, stream, lines, begin=begin, end=end), got[:, begin:end])


def test_out_of_order_is_refused(spm):
    recs = worked_table()
    stream, lines = make_stream(recs)
    counts = np.full((8, REF_LEN), 7, np.uint32)
    src = ctypes.create_string_buffer(stream, len(stream))
    call = spm.capi.lib().spm_hip_bam_pileup_host
    assert call(src, len(stream), lines.ctypes.data, len(lines), REF_LEN, None, counts.ctypes.data) == 0 and np.array_equal(counts, as_counts(WORKED_WANT))
    rng = np.random.default_rng(5)
    refused = 0
    for _ in range(8):
        order = rng.permutation(len(recs))
        s, l = make_stream([recs[i] for i in order])
        pos = [recs[i]["pos"] if recs[i].get("ref_id", 0) == 0 else 1 << 40 for i in order]
        counts[:] = 7
        src = ctypes.create_string_buffer(s, len(s))
        rc = call(src, len(s), l.ctypes.data, len(l), REF_LEN, None, counts.ctypes.data)
        if pos == sorted(pos):
            assert rc == 0
        else:
            refused += 1
            assert rc == INVALID and (counts == 7).all()
            with pytest.raises(spm.SpmError, match="-1.*order"):
                spm.bam_pileup_host(s, l, REF_LEN)
    assert refused >= 6


def disagreements():
    """{name: (stream, lines, ref_len)}: each a hand-built stream with one thing wrong -- shared with the device's tests"""
    base = worked_table()
    stream, lines = make_stream(base)
    out = {}

    def with_lines(name, **change):
        bad = lines.copy()
        for field, (i, v) in change.items():
            bad[field][i] = v
        out[name] = (stream, bad, REF_LEN)

    def with_bytes(name, at, value):
        b = bytearray(stream)
        b[at:at + len(value)] = value
        out[name] = (bytes(b), lines, REF_LEN)

    last = len(lines) - 1
    o0, o3, o10 = int(lines["offset"][0]), int(lines["offset"][3]), int(lines["offset"][10])
    with_lines("line_leaves_the_stream", len=(last, int(lines["len"][last]) + 1))
    with_lines("offset_beyond_the_stream", offset=(last, len(stream) + 1))
    with_lines("block_size_is_not_len_less_4", len=(2, int(lines["len"][2]) - 4))
    with_bytes("name_leaves_the_record", o3 + 12, b"\xff")
    with_bytes("cigar_leaves_the_record", o3 + 16, struct.pack("<H", 60000))
    with_bytes("seq_leaves_the_record", o3 + 20, struct.pack("<I", 0xFFFFFFFF))
    with_bytes("qual_leaves_the_record", o3 + 20, struct.pack("<I", 5))           # l_seq 5 of 4: one more SEQ byte, one more quality
    with_bytes("refid_1", int(lines["offset"][9]) + 4, struct.pack("<i", 1))      # the last record that takes part
    with_bytes("negative_pos", o0 + 8, struct.pack("<i", -1))
    out["end_beyond_ref_len"] = (stream, lines, 18)                               # records 3 and 8 end at 19
    with_bytes("op_code_9", o3 + 36 + 2, struct.pack("<I", 2 << 4 | 9))           # the first CIGAR word of record 3 (name "r\0")
    out["query_length_is_not_l_seq"] = make_stream(base[:3] + [dict(pos=12, cigar="4M", seq="ACGTA")] + base[4:]) + (REF_LEN,)
    out["pos_descends"] = make_stream(base[:2] + [base[3], base[2]] + base[4:]) + (REF_LEN,)
    out["placed_behind_unplaced"] = make_stream(base[:5] + [base[11]] + base[5:11]) + (REF_LEN,)
    out["excluded_record_out_of_order"] = make_stream(base[:10] + [dict(base[10], pos=3)] + base[11:]) + (REF_LEN,)
    return out


def test_counted_disagreements(spm):
    cases = disagreements()
    assert len(cases) == 15
    call = spm.capi.lib().spm_hip_bam_pileup_host
    for name, (stream, lines, ref_len) in cases.items():
        with pytest.raises(spm.SpmError, match="-1.*disagree"):
            spm.bam_pileup_host(stream, lines, ref_len)
        src = ctypes.create_string_buffer(stream, len(stream))
        counts = np.full((8, ref_len), 7, np.uint32)
        assert call(src, len(stream), lines.ctypes.data, len(lines), ref_len, None, counts.ctypes.data) == INVALID, name
        assert (counts == 7).all(), name                            # nothing written
    # what is NOT a disagreement: the same conditions on records that do not take part
    base = worked_table()
    quiet = base[:10] + [dict(pos=15, cigar="3M", seq="AAA", flag=0x400, ref_id=1), dict(pos=990, cigar="30M", flag=0x100),
                         dict(pos=995, words=[3 << 4 | 12], seq="AAA", flag=0x200), dict(pos=996, cigar="4M", seq="AAA", flag=0x400)] + base[11:]
    stream, lines = make_stream(quiet[:10] + quiet[11:])            # (without the refID 1 record, which would break the order)
    assert np.array_equal(spm.bam_pileup_host(stream, lines, REF_LEN), as_counts(WORKED_WANT))
    stream, lines = make_stream(base[:11] + [dict(pos=20, cigar="3M", seq="AAA", flag=4, ref_id=1)] + base[11:])   # refID 1 behind refID 0, skipped
    assert np.array_equal(spm.bam_pileup_host(stream, lines, REF_LEN), as_counts(WORKED_WANT))
    stream, lines = make_stream(base)
    assert np.array_equal(spm.bam_pileup_host(stream, lines, 19), as_counts(WORKED_WANT, 19))   # end == ref_len


def test_host_refusals(spm):
    lib = spm.capi.lib()
    stream, lines = make_stream(worked_table())
    src = ctypes.create_string_buffer(stream, len(stream))
    counts = np.full((8, REF_LEN), 7, np.uint32)
    Opts = spm.capi.PileupOpts

    def call(records=src, n_bytes=len(stream), l=lines.ctypes.data, n=len(lines), ref_len=REF_LEN, opts=None, c=counts.ctypes.data):
        return lib.spm_hip_bam_pileup_host(records, n_bytes, l, n, ref_len, ctypes.byref(opts) if opts is not None else None, c)

    for rc, kw in ((INVALID, dict(records=None)), (INVALID, dict(l=None)), (INVALID, dict(c=None)), (INVALID, dict(n=0)), (INVALID, dict(n_bytes=0)),
                   (INVALID, dict(opts=Opts(flags=1))), (INVALID, dict(opts=Opts(reserved0=1))), (INVALID, dict(opts=Opts(reserved1=1))),
                   (INVALID, dict(opts=Opts(min_baseq=94))), (INVALID, dict(opts=Opts(begin=11, end=10))), (INVALID, dict(opts=Opts(end=REF_LEN + 1))),
                   (INVALID, dict(opts=Opts(begin=REF_LEN + 1))), (UNSUPPORTED, dict(ref_len=(1 << 31) + 1)), (UNSUPPORTED, dict(n=1 << 32))):
        assert call(**kw) == rc, kw
        assert (counts == 7).all()
    assert call(opts=Opts(min_baseq=93, min_mapq=255)) == 0 and not counts.any()
    assert call(opts=Opts(begin=REF_LEN)) == 0 and call(opts=Opts(begin=5, end=5), c=None) == 0   # empty regions
    with pytest.raises(spm.SpmError, match="-1.*min_baseq"):
        spm.bam_pileup_host(stream, lines, REF_LEN, min_baseq=94)
    with pytest.raises(spm.SpmError, match="-1.*region"):
        spm.bam_pileup_host(stream, lines, REF_LEN, begin=30, end=20)


def site_columns():
    """hand-made columns: (8, n) counts, the reference ranks under them"""
    cols = [  # (reference rank, {plane: count})
        (0, {A: 3, C: 2}),               # depth 5, alt 2
        (0, {A: 4, C: 1}),               # alt 1 = min_alt - 1
        (1, {C: 8, T: 2}),               # depth 10, alt 2: 1000 * 2 == 200 * 10
        (1, {C: 9, T: 2}),               # depth 11, alt 2: 2000 < 2200
        (0, {A: 5, INS: 2}),             # INS is in alt, not in depth
        (2, {LOWQ: 9}),                  # LOWQ is outside both: depth 0
        (3, {T: 2, DEL: 3, N: 1}),       # DEL and N count in depth and in alt
        (4, {N: 4, A: 2}),               # a reference rank above 3 takes plane N
        (2, {}),                         # an empty column
        (3, {A: 1, C: 1, G: 1, T: 1, N: 1, DEL: 1, INS: 2, LOWQ: 1}),   # alt 7 above depth 6
    ]
    counts = np.zeros((8, len(cols)), np.uint32)
    for k, (_r, planes) in enumerate(cols):
        for plane, v in planes.items():
            counts[plane, k] = v
    return counts, np.array([r for r, _p in cols], np.uint8)


def test_sites_thresholds_at_their_edges(spm):
    counts, ranks = site_columns()
    begin = 40
    ref = np.concatenate([np.zeros(begin, np.uint8), ranks, np.zeros(7, np.uint8)])
    got = spm.pileup_sites_host(counts, begin, ref)                 # the defaults: 1, 2, 200
    assert got.dtype == spm.PILEUP_SITE_DTYPE and got.dtype.itemsize == 32
    assert sites_as_tuples(got) == py_sites(counts, begin, ref) == [
        (40, 5, 2, (3, 2, 0, 0), 0), (42, 10, 2, (0, 8, 0, 2), 1), (44, 5, 2, (5, 0, 0, 0), 0), (46, 6, 4, (0, 0, 0, 2), 3),
        (47, 6, 2, (2, 0, 0, 0), 4), (49, 6, 7, (1, 1, 1, 1), 3)]
    assert not got["reserved"].any()
    for kw in (dict(min_alt=1), dict(min_alt=3), dict(min_alt_permille=199), dict(min_alt_permille=201), dict(min_alt_permille=400),
               dict(min_alt_permille=401), dict(min_depth=6), dict(min_depth=7), dict(min_depth=0, min_alt=0, min_alt_permille=0),
               dict(min_depth=0, min_alt=0, min_alt_permille=1000), dict(min_alt_permille=1001)):
        got = sites_as_tuples(spm.pileup_sites_host(counts, begin, ref, **kw))
        assert got == py_sites(counts, begin, ref, **kw), kw
    pos = lambda **kw: [s[0] for s in sites_as_tuples(spm.pileup_sites_host(counts, begin, ref, **kw))]
    assert 41 in pos(min_alt=1) and 41 not in pos(min_alt=2)        # alt == min_alt - 1 stays out
    assert 42 in pos(min_alt_permille=200) and 42 not in pos(min_alt_permille=201) and 43 not in pos(min_alt_permille=200)
    assert pos(min_depth=0, min_alt=0, min_alt_permille=0) == list(range(40, 50)) and 45 not in pos(min_depth=1, min_alt=0, min_alt_permille=0)
    assert pos(min_alt_permille=1001) == [49]                       # INS lifts alt above depth there alone
    # refusals: a reference shorter than the pileup's end, flags, a capacity that is too small (the count is still written)
    lib, Opts = spm.capi.lib(), spm.capi.PileupSiteOpts
    dst, n = np.zeros(10, spm.PILEUP_SITE_DTYPE), ctypes.c_uint64(77)
    args = lambda ref_len=len(ref), opts=None, cap=10: (counts.ctypes.data, begin, counts.shape[1], ref.ctypes.data, ref_len,
                                                        ctypes.byref(opts) if opts is not None else None, dst.ctypes.data, cap, ctypes.byref(n))
    assert lib.spm_hip_pileup_sites_host(*args()) == 0 and n.value == 6
    assert lib.spm_hip_pileup_sites_host(*args(ref_len=begin + 9)) == INVALID
    assert lib.spm_hip_pileup_sites_host(*args(ref_len=begin + 10)) == 0
    assert lib.spm_hip_pileup_sites_host(*args(opts=Opts(1, 2, 200, 1))) == INVALID
    n.value = 0
    assert lib.spm_hip_pileup_sites_host(*args(cap=5)) == OVERFLOW and n.value == 6
    with pytest.raises(spm.SpmError, match="-1.*shorter"):
        spm.pileup_sites_host(counts, begin, ref[:begin + 9])


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_pileup_opts, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_pileup_stats, f))
#define T(f) printf("site.%s %zu\n", #f, offsetof(spm_pileup_site, f))
#define U(f) printf("siteopts.%s %zu\n", #f, offsetof(spm_pileup_site_opts, f))
int main(void)
{
    O(begin); O(end); O(exclude_flags); O(min_mapq); O(min_baseq); O(reserved0); O(flags); O(reserved1);
    S(ms_total); S(ms_records); S(ms_scan); S(ms_tiles); S(ms_summary); S(ms_host); S(tile_positions); S(reserved); S(n_records);
    S(n_taking_part); S(n_evidence); S(n_covered); S(sum_depth); S(max_depth); S(n_tile_visits);
    T(pos); T(depth); T(alt); T(counts); T(ref); T(reserved);
    U(min_depth); U(min_alt); U(min_alt_permille); U(flags);
    printf("sizeof.opts %zu\nsizeof.stats %zu\nsizeof.site %zu\nsizeof.siteopts %zu\n", sizeof(spm_pileup_opts), sizeof(spm_pileup_stats),
           sizeof(spm_pileup_site), sizeof(spm_pileup_site_opts));
    printf("planes.n %d\nplanes.lowq %d\nplanes.del %d\n", SPM_PILEUP_PLANES, SPM_PILEUP_LOWQ, SPM_PILEUP_DEL);
    return 0;
}
"""
CALLS = ("spm_hip_bam_pileup", "spm_hip_bam_pileup_records", "spm_hip_bam_pileup_host", "spm_hip_pileup_view", "spm_hip_pileup_device",
         "spm_hip_pileup_stats", "spm_hip_pileup_destroy", "spm_hip_pileup_sites", "spm_hip_pileup_sites_view", "spm_hip_pileup_sites_device",
         "spm_hip_pileup_sites_destroy", "spm_hip_pileup_sites_host")


def test_layouts_and_names(spm, tmp_path):
    kinds = {"opts": spm.capi.PileupOpts, "stats": spm.capi.PileupStats, "site": spm.capi.PileupSite, "siteopts": spm.capi.PileupSiteOpts}
    want = c_layout(tmp_path, LAYOUT_C)
    assert (want.pop("planes.n"), want.pop("planes.lowq"), want.pop("planes.del")) == ("8", "7", "5") and len(spm.PILEUP_PLANES) == 8
    sizes = {k: int(want.pop("sizeof." + k)) for k in kinds}
    assert sizes == {"opts": 32, "stats": 88, "site": 32, "siteopts": 16} == {k: ctypes.sizeof(t) for k, t in kinds.items()}
    seen = dict.fromkeys(kinds, 0)
    for name, off in want.items():
        kind, field = name.split(".")
        assert getattr(kinds[kind], field).offset == int(off), name
        seen[kind] += 1
    assert seen == {k: len(t._fields_) for k, t in kinds.items()} == {"opts": 8, "stats": 15, "site": 6, "siteopts": 4}
    assert spm.PILEUP_SITE_DTYPE.itemsize == 32 and spm.PILEUP_SITE_DTYPE["counts"].shape == (4,)
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    for f in (spm.Bam.pileup, spm.Context.bam_pileup, spm.bam_pileup_host, spm.pileup_sites_host, spm.engine.Pileup.counts, spm.engine.Pileup.device,
              spm.engine.Pileup.stats, spm.engine.Pileup.depth, spm.engine.Pileup.sites):
        assert callable(f)
    assert list(inspect.signature(spm.Bam.pileup).parameters) == ["self", "begin", "end", "min_mapq", "min_baseq", "exclude_flags"]
    assert [p.default for p in inspect.signature(spm.Bam.pileup).parameters.values()][1:] == [0, None, 0, 0, None]
    assert list(inspect.signature(spm.engine.Pileup.sites).parameters) == ["self", "reference", "min_depth", "min_alt", "min_alt_permille"]
    assert [p.default for p in inspect.signature(spm.engine.Pileup.sites).parameters.values()][2:] == [1, 2, 200]
