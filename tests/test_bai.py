"""CPU: the BAI index of a coordinate-sorted record stream by the serial host builder (spm_hip_bai_build_host) against the
builder of tests/bai_decode.py, which is written from the specification over the records tests/bam_decode.py decodes; the
standard region query through the index against a full scan; what the builder refuses; layouts and exported names."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

import bai_decode
from bam_decode import bam_to_sam, reg2bin, render_records
from cpp_programs import c_layout
from test_sam import LINE

INVALID, UNSUPPORTED = -1, -4
REF_LEN = 1 << 27                                                   # the smallest power of two behind the 2^26 border
BLOCK_SIZES = (1, 7, 256, 65280)


def make_stream(recs):
    """recs: (ref_id, pos, flag, cigar words) -> (the record stream, its LINE records).  36 fixed bytes, a two-byte name, the words;
    the bin is the specification's reg2bin over the record's interval."""
    out, lines = b"", np.zeros(len(recs), LINE)
    for i, (ref_id, pos, flag, words) in enumerate(recs):
        span = 0 if flag & 4 else sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))
        bin_ = reg2bin(pos, pos + max(span, 1)) if ref_id >= 0 else 4680
        body = struct.pack("<iiBBHHHIiii", ref_id, pos, 2, 0, bin_, len(words), flag, 0, -1, -1, 0) + b"r\0" + struct.pack(f"<{len(words)}I", *words)
        lines[i]["offset"], lines[i]["len"], lines[i]["flag"] = len(out), len(body) + 4, flag
        out += struct.pack("<i", len(body)) + body
    return out, lines


def stored_offsets(n_bytes, D, first):
    """the file offsets of stored blocks behind `first` bytes: n_blocks + 1 of them"""
    nb = (n_bytes + D - 1) // D
    return np.array([first + b * (D + 31) for b in range(nb)] + [first + n_bytes + 31 * nb], np.uint64)


M = lambda n: n << 4
NO_COOR = (-1, -1, 4, [])


def border_records():
    """at both sides of, on and across every bin-level border, two strands at one position, identical records, a placed
    unmapped mate, a long deletion, and two records without a position; windows 2 .. 6 and many more stay empty"""
    recs = [(0, 5, 0, [M(20)]), (0, 5, 16, [M(20)]), (0, 70, 0, [M(30), 5 << 4 | 1, 20 << 4 | 2, M(4)])]
    for shift in (14, 17, 20, 23, 26):
        at = 1 << shift
        recs += [(0, at - 40, 0, [M(30)]), (0, at - 40, 0, [M(30)]), (0, at - 10, 16, [M(20)]), (0, at - 1, 0, [M(1)]),
                 (0, at, 0, [M(30)]), (0, at, 0x85, []), (0, at + 1, 0, [7 << 4 | 7, 40000 << 4 | 3, 9 << 4 | 8])]
    return recs + [NO_COOR, NO_COOR]


CASES = {"borders": border_records(), "single": [(0, 16383, 0, [M(1)])], "only_no_coor": [NO_COOR] * 3, "none": [],
         "one_bin": [(0, 100 + i, 16 * (i & 1), [M(10)]) for i in range(12)]}


@pytest.mark.parametrize("D", BLOCK_SIZES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_host_builder_equals_the_specification(spm, case, D):
    stream, lines = make_stream(CASES[case])
    offsets = stored_offsets(len(stream), D, 123)
    got = spm.bai_build_host(stream, lines, offsets, D)
    records = render_records(stream, [("chr", REF_LEN)])
    assert [(o, n) for o, n, _l in records] == list(zip(lines["offset"].tolist(), lines["len"].tolist()))
    want = bai_decode.build_bai(records, offsets, D)
    assert got == want, (got.hex()[:400], want.hex()[:400])
    bai = bai_decode.parse_bai(got)
    n_placed = sum(1 for r in CASES[case] if r[0] == 0)
    assert bai["n_no_coor"] == len(CASES[case]) - n_placed and (bai["pseudo"] is not None) == (n_placed > 0)
    if case == "none":
        assert got == bytes.fromhex("42414901 01000000 00000000 00000000 0000000000000000") and len(got) == 24
    if case == "only_no_coor":
        assert len(got) == 24 and bai["n_no_coor"] == 3
    if case == "single":
        assert len(bai["ioffset"]) == 1 and bai["bins"] == [(4681, [(int(offsets[0]) << 16, bai_decode.voffset(offsets, D, len(stream)))])]
    if case == "one_bin":                                           # twelve consecutive records of one bin: one chunk
        assert [len(c) for _b, c in bai["bins"]] == [1] and bai["pseudo"][1] == (12, 0)
    if case == "borders":
        # (the record with the long N behind 2^14 reaches window 3; windows 4 .. 6 are empty and take window 7's value)
        assert bai["ioffset"][4] == bai["ioffset"][7] > bai["ioffset"][3] and bai["pseudo"][1] == (n_placed - 5, 5)
        assert len(bai["ioffset"]) == (((1 << 26) + 1 + 7 + 40000 + 9 - 1) >> 14) + 1
    if D == 65280 and case != "none":                               # the default block size by its 0
        assert spm.bai_build_host(stream, lines, offsets, 0) == got


@pytest.mark.parametrize("D", BLOCK_SIZES)
def test_fetch_finds_what_a_full_scan_finds(spm, D):
    stream, lines = make_stream(CASES["borders"])
    header = spm.bam_header("chr", REF_LEN, D, sorted=True)
    raw = header + spm.bgzf_frame_host(stream, D)
    text, payload, records, blocks = bam_to_sam(raw, D)
    assert payload == stream and text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n")
    record_blocks = [b for b in blocks if b[0] >= len(header)]
    offsets = stored_offsets(len(stream), D, len(header))
    assert [o for o, _p in record_blocks] == offsets[:-1].tolist()
    bai = bai_decode.parse_bai(spm.bai_build_host(stream, lines, offsets, D))
    qs = bai_decode.queries(bai_decode.intervals(records), REF_LEN)
    assert len(qs) > 60 and any(not bai_decode.scan(stream, b, e) for b, e in qs)
    for beg, end in qs:
        assert bai_decode.fetch(bai, record_blocks, beg, end) == bai_decode.scan(stream, beg, end), (beg, end)
    assert len(bai_decode.scan(stream, 0, REF_LEN)) == sum(1 for r in CASES["borders"] if r[0] == 0)


def test_refusals(spm):
    recs = [(0, 100, 0, [M(10)]), (0, 100, 16, [M(10)]), (0, 200, 0, [M(10)]), NO_COOR]
    stream, lines = make_stream(recs)
    D = 7
    offsets = stored_offsets(len(stream), D, 0)
    assert spm.bai_build_host(stream, lines, offsets, D)

    def refused(s=stream, l=lines, o=offsets, d=D, word="disagree"):
        with pytest.raises(spm.SpmError, match=f"-1.*{word}"):
            spm.bai_build_host(s, l, o, d)

    for order in ([1, 0, 2, 3], [0, 2, 1, 3], [0, 1, 3, 2], [3, 0, 1, 2]):   # out of coordinate order
        refused(*make_stream([recs[i] for i in order]), word="order")
    bad = lines.copy()
    bad["offset"][1] += 1                                           # does not follow the line before it
    refused(l=bad)
    bad = lines.copy()
    bad["len"][3] -= 1                                              # the last line does not end the stream
    refused(l=bad)
    bad = lines.copy()
    bad["len"][3] += 1                                              # ... or leaves it
    refused(l=bad)
    bad = lines.copy()
    bad["len"][2] += 4                                              # block_size is not len - 4
    refused(l=bad)
    broken = bytearray(stream)
    broken[int(lines["offset"][2]) + 16] = 9                        # a CIGAR that leaves its record
    refused(s=bytes(broken))
    broken = bytearray(stream)
    broken[int(lines["offset"][2]) + 4] = 1                         # refID 1 of one reference
    refused(s=bytes(broken))
    refused(*make_stream([(0, (1 << 29) - 5, 0, [M(6)])]), o=stored_offsets(42, D, 0))     # ends beyond 2^29
    assert spm.bai_build_host(*make_stream([(0, (1 << 29) - 5, 0, [M(5)])]), stored_offsets(42, D, 0), D)
    refused(o=offsets[:-1], word="n_blocks")
    refused(d=65281, word="block_data")
    refused(l=lines[:0], word="without")
    lib = spm.capi.lib()
    need = ctypes.c_uint64(7)
    assert lib.spm_hip_bai_build_host(None, 0, None, 0, offsets.ctypes.data, 0, D, None, 0, None) == INVALID
    assert lib.spm_hip_bai_build_host(None, 5, None, 0, offsets.ctypes.data, 1, D, None, 0, ctypes.byref(need)) == INVALID
    assert lib.spm_hip_bai_build_host(None, 0, None, 0, None, 0, D, None, 0, ctypes.byref(need)) == INVALID
    assert lib.spm_hip_bai_build_host(None, 0, None, 0, offsets.ctypes.data, 0, D, None, 0, ctypes.byref(need)) == -5 and need.value == 24
    with pytest.raises(spm.SpmError):
        spm.sam_header("*", 10, sorted=True)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_bam_sort_opts, f))
#define F(f) printf("sort.%s %zu\n", #f, offsetof(spm_bam_sort_stats, f))
#define S(f) printf("bai.%s %zu\n", #f, offsetof(spm_bai_stats, f))
int main(void)
{
    O(reserved);
    F(ms_total); F(ms_keys); F(ms_sort); F(ms_place); F(ms_gather); F(ms_frame); F(ms_host); F(key_bits); F(n_records); F(n_record_bytes);
    S(ms_total); S(ms_records); S(ms_chunks); S(ms_bins); S(ms_write); S(ms_host); S(n_bins); S(n_chunks); S(n_intv); S(n_mapped);
    S(n_unmapped); S(n_no_coor); S(n_bytes);
    printf("sizeof.opts %zu\nsizeof.sort %zu\nsizeof.bai %zu\n", sizeof(spm_bam_sort_opts), sizeof(spm_bam_sort_stats), sizeof(spm_bai_stats));
    return 0;
}
"""
CALLS = ("spm_hip_bam_sort", "spm_hip_bam_sort_stats", "spm_hip_sam_header_sorted", "spm_hip_bam_header_sorted", "spm_hip_bam_index",
         "spm_hip_bai_build", "spm_hip_bai_build_host", "spm_hip_bai_view", "spm_hip_bai_device", "spm_hip_bai_stats", "spm_hip_bai_destroy")


def test_layouts_and_names(spm, tmp_path):
    kinds = {"opts": spm.capi.BamSortOpts, "sort": spm.capi.BamSortStats, "bai": spm.capi.BaiStats}
    want = c_layout(tmp_path, LAYOUT_C)
    sizes = {k: int(want.pop("sizeof." + k)) for k in kinds}
    assert sizes == {"opts": 8, "sort": 48, "bai": 80} == {k: ctypes.sizeof(t) for k, t in kinds.items()}
    seen = dict.fromkeys(kinds, 0)
    for name, off in want.items():
        kind, field = name.split(".")
        assert getattr(kinds[kind], field).offset == int(off), name
        seen[kind] += 1
    assert seen == {k: len(t._fields_) for k, t in kinds.items()} == {"opts": 1, "sort": 10, "bai": 13}
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    Bai = spm.engine.Bai                                            # the handle of an index: closed and released as every other handle is
    assert Bai._PREFIX == "bai" and Bai.close is spm.Bam.close and Bai.__del__ is spm.Bam.__del__
    for f in (spm.Bam.sort, spm.Bam.sort_stats, spm.Bam.index, Bai.bytes, Bai.device, Bai.stats, Bai.close, spm.Context.bai,
              spm.bai_build_host):
        assert callable(f)
    assert list(inspect.signature(spm.Bam.index).parameters)[1:] == ["deflated"] and list(inspect.signature(spm.Bam.sort).parameters) == ["self"]
    assert list(inspect.signature(spm.Context.bai).parameters)[1:] == ["records", "n_record_bytes", "lines", "n_lines", "block_offsets",
                                                                       "n_blocks", "block_data"]
    assert inspect.signature(spm.sam_header).parameters["sorted"].default is False
    assert inspect.signature(spm.bam_header).parameters["sorted"].default is False
    # the existing header calls keep their bytes; the siblings differ in the SO field alone
    assert spm.sam_header("chr", 100) == b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr\tLN:100\n"
    assert spm.sam_header("chr", 100, sorted=True) == b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr\tLN:100\n"
    plain = bam_to_sam(spm.bam_header("chr", 100, sorted=True) + spm.bgzf_frame_host(b""))
    assert plain[0] == spm.sam_header("chr", 100, sorted=True) and plain[1] == b""
