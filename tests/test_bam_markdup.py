"""CPU: duplicate marking by the serial host builder (spm_hip_bam_markdup_host) on hand-built record streams: the worked cases
of spm_hip.h, against the header's own table and against the rule written again in tests/markdup_rule.py over the SAM text of
the records; every refusal on the host, every counted disagreement; layouts and exported names."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

from bam_decode import reg2bin
from cpp_programs import c_layout
from markdup_rule import py_markdup
from test_gpu_sam_qual_md import decode_records
from test_sam import LINE

INVALID, UNSUPPORTED = -1, -4
REF_LEN = 10000
EQ = lambda n: n << 4 | 7


def make_stream(recs, name=b"r"):
    """recs: dicts with read, flag, pos, words and optionally ref_id, l_seq (the CIGAR's query length), qual (Phred values; ff
    without), secondary stuff left out -> (the record stream, its LINE records).  36 fixed bytes, the name, the words, a SEQ of A,
    the qualities; the bin is the specification's."""
    out, lines = b"", np.zeros(len(recs), LINE)
    for i, r in enumerate(recs):
        words, flag, pos, ref_id = r.get("words", []), r["flag"], r["pos"], r.get("ref_id", 0)
        span = 0 if flag & 4 else sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))
        l_seq = r.get("l_seq", sum(w >> 4 for w in words if (w & 15) in (0, 1, 4, 7, 8)))
        qual = bytes(r["qual"]) if "qual" in r else b"\xff" * l_seq
        assert len(qual) == l_seq
        bin_ = reg2bin(pos, pos + max(span, 1)) if pos >= 0 else 4680
        nm = name + b"\0"
        body = (struct.pack("<iiBBHHHIiii", ref_id, pos, len(nm), 0, bin_, len(words), flag, l_seq, -1, -1, 0) + nm +
                struct.pack(f"<{len(words)}I", *words) + b"\x11" * (l_seq // 2) + (b"\x10" if l_seq & 1 else b"") + qual)
        lines[i]["offset"], lines[i]["len"], lines[i]["flag"], lines[i]["read"] = len(out), len(body) + 4, flag, r["read"]
        out += struct.pack("<i", len(body)) + body
    return out, lines


def sam_lines(stream):
    return [line for _o, _n, line in decode_records(stream, [("chr", REF_LEN)])]


def worked_cases(quals=False):
    """the table of spm_hip.h; read 5 is an unmapped read without a position"""
    R = lambda read, flag, pos, *words, **kw: dict(read=read, flag=flag, pos=pos, words=list(words), **kw)
    q0 = dict(qual=[10] * 40) if quals else {}
    q1 = dict(qual=[30] * 30) if quals else {}
    return [R(0, 0, 100, EQ(40), **q0), R(1, 0, 100, EQ(30), **q1), R(2, 16, 111, EQ(30)), R(3, 16, 101, EQ(40)), R(4, 16, 100, EQ(40)),
            R(5, 4, -1, ref_id=-1, l_seq=20),
            R(6, 97, 1000, EQ(100)), R(7, 145, 1100, EQ(100)), R(8, 97, 1000, EQ(100)), R(9, 145, 1100, EQ(100)),
            R(10, 97, 1000, EQ(100)), R(11, 145, 1200, EQ(100)), R(12, 73, 1000, EQ(50)), R(13, 133, 1000, l_seq=50)]


def test_worked_cases_of_the_header(spm):
    stream, lines = make_stream(worked_cases())
    got = spm.bam_markdup_host(stream, lines, REF_LEN)
    assert got.dtype == np.uint8 and got.tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0]
    want, counts = py_markdup(sam_lines(stream), lines["read"])
    assert want == got.tolist()
    assert counts == dict(n_records=14, n_pairs=3, n_fragments=6, n_dup_pairs=1, n_dup_fragments=3, n_dup_records=5,
                          n_fragments_beside_pairs=1)
    # the variation: with qualities the shorter read 1 scores 900, read 0 nothing (Phred 10 lies below the default min_qual)
    stream, lines = make_stream(worked_cases(quals=True))
    got = spm.bam_markdup_host(stream, lines, REF_LEN)
    assert got.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0] == py_markdup(sam_lines(stream), lines["read"])[0]
    got = spm.bam_markdup_host(stream, lines, REF_LEN, min_qual=10)  # 400 against 900: the same
    assert got.tolist()[:2] == [1, 0] and got.tolist() == py_markdup(sam_lines(stream), lines["read"], 10)[0]
    got = spm.bam_markdup_host(stream, lines, REF_LEN, min_qual=31)  # 0 against 0: the lowest read stays
    assert got.tolist()[:2] == [0, 1] and got.tolist() == py_markdup(sam_lines(stream), lines["read"], 31)[0]


def test_order_flags_and_scores(spm):
    rng = np.random.default_rng(77)
    # any order of the records gives the same marks by read; an incoming 0x400 is ignored
    recs = worked_cases(quals=True)
    base = spm.bam_markdup_host(*make_stream(recs), REF_LEN)
    for _ in range(6):
        order = rng.permutation(len(recs))
        shuffled = [dict(recs[i], flag=recs[i]["flag"] | (0x400 if rng.integers(2) else 0)) for i in order]
        stream, lines = make_stream(shuffled)
        got = spm.bam_markdup_host(stream, lines, REF_LEN)
        assert got.tolist() == base[order].tolist() == py_markdup(sam_lines(stream), lines["read"])[0]
    # secondary and supplementary records beside duplicates stay clear and do not count as a second primary
    recs = worked_cases() + [dict(read=1, flag=0x100, pos=100, words=[EQ(30)], l_seq=0), dict(read=0, flag=0x800, pos=100, words=[EQ(40)])]
    stream, lines = make_stream(recs)
    got = spm.bam_markdup_host(stream, lines, REF_LEN)
    assert got.tolist()[-2:] == [0, 0] and got.tolist() == py_markdup(sam_lines(stream), lines["read"])[0]
    # values above 93 do not count; the clamp at 2^24 - 1 makes a tie that the lowest read wins
    big = 183_000                                                   # 183 000 x 92 > 2^24 - 1
    recs = [dict(read=0, flag=0, pos=5, words=[EQ(big)], qual=[92] * big), dict(read=1, flag=0, pos=5, words=[EQ(big)], qual=[93] * big),
            dict(read=2, flag=0, pos=5, words=[EQ(4)], qual=[94, 200, 255, 93]), dict(read=3, flag=0, pos=5, words=[EQ(3)], qual=[40, 40, 14])]
    stream, lines = make_stream(recs)
    assert big * 92 > (1 << 24) - 1
    assert spm.bam_markdup_host(stream, lines, 1 << 20).tolist() == [0, 1, 1, 1]
    recs = recs[2:]
    stream, lines = make_stream([dict(r, read=i) for i, r in enumerate(recs)])
    assert spm.bam_markdup_host(stream, lines, 1 << 20).tolist() == [0, 1]       # 93 against 80
    assert spm.bam_markdup_host(stream, lines, 1 << 20, min_qual=1).tolist() == [1, 0]   # 93 against 94
    assert len(spm.bam_markdup_host(b"", np.zeros(0, LINE), REF_LEN)) == 0


def test_host_refusals(spm):
    lib = spm.capi.lib()
    stream, lines = make_stream(worked_cases())
    src = ctypes.create_string_buffer(stream, len(stream))
    dup = np.full(len(lines), 7, np.uint8)
    Opts = spm.capi.BamMarkdupOpts

    def call(records=src, n_bytes=len(stream), l=lines.ctypes.data, n=len(lines), ref_len=REF_LEN, opts=None, d=dup.ctypes.data):
        return lib.spm_hip_bam_markdup_host(records, n_bytes, l, n, ref_len, ctypes.byref(opts) if opts is not None else None, d)

    assert call() == 0 and dup.tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0]                 # NULL opts: the defaults
    dup[:] = 7
    for rc, kw in ((INVALID, dict(records=None)), (INVALID, dict(l=None)), (INVALID, dict(d=None)), (INVALID, dict(n=0)),
                   (INVALID, dict(n_bytes=0)), (INVALID, dict(opts=Opts(0, 1, 0))), (INVALID, dict(opts=Opts(0, 0, 1))),
                   (INVALID, dict(opts=Opts(94, 0, 0))), (UNSUPPORTED, dict(ref_len=1 << 30)), (UNSUPPORTED, dict(n=1 << 32))):
        assert call(**kw) == rc, kw
        assert dup.tolist() == [7] * len(dup)
    assert call(opts=Opts(93, 0, 0)) == 0 and call(ref_len=(1 << 30) - 1) == 0
    assert call(records=None, n_bytes=0, l=None, n=0, d=None) == 0   # nothing to mark
    with pytest.raises(spm.SpmError, match="-1.*min_qual"):
        spm.bam_markdup_host(stream, lines, REF_LEN, min_qual=94)
    with pytest.raises(spm.SpmError, match="-4.*2\\^30"):
        spm.bam_markdup_host(stream, lines, 1 << 30)


def disagreements():
    """{name: (stream, lines, ref_len)}: each a hand-built stream with one thing wrong -- shared with the device's tests"""
    base = worked_cases()
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

    o3 = int(lines["offset"][3])
    out["second_primary"] = make_stream(base + [dict(read=2, flag=0, pos=300, words=[EQ(20)])]) + (REF_LEN,)
    with_lines("read_beyond_the_lines", read=(4, len(lines)))
    out["an_S_item"] = make_stream(base[:4] + [dict(read=4, flag=0, pos=100, words=[5 << 4 | 4, EQ(35)])]) + (REF_LEN,)
    out["an_H_item"] = make_stream(base[:4] + [dict(read=4, flag=16, pos=100, words=[EQ(35), 5 << 4 | 5], l_seq=35)]) + (REF_LEN,)
    out["end_beyond_ref_len"] = (stream, lines, 1299)               # read 11 ends at 1300
    with_bytes("qual_leaves_the_record", o3 + 20, struct.pack("<I", 41))          # l_seq 41 of 40: seq stays 20 bytes, qual 41
    with_bytes("seq_leaves_the_record", o3 + 20, struct.pack("<I", 0xFFFFFFFF))
    with_lines("line_leaves_the_stream", len=(13, int(lines["len"][13]) + 1))
    with_lines("offset_beyond_the_stream", offset=(13, len(stream) + 1))
    with_lines("block_size_is_not_len_less_4", len=(2, int(lines["len"][2]) - 4))
    with_bytes("cigar_leaves_the_record", o3 + 16, struct.pack("<H", 60))
    with_bytes("name_leaves_the_record", o3 + 12, b"\xff")
    with_bytes("refid_1", o3 + 4, struct.pack("<i", 1))
    with_bytes("negative_pos", o3 + 8, struct.pack("<i", -1))
    return out


def test_counted_disagreements(spm):
    cases = disagreements()
    assert {"second_primary", "read_beyond_the_lines", "an_S_item", "end_beyond_ref_len", "qual_leaves_the_record"} <= set(cases)
    for name, (stream, lines, ref_len) in cases.items():
        with pytest.raises(spm.SpmError, match="-1.*disagree"):
            spm.bam_markdup_host(stream, lines, ref_len)
        src = ctypes.create_string_buffer(stream, len(stream))
        dup = np.full(len(lines), 7, np.uint8)
        assert spm.capi.lib().spm_hip_bam_markdup_host(src, len(stream), lines.ctypes.data, len(lines), ref_len, None, dup.ctypes.data) == INVALID
        assert dup.tolist() == [7] * len(lines), name               # nothing written
    # what is NOT a disagreement: the same conditions on records that do not take part
    stream, lines = make_stream(worked_cases() + [dict(read=1, flag=0x100, pos=9990, words=[EQ(30)], l_seq=0),      # a secondary beyond the end
                                                  dict(read=2, flag=0x800, pos=50, words=[5 << 4 | 5, EQ(30)], l_seq=30)])  # a clipped supplementary
    assert spm.bam_markdup_host(stream, lines, REF_LEN).tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0]
    assert spm.bam_markdup_host(*make_stream(worked_cases()), 1300).sum() == 5      # end == ref_len


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_bam_markdup_opts, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_bam_markdup_stats, f))
int main(void)
{
    O(min_qual); O(flags); O(reserved);
    S(ms_total); S(ms_keys); S(ms_sort); S(ms_mark); S(ms_write); S(ms_frame); S(ms_host); S(reserved); S(n_records); S(n_pairs);
    S(n_fragments); S(n_dup_pairs); S(n_dup_fragments); S(n_dup_records); S(n_fragments_beside_pairs);
    printf("sizeof.opts %zu\nsizeof.stats %zu\n", sizeof(spm_bam_markdup_opts), sizeof(spm_bam_markdup_stats));
    return 0;
}
"""
CALLS = ("spm_hip_bam_markdup", "spm_hip_bam_markdup_stats", "spm_hip_bam_markdup_records", "spm_hip_bam_markdup_host")


def test_layouts_and_names(spm, tmp_path):
    kinds = {"opts": spm.capi.BamMarkdupOpts, "stats": spm.capi.BamMarkdupStats}
    want = c_layout(tmp_path, LAYOUT_C)
    sizes = {k: int(want.pop("sizeof." + k)) for k in kinds}
    assert sizes == {"opts": 16, "stats": 88} == {k: ctypes.sizeof(t) for k, t in kinds.items()}
    seen = dict.fromkeys(kinds, 0)
    for name, off in want.items():
        kind, field = name.split(".")
        assert getattr(kinds[kind], field).offset == int(off), name
        seen[kind] += 1
    assert seen == {k: len(t._fields_) for k, t in kinds.items()} == {"opts": 3, "stats": 15}
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    for f in (spm.Bam.markdup, spm.Bam.markdup_stats, spm.Context.bam_markdup, spm.bam_markdup_host, spm.bam_markdup_opts):
        assert callable(f)
    assert list(inspect.signature(spm.Bam.markdup).parameters) == ["self", "min_qual"]
    assert list(inspect.signature(spm.Context.bam_markdup).parameters)[1:] == ["records", "n_record_bytes", "lines", "n_lines", "ref_len",
                                                                               "dup_ptr", "min_qual"]
    assert list(inspect.signature(spm.bam_markdup_host).parameters) == ["records", "lines", "ref_len", "min_qual"]
    assert inspect.signature(spm.Bam.markdup).parameters["min_qual"].default == 0
