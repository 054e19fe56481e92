"""The BAI index on the device: spm_hip_bam_index of a sorted handle, of its stored file and of its deflated file, and
spm_hip_bai_build over uploaded streams, byte for byte against spm_hip_bai_build_host and against the builder of
tests/bai_decode.py, which is written from the specification; the standard region query through the index against a full scan."""
import ctypes

import numpy as np
import pytest

import bai_decode
import bgzf_inflate
from bam_decode import bam_to_sam
from cpp_programs import download
from test_bai import CASES, M, NO_COOR, make_stream, stored_offsets
from test_gpu_bam_sort import RNAME, _border_reads
from test_gpu_sam import _names
from test_rescue import _chain_of
from test_sam import LINE

gpu = pytest.mark.gpu
INVALID = -1
COUNTS = ("n_bins", "n_chunks", "n_intv", "n_mapped", "n_unmapped", "n_no_coor", "n_bytes")


class _Device:
    """host bytes in a device allocation of their own"""

    def __init__(self, data):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        data = bytes(data)
        self.n = len(data)
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), max(self.n, 1)) == 0
        if self.n:
            assert self.hip.hipMemcpy(self.ptr, data, self.n, 1) == 0

    def close(self):
        assert self.hip.hipFree(self.ptr) == 0


def _check_counts(st, bai, got):
    n_chunks = sum(len(c) for _b, c in bai["bins"])
    pseudo = bai["pseudo"]
    want = (len(bai["bins"]) + (pseudo is not None), n_chunks, len(bai["ioffset"]), pseudo[1][0] if pseudo else 0,
            pseudo[1][1] if pseudo else 0, bai["n_no_coor"], len(got))
    assert tuple(int(getattr(st, c)) for c in COUNTS) == want
    assert st.ms_host > 0 and st.ms_total >= 0


def _check_index(ctx, spm, z, stream, lines, records, offsets, D, record_blocks, ref_len):
    """a device index against the host builder, the specification's builder and the query -> its bytes"""
    got = z.bytes()
    assert got == spm.bai_build_host(stream, lines, offsets, D)
    assert got == bai_decode.build_bai(records, offsets, D or 65280)
    d, n = z.device()
    assert n == len(got) and download(ctx, d, n, np.uint8).tobytes() == got
    bai = bai_decode.parse_bai(got)
    _check_counts(z.stats(), bai, got)
    for beg, end in bai_decode.queries(bai_decode.intervals(records), ref_len):
        assert bai_decode.fetch(bai, record_blocks, beg, end) == bai_decode.scan(stream, beg, end), (beg, end)
    return got


@gpu
def test_index_of_the_stored_and_of_the_deflated_file(spm, ctx):
    t, reads, _at = _border_reads()
    ref_len = len(t["ref"])
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    lib = spm.capi.lib()
    for D, opt in ((0, dict(names=_names(len(reads)), secondary=True)), (1000, dict(cigar_m=True)), (257, dict(secondary=True)), (7, dict())):
        Dv = D or 65280
        b = lc.bam(rd, ps, RNAME, ref_len, block_data=D, **opt)
        s = b.sort()
        raw = s.bytes()
        _text, stream, records, blocks = bam_to_sam(raw, Dv)
        lines, st = s.lines(), s.stats()
        items = bai_decode.intervals(records)
        assert sum(1 for it in items if not it[2]) >= 1 and len({bai_decode.reg2bin(it[3], it[4]) for it in items if it[2]}) >= 8
        # ---- the stored file ----
        record_blocks = [x for x in blocks if x[0] >= st.header_file_bytes]
        offsets = stored_offsets(len(stream), Dv, int(st.header_file_bytes))
        z = s.index()
        got = _check_index(ctx, spm, z, stream, lines, records, offsets, D, record_blocks, ref_len)
        again = s.index()
        assert again.bytes() == got
        again.close()
        z.close()
        # ---- the deflated file ----
        f = s.deflate(block_data=D)
        fraw = f.bytes()
        fblocks = bgzf_inflate.parse(fraw, Dv, sections=2)
        n_prefix = int(f.deflate_stats().n_prefix_bytes)
        frecord_blocks = [x for x in fblocks if x[0] >= n_prefix]
        assert bgzf_inflate.payload_of(frecord_blocks) == stream
        foffsets = f.block_offsets()
        assert foffsets.tolist() == [o for o, _p, _t in frecord_blocks] + [len(fraw) - 28]
        zf = s.index(f)
        fgot = _check_index(ctx, spm, zf, stream, lines, records, foffsets, D, frecord_blocks, ref_len)
        assert (fgot != got or len(stream) <= Dv) and len(fgot) == len(got)
        zf.close()
        # ---- refused: an unsorted handle; the deflated file of another handle, of another block size ----
        out = ctypes.c_void_p(1)
        assert lib.spm_hip_bam_index(b._h, None, ctypes.byref(out)) == INVALID and not out.value
        assert b"order" in lib.spm_hip_last_error(ctx._h)
        with pytest.raises(spm.SpmError, match="-1.*order"):
            b.index()
        other = s.deflate(block_data=Dv - 1)
        with pytest.raises(spm.SpmError, match="-1.*deflated"):
            s.index(other)
        other.close()
        if D == 0:
            b2 = lc.bam(rd, ps, RNAME, ref_len, block_data=D, cigar_m=True)         # another handle: another stream length
            s2 = b2.sort()
            assert s2.stats().n_record_bytes != st.n_record_bytes
            with pytest.raises(spm.SpmError, match="-1.*deflated"):
                s2.index(f)
            s2.close()
            b2.close()
        assert s.index().bytes() == got                             # and after all of this the call answers as before
        for x in (f, s, b):
            x.close()
    assert lib.spm_hip_bam_index(None, None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.spm_hip_bai_view(None, None, None) == INVALID and lib.spm_hip_bai_device(None, None, None) == INVALID
    assert lib.spm_hip_bai_stats(None, None) == INVALID
    lib.spm_hip_bai_destroy(None)
    # zero reads: the sorted empty BAM and its 24 bytes
    rd0 = lc.reads(0, 2)
    ps0 = ctx.patterns(spm.ALGO_MYERS, [], k=1, both_strands=True)
    e = lc.bam(rd0, ps0, RNAME, ref_len)
    for h in (e, e.sort()):                                         # (no record is out of order)
        z = h.index()
        assert z.bytes() == bytes.fromhex("42414901 01000000 00000000 00000000 0000000000000000") and z.stats().n_bytes == 24
        z.close()
        if h is not e:
            h.close()
    for x in (e, ps0, rd0, rd, lc, ps, ref_text) + rest:
        x.close()


def _raw(ctx, spm, stream, lines, offsets, D):
    dev = [_Device(stream), _Device(np.ascontiguousarray(lines, LINE).tobytes()), _Device(np.ascontiguousarray(offsets, np.uint64).tobytes())]
    try:
        z = ctx.bai(dev[0].ptr.value, len(stream), dev[1].ptr.value, len(lines), dev[2].ptr.value, len(offsets) - 1, D)
        got, st = z.bytes(), z.stats()
        z.close()
        return got, st
    finally:
        ctx.synchronize()
        for d in dev:
            d.close()


@gpu
def test_raw_form_over_uploaded_streams(spm, ctx):
    far = [(0, 5, 0, [M(20)]), (0, (1 << 28) - 10, 16, [M(20)]), (0, (1 << 29) - 70, 0, [M(30)]), (0, (1 << 29) - 70, 0x85, []),
           (0, (1 << 29) - 40, 0, [7 << 4 | 7, 20 << 4 | 2, 13 << 4 | 8]), (0, (1 << 29) - 1, 16, [M(1)]), NO_COOR]
    for name, recs in sorted(CASES.items()) + [("far", far)]:
        stream, lines = make_stream(recs)
        for D in (1, 7, 256, 0):
            offsets = stored_offsets(len(stream), D or 65280, 77)
            offsets[1:] += np.uint64(5)                             # any ascending table: the blocks need not be stored ones
            got, st = _raw(ctx, spm, stream, lines, offsets, D)
            assert got == spm.bai_build_host(stream, lines, offsets, D), (name, D)
            _check_counts(st, bai_decode.parse_bai(got), got)
            if name == "far":
                assert st.n_intv == 1 << 15 and st.n_no_coor == 1 and st.n_unmapped == 1
    # refused: counted on the device, nothing written
    stream, lines = make_stream(far)
    offsets = stored_offsets(len(stream), 7, 0)

    def refused(s=stream, l=lines, o=offsets, word="order"):
        with pytest.raises(spm.SpmError, match=f"-1.*{word}"):
            _raw(ctx, spm, s, l, o, 7)

    refused(*make_stream([far[i] for i in (1, 0, 2, 3, 4, 5, 6)]))
    refused(*make_stream([far[i] for i in (0, 1, 2, 3, 4, 6, 5)]))
    bad = lines.copy()
    bad["offset"][2] += 1
    refused(l=bad)
    bad = lines.copy()
    bad["len"][6] += 8                                              # leaves the stream
    refused(l=bad)
    bad = lines.copy()
    bad["len"][1] -= 4                                              # block_size is not len - 4
    refused(l=bad)
    broken = bytearray(stream)
    broken[int(lines["offset"][1]) + 16] = 99                       # a CIGAR that leaves its record
    refused(s=bytes(broken))
    refused(*make_stream([(0, (1 << 29) - 5, 0, [M(6)])]), o=stored_offsets(42, 7, 0))
    refused(o=offsets[:-1], word="n_blocks")
    assert _raw(ctx, spm, stream, lines, offsets, 7)[0] == spm.bai_build_host(stream, lines, offsets, 7)
