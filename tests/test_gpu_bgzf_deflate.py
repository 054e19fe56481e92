"""BGZF blocks deflated on the device: spm_hip_bgzf_deflate over raw device buffers at every length, block size and source
alignment of tests/test_gpu_bgzf.py, byte for byte against the host deflater and taken apart by tests/bgzf_inflate.py; the
blocks' offsets on host and device; Bam.deflate on the chain of tests/test_gpu_bam.py; Sam.bgzf_deflate; the refusals."""
import ctypes
import gzip
import struct

import numpy as np
import pytest

import bgzf_inflate
from bam_decode import parse_bam_header, render_records
from cpp_programs import download
from test_bgzf_deflate import records as synthetic_records

gpu = pytest.mark.gpu
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 65279, 65280, 65281, 200_000)
INVALID, UNSUPPORTED = -1, -4


def _mixed(n, seed):
    """runs, repeated records and random stretches: both block types in one call"""
    rng = np.random.default_rng(seed)
    rec = synthetic_records(320, seed)
    parts = [rng.integers(0, 256, 65280 + 700, dtype=np.uint8).tobytes(), rec, b"\xff" * 5000, rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(),
             b"ACGT" * 2000, rec[:30_000]]
    out = b"".join(parts)
    assert len(out) >= n
    return np.frombuffer(out[:n], np.uint8).copy()


class _DeviceBytes:
    """bytes in a device allocation of their own, with room in front for a misaligned start"""

    def __init__(self, host):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.host = np.ascontiguousarray(host, dtype=np.uint8)
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), len(self.host)) == 0 and self.ptr.value % 16 == 0
        assert self.hip.hipMemcpy(self.ptr, self.host.ctypes.data, len(self.host), 1) == 0

    def close(self):
        assert self.hip.hipFree(self.ptr) == 0


def _check(spm, ctx, src, off, n, D, eof=True, views=True):
    """one device call against the host deflater and the decoder -> the handle's deflate stats"""
    data = src.host[off:off + n].tobytes()
    z = ctx.bgzf_deflate(src.ptr.value + off, n, block_data=D, eof=eof)
    got = z.bytes()
    assert got == spm.bgzf_deflate_host(data, D, eof=eof), (n, off, D)
    blocks = bgzf_inflate.parse(got, D or 65280, eof=eof)
    assert bgzf_inflate.payload_of(blocks) == data
    st, ds = z.stats(), z.deflate_stats()
    n_blocks = (n + (D or 65280) - 1) // (D or 65280)
    assert (st.n_in, st.n_out, st.n_blocks) == (n, len(got), n_blocks) and st.ms_host > 0 and st.ms_frame >= 0
    assert (ds.n_in, ds.n_out, ds.n_blocks, ds.n_prefix_bytes) == (n, len(got), n_blocks, 0)
    assert ds.n_stored_blocks == sum(1 for _o, _p, t in blocks if t == 0)
    offsets = z.block_offsets()
    assert offsets.tolist() == [o for o, _p, _t in blocks] + [len(got) - (28 if eof else 0)]
    if views:
        d_ptr, d_n = z.device()
        assert d_n == len(got) and download(ctx, d_ptr, d_n, np.uint8).tobytes() == got
        d_off, d_blocks = z.block_offsets_device()
        assert d_blocks == n_blocks and download(ctx, d_off, n_blocks + 1, np.uint64).tolist() == offsets.tolist()
    z.close()
    return ds


@gpu
@pytest.mark.parametrize("kind", ["random", "mixed"])
def test_raw_buffers_at_every_length_and_alignment(spm, ctx, kind):
    n_max = max(LENGTHS) + 16
    host = np.random.default_rng(1711).integers(0, 256, n_max, dtype=np.uint8) if kind == "random" else _mixed(n_max, 1712)
    src = _DeviceBytes(host)
    for n in LENGTHS:
        for off in range(4):
            for D in (0, 257):
                ds = _check(spm, ctx, src, off, n, D)
                if kind == "mixed" and n == 200_000 and D == 0:
                    assert 0 < ds.n_stored_blocks < ds.n_blocks and ds.n_matches > 0 and ds.n_literals > 0
                if kind == "random" and n >= 65279 and D == 0:     # (the one byte behind 65280 is a 3-byte fixed block)
                    assert ds.n_stored_blocks == ds.n_blocks - (n == 65281) and ds.n_matches == 0
    src.close()


@gpu
def test_source_alignment(spm, ctx):
    rec = np.frombuffer(synthetic_records(120, 1713), np.uint8)     # records, then random bytes: a fixed and a stored block
    src = _DeviceBytes(np.concatenate([rec, np.random.default_rng(1713).integers(0, 256, 70_016 - len(rec), dtype=np.uint8)]))
    for off in range(16):
        for n, D in ((100, 7), (1000, 64), (4097, 1000), (70_000, 0)):
            _check(spm, ctx, src, off, n, D, eof=False, views=False)
    src.close()


@gpu
def test_edge_calls(spm, ctx):
    src = _DeviceBytes(_mixed(150_016, 1714))
    # blocks of one byte: as many workgroups as bytes
    ds = _check(spm, ctx, src, 5, 3000, 1)
    assert ds.n_blocks == 3000 and ds.n_stored_blocks == 0 and ds.n_literals == 3000
    # nothing to deflate
    z = ctx.bgzf_deflate(0, 0)
    assert z.bytes() == bgzf_inflate.EOF_BLOCK and z.device()[1] == 28 and z.block_offsets().tolist() == [0]
    z.close()
    z = ctx.bgzf_deflate(0, 0, eof=False)
    assert z.bytes() == b"" and z.device() == (0, 0) and z.stats().n_out == 0 and z.block_offsets().tolist() == [0]
    z.close()
    # two calls give the same bytes, and the result outlives its source
    a, b = ctx.bgzf_deflate(src.ptr.value + 1, 150_001), ctx.bgzf_deflate(src.ptr.value + 1, 150_001)
    src.close()
    assert a.bytes() == b.bytes() == spm.bgzf_deflate_host(src.host[1:150_002].tobytes())
    a.close()
    b.close()
    # a framed handle answers the same questions in closed form
    src = _DeviceBytes(np.arange(1000, dtype=np.uint8))
    z = ctx.bgzf(src.ptr.value, 1000, block_data=300)
    assert z.block_offsets().tolist() == [0, 331, 662, 993, 1124]
    d_off, d_blocks = z.block_offsets_device()
    assert d_blocks == 4 and download(ctx, d_off, 5, np.uint64).tolist() == [0, 331, 662, 993, 1124]
    ds = z.deflate_stats()
    assert (ds.n_blocks, ds.n_stored_blocks, ds.n_matches, ds.n_out) == (4, 4, 0, 1152)
    assert z.voffsets([0, 299, 300, 999]).tolist() == [0, 299, 331 << 16, 993 << 16 | 99]
    z.close()
    src.close()


@gpu
def test_bam_deflate(spm, ctx):
    from test_gpu_bam import REF_LEN
    from test_gpu_sam import _single_end_reads
    from test_rescue import _chain_of

    t, _reads, _at = _single_end_reads()
    ref = t["ref"]
    starts = np.random.default_rng(1715).integers(0, len(ref) - 150, 400)
    reads = [np.ascontiguousarray(ref[s:s + 150]) for s in starts.tolist()]
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    s = lc.sam(rd, ps, "chr7", secondary=True)
    b = lc.bam(rd, ps, "chr7", REF_LEN, secondary=True)
    stored, stream, lines = b.bytes(), b.records(), b.lines()
    assert len(stream) > 65280
    plain_header = gzip.decompress(spm.bam_header("chr7", REF_LEN))
    for D in (0, 1000):
        z = b.deflate(block_data=D)
        raw = z.bytes()
        assert gzip.decompress(raw) == gzip.decompress(stored) == plain_header + stream
        header = spm.bgzf_deflate_host(plain_header, D, eof=False)
        assert raw == header + spm.bgzf_deflate_host(stream, D, eof=False) + bgzf_inflate.EOF_BLOCK
        assert len(raw) < len(stored)
        ds = z.deflate_stats()
        assert (ds.n_prefix_bytes, ds.n_in, ds.n_out) == (len(header), len(stream), len(raw)) and z.prefix == b""
        blocks = bgzf_inflate.parse(raw, D or 65280, sections=2)
        record_blocks = [x for x in blocks if x[0] >= len(header)]
        assert z.block_offsets().tolist() == [o for o, _p, _t in record_blocks] + [len(raw) - 28]
        voff = z.voffsets(lines["offset"])
        for i in range(len(lines)):
            (block_size,) = struct.unpack("<i", bgzf_inflate.at_voffset(blocks, int(voff[i]), 4))
            assert block_size == int(lines["len"][i]) - 4, i
        _text, refs, first = parse_bam_header(bgzf_inflate.payload_of(blocks))
        assert first == len(plain_header)
        rendered = render_records(bgzf_inflate.payload_of(record_blocks), refs)
        assert b"".join(line for _o, _n, line in rendered) == s.text()
        d_ptr, d_n = z.device()
        assert d_n == len(raw) and download(ctx, d_ptr, d_n, np.uint8).tobytes() == raw
        again = b.deflate(block_data=D)
        assert again.bytes() == raw
        again.close()
        z.close()
    # the deflated file outlives the BAM handle; without the EOF block it ends in a data block
    z = b.deflate(eof=False)
    for x in (b, s, rd, lc, ps, ref_text) + rest:
        x.close()
    assert z.bytes() + bgzf_inflate.EOF_BLOCK == spm.bgzf_deflate_host(plain_header, eof=False) + spm.bgzf_deflate_host(stream)
    z.close()


@gpu
def test_sam_text_deflated_where_it_lies(spm, ctx):
    from test_gpu_sam import _single_end_reads
    from test_rescue import _chain_of

    t, reads, _at = _single_end_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    s = lc.sam(rd, ps, "chr7", secondary=True)
    text, header = s.text(), s.header(len(t["ref"]))
    assert len(text) > 2000
    for D in (0, 1000):
        z = s.bgzf_deflate(len(t["ref"]), block_data=D)
        raw = z.bytes()
        stored = s.bgzf(len(t["ref"]), block_data=D)
        assert gzip.decompress(raw) == header + text and len(raw) < len(stored.bytes())
        stored.close()
        assert z.prefix == spm.bgzf_deflate_host(header, D, eof=False)
        blocks = bgzf_inflate.parse(raw[len(z.prefix):], D or 65280)  # the header's blocks are its own: the text starts a block
        assert bgzf_inflate.payload_of(blocks) == text
        assert bgzf_inflate.payload_of(bgzf_inflate.parse(z.prefix, D or 65280, eof=False)) == header
        assert z.device()[1] == len(raw) - len(z.prefix) and z.stats().n_in == len(text)
        assert z.block_offsets().tolist() == [len(z.prefix) + o for o, _p, _t in blocks] + [len(raw) - 28]
        z.close()
        z = s.bgzf_deflate(block_data=D, eof=False)
        assert z.prefix == b"" and gzip.decompress(z.bytes()) == text
        z.close()
    for x in (s, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_refusals(spm, ctx):
    lib, capi = spm.capi.lib(), spm.capi
    err = lambda: lib.spm_hip_last_error(ctx._h)
    src = _DeviceBytes(np.arange(64, dtype=np.uint8))

    def refused(word, ptr=src.ptr, n=64, opts=None, no_opts=False, no_out=False):
        out = ctypes.c_void_p(1)                                   # (a refusal leaves NULL behind)
        o = None if no_opts else ctypes.byref(opts if opts is not None else spm.bgzf_deflate_opts())
        rc = lib.spm_hip_bgzf_deflate(ctx._h, ptr, n, o, None if no_out else ctypes.byref(out))
        assert rc == INVALID and (no_out or not out.value) and word in err(), (rc, out.value, err())

    refused(b"NULL opts", no_opts=True)
    refused(b"NULL out", no_out=True)
    refused(b"NULL device_src", ptr=None)
    refused(b"block_data", opts=capi.BgzfDeflateOpts(65281, 1, 1, 0))
    refused(b"flag", opts=capi.BgzfDeflateOpts(0, 3, 1, 0))
    refused(b"level", opts=capi.BgzfDeflateOpts(0, 1, 0, 0))
    refused(b"level", opts=capi.BgzfDeflateOpts(0, 1, 2, 0))
    refused(b"reserved", opts=capi.BgzfDeflateOpts(0, 1, 1, 5))
    out = ctypes.c_void_p(1)
    assert lib.spm_hip_bgzf_deflate(None, src.ptr, 64, ctypes.byref(spm.bgzf_deflate_opts()), ctypes.byref(out)) == INVALID and not out.value
    assert lib.spm_hip_bam_deflate(None, ctypes.byref(spm.bgzf_deflate_opts()), ctypes.byref(out)) == INVALID
    assert lib.spm_hip_bgzf_blocks(None, None, None) == INVALID and lib.spm_hip_bgzf_blocks_device(None, None, None) == INVALID
    assert lib.spm_hip_bgzf_deflate_stats(None, None) == INVALID
    # more than 2^31 - 2 blocks: refused on the host, before anything is read or allocated
    rc = lib.spm_hip_bgzf_deflate(ctx._h, src.ptr, 2 ** 31, ctypes.byref(spm.bgzf_deflate_opts(1)), ctypes.byref(out))
    assert rc == UNSUPPORTED and not out.value and b"2^31 - 2" in err()
    with pytest.raises(spm.SpmError, match="-1.*block_data"):
        ctx.bgzf_deflate(src.ptr.value, 64, block_data=70_000)
    z = ctx.bgzf_deflate(src.ptr.value, 64, block_data=65280)       # the largest block size is accepted
    assert z.bytes() == spm.bgzf_deflate_host(src.host.tobytes())
    z.close()
    src.close()
