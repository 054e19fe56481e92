"""SPM_BGZF_DYNAMIC on the device: spm_hip_bgzf_deflate with the flag over raw device buffers at every length, block size and
source alignment of tests/test_gpu_bgzf_deflate.py and over every kind of data of tests/test_bgzf_dynamic.py, byte for byte
against the host deflater with the flag and taken apart by tests/deflate_dynamic.py; the block types, stats and offsets of the
handle; Bam.deflate, Bam.index and Sam.bgzf_deflate with the flag."""
import gzip
import struct

import numpy as np
import pytest

import deflate_dynamic as dyn
from cpp_programs import download
from test_bgzf_dynamic import fibonacci_block, mixed, quality_records, uniform40
from test_gpu_bgzf_deflate import LENGTHS, _DeviceBytes

gpu = pytest.mark.gpu


def _check(spm, ctx, src, off, n, D, eof=True, views=True):
    """one flagged device call against the host deflater and the decoder -> (deflate stats, block types)"""
    data = src.host[off:off + n].tobytes()
    z = ctx.bgzf_deflate(src.ptr.value + off, n, block_data=D, eof=eof, dynamic=True)
    got = z.bytes()
    assert got == spm.bgzf_deflate_host(data, D, eof=eof, dynamic=True), (n, off, D)
    blocks = dyn.parse(got, D or 65280, eof=eof)
    assert dyn.payload_of(blocks) == data
    st, ds, types = z.stats(), z.deflate_stats(), z.block_types()
    n_blocks = (n + (D or 65280) - 1) // (D or 65280)
    assert types == dyn.types_of(blocks) and sum(types) == n_blocks
    assert (st.n_in, st.n_out, st.n_blocks) == (n, len(got), n_blocks) and st.ms_host > 0 and st.ms_frame >= 0
    assert (ds.n_in, ds.n_out, ds.n_blocks, ds.n_prefix_bytes, ds.n_stored_blocks) == (n, len(got), n_blocks, 0, types[0])
    assert (ds.n_matches + ds.n_literals > 0) == (types[0] < n_blocks)
    offsets = z.block_offsets()
    assert offsets.tolist() == [blk[0] for blk in blocks] + [len(got) - (28 if eof else 0)]
    if views:
        d_ptr, d_n = z.device()
        assert d_n == len(got) and download(ctx, d_ptr, d_n, np.uint8).tobytes() == got
        d_off, d_blocks = z.block_offsets_device()
        assert d_blocks == n_blocks and download(ctx, d_off, n_blocks + 1, np.uint64).tolist() == offsets.tolist()
    z.close()
    return ds, types


def _source(kind, n):
    if kind == "random":
        return np.random.default_rng(2111).integers(0, 256, n, dtype=np.uint8)
    if kind == "quality":
        data = quality_records(n // 296 + 2, 2112)
    elif kind == "uniform40":
        data = uniform40(n, 2113)
    elif kind == "equal":
        data = b"\xff" * n
    elif kind == "fibonacci":
        data = fibonacci_block() * (n // 46_367 + 1)
    else:
        data = mixed(2114) + mixed(2115)
    assert len(data) >= n
    return np.frombuffer(data[:n], np.uint8).copy()


@gpu
@pytest.mark.parametrize("kind", ["quality", "uniform40", "equal", "fibonacci", "mixed", "random"])
def test_raw_buffers_at_every_length_and_alignment(spm, ctx, kind):
    src = _DeviceBytes(_source(kind, max(LENGTHS) + 16))
    seen = [0, 0, 0]
    for n in LENGTHS:
        for off in range(4):
            for D in (0, 257):
                ds, types = _check(spm, ctx, src, off, n, D, views=off == 0)
                seen = [a + b for a, b in zip(seen, types)]
                if kind in ("quality", "uniform40", "fibonacci") and n >= 65279 and D == 0:
                    assert types[2] >= n // 65280 and types[0] == 0
                if kind == "random" and n >= 65279 and D == 0:     # (the one byte behind 65280 is a 3-byte fixed block)
                    assert types == ((n + 65279) // 65280 - (n == 65281), int(n == 65281), 0) and ds.n_matches == 0
    assert seen[2] > 0 or kind == "random"
    assert all(seen) or kind != "mixed"
    # the same source without the flag is what it was
    z = ctx.bgzf_deflate(src.ptr.value + 1, 200_000)
    assert z.bytes() == spm.bgzf_deflate_host(src.host[1:200_001].tobytes()) and z.block_types()[2] == 0
    assert z.block_types()[0] == z.deflate_stats().n_stored_blocks and sum(z.block_types()) == 4
    z.close()
    src.close()


@gpu
def test_source_alignment(spm, ctx):
    rec = np.frombuffer(quality_records(120, 2116), np.uint8)       # records, then random bytes: a dynamic and a stored block
    src = _DeviceBytes(np.concatenate([rec, np.random.default_rng(2116).integers(0, 256, 70_016 - len(rec), dtype=np.uint8)]))
    for off in range(16):
        for n, D in ((100, 7), (1000, 64), (4097, 1000), (70_000, 0)):
            _check(spm, ctx, src, off, n, D, eof=False, views=False)
    src.close()


@gpu
def test_edge_calls(spm, ctx):
    src = _DeviceBytes(_source("mixed", 150_016))
    # blocks of one byte: as many workgroups as bytes, every one fixed
    ds, types = _check(spm, ctx, src, 5, 3000, 1)
    assert types == (0, 3000, 0) and ds.n_literals == 3000
    # nothing to deflate
    z = ctx.bgzf_deflate(0, 0, dynamic=True)
    assert z.bytes() == dyn.EOF_BLOCK and z.device()[1] == 28 and z.block_offsets().tolist() == [0] and z.block_types() == (0, 0, 0)
    z.close()
    z = ctx.bgzf_deflate(0, 0, eof=False, dynamic=True)
    assert z.bytes() == b"" and z.device() == (0, 0) and z.stats().n_out == 0 and z.block_types() == (0, 0, 0)
    z.close()
    # two calls give the same bytes, and the result outlives its source
    a = ctx.bgzf_deflate(src.ptr.value + 1, 150_001, dynamic=True)
    b = ctx.bgzf_deflate(src.ptr.value + 1, 150_001, dynamic=True)
    src.close()
    assert a.bytes() == b.bytes() == spm.bgzf_deflate_host(src.host[1:150_002].tobytes(), dynamic=True)
    a.close()
    b.close()
    # a framed handle: every block stored
    src = _DeviceBytes(np.arange(1000, dtype=np.uint8))
    z = ctx.bgzf(src.ptr.value, 1000, block_data=300)
    assert z.block_types() == (4, 0, 0)
    z.close()
    src.close()


@gpu
def test_bam_deflate_dynamic(spm, ctx):
    from test_gpu_bam import REF_LEN
    from test_gpu_sam import _single_end_reads
    from test_rescue import _chain_of

    t, _reads, _at = _single_end_reads()
    ref = t["ref"]
    rng = np.random.default_rng(2117)
    starts = rng.integers(0, len(ref) - 150, 400)
    reads = [np.ascontiguousarray(ref[s:s + 150]) for s in starts.tolist()]
    qual = (41 - np.minimum(rng.geometric(0.25, (400, 150)) - 1, 39)).astype(np.uint8)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    b = lc.bam_ex(rd, ps, "chr7", REF_LEN, secondary=True, qualities=qual)
    stored, stream, lines = b.bytes(), b.records(), b.lines()
    assert len(stream) > 65280
    plain_header = gzip.decompress(spm.bam_header("chr7", REF_LEN))
    for D in (0, 1000):
        z = b.deflate(block_data=D, dynamic=True)
        raw = z.bytes()
        assert gzip.decompress(raw) == gzip.decompress(stored) == plain_header + stream
        header = spm.bgzf_deflate_host(plain_header, D, eof=False, dynamic=True)
        assert raw == header + spm.bgzf_deflate_host(stream, D, eof=False, dynamic=True) + dyn.EOF_BLOCK
        without = b.deflate(block_data=D)
        assert len(raw) <= len(without.bytes()) and without.block_types()[2] == 0
        without.close()
        ds = z.deflate_stats()
        assert (ds.n_prefix_bytes, ds.n_in, ds.n_out) == (len(header), len(stream), len(raw)) and z.prefix == b""
        blocks = dyn.parse(raw, D or 65280, sections=2)
        record_blocks = [x for x in blocks if x[0] >= len(header)]
        assert z.block_types() == dyn.types_of(record_blocks) and z.block_types()[2] >= 1
        assert z.block_offsets().tolist() == [x[0] for x in record_blocks] + [len(raw) - 28]
        voff = z.voffsets(lines["offset"])
        for i in range(len(lines)):
            (block_size,) = struct.unpack("<i", dyn.at_voffset(blocks, int(voff[i]), 4))
            assert block_size == int(lines["len"][i]) - 4, i
        z.close()
    # the BAI of the sorted handle's dynamic file is the host builder's over the downloaded file
    s = b.sort()
    z = s.deflate(dynamic=True)
    bai = s.index(z)
    assert bai.bytes() == spm.bai_build_host(s.records(), s.lines(), z.block_offsets())
    for x in (bai, z, s, b, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_sam_text_deflated_dynamic(spm, ctx):
    from test_gpu_sam import _single_end_reads
    from test_rescue import _chain_of

    t, reads, _at = _single_end_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    s = lc.sam(rd, ps, "chr7", secondary=True)
    text, header = s.text(), s.header(len(t["ref"]))
    for D in (0, 1000):
        z = s.bgzf_deflate(len(t["ref"]), block_data=D, dynamic=True)
        raw = z.bytes()
        assert gzip.decompress(raw) == header + text
        assert z.prefix == spm.bgzf_deflate_host(header, D, eof=False, dynamic=True)
        blocks = dyn.parse(raw[len(z.prefix):], D or 65280)
        assert dyn.payload_of(blocks) == text and z.block_types() == dyn.types_of(blocks) and z.block_types()[2] >= 1
        z.close()
    for x in (s, rd, lc, ps, ref_text) + rest:
        x.close()
