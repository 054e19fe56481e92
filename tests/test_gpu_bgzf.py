"""BGZF framing on the device: spm_hip_bgzf_frame over raw device buffers at every length and source alignment at which the
frame kernel takes another path, against the host framer and gzip; Sam.bgzf over the SAM text where it lies; the refusals."""
import ctypes
import gzip

import numpy as np
import pytest

from bam_decode import EOF_BLOCK, parse_bgzf, payload_of
from cpp_programs import download

gpu = pytest.mark.gpu
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 65279, 65280, 65281, 200_000)
INVALID = -1


class _DeviceBytes:
    """pseudo-random bytes in a device allocation of their own, with room in front for a misaligned start"""

    def __init__(self, n, seed):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.host = np.random.default_rng(seed).integers(0, 256, n + 16, dtype=np.uint8)
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), n + 16) == 0 and self.ptr.value % 16 == 0
        assert self.hip.hipMemcpy(self.ptr, self.host.ctypes.data, n + 16, 1) == 0

    def close(self):
        assert self.hip.hipFree(self.ptr) == 0


@gpu
def test_raw_buffers_at_every_length_and_alignment(spm, ctx):
    src = _DeviceBytes(max(LENGTHS), 1501)
    for n in LENGTHS:
        for off in range(4):
            data = src.host[off:off + n].tobytes()
            for D in (0, 257):
                z = ctx.bgzf(src.ptr.value + off, n, block_data=D)
                got = z.bytes()
                assert got == spm.bgzf_frame_host(data, D), (n, off, D)
                assert gzip.decompress(got) == data
                d_ptr, d_n = z.device()
                assert d_n == len(got) and download(ctx, d_ptr, d_n, np.uint8).tobytes() == got
                st = z.stats()
                n_blocks = (n + (D or 65280) - 1) // (D or 65280)
                assert (st.n_in, st.n_out, st.n_blocks) == (n, len(got), n_blocks) and st.ms_host > 0 and st.ms_frame >= 0
                z.close()
    # every alignment of the source against a 16-byte border, blocks that straddle it, no EOF block
    for off in range(16):
        for n, D in ((100, 7), (1000, 64), (4097, 1000), (70_000, 0)):
            data = src.host[off:off + n].tobytes()
            z = ctx.bgzf(src.ptr.value + off, n, block_data=D, eof=False)
            got = z.bytes()
            assert got == spm.bgzf_frame_host(data, D, eof=False), (n, off, D)
            assert payload_of(parse_bgzf(got, D or 65280, eof=False)) == data
            z.close()
    # blocks of one byte: as many workgroups as bytes
    z = ctx.bgzf(src.ptr.value + 5, 3000, block_data=1)
    assert z.bytes() == spm.bgzf_frame_host(src.host[5:3005].tobytes(), 1) and z.stats().n_blocks == 3000
    z.close()
    # nothing to frame
    z = ctx.bgzf(0, 0)
    assert z.bytes() == EOF_BLOCK and z.device()[1] == 28
    z.close()
    z = ctx.bgzf(0, 0, eof=False)
    assert z.bytes() == b"" and z.device() == (0, 0) and z.stats().n_out == 0
    z.close()
    # two calls give the same bytes, and the result outlives its source
    a, b = ctx.bgzf(src.ptr.value + 1, 150_001), ctx.bgzf(src.ptr.value + 1, 150_001)
    src.close()
    assert a.bytes() == b.bytes() == spm.bgzf_frame_host(src.host[1:150_002].tobytes())
    a.close()
    b.close()


@gpu
def test_sam_text_framed_where_it_lies(spm, ctx):
    from test_gpu_sam import _single_end_reads
    from test_rescue import _chain_of

    t, reads, _at = _single_end_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    s = lc.sam(rd, ps, "chr7", secondary=True)
    text, header = s.text(), s.header(len(t["ref"]))
    assert len(text) > 2000
    for D in (0, 1000):
        z = s.bgzf(len(t["ref"]), block_data=D)
        raw = z.bytes()
        assert gzip.decompress(raw) == header + text
        blocks = parse_bgzf(raw[len(z.prefix):], D or 65280)        # the header's blocks are its own: the text starts a block
        assert payload_of(blocks) == text and payload_of(parse_bgzf(z.prefix, D or 65280, eof=False)) == header
        assert z.device()[1] == len(raw) - len(z.prefix) and z.stats().n_in == len(text)
        z.close()
        z = s.bgzf(block_data=D, eof=False)
        assert z.prefix == b"" and gzip.decompress(z.bytes()) == text
        z.close()
    for x in (s, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_refusals(spm, ctx):
    lib, capi = spm.capi.lib(), spm.capi
    err = lambda: lib.spm_hip_last_error(ctx._h)
    src = _DeviceBytes(64, 1502)

    def refused(word, ptr=src.ptr, n=64, opts=None, no_opts=False, no_out=False):
        out = ctypes.c_void_p(1)                                   # (a refusal leaves NULL behind)
        o = None if no_opts else ctypes.byref(opts if opts is not None else spm.bgzf_opts())
        rc = lib.spm_hip_bgzf_frame(ctx._h, ptr, n, o, None if no_out else ctypes.byref(out))
        assert rc == INVALID and (no_out or not out.value) and word in err(), (rc, out.value, err())

    refused(b"NULL opts", no_opts=True)
    refused(b"NULL out", no_out=True)
    refused(b"NULL device_src", ptr=None)
    refused(b"block_data", opts=capi.BgzfOpts(65281, 1, 0))
    refused(b"flag", opts=capi.BgzfOpts(0, 3, 0))
    refused(b"reserved", opts=capi.BgzfOpts(0, 1, 5))
    with pytest.raises(spm.SpmError, match="-1.*block_data"):
        ctx.bgzf(src.ptr.value, 64, block_data=70_000)
    z = ctx.bgzf(src.ptr.value, 64, block_data=65280)               # the largest block size is accepted
    assert z.bytes() == spm.bgzf_frame_host(src.host[:64].tobytes())
    z.close()
    src.close()
