"""BGZF blocks with real deflate, the part that needs no device: spm_hip_bgzf_deflate_host over every length, block size and
kind of data at which the token rule takes another path, taken apart by tests/bgzf_inflate.py (zlib inflates every block, and
must consume exactly what BSIZE says) and by gzip; the conditions that follow from the format; the structs of spm_hip.h
against ctypes; the refusals of the host calls."""
import ctypes
import gzip

import numpy as np
import pytest

import bgzf_inflate
from cpp_programs import c_layout

OK, INVALID, UNSUPPORTED, OVERFLOW = 0, -1, -4, -5
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 65279, 65280, 65281, 200_000)
BLOCKS = (0, 257, 64, 1)


def rand(n, seed=1701):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def periodic(n, period, seed=1702):
    unit = rand(period, seed + period)
    return (unit * (n // period + 1))[:n]


def records(n_records, seed=1703):
    """a record stream shaped like the project's BAM records: 36 fixed bytes, a short name, one CIGAR word, 75 SEQ bytes, 150 ff,
    six 7-byte tags"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_records):
        fixed = bytearray(36)
        fixed[0:4] = (296).to_bytes(4, "little")
        fixed[8:12] = int(rng.integers(0, 1 << 20)).to_bytes(4, "little")
        fixed[12:16] = bytes([9, 40, 0x49, 0x12])
        fixed[20:24] = (150).to_bytes(4, "little")
        seq = bytes(int(x) for x in rng.choice(np.frombuffer(bytes.fromhex("11121418212224284142444881828488"), np.uint8), 75))
        tags = b"".join(t + bytes([int(rng.integers(0, 3)), 0, 0, 0]) for t in (b"NMi", b"XHi", b"XNI", b"X0I", b"X1I", b"XRi"))
        out.append(bytes(fixed) + b"r%06d\0" % i + (150 << 4 | 7).to_bytes(4, "little") + seq + b"\xff" * 150 + tags)
    return b"".join(out)


def sam_text(n_lines, seed=1704):
    rng = np.random.default_rng(seed)
    return b"".join(b"read%d\t%d\tchr7\t%d\t40\t150=\t*\t0\t0\t%s\t*\tNM:i:%d\tXH:i:0\tXN:i:1\n"
                    % (i, 16 * int(rng.integers(0, 2)), int(rng.integers(1, 1 << 24)), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150)),
                       int(rng.integers(0, 4))) for i in range(n_lines))


def check(spm, data, D=0, eof=True):
    """one host call taken apart -> (the file, its blocks)"""
    raw = spm.bgzf_deflate_host(data, D, eof=eof)
    blocks = bgzf_inflate.parse(raw, D or 65280, eof=eof)
    assert bgzf_inflate.payload_of(blocks) == data
    assert (gzip.decompress(raw) if raw else b"") == data
    assert len(raw) <= len(spm.bgzf_frame_host(data, D, eof=eof))  # the bound is the stored file
    return raw, blocks


@pytest.mark.parametrize("D", BLOCKS)
def test_every_length_inflates(spm, D):
    src = rand(max(LENGTHS) + 1)
    for n in LENGTHS:
        if D == 1 and n > 70_000:
            n = 3000                                                # (blocks of one byte: as many Python-side inflates as bytes)
        for eof in (True, False):
            data = src[1:1 + n]
            raw, blocks = check(spm, data, D, eof)
            assert len(blocks) == (n + (D or 65280) - 1) // (D or 65280)
            if n == 0:
                assert raw == (bgzf_inflate.EOF_BLOCK if eof else b"")
    # random bytes do not shrink: a block of them that is long enough for its 9-bit literals (112 of 256 values) to outweigh
    # the 5 bytes of a stored block comes out stored, and the file is the stored framer's, byte for byte
    if D in (0, 257):
        for n in ((257, 257 * 300) if D else (257, 65280, 65280 + 4000, 2 * 65280)):
            raw, blocks = check(spm, src[:n], D)
            assert all(t == 0 for _o, _p, t in blocks) and raw == spm.bgzf_frame_host(src[:n], D)


@pytest.mark.parametrize("period", [1, 2, 3, 4, 5, 255, 256, 257])
def test_periodic_data(spm, period):
    for n, D in ((5, 0), (257, 0), (600, 0), (65280, 0), (65281, 0), (70_000, 257), (3000, 64)):
        check(spm, periodic(n, period), D)
    if period == 1:
        # d equal bytes: per chunk one match of at most 18 bits (and lane 0's literal), so 3 + 8 + 18 chunks + 7 bits
        for d in (65280, 65279, 4096, 300, 64):
            raw, blocks = check(spm, b"\xff" * d, 0, eof=False)
            c = max(64, (d + 255) // 256)
            assert blocks[0][2] == 1 and len(raw) - 26 <= 4 + 3 * ((d + c - 1) // c), (d, len(raw))
        assert len(check(spm, b"\xff" * 65280, 0, eof=False)[0]) - 26 <= 772


def test_distances_runs_and_literal_widths(spm):
    # a repeat at distance exactly 32768 may be a match, one at 32769 must not be (zlib refuses a distance beyond its window)
    # (bytes below 144 are 8-bit literals: such a block is fixed Huffman whether anything matches or not)
    low = lambda n, seed: np.random.default_rng(seed).integers(0, 144, n, dtype=np.uint8).tobytes()
    unit = low(300, 5)
    sizes = []
    for dist in (32768, 32769):
        data = unit + low(dist - 300, 6) + unit + low(500, 7)
        raw, _b = check(spm, data)
        sizes.append(len(raw))
    assert sizes[0] + 200 < sizes[1]                                # (300 random bytes as a few matches, not as literals)
    # a run longer than 258 that ends exactly at a chunk's end, and one that ends at the block's end
    d = 65280
    c = (d + 255) // 256
    for end in (100 * c, d):
        data = bytearray(rand(d, 8))
        data[end - 700:end] = b"\x07" * 700
        raw, blocks = check(spm, bytes(data))
    short = rand(500, 9) + b"z" * 300                               # in a short last block, chunks of 64
    check(spm, rand(65280, 10) + short)
    check(spm, short, 0, eof=False)
    # 9-bit literals (bytes >= 144) beside 8-bit ones
    for lo, hi in ((0, 144), (144, 256), (140, 150)):
        data = np.random.default_rng(11).integers(lo, hi, 5000, dtype=np.uint8).tobytes()
        raw, blocks = check(spm, data)
        if hi <= 144:
            assert blocks[0][2] == 1 and len(raw) - 28 <= 26 + (3 + 8 * 5000 + 7 + 7) // 8


def test_records_and_text_shrink(spm):
    data = records(480)
    raw, blocks = check(spm, data)
    assert len(blocks) >= 3 and any(t == 1 for _o, _p, t in blocks) and len(raw) < len(spm.bgzf_frame_host(data))
    assert 2 * len(raw) < len(data)                                 # half of every record is a run of ff
    raw, blocks = check(spm, data[:4096])
    assert blocks[0][2] == 1
    for D in (0, 4096, 1000):
        raw, blocks = check(spm, sam_text(700), D)
        assert all(t == 1 for _o, _p, t in blocks)
    # two calls give equal bytes
    assert spm.bgzf_deflate_host(data) == spm.bgzf_deflate_host(data)
    # mixed data: both block types in one file
    mixed = rand(65280, 12) + data[:65280] + rand(30_000, 13) + b"\0" * 40_000
    raw, blocks = check(spm, mixed)
    assert [t for _o, _p, t in blocks] == [0, 1, 1, 1] or {t for _o, _p, t in blocks} == {0, 1}


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_bgzf_deflate_opts, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_bgzf_deflate_stats, f))
int main(void)
{
    O(block_data); O(flags); O(level); O(reserved);
    S(ms_parse); S(ms_scan); S(ms_place); S(ms_host); S(n_in); S(n_out); S(n_blocks); S(n_stored_blocks); S(n_matches); S(n_literals);
    S(n_prefix_bytes);
    printf("sizeof.opts %zu\nsizeof.stats %zu\n", sizeof(spm_bgzf_deflate_opts), sizeof(spm_bgzf_deflate_stats));
    return 0;
}
"""
CALLS = ("spm_hip_bgzf_deflate", "spm_hip_bgzf_blocks", "spm_hip_bgzf_blocks_device", "spm_hip_bgzf_deflate_stats",
         "spm_hip_bgzf_deflate_host", "spm_hip_bgzf_deflate_bound", "spm_hip_bam_deflate")


def test_layouts_and_names(spm, tmp_path):
    capi = spm.capi
    assert ctypes.sizeof(capi.BgzfDeflateOpts) == 16 and ctypes.sizeof(capi.BgzfDeflateStats) == 72
    want = c_layout(tmp_path, LAYOUT_C)
    assert (int(want.pop("sizeof.opts")), int(want.pop("sizeof.stats"))) == (16, 72)
    types = {"opts": capi.BgzfDeflateOpts, "stats": capi.BgzfDeflateStats}
    seen = dict.fromkeys(types, 0)
    for name, off in want.items():
        kind, field = name.split(".")
        assert getattr(types[kind], field).offset == int(off), name
        seen[kind] += 1
    assert seen == {k: len(t._fields_) for k, t in types.items()} == {"opts": 4, "stats": 11}
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    for f in (spm.Context.bgzf_deflate, spm.Sam.bgzf_deflate, spm.Bam.deflate, spm.Bgzf.block_offsets, spm.Bgzf.voffsets,
              spm.Bgzf.deflate_stats, spm.bgzf_deflate_host, spm.bgzf_deflate_opts):
        assert callable(f)


def test_host_calls_and_their_refusals(spm):
    lib, capi = spm.capi.lib(), spm.capi
    err = lambda: lib.spm_hip_last_error(None)
    data = records(20)
    src = ctypes.create_string_buffer(data, len(data))
    good = spm.bgzf_deflate_opts()
    need, bound = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.spm_hip_bgzf_deflate_bound(len(data), ctypes.byref(good), ctypes.byref(bound)) == OK
    assert bound.value == len(spm.bgzf_frame_host(data))
    # the length without a buffer, then a buffer one byte short: nothing is written
    assert lib.spm_hip_bgzf_deflate_host(src, len(data), ctypes.byref(good), None, 0, ctypes.byref(need)) == OVERFLOW
    want = spm.bgzf_deflate_host(data)
    assert need.value == len(want) <= bound.value
    dst = ctypes.create_string_buffer(b"\xaa" * (need.value + 8), need.value + 8)
    assert lib.spm_hip_bgzf_deflate_host(src, len(data), ctypes.byref(good), dst, need.value - 1, ctypes.byref(need)) == OVERFLOW
    assert dst.raw == b"\xaa" * (need.value + 8)
    assert lib.spm_hip_bgzf_deflate_host(src, len(data), ctypes.byref(good), dst, need.value, ctypes.byref(need)) == OK
    assert dst.raw[:need.value] == want and dst.raw[need.value:] == b"\xaa" * 8
    assert lib.spm_hip_bgzf_deflate_host(None, 0, ctypes.byref(good), None, 0, ctypes.byref(need)) == OVERFLOW and need.value == 28
    no_eof = spm.bgzf_deflate_opts(eof=False)
    assert lib.spm_hip_bgzf_deflate_host(None, 0, ctypes.byref(no_eof), None, 0, ctypes.byref(need)) == OK and need.value == 0

    def refused(word, opts):
        rc = lib.spm_hip_bgzf_deflate_host(src, len(data), ctypes.byref(opts) if opts is not None else None, dst, 10 ** 6, ctypes.byref(need))
        assert rc == INVALID and word in err(), (rc, err())
        rc = lib.spm_hip_bgzf_deflate_bound(len(data), ctypes.byref(opts) if opts is not None else None, ctypes.byref(bound))
        assert rc == INVALID and word in err(), (rc, err())

    refused(b"NULL opts", None)
    refused(b"block_data", capi.BgzfDeflateOpts(65281, 1, 1, 0))
    refused(b"flag", capi.BgzfDeflateOpts(0, 2, 1, 0))
    refused(b"level", capi.BgzfDeflateOpts(0, 1, 0, 0))
    refused(b"level", capi.BgzfDeflateOpts(0, 1, 6, 0))
    refused(b"reserved", capi.BgzfDeflateOpts(0, 1, 1, 7))
    assert lib.spm_hip_bgzf_deflate_host(None, 5, ctypes.byref(good), dst, 100, ctypes.byref(need)) == INVALID and b"NULL src" in err()
    assert lib.spm_hip_bgzf_deflate_host(src, 5, ctypes.byref(good), dst, 100, None) == INVALID and b"NULL len" in err()
    assert lib.spm_hip_bgzf_deflate_host(src, 5, ctypes.byref(good), None, 100, ctypes.byref(need)) == INVALID and b"NULL dst" in err()
    assert lib.spm_hip_bgzf_deflate_bound(2 ** 64 - 1, ctypes.byref(good), ctypes.byref(bound)) == UNSUPPORTED
    with pytest.raises(spm.SpmError, match="-1.*block_data"):
        spm.bgzf_deflate_host(b"abc", 70_000)
    for worked in (b"abcdef", b"a" * 300):                           # the worked cases of spm_hip.h: zlib inflates them
        check(spm, worked)
    assert spm.bgzf_deflate_host(b"abcdef").hex() == ("1f8b08040000000000ff0600424302002100" "4b4c4a4e494d0300" "ef398e4b" "06000000"
                                                     + bgzf_inflate.EOF_BLOCK.hex())
    assert spm.bgzf_deflate_host(b"a" * 300, eof=False).hex() == ("1f8b08040000000000ff0600424302002500" "4ba410500a28059402520000"
                                                                 "09199789" "2c010000")
