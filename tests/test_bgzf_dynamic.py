"""SPM_BGZF_DYNAMIC, the part that needs no device: spm_hip_bgzf_deflate_host with the flag over every length, block size and kind
of data at which the choice between stored, fixed and dynamic Huffman takes another path.  Every file is taken apart by
tests/deflate_dynamic.py (zlib inflates every block and must consume exactly what BSIZE says; the header of a dynamic block is
decoded bit by bit and held to the format's conditions) and by gzip; block by block it is compared with the same call without
the flag.  The worked cases of spm_hip.h, the refusals, the layouts."""
import ctypes
import gzip
import itertools

import numpy as np
import pytest

import deflate_dynamic as dyn
from test_bgzf_deflate import BLOCKS, LAYOUT_C, LENGTHS, rand, records, sam_text
from cpp_programs import c_layout

OK, INVALID = 0, -1


def uniform40(n, seed=2101):
    return np.random.default_rng(seed).integers(0, 40, n, dtype=np.uint8).tobytes()


def fibonacci_block():
    """46 367 bytes in which value v < 22 occurs F(v + 1) times (1, 1, 2, 3, ...), arranged so that the parse leaves the counts
    of the literal/length symbols steep enough for a code of 15 bits.  A plain shuffle does not: the greedy parse turns most of
    the frequent values into matches of 3 to 6 bytes (longest code 13).  The arrangement, deterministic:
      * in front, every byte of the values 0 .. 18 but 7 and 12, all of which stay literals: the far candidate of a position
        comes from EARLIER segments of 256 positions only, so the bytes are laid in periodic patterns of two to four values (x x y
        z, x y x z, x x y y, w x y z, x x y, x y z, x y) whose 4-grams start in one segment only, and no value stands three times
        in a row;
      * behind, what the patterns could not place of the most frequent of those values, then the values 7, 12, 19, 20 and 21,
        each as ONE run: one literal and a match per chunk.
    The counts are then 1, 1, 2, 3, 5, 8, 13 | 34, 55, 89, 144 | 233 .. 2584, about 3500, with the run tokens' length symbol
    (about 195) where 12's 233 stood, and a dozen symbols of count 1 or 2 below."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    literal = set(range(19)) - {7, 12}
    top = max(literal)
    left = [fib[v] if v in literal else 0 for v in range(22)]
    weight = lambda v: left[v] * (0.6 if v == top else 1.0)         # (the most frequent value may be left over: it goes last)
    out, first_segment = [], {}                                      # 4-gram -> the segment in which it first starts
    forms = [(0, 0, 1, 2), (0, 1, 0, 2), (0, 0, 1, 1), (0, 1, 2, 3), (0, 0, 1), (0, 1, 2), (0, 1)]

    def grams(seq, register):
        """the 4-grams that seq completes behind out: all new or of their own segment, no run of three -> True"""
        trial, base, local = out[-3:] + seq, len(out) - len(out[-3:]), {}
        for k in range(len(trial) - 3):
            start = base + k
            if start + 3 < len(out):
                continue
            g = tuple(trial[k:k + 4])
            seen = first_segment.get(g, local.get(g))
            local.setdefault(g, start // 256)
            if (seen is not None and seen != start // 256) or g[0] == g[1] == g[2] or g[1] == g[2] == g[3]:
                return False
        if register:
            for g, segment in local.items():
                first_segment.setdefault(g, segment)
        return True

    while sum(left):
        room = 256 - len(out) % 256
        order = sorted((v for v in range(22) if left[v]), key=lambda v: -weight(v))[:6]
        best = None
        for form in forms:
            for pick in itertools.permutations(order, max(form) + 1):
                unit = [pick[j] for j in form]
                n = min([room] + [(left[v] // unit.count(v)) * len(unit) + len(unit) - 1 for v in set(unit)])
                seq = [unit[j % len(unit)] for j in range(n)]
                while seq and any(seq.count(v) > left[v] for v in set(seq)):
                    seq.pop()
                score = (len(seq), sum(weight(v) for v in unit) / len(unit))
                if len(seq) >= min(room, 4) and (best is None or score > best[0]) and grams(seq[:len(unit) + 6], False):
                    best = (score, seq)
        if best is None:
            break                                                    # (what is left goes behind, as runs)
        assert grams(best[1], True)
        out += best[1]
        for v in best[1]:
            left[v] -= 1
    for v in sorted(range(22), key=lambda v: (v not in literal, v)):
        out += [v] * (fib[v] - out.count(v))
    assert len(out) == 46_367 and all(out.count(v) == fib[v] for v in range(22))
    return bytes(out)


def quality_records(n_records, seed=2103):
    """test_bgzf_deflate.records with the 150 ff bytes of every record replaced by Phred-like bytes: values 2 .. 41, skewed
    towards the high ones, one read in ten ending in a tail of 2s"""
    rng = np.random.default_rng(seed)
    base = records(n_records, seed)
    size = len(base) // n_records
    out = bytearray(base)
    for i in range(n_records):
        q = 41 - np.minimum(rng.geometric(0.25, 150) - 1, 39)
        if i % 10 == 9:
            q[150 - int(rng.integers(10, 60)):] = 2
        at = base.index(b"\xff" * 150, i * size)
        assert at < (i + 1) * size
        out[at:at + 150] = q.astype(np.uint8).tobytes()
    return bytes(out)


def mixed(seed=2104):
    """random bytes, quality records, a short tail: a stored block, dynamic blocks and a fixed one in one file"""
    return rand(65280, seed) + quality_records(440, seed)[:2 * 65280] + b"abcdefgh"


def check(spm, data, D=0, eof=True):
    """one flagged host call taken apart and held against the call without the flag -> (the file, its blocks)"""
    raw = spm.bgzf_deflate_host(data, D, eof=eof, dynamic=True)
    blocks = dyn.parse(raw, D or 65280, eof=eof)
    assert dyn.payload_of(blocks) == data
    assert (gzip.decompress(raw) if raw else b"") == data
    plain = spm.bgzf_deflate_host(data, D, eof=eof)
    plain_blocks = dyn.parse(plain, D or 65280, eof=eof)
    end, plain_end = len(raw) - (28 if eof else 0), len(plain) - (28 if eof else 0)
    sizes, plain_sizes = dyn.sizes_of(blocks, end), dyn.sizes_of(plain_blocks, plain_end)
    assert len(sizes) == len(plain_sizes) and all(a <= b for a, b in zip(sizes, plain_sizes))
    for (o, p, t, _h), (po, _pp, pt, _ph), size, plain_size in zip(blocks, plain_blocks, sizes, plain_sizes):
        assert pt in (0, 1) and (size < plain_size if t == 2 else (t == pt and raw[o:o + size] == plain[po:po + plain_size]))
        assert t == (raw[o + 18] >> 1) & 3 and size <= len(p) + 31
    return raw, blocks


@pytest.mark.parametrize("D", BLOCKS)
def test_every_length_inflates(spm, D):
    src = rand(max(LENGTHS) + 1)
    low = uniform40(max(LENGTHS) + 1)
    for n in LENGTHS:
        if D == 1 and n > 70_000:
            n = 3000                                                # (blocks of one byte: as many Python-side inflates as bytes)
        for eof in (True, False):
            raw, blocks = check(spm, src[1:1 + n], D, eof)
            assert len(blocks) == (n + (D or 65280) - 1) // (D or 65280)
            if n == 0:
                assert raw == (dyn.EOF_BLOCK if eof else b"")
        if D != 1 or n <= 3000:
            raw, blocks = check(spm, low[1:1 + n], D)
            if D == 0 and n >= 255:
                assert blocks[0][2] == 2
    # random bytes do not shrink in any code: blocks long enough stay stored, and the file is the stored framer's
    if D in (0, 257):
        for n in ((257, 257 * 300) if D else (257, 65280, 65280 + 4000, 2 * 65280)):
            raw, blocks = check(spm, src[:n], D)
            assert dyn.types_of(blocks) == (len(blocks), 0, 0) and raw == spm.bgzf_frame_host(src[:n], D)
    assert spm.bgzf_deflate_host(low[:70_000], D, dynamic=True) == spm.bgzf_deflate_host(low[:70_000], D, dynamic=True)


def test_one_byte_repeated(spm):
    # one literal, matches at distance 1: a single distance symbol, so step 1's padding is live in the distance code
    for d, D in ((65280, 0), (65279, 0), (5000, 0), (70_000, 0), (20_000, 4096)):
        raw, blocks = check(spm, b"\xff" * d, D, eof=False)
        assert dyn.types_of(blocks)[2] >= 1
        for _o, _p, t, h in blocks:
            if t == 2:
                assert h["dd"] == [1, 1] and h["hdist"] == 1
    raw, blocks = check(spm, b"\xff" * 65280, 0, eof=False)
    assert len(raw) < len(spm.bgzf_deflate_host(b"\xff" * 65280, eof=False)) // 2


def test_uniform_over_forty_values(spm):
    # an optimal code costs no more than a flat 6-bit code over the at most 64 symbols in use; the header is below 300 bytes
    d = 65280
    raw, blocks = check(spm, uniform40(d), 0, eof=False)
    assert len(blocks) == 1 and blocks[0][2] == 2 and len(raw) <= 3 * d // 4 + 400, len(raw)
    assert blocks[0][3]["bits"] < 300 * 8


def test_fibonacci_counts_engage_the_limit(spm):
    """The block of Fibonacci byte counts, arranged as fibonacci_block() says, has a longest literal/length code of exactly 15
    bits.  (The block reaches the limit; it does not exceed it: the end-of-block symbol's count of 1 and the run tokens' length
    symbols make the tree bushier than the bare counts, and an arrangement whose unlimited code is deeper than 15 would need more
    distinct 4-grams among the four most frequent values than there are.  Histograms that DO exceed it -- Fibonacci counts over
    17, 22 and 30 symbols -- go through the same routine in tests/cpp/bgzf_huffman_core_cases.cpp, cost held against a textbook
    package-merge.)"""
    data = fibonacci_block()
    raw, blocks = check(spm, data, 0, eof=False)
    assert len(blocks) == 1 and blocks[0][2] == 2
    assert max(blocks[0][3]["ll"]) == 15, sorted(blocks[0][3]["ll"])[-8:]


def test_text_and_quality_records(spm):
    for D in (0, 4096, 1000):
        raw, blocks = check(spm, sam_text(700), D)
        assert dyn.types_of(blocks)[0] == 0 and dyn.types_of(blocks)[2] >= 1
    data = quality_records(480)
    raw, blocks = check(spm, data)
    assert len(blocks) >= 2 and dyn.types_of(blocks)[2] >= 1
    assert len(raw) < len(spm.bgzf_deflate_host(data))
    assert spm.bgzf_deflate_host(data, dynamic=True) == raw
    check(spm, data, 3000)
    raw, blocks = check(spm, records(480))                          # the ff fill
    assert len(raw) < len(spm.bgzf_deflate_host(records(480)))
    # all three types in one file
    raw, blocks = check(spm, mixed())
    assert all(n >= 1 for n in dyn.types_of(blocks)), dyn.types_of(blocks)
    assert [blk[2] for blk in blocks] == [0, 2, 2, 1]


def test_worked_cases_and_short_blocks(spm):
    # the worked cases of spm_hip.h
    assert spm.bgzf_deflate_host(b"ab" * 20, eof=False, dynamic=True).hex() == (
        "1f8b08040000000000ff0600424302002e00" "05c181000000008020d6f387b89224499224499264" "135ad4bc" "28000000")
    assert spm.bgzf_deflate_host(b"a" * 1000, eof=False, dynamic=True).hex() == (
        "1f8b08040000000000ff0600424302003400" "a5c1010d000000c2a0acf62f61856fc090524a29a594524a29551d" "03da389a" "e8030000")
    for worked in (b"ab" * 20, b"a" * 1000):
        raw, blocks = check(spm, worked)
        assert blocks[0][2] == 2
    h = dyn.parse(spm.bgzf_deflate_host(b"ab" * 20, dynamic=True))[0][3]
    assert (h["hlit"], h["hdist"], h["hclen"], h["bits"]) == (0, 1, 14, 105)
    assert (h["ll"][97], h["ll"][98], h["ll"][256], h["dd"]) == (2, 1, 2, [1, 1])
    # short blocks keep their fixed form: the dynamic header alone outweighs them
    fixed = spm.bgzf_deflate_host(b"abcdef")
    assert spm.bgzf_deflate_host(b"abcdef", dynamic=True) == fixed and fixed[18] & 7 == 3
    assert spm.bgzf_deflate_host(b"x", dynamic=True) == spm.bgzf_deflate_host(b"x") and spm.bgzf_deflate_host(b"x")[18] & 7 == 3
    assert spm.bgzf_deflate_host(b"a" * 300, dynamic=True) == spm.bgzf_deflate_host(b"a" * 300)


def test_flags_layouts_and_names(spm, tmp_path):
    lib, capi = spm.capi.lib(), spm.capi
    err = lambda: lib.spm_hip_last_error(None)
    data = quality_records(20)
    src = ctypes.create_string_buffer(data, len(data))
    dst = ctypes.create_string_buffer(len(data) + 100)
    need, bound = ctypes.c_uint64(), ctypes.c_uint64()
    assert capi.BGZF_DYNAMIC == 4
    for flags in (4, 5):
        opts = capi.BgzfDeflateOpts(0, flags, 1, 0)
        assert lib.spm_hip_bgzf_deflate_bound(len(data), ctypes.byref(opts), ctypes.byref(bound)) == OK
        assert bound.value == len(spm.bgzf_frame_host(data, eof=bool(flags & 1)))            # the bound stays the stored size
        assert lib.spm_hip_bgzf_deflate_host(src, len(data), ctypes.byref(opts), dst, len(data) + 100, ctypes.byref(need)) == OK
        assert dst.raw[:need.value] == spm.bgzf_deflate_host(data, eof=bool(flags & 1), dynamic=True)
    assert spm.bgzf_deflate_opts(dynamic=True).flags == 5 and spm.bgzf_deflate_opts(7, False, dynamic=True).flags == 4
    assert spm.bgzf_deflate_opts().flags == 1
    for flags in (2, 3, 6, 8):
        opts = capi.BgzfDeflateOpts(0, flags, 1, 0)
        rc = lib.spm_hip_bgzf_deflate_host(src, len(data), ctypes.byref(opts), dst, len(data) + 100, ctypes.byref(need))
        assert rc == INVALID and b"flag" in err(), (flags, rc, err())
        rc = lib.spm_hip_bgzf_deflate_bound(len(data), ctypes.byref(opts), ctypes.byref(bound))
        assert rc == INVALID and b"flag" in err(), (flags, rc, err())
    for level in (0, 2, 6):
        opts = capi.BgzfDeflateOpts(0, 5, level, 0)
        assert lib.spm_hip_bgzf_deflate_bound(len(data), ctypes.byref(opts), ctypes.byref(bound)) == INVALID and b"level" in err()
    # the frame calls go on refusing the flag
    for flags in (4, 5):
        opts = capi.BgzfOpts(0, flags, 0)
        assert lib.spm_hip_bgzf_framed_size(len(data), ctypes.byref(opts), ctypes.byref(bound)) == INVALID
        assert lib.spm_hip_bgzf_frame_host(src, len(data), ctypes.byref(opts), dst, len(data) + 100, ctypes.byref(need)) == INVALID
    # the layouts are what they were
    assert ctypes.sizeof(capi.BgzfDeflateOpts) == 16 and ctypes.sizeof(capi.BgzfDeflateStats) == 72
    want = c_layout(tmp_path, LAYOUT_C)
    assert (int(want.pop("sizeof.opts")), int(want.pop("sizeof.stats"))) == (16, 72) and len(want) == 4 + 11
    assert len(capi.BgzfDeflateOpts._fields_) == 4 and len(capi.BgzfDeflateStats._fields_) == 11
    flag = c_layout(tmp_path, '#include <stdio.h>\n#include "spm_hip.h"\nint main(void) { printf("flag %u\\n", SPM_BGZF_DYNAMIC); return 0; }\n')
    assert flag == {"flag": "4"}
    assert "spm_hip_bgzf_block_types" in capi.EXPORTS and hasattr(lib, "spm_hip_bgzf_block_types")
    assert lib.spm_hip_bgzf_block_types(None, None) == INVALID
    assert callable(spm.Bgzf.block_types)
