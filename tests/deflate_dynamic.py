"""A strict parser of BGZF files whose blocks hold ONE deflate block each -- stored, fixed Huffman or dynamic Huffman -- written
from RFC 1951 and RFC 1952 alone: what the tests of SPM_BGZF_DYNAMIC share.  A plain module; it shares nothing with the C++.  The
inflating is zlib's; the header of a dynamic block is decoded here, bit by bit, and held to the conditions the format sets."""
import struct
import zlib
from fractions import Fraction

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
BLOCK_DATA = 65280
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class _Bits:
    """a deflate bit stream: bits leave every byte from its least significant end"""

    def __init__(self, data, at=0):
        self.data, self.at = data, at

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.at >> 3] >> (self.at & 7)) & 1) << i
            self.at += 1
        return v

    def symbol(self, table):
        """one Huffman code, first bit first; table: {(length, code): symbol}"""
        code = 0
        for length in range(1, 16):
            code = code << 1 | self.take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise AssertionError("no code of at most 15 bits matches")


def canonical(lengths):
    """RFC 1951 3.2.2 -> {(length, code): symbol}"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, next_code = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        next_code[bits] = code
    table = {}
    for sym, n in enumerate(lengths):
        if n:
            table[(n, next_code[n])] = sym
            next_code[n] += 1
    return table


def kraft(lengths):
    return sum(Fraction(1, 1 << n) for n in lengths if n)


def dynamic_header(deflated):
    """The header of a dynamic block -> {hlit, hdist, hclen, cl, ll, dd, bits}: the three counts as transmitted, the three length
    vectors (19, hlit + 257 and hdist + 1 entries) and the number of bits up to the first token.  Asserts what a complete code
    needs: Kraft sum exactly 1 for each of the three codes, no length above 15 (7 for the code-length code), a code for symbol
    256, HCLEN + 4 ending at the last nonzero entry of the permuted order (or at 4), no repeat without a predecessor or past the
    end."""
    b = _Bits(deflated)
    assert b.take(1) == 1 and b.take(2) == 2
    hlit, hdist, hclen = b.take(5), b.take(5), b.take(4)
    assert hlit <= 29 and hdist <= 29
    cl = [0] * 19
    for i in range(hclen + 4):
        cl[CL_ORDER[i]] = b.take(3)
    assert hclen == 0 or cl[CL_ORDER[hclen + 3]] != 0, (hclen, cl)
    assert max(cl) <= 7 and kraft(cl) == 1, cl
    table = canonical(cl)
    n = hlit + 257 + hdist + 1
    seq = []
    while len(seq) < n:
        s = b.symbol(table)
        if s < 16:
            seq.append(s)
        elif s == 16:
            assert seq, "a repeat with nothing in front of it"
            seq += [seq[-1]] * (3 + b.take(2))
        elif s == 17:
            seq += [0] * (3 + b.take(3))
        else:
            seq += [0] * (11 + b.take(7))
    assert len(seq) == n, (len(seq), n)
    ll, dd = seq[:hlit + 257], seq[hlit + 257:]
    assert ll[-1] != 0 or hlit == 0
    assert dd[-1] != 0 or hdist == 0
    assert max(ll) <= 15 and max(dd) <= 15 and ll[256] != 0
    assert kraft(ll) == 1 and kraft(dd) == 1, (kraft(ll), kraft(dd))
    return {"hlit": hlit, "hdist": hdist, "hclen": hclen, "cl": cl, "ll": ll, "dd": dd, "bits": b.at}


def parse(raw, block_data=BLOCK_DATA, eof=True, sections=1):
    """-> [(file offset, payload, btype, header)] of the data blocks; header is dynamic_header() of a dynamic block, else None.
    Per block: the 16 fixed header bytes; BSIZE inside the file; the first payload byte says BFINAL 1 and BTYPE 00, 01 or 10;
    zlib's raw inflate consumes exactly the BSIZE - 25 bytes between header and CRC, reaches the end of the stream there and
    leaves nothing over; CRC32 and ISIZE of what came out; at most d + 31 bytes.  Every block but the last of a section holds
    block_data bytes and none is empty.  The file ends in the end-of-file block (eof) or in a data block."""
    raw = bytes(raw)
    end = len(raw)
    if eof:
        assert raw[-28:] == EOF_BLOCK, raw[-28:].hex()
        end -= 28
    blocks, at = [], 0
    while at < end:
        assert end - at >= 18 + 8, (at, end)
        assert raw[at:at + 16] == HEAD, (at, raw[at:at + 16].hex())
        (bsize,) = struct.unpack_from("<H", raw, at + 16)
        total = bsize + 1
        assert at + total <= end and total > 26, (at, bsize, end)
        deflated = raw[at + 18:at + total - 8]
        assert len(deflated) == bsize - 25
        bfinal, btype = deflated[0] & 1, (deflated[0] >> 1) & 3
        assert bfinal == 1 and btype in (0, 1, 2), (at, deflated[0])
        z = zlib.decompressobj(-15)
        payload = z.decompress(deflated)
        assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b"", (at, len(z.unused_data))
        crc, isize = struct.unpack_from("<II", raw, at + total - 8)
        assert crc == zlib.crc32(payload) and isize == len(payload), (at, hex(crc), isize, len(payload))
        d = len(payload)
        assert 1 <= d <= block_data and total <= d + 31, (at, d, total)
        if btype == 0:
            assert total == d + 31
        blocks.append((at, payload, btype, dynamic_header(deflated) if btype == 2 else None))
        at += total
    assert at == end
    short = [i for i, blk in enumerate(blocks[:-1]) if len(blk[1]) != block_data]
    assert len(short) <= sections - 1, short
    return blocks


def payload_of(blocks):
    return b"".join(blk[1] for blk in blocks)


def types_of(blocks):
    """(stored, fixed, dynamic)"""
    return tuple(sum(1 for blk in blocks if blk[2] == t) for t in (0, 1, 2))


def sizes_of(blocks, end):
    """the blocks' bytes in the file, whose data blocks end at `end`"""
    starts = [blk[0] for blk in blocks] + [end]
    return [starts[i + 1] - starts[i] for i in range(len(blocks))]


def at_voffset(blocks, voffset, n):
    """n payload bytes from the virtual offset on, read across block borders as a BGZF reader does"""
    coffset, uoffset = voffset >> 16, voffset & 0xFFFF
    i = [blk[0] for blk in blocks].index(coffset)
    assert uoffset < len(blocks[i][1])
    out = blocks[i][1][uoffset:uoffset + n]
    while len(out) < n:
        i += 1
        out += blocks[i][1][:n - len(out)]
    return out
