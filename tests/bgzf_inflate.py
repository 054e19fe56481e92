"""A strict parser of BGZF files whose blocks hold ONE deflate block each, stored or fixed Huffman, written from RFC 1951 and
RFC 1952 alone: what the tests of the deflated container share.  A plain module; it shares nothing with the C++, and the
inflating is zlib's."""
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
BLOCK_DATA = 65280


def parse(raw, block_data=BLOCK_DATA, eof=True, sections=1):
    """-> [(file offset, payload, btype)] of the data blocks.  Per block: the 16 fixed header bytes; BSIZE inside the file; the
    first payload byte says BFINAL 1 and BTYPE 00 or 01; zlib's raw inflate consumes exactly the BSIZE - 25 bytes between header
    and CRC, reaches the end of the stream there and leaves nothing over; CRC32 and ISIZE of what came out; at most d + 31 bytes.
    Every block but the last of a section holds block_data bytes and none is empty.  The file ends in the end-of-file block (eof)
    or in a data block.  sections: how many runs of blocks, each with a short last block of its own, the file may hold."""
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
        assert bfinal == 1 and btype in (0, 1), (at, deflated[0])
        z = zlib.decompressobj(-15)
        payload = z.decompress(deflated)
        assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b"", (at, len(z.unused_data))
        crc, isize = struct.unpack_from("<II", raw, at + total - 8)
        assert crc == zlib.crc32(payload) and isize == len(payload), (at, hex(crc), isize, len(payload))
        d = len(payload)
        assert 1 <= d <= block_data and total <= d + 31, (at, d, total)
        if btype == 0:
            assert total == d + 31
        blocks.append((at, payload, btype))
        at += total
    assert at == end
    short = [i for i, (_o, p, _t) in enumerate(blocks[:-1]) if len(p) != block_data]
    assert len(short) <= sections - 1, short
    return blocks


def payload_of(blocks):
    return b"".join(p for _o, p, _t in blocks)


def at_voffset(blocks, voffset, n):
    """n payload bytes from the virtual offset on, read across block borders as a BGZF reader does"""
    coffset, uoffset = voffset >> 16, voffset & 0xFFFF
    starts = [o for o, _p, _t in blocks]
    i = starts.index(coffset)                                       # a virtual offset names the first byte of a block
    assert uoffset < len(blocks[i][1])
    out = blocks[i][1][uoffset:uoffset + n]
    while len(out) < n:
        i += 1
        out += blocks[i][1][:n - len(out)]
    return out
