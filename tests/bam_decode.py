"""What the container tests share, written from the SAM / BAM specification and RFC 1952 alone: a strict parser of BGZF files
whose blocks hold one stored deflate block each.  A plain module, imported by the test files that need it; it shares nothing
with the C++."""
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK_DATA = 65280


def parse_bgzf(raw, block_data=BLOCK_DATA, eof=True):
    """-> [(file offset, payload)] of the data blocks.  Every byte of every block is checked: the gzip header with the BC extra
    field, BSIZE, the stored deflate block's BFINAL / LEN / NLEN, the CRC32 of the payload by zlib and ISIZE; that every block
    but the last holds block_data bytes and none is empty; that the file ends in the end-of-file block (eof) or in a data block."""
    raw = bytes(raw)
    end = len(raw)
    if eof:
        assert raw[-28:] == EOF_BLOCK, raw[-28:].hex()
        end -= 28
    blocks, at = [], 0
    while at < end:
        assert end - at >= 31 + 1, (at, end)
        head = raw[at:at + 18]
        assert head[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), (at, head.hex())
        (bsize,) = struct.unpack_from("<H", head, 16)
        d = bsize - 30
        assert 1 <= d <= block_data and at + d + 31 <= end, (at, bsize)
        bfinal, ln, nln = struct.unpack_from("<BHH", raw, at + 18)
        assert bfinal == 1 and ln == d and nln == (~d & 0xFFFF), (at, bfinal, ln, nln)
        payload = raw[at + 23:at + 23 + d]
        crc, isize = struct.unpack_from("<II", raw, at + 23 + d)
        assert crc == zlib.crc32(payload) and isize == d, (at, hex(crc), hex(zlib.crc32(payload)), isize)
        blocks.append((at, payload))
        at += d + 31
    assert at == end
    assert all(len(p) == block_data for _o, p in blocks[:-1])
    return blocks


def payload_of(blocks):
    return b"".join(p for _o, p in blocks)


def at_voffset(blocks, voffset, n):
    """n payload bytes from the virtual offset on, read across block borders as a BGZF reader does"""
    coffset, uoffset = voffset >> 16, voffset & 0xFFFF
    starts = [o for o, _p in blocks]
    i = starts.index(coffset)                                       # a virtual offset names the first byte of a block
    assert uoffset < len(blocks[i][1])
    out = blocks[i][1][uoffset:uoffset + n]
    while len(out) < n:
        i += 1
        out += blocks[i][1][:n - len(out)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# BAM (SAM specification, section 4): the uncompressed stream back into SAM text
# ---------------------------------------------------------------------------------------------------------------------
SEQ_LETTERS = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
TAG_FORMATS = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def reg2bin(beg, end):
    """section 5.3, in Python's own arithmetic"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def parse_bam_header(stream):
    """-> (the header text, [(name, length)], the offset of the first record)"""
    assert stream[:4] == b"BAM\x01"
    (l_text,) = struct.unpack_from("<i", stream, 4)
    text = stream[8:8 + l_text]
    at = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", stream, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", stream, at)
        name = stream[at + 4:at + 4 + l_name]
        assert l_name >= 2 and name[-1] == 0 and 0 not in name[:-1]
        (l_ref,) = struct.unpack_from("<i", stream, at + 4 + l_name)
        refs.append((name[:-1].decode(), l_ref))
        at += 8 + l_name
    return text, refs, at


def render_records(stream, refs):
    """the records of an uncompressed record stream -> [(offset, length, the SAM line as bytes)], every record, in order.
    Every length is checked against the record's own block_size, and the bin against reg2bin."""
    out, at = [], 0
    while at < len(stream):
        (block_size,) = struct.unpack_from("<i", stream, at)
        assert block_size >= 32 and at + 4 + block_size <= len(stream), (at, block_size)
        ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_id, next_pos, tlen = struct.unpack_from("<iiBBHHHIiii", stream, at + 4)
        p = at + 36
        name = stream[p:p + l_name]
        assert l_name >= 2 and name[-1] == 0 and 0 not in name[:-1]
        p += l_name
        words = struct.unpack_from(f"<{n_cigar}I", stream, p)
        p += 4 * n_cigar
        assert all((w & 15) < len(CIGAR_OPS) and (w >> 4) >= 1 for w in words)
        cigar = "".join(f"{w >> 4}{CIGAR_OPS[w & 15]}" for w in words) or "*"
        packed = stream[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(SEQ_LETTERS[b >> 4] + SEQ_LETTERS[b & 15] for b in packed)[:l_seq] or "*"
        if l_seq & 1:
            assert packed[-1] & 15 == 0
        qual = stream[p:p + l_seq]
        p += l_seq
        assert qual == b"\xff" * l_seq                              # absent qualities; SAM prints *
        tags = []
        end = at + 4 + block_size
        while p < end:
            tag, typ = stream[p:p + 2].decode(), chr(stream[p + 2])
            fmt = TAG_FORMATS[typ]
            (v,) = struct.unpack_from(fmt, stream, p + 3)
            tags.append(f"{tag}:i:{v}")                             # SAM prints every integer type as i
            p += 3 + struct.calcsize(fmt)
        assert p == end, (at, p, end)
        span = sum(w >> 4 for w in words if CIGAR_OPS[w & 15] in "MDN=X")
        assert bin_ == (4680 if pos < 0 else reg2bin(pos, pos + max(span, 1))), (at, bin_, pos, span)
        assert -1 <= ref_id < len(refs) and -1 <= next_id < len(refs) and pos >= -1 and next_pos >= -1
        rname = refs[ref_id][0] if ref_id >= 0 else "*"
        rnext = "*" if next_id < 0 else "=" if next_id == ref_id else refs[next_id][0]
        fields = [name[:-1].decode("latin-1"), str(flag), rname, str(pos + 1), str(mapq), cigar, rnext, str(next_pos + 1), str(tlen),
                  seq, "*"] + tags
        out.append((at, 4 + block_size, ("\t".join(fields) + "\n").encode("latin-1")))
        at += 4 + block_size
    assert at == len(stream)
    return out


def bam_to_sam(raw, block_data=BLOCK_DATA):
    """a BAM file -> (the SAM text with its header, the record stream, the records of render_records, the data blocks).  The
    header section ends at a block border; the record blocks behind it are full but the last."""
    blocks = parse_bgzf_sections(raw, block_data)
    stream = payload_of(blocks)
    text, refs, first = parse_bam_header(stream)
    records = render_records(stream[first:], refs)
    return text + b"".join(line for _o, _n, line in records), stream[first:], records, blocks


def parse_bgzf_sections(raw, block_data=BLOCK_DATA):
    """the blocks of a file of two sections (header, records), each framed on its own: like parse_bgzf, but the last block of
    the header section may be short too.  The header of one reference fits one block unless block_data is small."""
    raw = bytes(raw)
    assert raw[-28:] == EOF_BLOCK
    # the header section's length follows from its content: walk blocks until the header is complete
    blocks, at, got = [], 0, b""
    need = None
    while need is None or len(got) < need:
        (bsize,) = struct.unpack_from("<H", raw, at + 16)
        blocks += parse_bgzf(raw[at:at + bsize + 1], block_data, eof=False)
        blocks[-1] = (at, blocks[-1][1])
        got += blocks[-1][1]
        at += bsize + 1
        if need is None and len(got) >= 8:
            l_text = struct.unpack_from("<i", got, 4)[0]
            if len(got) >= 8 + l_text + 8:
                l_name = struct.unpack_from("<i", got, 8 + l_text + 4)[0]     # one reference
                assert struct.unpack_from("<i", got, 8 + l_text)[0] == 1
                need = 8 + l_text + 8 + l_name + 4
    assert len(got) == need
    assert all(len(p) == block_data for _o, p in blocks[:-1])
    rest = parse_bgzf(raw[at:], block_data, eof=True)
    return blocks + [(o + at, p) for o, p in rest]
