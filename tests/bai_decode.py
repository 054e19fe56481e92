"""What the index tests share, written from the SAM specification (sections 4.2, 5.2, 5.3) alone: a strict parser of BAI files,
an independent builder over the records that tests/bam_decode.py decodes, and the standard region query over a BGZF file and its
index.  A plain module, imported by the test files that need it; it shares nothing with the C++."""
import struct

from bam_decode import reg2bin

PSEUDO_BIN = 37450
MAX_BIN = 37449                                                     # ((1 << 18) - 1) / 7: bins 0 .. 37448 hold records
WINDOW = 14


# ---------------------------------------------------------------------------------------------------------------------
# the parser
# ---------------------------------------------------------------------------------------------------------------------
def parse_bai(raw):
    """-> dict(bins=[(bin, [(begin, end)])] in file order without the pseudo-bin, pseudo=None or ((begin, end), (n_mapped,
    n_unmapped)), ioffset=[...], n_no_coor).  One reference.  Strict: the magic, bins strictly ascending with the pseudo-bin
    last, no bin without chunks, every chunk begin < end, a bin's chunks in file order and disjoint, the linear index
    non-decreasing, n_no_coor present, nothing behind it."""
    raw = bytes(raw)
    assert raw[:4] == b"BAI\x01", raw[:4]
    n_ref, n_bin = struct.unpack_from("<ii", raw, 4)
    assert n_ref == 1 and n_bin >= 0
    at = 12
    bins, pseudo = [], None
    for b in range(n_bin):
        bin_, n_chunk = struct.unpack_from("<Ii", raw, at)
        at += 8
        chunks = [struct.unpack_from("<QQ", raw, at + 16 * c) for c in range(n_chunk)]
        at += 16 * n_chunk
        if bin_ == PSEUDO_BIN:
            assert b == n_bin - 1 and n_chunk == 2, (b, n_bin, n_chunk)
            pseudo = (chunks[0], chunks[1])
            continue
        assert bin_ < MAX_BIN and n_chunk >= 1, (bin_, n_chunk)
        assert not bins or bins[-1][0] < bin_, (bins[-1][0], bin_)
        assert all(x < y for x, y in chunks), (bin_, chunks)
        assert all(chunks[c - 1][1] <= chunks[c][0] for c in range(1, n_chunk)), (bin_, chunks)
        bins.append((bin_, chunks))
    (n_intv,) = struct.unpack_from("<i", raw, at)
    assert 0 <= n_intv <= 1 << 15
    ioffset = list(struct.unpack_from(f"<{n_intv}Q", raw, at + 4))
    at += 4 + 8 * n_intv
    assert all(a <= b for a, b in zip(ioffset, ioffset[1:]))
    (n_no_coor,) = struct.unpack_from("<Q", raw, at)
    assert at + 8 == len(raw), (at, len(raw))
    assert (pseudo is None) == (not bins) and (n_intv == 0) == (not bins)
    return dict(bins=bins, pseudo=pseudo, ioffset=ioffset, n_no_coor=n_no_coor)


# ---------------------------------------------------------------------------------------------------------------------
# the records of a decoded file, and the order
# ---------------------------------------------------------------------------------------------------------------------
def intervals(records):
    """the records of bam_decode.render_records -> [(offset, len, placed, pos, end, flag)]: what the index takes of a SAM line.
    pos is 0-based; end = pos + max(reference symbols of the CIGAR, 1), pos + 1 for an unmapped line or one without CIGAR."""
    out = []
    for offset, n, line in records:
        f = line[:-1].decode("latin-1").split("\t")
        flag, rname, pos, cigar = int(f[1]), f[2], int(f[3]) - 1, f[5]
        span, num = 0, ""
        if cigar != "*" and not flag & 4:
            for ch in cigar:
                if ch.isdigit():
                    num += ch
                else:
                    span += int(num) if ch in "MDN=X" else 0
                    num = ""
        out.append((offset, n, rname != "*", pos, pos + max(span, 1), flag))
    return out


def sort_key(item):
    """coordinate order: records of the reference first, by position, forward before reverse; Python's sorted keeps ties"""
    _offset, _n, placed, pos, _end, flag = item
    return (0 if placed else 1, pos, 1 if flag & 16 else 0)


def voffset(block_offsets, block_data, u):
    """the virtual offset of offset u of the uncompressed stream"""
    return int(block_offsets[u // block_data]) << 16 | u % block_data


# ---------------------------------------------------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------------------------------------------------
def build_bai(records, block_offsets, block_data):
    """the .bai of a coordinate-sorted record stream: records as render_records gives them, block_offsets the n_blocks + 1 file
    offsets of the stream's blocks.  Chunks are maximal runs of consecutive records of one bin and are not merged further."""
    items = intervals(records)
    assert all(sort_key(a) <= sort_key(b) for a, b in zip(items, items[1:])), "not in coordinate order"
    v = lambda u: voffset(block_offsets, block_data, u)
    bins, linear = {}, {}
    last_bin, n_mapped, n_unmapped, n_no_coor, max_end = None, 0, 0, 0, 0
    first = last = None
    for offset, n, placed, pos, end, flag in items:
        if not placed:
            n_no_coor += 1
            last_bin = None
            continue
        b, beg_v, end_v = reg2bin(pos, end), v(offset), v(offset + n)
        if b == last_bin:
            bins[b][-1][1] = end_v
        else:
            bins.setdefault(b, []).append([beg_v, end_v])
        last_bin = b
        n_mapped, n_unmapped = n_mapped + (not flag & 4), n_unmapped + bool(flag & 4)
        first, last = (beg_v if first is None else first), end_v
        max_end = max(max_end, end)
        for w in range(pos >> WINDOW, ((end - 1) >> WINDOW) + 1):
            linear[w] = min(linear.get(w, beg_v), beg_v)
    out = [b"BAI\x01", struct.pack("<ii", 1, len(bins) + (1 if bins else 0))]
    for b in sorted(bins):
        out.append(struct.pack("<Ii", b, len(bins[b])))
        out += [struct.pack("<QQ", x, y) for x, y in bins[b]]
    if bins:
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, first, last, n_mapped, n_unmapped))
    n_intv = ((max_end - 1) >> WINDOW) + 1 if bins else 0
    filled, nxt = [0] * n_intv, None
    for w in range(n_intv - 1, -1, -1):                             # an empty window: the next one to its right that is not
        nxt = linear.get(w, nxt)
        filled[w] = nxt
    out.append(struct.pack(f"<i{n_intv}Q", n_intv, *filled))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# the query
# ---------------------------------------------------------------------------------------------------------------------
def reg2bins(beg, end):
    """section 5.3: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += list(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


class _Reader:
    """the payload of BGZF blocks [(file offset, payload, ...)] read from a virtual offset on, as a BGZF reader does"""

    def __init__(self, blocks, v):
        self.blocks = blocks
        self.i = [b[0] for b in blocks].index(v >> 16)
        self.u = v & 0xFFFF
        assert self.u < len(blocks[self.i][1])

    def _settle(self):
        while self.i + 1 < len(self.blocks) and self.u == len(self.blocks[self.i][1]):
            self.i, self.u = self.i + 1, 0

    def at_end(self):
        self._settle()
        return self.u == len(self.blocks[self.i][1])

    def tell(self):
        self._settle()
        return self.blocks[self.i][0] << 16 | self.u

    def read(self, n):
        out = b""
        while len(out) < n:
            self._settle()
            got = self.blocks[self.i][1][self.u:self.u + n - len(out)]
            assert got, "read beyond the last block"
            out += got
            self.u += len(got)
        return out


def _overlaps(rec, beg, end):
    """a raw record (block_size and all): placed on the reference and overlapping [beg, end)?  -> (overlaps, pos)"""
    ref_id, pos = struct.unpack_from("<ii", rec, 4)
    l_name, n_cigar, flag = rec[12], *struct.unpack_from("<HH", rec, 16)
    span = 0
    if not flag & 4:
        for (w,) in struct.iter_unpack("<I", rec[36 + l_name:36 + l_name + 4 * n_cigar]):
            span += w >> 4 if (w & 15) in (0, 2, 3, 7, 8) else 0
    return ref_id == 0 and pos < end and pos + max(span, 1) > beg, pos


def fetch(bai, blocks, beg, end):
    """the standard query: the records overlapping [beg, end) of the one reference, as raw bytes in file order.  bai: what
    parse_bai returns; blocks: the data blocks of the file behind its header section.  The candidate bins of reg2bins, of their
    chunks those that end above ioffset[beg >> 14], read by virtual offset."""
    ioffset = bai["ioffset"]
    if not ioffset:
        return []
    min_off = ioffset[min(beg >> WINDOW, len(ioffset) - 1)]
    want = set(reg2bins(beg, end))
    chunks = sorted((x, y) for b, cs in bai["bins"] if b in want for x, y in cs if y > min_off)
    out = []
    for x, y in chunks:
        r = _Reader(blocks, x)
        while not r.at_end() and r.tell() < y:
            (block_size,) = struct.unpack("<i", r.read(4))
            rec = struct.pack("<i", block_size) + r.read(block_size)
            hit, pos = _overlaps(rec, beg, end)
            if hit:
                out.append(rec)
            if pos >= end:
                break
    return out


def scan(stream, beg, end):
    """what fetch has to find: every record of the uncompressed record stream that overlaps [beg, end), by a full walk"""
    out, at = [], 0
    while at < len(stream):
        (block_size,) = struct.unpack_from("<i", stream, at)
        rec = stream[at:at + 4 + block_size]
        if _overlaps(rec, beg, end)[0]:
            out.append(rec)
        at += 4 + block_size
    return out


def queries(items, ref_len):
    """the query set of the tests: every bin-level border inside the reference +- 1, each record's first and last base, the whole
    reference, and an empty stretch if there is one"""
    out = [(0, ref_len)]
    for shift in (14, 17, 20, 23, 26):
        at = 1 << shift
        if at < ref_len:
            out += [(at - 1, at), (at, at + 1), (at - 1, at + 1), (at - 100, at - 1)]
    covered = []
    for _o, _n, placed, pos, end, _f in items:
        if placed:
            out += [(pos, pos + 1), (end - 1, end)]
            covered.append((pos, end))
    covered.sort()
    reach = 0
    for pos, end in covered:                                        # the first gap of at least two bases between records
        if pos > reach + 2:
            out.append((reach + 1, pos - 1))
            break
        reach = max(reach, end)
    return out
