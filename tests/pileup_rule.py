"""The pileup rule of spm_hip.h (spm_hip_bam_pileup, spm_hip_pileup_sites) written again in Python over the records of an
uncompressed BAM record stream, decoded here with struct and the tables of bam_decode.py: one loop per record and column, no
tiles, independent of the C record parser.  Also a maker of record streams with real SEQ nibbles, qualities, names of any
length and arbitrary CIGAR words.  A plain module, imported by the test files that need it."""
import re
import struct

import numpy as np

from bam_decode import CIGAR_OPS, SEQ_LETTERS, reg2bin
from test_sam import LINE

PLANES = ("A", "C", "G", "T", "N", "DEL", "INS", "LOWQ")
DEFAULT_EXCLUDE = 0x704
_ITEM = re.compile(r"([0-9]+)([MIDNSHP=X])")


def words_of(cigar):
    """'4M2D3M' -> the BAM CIGAR words"""
    return [int(n) << 4 | CIGAR_OPS.index(op) for n, op in _ITEM.findall(cigar)]


def make_stream(recs):
    """recs: dicts with pos and cigar (a string, or words: a list of CIGAR words), and optionally flag (0), seq (letters; A's of the
    CIGAR's query length), qual (Phred values; ff without), name (bytes, b"r"), mapq (60), ref_id (0), read (the record's index),
    l_seq (to disagree with the CIGAR) -> (the record stream, its LINE records).  The bin is the specification's."""
    out, lines = b"", np.zeros(len(recs), LINE)
    for i, r in enumerate(recs):
        words = list(r["words"]) if "words" in r else words_of(r.get("cigar", ""))
        flag, pos, ref_id = r.get("flag", 0), r["pos"], r.get("ref_id", 0)
        query = sum(w >> 4 for w in words if (w & 15) in (0, 1, 4, 7, 8))
        seq = r.get("seq", "A" * r.get("l_seq", query))
        l_seq = r.get("l_seq", len(seq))
        codes = [SEQ_LETTERS.index(c) for c in seq] + [0] * (l_seq + 1)
        packed = bytes(codes[2 * k] << 4 | codes[2 * k + 1] for k in range((l_seq + 1) // 2))
        qual = bytes(r["qual"]) if "qual" in r else b"\xff" * l_seq
        assert len(qual) == l_seq
        span = 0 if flag & 4 else sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))
        bin_ = reg2bin(pos, pos + max(span, 1)) if pos >= 0 else 4680
        nm = r.get("name", b"r") + b"\0"
        body = (struct.pack("<iiBBHHHIiii", ref_id, pos, len(nm), r.get("mapq", 60), bin_, len(words), flag, l_seq, -1, -1, 0) + nm +
                struct.pack(f"<{len(words)}I", *words) + packed + qual)
        lines[i]["offset"], lines[i]["len"], lines[i]["flag"], lines[i]["read"] = len(out), len(body) + 4, flag, r.get("read", i)
        lines[i]["mapq"] = r.get("mapq", 60)
        out += struct.pack("<i", len(body)) + body
    return out, lines


def parse_records(stream, lines):
    """the records the lines name -> dicts (ref_id, pos, mapq, flag, words, codes: the 4-bit SEQ codes, qual: the bytes)"""
    out = []
    for o, n in zip(lines["offset"].tolist(), lines["len"].tolist()):
        block_size, ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiiBBHHHI", stream, o)
        assert block_size == n - 4
        p = o + 36 + l_name
        words = struct.unpack_from(f"<{n_cigar}I", stream, p)
        p += 4 * n_cigar
        packed = stream[p:p + (l_seq + 1) // 2]
        codes = [(packed[k // 2] >> (0 if k & 1 else 4)) & 15 for k in range(l_seq)]
        p += (l_seq + 1) // 2
        qual = stream[p:p + l_seq]
        assert p + l_seq <= o + n
        out.append(dict(ref_id=ref_id, pos=pos, mapq=mapq, flag=flag, words=words, codes=codes, qual=qual))
    return out


def py_pileup(stream, lines, ref_len, begin=0, end=None, min_mapq=0, min_baseq=0, exclude_flags=None):
    """-> the (8, end - begin) uint32 counts; the inputs are taken to be in order and to agree"""
    end = ref_len if not end else end
    exclude = (exclude_flags or DEFAULT_EXCLUDE) | 4
    counts = np.zeros((8, end - begin), np.uint32)
    plane_of = {1: 0, 2: 1, 4: 2, 8: 3}

    def add(plane, col):
        if begin <= col < end:
            counts[plane, col - begin] += 1

    for rec in parse_records(stream, lines):
        if rec["flag"] & exclude or rec["mapq"] < min_mapq or not rec["words"]:
            continue
        pos = r = rec["pos"]
        q = 0
        assert rec["ref_id"] == 0 and pos >= 0
        for w in rec["words"]:
            op, n = CIGAR_OPS[w & 15], w >> 4
            if op in "M=X":
                for j in range(n):
                    v = rec["qual"][q + j]
                    add(7 if v != 0xff and v < min_baseq else plane_of.get(rec["codes"][q + j], 4), r + j)
                r, q = r + n, q + n
            elif op == "D":
                for j in range(n):
                    add(5, r + j)
                r += n
            elif op == "N":
                r += n
            elif op == "I":
                if r > pos:
                    add(6, r - 1)
                q += n
            elif op == "S":
                q += n
        assert q == len(rec["codes"]) and r <= ref_len
    return counts


def py_sites(counts, begin, ref, min_depth=1, min_alt=2, min_alt_permille=200):
    """-> [(pos, depth, alt, (A, C, G, T), ref rank)] in position order"""
    out = []
    for k in range(counts.shape[1]):
        col = [int(v) for v in counts[:, k]]
        depth = sum(col[:6])
        rank = int(ref[begin + k])
        alt = depth - col[rank if rank < 4 else 4] + col[6]
        if depth >= min_depth and alt >= min_alt and 1000 * alt >= min_alt_permille * depth:
            out.append((begin + k, depth, alt, tuple(col[:4]), rank))
    return out


def sites_as_tuples(sites):
    """PILEUP_SITE_DTYPE records -> py_sites' tuples"""
    return [(int(s["pos"]), int(s["depth"]), int(s["alt"]), tuple(int(c) for c in s["counts"]), int(s["ref"])) for s in sites]
