"""Base qualities and the MD tag on the device: spm_hip_jst_ref_loci_sam_ex / spm_hip_jst_ref_loci_bam_ex and their binding.

Nothing expected comes from the code under test.  The lines without the two fields are the rule of tests/test_gpu_sam.py
(np_sam); QUAL is the read's values, back to front on a reverse line; MD is test_sam_md.py's py_md over the line's own CIGAR,
the needle and the reference, column by column.  Independently of both, the reference stretch of every mapped line is rebuilt
from (SEQ, CIGAR, MD) and compared with the reference.  The BAM of the same inputs is decoded by a decoder of this file (the
shared one insists on ff qualities and integer tags) and compared with the text, record for record; its sorted, indexed and
deflated forms are held to what tests/test_gpu_bam_sort.py and tests/test_gpu_bai.py ask of theirs."""
import ctypes
import re
import struct

import numpy as np
import pytest

import bai_decode
import bgzf_inflate
from bam_decode import CIGAR_OPS, SEQ_LETTERS, TAG_FORMATS, parse_bam_header, parse_bgzf_sections, payload_of, reg2bin
from cpp_programs import download
from test_bai import stored_offsets
from test_gpu_sam import LOCUS, RESCUE, SECONDARY, UNMAPPED, _names, _rescue_reads, _views, np_sam
from test_jst_project import _hap, _make_tree
from test_pairs import MAX_TLEN, MIN_TLEN, _chain, _free_stretches, _planted_chain, _planted_pairs
from test_rescue import K, _chain_of, _open, stranded
from test_sam import LINE
from test_sam_md import MD_RE, letters, py_md, rebuild_reference
from test_strands import np_revcomp

gpu = pytest.mark.gpu
INVALID = -1
RNAME = "chr7"
COMBOS = ((True, False), (False, True), (True, True))              # (qualities, md)


# ---------------------------------------------------------------------------------------------------------------------
# the expected lines, and a decoder of records that carry qualities and a Z tag
# ---------------------------------------------------------------------------------------------------------------------
def np_qualities(reads, seed):
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 94, len(r), dtype=np.uint8) for r in reads]
    for q in out[:8]:
        q[0], q[-1] = 0, 93                                         # '!' and '~': the ends of the range, at the ends of a read
    return out


def with_extras(want, recs, loci, rescues, needles, quals, md, ref, strands, symbols="ACGT"):
    """the lines of np_sam with QUAL and MD:Z: put in by the rule of spm_hip.h -> (lines, records)"""
    out = []
    for line, rec in zip(want, recs):
        f = line[:-1].decode().split("\t")
        kind, src = int(rec["kind"]), int(rec["source"])
        if quals is not None and f[9] != "*":
            q = quals[int(rec["read"])]
            reverse = (kind == LOCUS and strands == 2 and int(loci["pattern"][src]) & 1) or (kind == RESCUE and int(rescues["flag"][src]) & 0x10)
            f[10] = "".join(chr(33 + int(v)) for v in (q[::-1] if reverse else q))
        if md and kind != UNMAPPED:
            pattern = int((rescues if kind == RESCUE else loci)["pattern"][src])
            assert f[11].startswith("NM:i:")
            f.insert(12, "MD:Z:" + py_md(f[5], needles[pattern], ref, int(f[3]) - 1, symbols))
        out.append(("\t".join(f) + "\n").encode())
    new = recs.copy()
    new["len"] = [len(x) for x in out]
    new["offset"] = np.concatenate([[0], np.cumsum(new["len"][:-1])]) if len(out) else []
    return out, new


def decode_records(stream, refs):
    """an uncompressed record stream -> [(offset, length, the SAM line as bytes)]: bam_decode.render_records for records whose
    qualities may be values (all ff prints *) and whose tags may be of type Z.  block_size and bin are checked."""
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
        assert not l_seq & 1 or packed[-1] & 15 == 0
        qual = stream[p:p + l_seq]
        p += l_seq
        if qual == b"\xff" * l_seq:
            qual = "*"
        else:
            assert max(qual) <= 93
            qual = "".join(chr(33 + v) for v in qual)
        tags, end = [], at + 4 + block_size
        while p < end:
            tag, typ = stream[p:p + 2].decode(), chr(stream[p + 2])
            if typ == "Z":
                z = stream.index(b"\0", p + 3, end)
                tags.append(f"{tag}:Z:{stream[p + 3:z].decode('ascii')}")
                p = z + 1
            else:
                (v,) = struct.unpack_from(TAG_FORMATS[typ], stream, p + 3)
                tags.append(f"{tag}:i:{v}")
                p += 3 + struct.calcsize(TAG_FORMATS[typ])
        assert p == end, (at, p, end)
        span = sum(w >> 4 for w in words if CIGAR_OPS[w & 15] in "MDN=X")
        assert bin_ == (4680 if pos < 0 else reg2bin(pos, pos + max(span, 1))), (at, bin_, pos, span)
        rname = refs[ref_id][0] if ref_id >= 0 else "*"
        rnext = "*" if next_id < 0 else "=" if next_id == ref_id else refs[next_id][0]
        fields = [name[:-1].decode("latin-1"), str(flag), rname, str(pos + 1), str(mapq), cigar, rnext, str(next_pos + 1), str(tlen),
                  seq, qual] + tags
        out.append((at, 4 + block_size, ("\t".join(fields) + "\n").encode("latin-1")))
        at += 4 + block_size
    assert at == len(stream)
    return out


def decode_bam(raw, block_data=65280):
    """-> (the header text, the record stream, its records, the data blocks)"""
    blocks = parse_bgzf_sections(raw, block_data)
    stream = payload_of(blocks)
    text, refs, first = parse_bam_header(stream)
    return text, stream[first:], decode_records(stream[first:], refs), blocks


def test_decoder_on_a_hand_made_record():
    """CPU: worked record 1 of spm_hip.h with qualities 2 .. 33 back to front and MD 20G11, put together by hand"""
    fixed = bytes.fromhex("8a000000 00000000 63000000 02 28 4912 0300 1000 20000000 ffffffff ffffffff 00000000 3700".replace(" ", ""))
    body = bytes.fromhex("47010000 18000000 b7000000".replace(" ", "")) + b"\x88" * 10 + b"\x18" + b"\x88" * 5 + bytes(range(33, 1, -1))
    tags = (b"NMi" + struct.pack("<i", 1) + b"MDZ20G11\0" + b"XHi" + struct.pack("<i", 0) + b"XNI" + struct.pack("<I", 2) + b"X0I" +
            struct.pack("<I", 1) + b"X1I" + struct.pack("<I", 1))
    rec = fixed + body + tags
    assert len(rec) == 142
    ((at, n, line),) = decode_records(rec, [("chr", 1000)])
    q = "".join(chr(33 + v) for v in range(33, 1, -1))
    assert (at, n) == (0, 142) and line == ("7\t16\tchr\t100\t40\t20=1X11=\t*\t0\t0\t" + "T" * 20 + "A" + "T" * 11 + "\t" + q +
                                            "\tNM:i:1\tMD:Z:20G11\tXH:i:0\tXN:i:2\tX0:i:1\tX1:i:1\n").encode()


# ---------------------------------------------------------------------------------------------------------------------
# one set of inputs against the rule: every combination of the two fields, text and file
# ---------------------------------------------------------------------------------------------------------------------
def _items(cigar):
    return [(int(n), op) for n, op in re.findall(r"([0-9]+)([MIDX=])", cigar)]


def _check_ex(spm, ctx, lc, rd, ps, ref_text, ref, needles, quals, strands=2, pr=None, rs=None, names=None, cigar_m=False, files=True):
    """-> the device's lines with both fields (fields split), and their records"""
    loci, ops, members, reads, pairs, rescues, rops = _views(lc, rd, pr, rs)
    opts = dict(rname=RNAME, symbols="ACGT", strands=strands, cigar_m=cigar_m, secondary=True)
    base, base_recs = np_sam(loci, ops, members, reads, pairs, rescues, rops, needles, names, opts)
    kw = dict(pairs=pr, rescues=rs, names=names, cigar_m=cigar_m, secondary=True)
    old = lc.sam(rd, ps, RNAME, **kw)
    assert old.text() == b"".join(base)
    none = lc.sam_ex(rd, ps, RNAME, **kw)                          # extras == NULL: the bytes of the old call
    assert none.text() == old.text() and none.lines().tobytes() == old.lines().tobytes()
    none.close()
    both = None
    for with_q, with_md in COMBOS:
        ex = dict(qualities=quals if with_q else None, md=with_md, reference=ref_text if with_md else None)
        want, recs = with_extras(base, base_recs, loci, rescues, needles, quals if with_q else None, with_md, ref, strands)
        s = lc.sam_ex(rd, ps, RNAME, **ex, **kw)
        got, lines = s.text(), s.lines()
        if got != b"".join(want):
            have = got.split(b"\n")
            raise AssertionError([(i, have[i] if i < len(have) else None, w) for i, w in enumerate(want) if i >= len(have) or have[i] + b"\n" != w][:3])
        assert lines.tobytes() == recs.tobytes()
        d_text, n_bytes, d_lines, n_lines = s.device()              # host and device views are equal
        assert n_bytes == len(got) and n_lines == len(recs) and s.stats().n_bytes == len(got)
        assert download(ctx, d_text, n_bytes, np.uint8).tobytes() == got and download(ctx, d_lines, n_lines, LINE).tobytes() == recs.tobytes()
        again = lc.sam_ex(rd, ps, RNAME, **ex, **kw)                # two calls give equal bytes
        assert again.text() == got and again.lines().tobytes() == recs.tobytes()
        again.close()
        s.close()
        if with_md:                                                 # what MD is for, without the rule: the reference, rebuilt
            for line, rec in zip(want, recs):
                f = line[:-1].decode().split("\t")
                if int(rec["kind"]) == UNMAPPED:
                    assert not any(x.startswith("MD:") for x in f[11:])
                    continue
                assert f[12].startswith("MD:Z:") and MD_RE.fullmatch(f[12][5:]), f[12]
                src = (rescues if int(rec["kind"]) == RESCUE else loci)[int(rec["source"])]
                seq = letters(needles[int(src["pattern"])])
                assert f[9] in ("*", seq)
                span = sum(n for n, op in _items(f[5]) if op != "I")
                assert rebuild_reference(seq, f[5], f[12][5:]) == letters(ref[int(f[3]) - 1:int(f[3]) - 1 + span]), f[:6]
        if files:
            b = lc.bam_ex(rd, ps, RNAME, len(ref), **ex, **kw)
            raw = b.bytes()
            text, stream, records, _blocks = decode_bam(raw)
            assert text == spm.sam_header(RNAME, len(ref)) and [r[2] for r in records] == want
            bl = b.lines()
            assert bl["offset"].tolist() == [o for o, _n, _l in records] and bl["len"].tolist() == [n for _o, n, _l in records]
            assert b.records() == stream
            d_file, n_file, d_rec, n_rec, _dl, _nl = b.device()
            assert download(ctx, d_file, n_file, np.uint8).tobytes() == raw and download(ctx, d_rec, n_rec, np.uint8).tobytes() == stream
            again = lc.bam_ex(rd, ps, RNAME, len(ref), **ex, **kw)
            assert again.bytes() == raw
            again.close()
            if with_q and with_md:
                _check_sorted_indexed_deflated(spm, b, records, stream, len(ref))
            b.close()
        if with_q and with_md:
            both = ([x[:-1].decode().split("\t") for x in want], recs)
    nb = lc.bam_ex(rd, ps, RNAME, len(ref), **kw)                   # extras == NULL: the bytes of the old call
    ob = lc.bam(rd, ps, RNAME, len(ref), **kw)
    assert nb.bytes() == ob.bytes()
    nb.close()
    ob.close()
    old.close()
    return both


def _check_sorted_indexed_deflated(spm, b, in_records, in_stream, ref_len):
    """sort(), index() and deflate() of a file whose records carry qualities and MD: the order of Python's sorted(), the index of
    the host builder and of the specification's, the deflated blocks inflated by zlib"""
    D = 65280
    items = bai_decode.intervals(in_records)
    order = sorted(range(len(items)), key=lambda i: bai_decode.sort_key(items[i]))
    s = b.sort()
    raw = s.bytes()
    text, stream, records, blocks = decode_bam(raw)
    assert text == spm.sam_header(RNAME, ref_len, sorted=True)
    assert [r[2] for r in records] == [in_records[i][2] for i in order]
    assert stream == b"".join(in_stream[in_records[i][0]:in_records[i][0] + in_records[i][1]] for i in order) == s.records()
    lines, st = s.lines(), s.stats()
    assert lines["offset"].tolist() == [o for o, _n, _l in records] and lines["len"].tolist() == [n for _o, n, _l in records]
    offsets = stored_offsets(len(stream), D, int(st.header_file_bytes))
    z = s.index()
    got = z.bytes()
    assert got == spm.bai_build_host(stream, lines, offsets, 0) == bai_decode.build_bai(records, offsets, D)
    bai = bai_decode.parse_bai(got)
    record_blocks = [x for x in blocks if x[0] >= st.header_file_bytes]
    for beg, end in bai_decode.queries(bai_decode.intervals(records), ref_len)[:40]:
        assert bai_decode.fetch(bai, record_blocks, beg, end) == bai_decode.scan(stream, beg, end), (beg, end)
    z.close()
    f = s.deflate()
    fraw = f.bytes()
    fblocks = bgzf_inflate.parse(fraw, D, sections=2)
    n_prefix = int(f.deflate_stats().n_prefix_bytes)
    frecord_blocks = [x for x in fblocks if x[0] >= n_prefix]
    assert bgzf_inflate.payload_of(frecord_blocks) == stream
    foffsets = f.block_offsets()
    zf = s.index(f)
    assert zf.bytes() == spm.bai_build_host(stream, lines, foffsets, 0) == bai_decode.build_bai(records, foffsets, D)
    for x in (zf, f, s):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 1: single-end, both strands, every shape of transcript the MD walk has a case for
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = (63, 64, 65, 130)
_single = {}


def _other(rng, *avoid):
    return int(rng.choice([x for x in range(4) if x not in {int(a) for a in avoid}]))


def _shaped_reads():
    """the tree, the reads, their k and {name: read index}"""
    if _single:
        return _single["t"], _single["reads"], _single["k"], _single["at"]
    seed, n_ref = 7301, 12_000
    ref0 = _make_tree(seed, n_ref, 4, 6, 8)["ref"]                   # (the reference does not depend on the alleles)
    rng = np.random.default_rng(7302)
    snp_begin, snp_end, p_del, p_ins, p_dx = 2000, 2600, 3400, 4300, 5200
    while ref0[p_dx - 1] == ref0[p_dx + 2]:                          # the deletion cannot move left: it stays in front of the SNP
        p_dx += 1
    ins_alt = rng.integers(0, 4, 100, dtype=np.uint8)
    snp = lambda p: [(int(ref0[p]) + 1) & 3]
    extra = [(snp_begin, 1, snp(snp_begin), (0,)), (snp_end, 1, snp(snp_end), (0,)), (p_del, 70, [], (1,)), (p_ins, 0, ins_alt, (2,)),
             (p_dx, 3, [], (3,)), (p_dx + 3, 1, snp(p_dx + 3), (3,))]
    t = _make_tree(seed, n_ref, 4, 6, 8, extra=extra)
    ref = t["ref"]
    assert np.array_equal(ref, ref0)
    reads, ks, at = [], [], {}

    def add(name, r, k=3):
        at[name] = len(reads)
        reads.append(np.ascontiguousarray(r, np.uint8))
        ks.append(k)

    first = lambda h, pos: (_hap(t, h)[0], int(np.searchsorted(_hap(t, h)[1].org, pos)))   # the first symbol at or behind pos
    hp, x = first(0, snp_begin)
    add("begins_in_x", hp[x:x + 64])                                # exact on haplotype 0, whose first symbol here is the SNP
    hp, x = first(0, snp_end)
    add("ends_in_x", hp[x - 62:x + 1])
    hp, x = first(1, p_del)
    add("deletion_70", hp[x - 60:x + 70])                           # 60 symbols, the 70 deleted positions, 70 symbols
    hp, x = first(2, p_ins)
    assert np.array_equal(hp[x:x + 100], ins_alt)
    add("inside_insertion", hp[x + 10:x + 74])
    hp, x = first(3, p_dx)
    add("d_then_x", hp[x - 30:x + 35])
    spots = iter(_free_stretches(t, 400, 8, first=6000))
    s = next(spots) + 40
    r = ref[s:s + 64].copy()
    r[30], r[31] = _other(rng, r[30]), _other(rng, r[31])
    add("mismatch_run", r)
    s = next(spots) + 40
    r = np.delete(ref[s:s + 66], 30)
    r[30] = _other(rng, ref[s + 30], ref[s + 31])
    add("d_then_x_edited", np_revcomp(r))
    s = next(spots) + 40
    add("insertion", np.insert(ref[s:s + 63], 20, _other(rng, ref[s + 20], ref[s + 19])))
    # 200 symbols, a substitution at every fifth position and one inserted symbol behind the fourth of them: 35 edits, 70 words,
    # and the X words stand at even indices behind the insertion, so that word 64 follows an open run
    s = next(spots) + 40
    r = ref[s:s + 199].copy()
    for j in range(34):
        r[4 + 5 * j] = _other(rng, r[4 + 5 * j])
    add("long_200", np.insert(r, 20, _other(rng, ref[s + 20], ref[s + 19], r[19])), k=36)
    for i in range(240):                                            # the bulk: from every haplotype, both strands, up to 2 substitutions
        hp = _hap(t, i % 4)[0]
        m = LENGTHS[(i // 4) % 4]
        o = int(rng.integers(0, len(hp) - m))
        r = hp[o:o + m].copy()
        for _ in range(int(rng.integers(0, 3))):
            j = int(rng.integers(0, m))
            r[j] = _other(rng, r[j])
        add(f"bulk{i}", np_revcomp(r) if i & 1 else r)
    for m in (63, 65):
        add(f"noise{m}", rng.integers(0, 4, m, dtype=np.uint8))
    _single.update(t=t, reads=reads, k=np.array(ks, np.uint16), at=at)
    return t, reads, _single["k"], at


def test_planted_reads_have_their_lengths():
    """CPU: a few hundred reads of lengths around the wave, and one of 200"""
    _t, reads, k, at = _shaped_reads()
    n = {m: sum(1 for r in reads if len(r) == m) for m in LENGTHS + (200,)}
    assert all(n[m] >= 60 for m in LENGTHS) and n[200] == 1 and len(reads) == len(k) >= 250
    assert len(reads[at["long_200"]]) == 200 and k[at["long_200"]] == 36


def _shapes(lines, recs):
    """which shapes of transcript the mapped lines hold, from their CIGAR (= and X) and MD"""
    seen = set()
    for f, rec in zip(lines, recs):
        if int(rec["kind"]) == UNMAPPED:
            continue
        items, md = _items(f[5]), f[12][5:]
        ops = [op for _n, op in items]
        seen |= {"mismatch_run"} if any(op == "X" and n >= 2 for n, op in items) else set()
        seen |= {"d_then_x"} if any(a == "D" and b == "X" for a, b in zip(ops, ops[1:])) else set()
        seen |= {"eq_i_eq"} if any(x == ("=", "I", "=") for x in zip(ops, ops[1:], ops[2:])) else set()
        seen |= {"begins_in_x"} if ops[0] == "X" else set()
        seen |= {"ends_in_x"} if ops[-1] == "X" else set()
        seen |= {"deletion_70"} if any(op == "D" and n >= 70 for n, op in items) and re.search(r"\^[A-Z]{70}", md) else set()
        seen |= {"inside_insertion"} if set(ops) == {"I"} and md == "0" else set()
        seen |= {"reverse"} if int(f[1]) & 16 else {"forward"}
        if len(items) > 64:
            c = 0
            for n, op in items[:64]:
                c = 0 if op in "XD" else c + (n if op == "=" else 0)
            seen |= {"open_count_crosses_a_pass"} if c > 0 else {"more_than_64_words"}
    return seen


WANTED = {"mismatch_run", "d_then_x", "eq_i_eq", "begins_in_x", "ends_in_x", "deletion_70", "inside_insertion", "reverse", "forward",
          "open_count_crosses_a_pass"}


@gpu
def test_single_end_stranded(spm, ctx):
    t, reads, k, at = _shaped_reads()
    ref = t["ref"]
    needles = stranded(reads)
    quals = np_qualities(reads, 7303)
    ref_text, jst, ps = _open(spm, ctx, t, reads, k)
    h = jst.search_device(ps, max_hits=1 << 21)
    lc = _chain(h, best=1, across=True, strands=True)
    rd = lc.reads(len(reads), 2)
    lines, recs = _check_ex(spm, ctx, lc, rd, ps, ref_text, ref, needles, quals, cigar_m=False)
    seen = _shapes(lines, recs)
    assert WANTED <= seen, sorted(WANTED - seen)
    for name in ("begins_in_x", "ends_in_x", "deletion_70", "inside_insertion", "d_then_x", "mismatch_run", "insertion", "long_200"):
        assert any(int(r["read"]) == at[name] and int(r["kind"]) == LOCUS for r in recs), name
    rev = [f for f, r in zip(lines, recs) if int(r["kind"]) == LOCUS and int(f[1]) & 16]
    assert rev and all(f[10] == "".join(chr(33 + int(v)) for v in quals[int(f[0])][::-1]) for f in rev)
    unm = [f for f, r in zip(lines, recs) if int(r["kind"]) == UNMAPPED]
    assert unm and all(f[10] == "".join(chr(33 + int(v)) for v in quals[int(f[0])]) and len(f) == 11 for f in unm)
    assert all(f[9] == "*" and f[10] == "*" for f, r in zip(lines, recs) if int(r["kind"]) == SECONDARY)
    _check_ex(spm, ctx, lc, rd, ps, ref_text, ref, needles, quals, cigar_m=True, names=_names(len(reads)))
    # qualities as one 2-D array: reads of one length
    same = [r for r in reads if len(r) == 64]
    ps2 = ctx.patterns(spm.ALGO_MYERS, same, k=3, both_strands=True)
    h2 = jst.search_device(ps2, max_hits=1 << 21)
    lc2 = _chain(h2, best=1, across=True, strands=True)
    rd2 = lc2.reads(len(same), 2)
    q2 = np.stack([q for q, r in zip(quals, reads) if len(r) == 64])
    a = lc2.sam_ex(rd2, ps2, RNAME, qualities=q2)
    b = lc2.sam_ex(rd2, ps2, RNAME, qualities=list(q2))
    assert a.text() == b.text() and a.text() != lc2.sam(rd2, ps2, RNAME).text()
    for x in (a, b, rd2, lc2, h2, ps2, rd, lc, h, ps, jst, ref_text):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 2 and 3: paired, without and with rescues
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_paired_without_rescues(spm, ctx):
    t, reads, _classes = _planted_pairs()
    needles = stranded(reads)
    quals = np_qualities(reads, 7304)
    lc, rd, rest = _planted_chain(spm, ctx)
    _h, ps, _jst, ref_text = rest
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    for cigar_m, names in ((False, None), (True, _names(len(reads) // 2))):
        lines, recs = _check_ex(spm, ctx, lc, rd, ps, ref_text, t["ref"], needles, quals, pr=pr, cigar_m=cigar_m, names=names)
    kinds = set(recs["kind"].tolist())
    assert {UNMAPPED, LOCUS, SECONDARY} <= kinds
    placed = [f for f, r in zip(lines, recs) if int(r["kind"]) == UNMAPPED and f[2] != "*"]
    assert placed and all(len(f) == 11 and f[10] != "*" for f in placed)   # an unmapped mate beside its mate: forward qualities, no MD
    for x in (pr, rd, lc) + rest:
        x.close()


@gpu
def test_paired_with_rescues(spm, ctx):
    t, reads, planted = _rescue_reads()
    needles = stranded(reads)
    quals = np_qualities(reads, 7305)
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    for cigar_m in (False, True):
        lines, recs = _check_ex(spm, ctx, lc, rd, ps, ref_text, t["ref"], needles, quals, pr=pr, rs=rs, cigar_m=cigar_m)
    resc = [(f, r) for f, r in zip(lines, recs) if int(r["kind"]) == RESCUE]
    assert len(resc) >= 12 and {int(f[1]) & 16 for f, _r in resc} == {0, 16}
    rescues, _ops = rs.view()
    for f, r in resc:                                               # a rescue's qualities turn with its flag 0x10
        q = quals[int(r["read"])]
        assert bool(int(f[1]) & 16) == bool(int(rescues["flag"][int(r["source"])]) & 16)
        assert f[10] == "".join(chr(33 + int(v)) for v in (q[::-1] if int(f[1]) & 16 else q)) and f[12].startswith("MD:Z:") and f[13] == "XR:i:1"
    # k = 40: the 150-symbol mate with its 35 scattered substitutions, a rescue transcript of more than 64 words
    rs40 = pr.rescue(lc, rd, ref_text, ps, 40, MIN_TLEN, MAX_TLEN)
    for cigar_m in (False, True):
        lines, recs = _check_ex(spm, ctx, lc, rd, ps, ref_text, t["ref"], needles, quals, pr=pr, rs=rs40, cigar_m=cigar_m, files=not cigar_m)
    p = planted["long"][0]
    (f,) = [f for f, r in zip(lines, recs) if int(r["kind"]) == RESCUE and int(r["read"]) == 2 * p + 1]
    assert len(re.findall(r"[A-Z]", f[12][5:])) >= 33 and len(f[9]) == len(f[10]) == 150
    for x in (rs40, rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU 4: what is refused, what is counted, zero reads
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_a_wrong_reference_and_zero_reads(spm, ctx):
    t, reads, k, at = _shaped_reads()
    ref = t["ref"]
    few = reads[:12]
    needles = stranded(few)
    ref_text, jst, ps = _open(spm, ctx, t, few, k[:12])
    h = jst.search_device(ps, max_hits=1 << 21)
    lc = _chain(h, best=1, across=True, strands=True)
    rd = lc.reads(len(few), 2)
    lib = spm.capi.lib()
    err = lambda: lib.spm_hip_last_error(ctx._h)
    quals = np.concatenate(np_qualities(few, 7306))
    n_qual = len(quals)
    good = lc.sam_ex(rd, ps, RNAME, qualities=np_qualities(few, 7306), md=True, reference=ref_text, secondary=True)
    good_text = good.text()

    def extras(qual=quals, n=n_qual, reference=ref_text, flags=1, reserved=0):
        e = spm.capi.SamExtras(qual=qual.ctypes.data if qual is not None else None, n_qual=n, reference=reference._h if reference else None,
                               flags=flags, reserved=reserved)
        e._keep = qual
        return e

    def call(e, bam=False):
        out = ctypes.c_void_p(1)
        if bam:
            o = spm.capi.BamOpts(sam=spm.sam_opts(RNAME, secondary=True), ref_len=len(ref), block_data=0, reserved=0)
            rc = lib.spm_hip_jst_ref_loci_bam_ex(lc._h, rd._h, None, None, ps._h, ctypes.byref(o), ctypes.byref(e) if e is not None else None,
                                                 ctypes.byref(out))
        else:
            o = spm.sam_opts(RNAME, secondary=True)
            rc = lib.spm_hip_jst_ref_loci_sam_ex(lc._h, rd._h, None, None, ps._h, ctypes.byref(o), ctypes.byref(e) if e is not None else None,
                                                 ctypes.byref(out))
        return rc, out

    def refused(word, e, bam=None):
        for is_bam in ((False, True) if bam is None else (bam,)):
            rc, out = call(e, is_bam)
            assert rc == INVALID and not out.value, (word, rc, out.value, err())
            assert word in err(), (word, err())

    for is_bam, destroy in ((False, lib.spm_hip_sam_destroy), (True, lib.spm_hip_bam_destroy)):
        rc, out = call(extras(), is_bam)                            # the arguments of every refusal below, unchanged: accepted
        assert rc == 0 and out.value, err()
        destroy(out)
    rc, out = call(spm.capi.SamExtras())                            # an all-zero extras: the bytes of the old call
    assert rc == 0
    zero = spm.Sam(ctx, out, RNAME)
    old = lc.sam(rd, ps, RNAME, secondary=True)
    assert zero.text() == old.text()
    zero.close()
    refused(b"flags", extras(flags=3))
    refused(b"flags", extras(flags=0x80000001))
    refused(b"reserved", extras(reserved=1))
    refused(b"reference", extras(reference=None))                   # SPM_SAM_MD without a reference
    refused(b"SPM_SAM_MD", extras(flags=0))                         # a reference without SPM_SAM_MD
    other = spm.Context(0)
    other_ref = other.upload(ref, sigma=4)
    refused(b"context", extras(reference=other_ref))
    other_ref.close()
    other.close()
    ref5 = ctx.upload(ref, sigma=5)
    refused(b"sigma", extras(reference=ref5))
    refused(b"n_qual", extras(n=0))                                 # qual without n_qual
    refused(b"qual", extras(qual=None))                             # n_qual without qual
    refused(b"n_qual", extras(n=n_qual - 1))
    longer = np.concatenate([quals, quals[:1]])
    refused(b"n_qual", extras(qual=longer, n=n_qual + 1))
    high = quals.copy()
    high[len(high) // 2] = 94
    refused(b"qual[", extras(qual=high))
    short = ctx.upload(ref[:-1], sigma=4)
    refused(b"ref_len", extras(reference=short), bam=True)          # the BAM call only: not ref_len symbols
    rc, out = call(extras(reference=short))                         # ... the text does not mind: every locus lies inside
    assert rc == 0
    lib.spm_hip_sam_destroy(out)
    # counted on the device: a locus outside the reference; an X column whose reference rank is the read's
    cut = ctx.upload(ref[:int(lc.view()["ref_end"].max()) - 1], sigma=4)
    refused(b"disagree", extras(reference=cut), bam=False)
    lines = [x.split(b"\t") for x in old.text().split(b"\n")[:-1]]
    recs = old.lines()
    i = next(i for i, f in enumerate(lines) if b"X" in f[5])
    src = lc.view()[int(recs[i]["source"])]
    q, r, at_x = 0, int(src["ref_begin"]), None
    for n, op in _items(lines[i][5].decode()):
        if op == "X":
            at_x = (q, r)
            break
        q, r = q + (n if op != "D" else 0), r + (n if op != "I" else 0)
    wrong = ref.copy()
    wrong[at_x[1]] = needles[int(src["pattern"])][at_x[0]]
    assert wrong[at_x[1]] != ref[at_x[1]]
    wrong_text = ctx.upload(wrong, sigma=4)
    refused(b"disagree", extras(reference=wrong_text))
    with pytest.raises(spm.SpmError, match="-1"):
        lc.bam_ex(rd, ps, RNAME, len(ref), md=True, reference=wrong_text)
    after = lc.sam_ex(rd, ps, RNAME, qualities=np_qualities(few, 7306), md=True, reference=ref_text, secondary=True)
    assert after.text() == good_text                                # and after all of this the call answers as before
    # zero reads
    rd0 = lc.reads(0, 2)
    ps0 = ctx.patterns(spm.ALGO_MYERS, [], k=1, both_strands=True)
    e = lc.sam_ex(rd0, ps0, RNAME, qualities=[], md=True, reference=ref_text)
    assert e.text() == b"" and len(e.lines()) == 0
    b = lc.bam_ex(rd0, ps0, RNAME, len(ref), qualities=np.zeros((0, 64), np.uint8), md=True, reference=ref_text)
    plain = lc.bam(rd0, ps0, RNAME, len(ref))
    assert b.bytes() == plain.bytes() and len(b) == 0
    for x in (plain, b, e, ps0, rd0, after, wrong_text, cut, short, ref5, old, good, rd, lc, h, ps, jst, ref_text):
        x.close()
