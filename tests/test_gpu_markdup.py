"""Duplicate reads and pairs marked on the device: spm_hip_bam_markdup, its raw form and the serial host builder against the
rule of spm_hip.h written again in tests/markdup_rule.py over the SAM text of the decoded records.  Single-end on a small
planted tree (groups of copies that cross a wave and a workgroup, both strands, every alignment of the qualities), paired on
the planted pairs of test_pairs.py with copies added, then the properties of the call and what it refuses."""
import ctypes
import struct

import numpy as np
import pytest

import bgzf_inflate
from cpp_programs import download
from markdup_rule import fields_of, py_markdup
from test_bai import stored_offsets
from test_bam_markdup import REF_LEN as HAND_REF_LEN, disagreements, make_stream, worked_cases
from test_gpu_bai import _Device
from test_gpu_sam import _names
from test_gpu_sam_qual_md import decode_bam
from test_jst_project import _make_tree
from test_pairs import MAX_TLEN, MIN_TLEN, _free_stretches, _planted_chain, _planted_pairs
from test_rescue import K, _chain_of
from test_sam import LINE
from test_strands import np_revcomp

gpu = pytest.mark.gpu
INVALID = -1
RNAME = "chr7"
GROUPS = (1, 2, 3, 64, 65, 300)                                     # copies of one read: runs that cross a wave and a workgroup
COUNTS = ("n_records", "n_pairs", "n_fragments", "n_dup_pairs", "n_dup_fragments", "n_dup_records", "n_fragments_beside_pairs")
_single = {}


def _single_reads():
    """the tree, the reads, {case: [read indices]} and per read its qualities"""
    if _single:
        return _single["t"], _single["reads"], _single["at"], _single["quals"]
    t = _make_tree(8101, 40_000, 4, 6, 8)
    rng = np.random.default_rng(8102)
    ref = t["ref"]
    spots = iter(_free_stretches(t, 300, 40, first=1000))
    reads, quals, at = [], [], {}

    def add(name, r, q=None):
        at.setdefault(name, []).append(len(reads))
        reads.append(np.ascontiguousarray(r, np.uint8))
        quals.append(np.full(len(r), 20, np.uint8) if q is None else np.asarray(q, np.uint8))

    lens = iter((30, 31, 32, 33, 63, 64, 65, 150, 97, 126))
    for g in GROUPS:                                                # with qualities the best of a group is its first, middle or last
        x, m = next(spots) + 40, next(lens)
        best = {1: 0, 2: 1, 3: 1, 64: 0, 65: 32, 300: 299}[g]
        for j in range(g):
            add(f"group{g}", ref[x:x + m], np.full(m, 40 if j == best else 20 + j % 3, np.uint8))
    x = next(spots) + 40                                            # forward reads of different length at one POS
    for m, q in ((40, 16), (30, 40), (35, 14)):
        add("forward_one_pos", ref[x:x + m], np.full(m, q, np.uint8))
    x = next(spots) + 40                                            # reverse reads of different length ending at one reference end
    for m in (40, 30, 57):
        add("reverse_one_end", np_revcomp(ref[x + 60 - m:x + 60]))
    x = next(spots) + 40                                            # a forward and a reverse read at the same POS
    add("strands", ref[x:x + 40])
    add("strands", np_revcomp(ref[x:x + 40]))
    a, b = next(spots) + 30, next(spots) + 30                       # two best loci: a primary and a secondary record per copy
    ref[b:b + 33] = ref[a:a + 33]
    for _ in range(3):
        add("two_best", ref[a:a + 33])
    for _ in range(2):
        add("unmapped", rng.integers(0, 4, 33, dtype=np.uint8))
    for m in range(30, 151, 7):                                     # lengths that move qual through every alignment, twice each:
        x = next(spots) + 17                                        # values at both ends of the range, some beyond it
        for j in range(2):
            q = rng.integers(0, 94, m, dtype=np.uint8)
            q[0], q[-1] = 0, 93
            add(f"m{m}", ref[x:x + m], q)
    _single.update(t=t, reads=reads, at=at, quals=quals)
    return t, reads, at, quals


def _qual_spans(stream, lines):
    """[(first, behind)] of every record's quality bytes in the stream, by the record's own fields"""
    out = []
    for o in lines["offset"].tolist():
        l_name, n_cigar, l_seq = stream[o + 12], struct.unpack_from("<H", stream, o + 16)[0], struct.unpack_from("<I", stream, o + 20)[0]
        q0 = o + 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2
        out.append((q0, q0 + l_seq))
    return out


def _raw_marks(ctx, stream, lines, ref_len, min_qual=0, shift=0, preset=0):
    """Context.bam_markdup over an uploaded stream that starts `shift` bytes behind a 4-byte border -> (dup, the stats)"""
    dev = [_Device(b"\x5d" * shift + stream), _Device(np.ascontiguousarray(lines, LINE).tobytes()), _Device(bytes([preset]) * max(len(lines), 1))]
    try:
        st = ctx.bam_markdup(dev[0].ptr.value + shift, len(stream), dev[1].ptr.value, len(lines), ref_len, dev[2].ptr.value, min_qual)
        return download(ctx, dev[2].ptr.value, len(lines), np.uint8), st
    finally:
        ctx.synchronize()
        for d in dev:
            d.close()


def _check_marked(spm, ctx, b, ref_len, min_qual=0):
    """b.markdup() against the rule over the decoded records of b -> (the marked Bam, dup by line, the rule's counts)"""
    raw_in = b.bytes()
    in_text, in_stream, in_records, _blocks = decode_bam(raw_in)
    in_lines = b.lines()
    want, counts = py_markdup([r[2] for r in in_records], in_lines["read"], min_qual)
    want = np.array(want, np.uint8)
    m = b.markdup(min_qual)
    raw = m.bytes()
    text, stream, records, blocks = decode_bam(raw)                 # the file parses block by block, CRCs and all
    assert text == in_text and raw[:int(m.stats().header_file_bytes)] == raw_in[:int(b.stats().header_file_bytes)]
    lines = m.lines()
    # ---- the three routes equal the rule ----
    got = (lines["flag"] >> 10) & 1
    assert got.tolist() == want.tolist(), [(i, int(g), int(w), in_records[i][2][:60]) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    host = spm.bam_markdup_host(in_stream, in_lines, ref_len, min_qual)
    assert host.tolist() == want.tolist()
    d_file, n_file, d_rec, n_rec, d_lines, n_lines = b.device()
    dup = _Device(bytes([7]) * max(n_lines, 1))
    st_raw = ctx.bam_markdup(d_rec, n_rec, d_lines, n_lines, ref_len, dup.ptr.value, min_qual)
    assert download(ctx, dup.ptr.value, n_lines, np.uint8).tolist() == want.tolist()
    dup.close()
    # ---- the stream differs in bit 2 of byte offset + 19 alone, the lines in flag alone, the records in FLAG alone ----
    assert len(stream) == len(in_stream) == len(m.records()) and m.records() == stream
    diff = np.flatnonzero(np.frombuffer(stream, np.uint8) != np.frombuffer(in_stream, np.uint8))
    at_flag = {int(o) + 19: i for i, o in enumerate(in_lines["offset"])}
    assert all(int(d) in at_flag and (stream[d] ^ in_stream[d]) == 4 for d in diff)
    assert [(stream[o + 19] >> 2) & 1 for o in in_lines["offset"].tolist()] == want.tolist()
    for f in ("offset", "len", "read", "source", "mapq", "kind"):
        assert np.array_equal(lines[f], in_lines[f]), f
    assert np.array_equal(lines["flag"] & ~np.uint16(0x400), in_lines["flag"] & ~np.uint16(0x400))
    for (o, n, line), (oi, ni, li), w in zip(records, in_records, want):
        f, fi = line.split(b"\t"), li.split(b"\t")
        assert (o, n) == (oi, ni) and f[:1] + f[2:] == fi[:1] + fi[2:] and int(f[1]) == (int(fi[1]) & ~0x400) | (0x400 if w else 0)
        assert not (w and int(f[1]) & 0x904)                        # secondary and unmapped records stay clear
    # ---- the counts ----
    st, bst, mst = m.markdup_stats(), b.stats(), m.stats()
    assert {c: int(getattr(st, c)) for c in COUNTS} == counts == {c: int(getattr(st_raw, c)) for c in COUNTS}
    assert st.n_dup_records == int(want.sum()) == 2 * st.n_dup_pairs + st.n_dup_fragments
    assert st.ms_host > 0 and st.ms_total >= 0 and st_raw.ms_write == 0 and st_raw.ms_frame == 0
    for c in ("n_records", "n_record_bytes", "n_file_bytes", "header_file_bytes", "n_record_blocks", "n_reported", "n_secondary", "n_unmapped",
              "n_rescue_lines"):
        assert getattr(mst, c) == getattr(bst, c), c
    assert len(raw) == len(raw_in) == mst.n_file_bytes
    with pytest.raises(spm.SpmError):
        b.markdup_stats()                                           # no markdup made this handle
    # ---- host and device views are equal; two calls; marking a marked handle ----
    d_file, n_file, d_rec, n_rec, d_lines, n_lines = m.device()
    assert (n_file, n_rec, n_lines) == (len(raw), len(stream), len(lines))
    assert download(ctx, d_file, n_file, np.uint8).tobytes() == raw and download(ctx, d_rec, n_rec, np.uint8).tobytes() == stream
    assert download(ctx, d_lines, n_lines, LINE).tobytes() == lines.tobytes()
    for again in (b.markdup(min_qual), m.markdup(min_qual)):
        assert again.bytes() == raw and again.records() == stream and again.lines().tobytes() == lines.tobytes()
        again.close()
    return m, want, counts


def _check_sorted_marked(spm, b, m, ref_len):
    """sort-then-mark and mark-then-sort are one file; its index is the host builder's; its deflated blocks inflate to the stream"""
    s = b.sort()
    sm, ms = s.markdup(), m.sort()
    raw, stream, lines = sm.bytes(), sm.records(), sm.lines()
    assert ms.bytes() == raw and ms.records() == stream and ms.lines().tobytes() == lines.tobytes()
    assert raw.startswith(spm.bam_header(RNAME, ref_len, sorted=True)) and sm.sort_stats().n_records == len(lines) == sm.markdup_stats().n_records
    assert int(((lines["flag"] >> 10) & 1).sum()) == int(((m.lines()["flag"] >> 10) & 1).sum())
    z = sm.index()
    offsets = stored_offsets(len(stream), 65280, int(sm.stats().header_file_bytes))
    assert z.bytes() == spm.bai_build_host(stream, lines, offsets, 0)
    f = sm.deflate()
    blocks = bgzf_inflate.parse(f.bytes(), 65280, sections=2)
    assert bgzf_inflate.payload_of([x for x in blocks if x[0] >= int(f.deflate_stats().n_prefix_bytes)]) == stream
    for x in (f, z, ms, sm, s):
        x.close()


@gpu
def test_single_end_groups_strands_and_alignments(spm, ctx):
    t, reads, at, quals = _single_reads()
    ref_len = len(t["ref"])
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    names = _names(len(reads))
    for with_q, with_names in ((False, False), (True, True)):
        b = lc.bam_ex(rd, ps, RNAME, ref_len, qualities=quals if with_q else None, names=names if with_names else None, secondary=True)
        m, dup, counts = _check_marked(spm, ctx, b, ref_len)
        lines = m.lines()
        stream = m.records()
        primary = {int(r): i for i, (r, f) in enumerate(zip(lines["read"], lines["flag"])) if not f & 0x900}
        marks = lambda name: [int(dup[primary[r]]) for r in at[name]]
        for g in GROUPS:                                            # one of every group stays: the best, or without qualities the first
            best = {1: 0, 2: 1, 3: 1, 64: 0, 65: 32, 300: 299}[g] if with_q else 0
            assert marks(f"group{g}") == [int(j != best) for j in range(g)], g
        assert marks("forward_one_pos") == ([1, 0, 1] if with_q else [0, 1, 1])      # 40 x 16 against 30 x 40 against nothing
        assert marks("reverse_one_end") == ([1, 1, 0] if with_q else [0, 1, 1])      # equal qualities: the longest read scores most
        pos = [fields_of(decode_bam(b.bytes())[2][primary[r]][2])[1] for r in at["reverse_one_end"]]
        assert len(set(pos)) == 3                                   # ... although POS differs
        assert marks("strands") == [0, 0] and marks("two_best") == [0, 1, 1] and marks("unmapped") == [0, 0]
        kinds = lines["flag"]
        assert int(((kinds & 0x100) != 0).sum()) >= 3 and int(((kinds & 0x4) != 0).sum()) == 2 and not (kinds[(kinds & 0x104) != 0] & 0x400).any()
        assert counts["n_pairs"] == 0 and counts["n_fragments"] == len(reads) - 2 and counts["n_dup_records"] == counts["n_dup_fragments"]
        spans = _qual_spans(stream, lines)
        assert {q0 % 4 for q0, _q1 in spans} == {0, 1, 2, 3} == {q1 % 4 for _q0, q1 in spans}
        if with_q:                                                  # min_qual decides: 14 counts from 14 on, and nothing counts at 93 but 93
            for min_qual in (14, 93, 1):
                m2, dup2, _c = _check_marked(spm, ctx, b, ref_len, min_qual)
                if min_qual == 14:
                    assert [int(dup2[primary[r]]) for r in at["forward_one_pos"]] == [1, 0, 1]
                m2.close()
            _check_sorted_marked(spm, b, m, ref_len)
        m.close()
        b.close()
    for x in (rd, lc, ps, ref_text) + rest:
        x.close()


_paired = {}


def _paired_reads():
    """the planted pairs of test_pairs.py with copies added -> (the tree, the reads, {case: [pairs]}, the qualities)"""
    if _paired:
        return _paired["t"], _paired["reads"], _paired["at"], _paired["quals"]
    t, planted, classes = _planted_pairs()
    ref = t["ref"]
    rng = np.random.default_rng(8201)
    reads, at = [r.copy() for r in planted], {}
    spots = _free_stretches(t, 240, 30)[26:]                        # behind the stretches the planted pairs took
    noise = lambda: rng.integers(0, 4, 34, dtype=np.uint8)

    def pair(name, mate1, mate2):
        at.setdefault(name, []).append(len(reads) // 2)
        reads.extend([np.ascontiguousarray(mate1, np.uint8), np.ascontiguousarray(mate2, np.uint8)])

    x = spots[0] + 20
    for _ in range(3):                                              # duplicate pairs
        pair("copies", ref[x:x + 33], np_revcomp(ref[x + 107:x + 140]))
    pair("mates_swapped", np_revcomp(ref[x + 107:x + 140]), ref[x:x + 33])       # the same two ends: which mate is lower is no part of the key
    pair("one_end_shared", ref[x:x + 31], np_revcomp(ref[x + 117:x + 150]))     # the same lower end, another upper end
    pair("fragment_on_a_pair_end", ref[x:x + 36], noise())          # its mate is unmapped: a fragment where a pair end sits
    y = spots[1] + 20
    pair("fragments_alone", ref[y:y + 33], noise())
    pair("fragments_alone", noise(), ref[y:y + 30])
    for cls in ("rescued", "same_strand", "outside"):               # a rescued pair and two discordant ones, once more
        p = classes[cls][0][0]
        at[cls] = [p]
        pair(cls, planted[2 * p], planted[2 * p + 1])
    quals = [np.full(len(r), 25, np.uint8) for r in reads]
    quals[2 * at["copies"][1]] = np.full(33, 30, np.uint8)         # with qualities the second copy is the best pair
    quals[2 * at["fragments_alone"][1] + 1] = np.full(30, 60, np.uint8)
    _paired.update(t=t, reads=reads, at=at, quals=quals)
    return t, reads, at, quals


@gpu
def test_paired_with_copies_and_rescues(spm, ctx):
    t, reads, at, quals = _paired_reads()
    ref_len = len(t["ref"])
    lc, rd, rest = _planted_chain(spm, ctx, reads)
    ps, ref_text = rest[1], rest[3]
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    for with_q, with_rescues in ((False, True), (True, True), (True, False)):
        b = lc.bam_ex(rd, ps, RNAME, ref_len, qualities=quals if with_q else None, pairs=pr, rescues=rs if with_rescues else None,
                      names=_names(len(reads) // 2), secondary=True)
        m, dup, counts = _check_marked(spm, ctx, b, ref_len)
        lines = m.lines()
        primary = {int(r): i for i, (r, f) in enumerate(zip(lines["read"], lines["flag"])) if not f & 0x900}
        marks = lambda name: [(int(dup[primary[2 * p]]), int(dup[primary[2 * p + 1]])) for p in at[name]]
        assert marks("copies") == ([(1, 1), (0, 0), (1, 1)] if with_q else [(0, 0), (1, 1), (1, 1)])
        assert marks("mates_swapped") == [(1, 1)] and marks("one_end_shared") == [(0, 0)]
        assert marks("fragment_on_a_pair_end") == [(1, 0)]
        assert marks("fragments_alone") == ([(1, 0), (0, 0)] if with_q else [(0, 0), (0, 1)])
        assert marks("same_strand") == [(0, 0), (1, 1)] and marks("outside") == [(0, 0), (1, 1)]
        if with_rescues:                                            # both mates of a rescued pair are placed: a pair, and its copy a duplicate
            assert marks("rescued") == [(0, 0), (1, 1)] and int(m.stats().n_rescue_lines) == int((lines["kind"] == 2).sum())
        assert counts["n_dup_pairs"] >= 5 and counts["n_fragments_beside_pairs"] >= 1 and counts["n_dup_fragments"] >= 2
        if with_q and with_rescues:
            _check_sorted_marked(spm, b, m, ref_len)
        m.close()
        b.close()
    for x in (rs, pr, rd, lc) + rest:
        x.close()


@gpu
def test_raw_form_presets_zero_reads_and_refusals(spm, ctx):
    lib = spm.capi.lib()
    # ---- the raw form over uploaded hand-built streams: the worked cases at every alignment of the buffer; a pre-set 0x400 and
    # whatever the dup buffer held are recomputed ----
    for quals in (False, True):
        recs = [dict(r, flag=r["flag"] | (0x400 if i % 3 == 0 else 0)) for i, r in enumerate(worked_cases(quals))]
        stream, lines = make_stream(recs)
        want = spm.bam_markdup_host(stream, lines, HAND_REF_LEN)
        assert want.tolist() == ([1, 0] if quals else [0, 1]) + [0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0]
        for shift in range(4):
            got, st = _raw_marks(ctx, stream, lines, HAND_REF_LEN, shift=shift, preset=1)
            assert got.tolist() == want.tolist(), (quals, shift)
            assert (st.n_records, st.n_pairs, st.n_fragments, st.n_dup_pairs, st.n_dup_fragments, st.n_dup_records, st.n_fragments_beside_pairs) == (
                14, 3, 6, 1, 3, 5, 1)
    # ---- the counted disagreements: SPM_E_INVALID, nothing written, and the context stays usable ----
    good_stream, good_lines = make_stream(worked_cases())
    for name, (stream, lines, ref_len) in sorted(disagreements().items()):
        dev = [_Device(stream), _Device(lines.tobytes()), _Device(bytes([7]) * len(lines))]
        rc = lib.spm_hip_bam_markdup_records(ctx._h, dev[0].ptr, len(stream), dev[1].ptr, len(lines), ref_len, None, dev[2].ptr, None)
        assert rc == INVALID and b"disagree" in lib.spm_hip_last_error(ctx._h), name
        assert download(ctx, dev[2].ptr.value, len(lines), np.uint8).tolist() == [7] * len(lines), name
        for d in dev:
            d.close()
        assert _raw_marks(ctx, good_stream, good_lines, HAND_REF_LEN)[0].sum() == 5, name
    # ---- refused on the host ----
    dev = [_Device(good_stream), _Device(good_lines.tobytes()), _Device(bytes(len(good_lines)))]
    Opts, n, nb = spm.capi.BamMarkdupOpts, len(good_lines), len(good_stream)
    raw = lambda c=ctx._h, s=dev[0].ptr, sb=nb, l=dev[1].ptr, ln=n, ref=HAND_REF_LEN, o=None, d=dev[2].ptr: lib.spm_hip_bam_markdup_records(
        c, s, sb, l, ln, ref, ctypes.byref(o) if o is not None else None, d, None)
    assert raw() == 0
    for rc, kw in ((INVALID, dict(c=None)), (INVALID, dict(s=None)), (INVALID, dict(l=None)), (INVALID, dict(d=None)), (INVALID, dict(sb=0)),
                   (INVALID, dict(ln=0)), (INVALID, dict(o=Opts(0, 2, 0))), (INVALID, dict(o=Opts(0, 0, 3))), (INVALID, dict(o=Opts(94, 0, 0))),
                   (-4, dict(ref=1 << 30)), (-4, dict(ln=1 << 32))):
        assert raw(**kw) == rc, kw
    assert raw(s=None, sb=0, l=None, ln=0, d=None) == 0             # nothing to mark
    for d in dev:
        d.close()
    # ---- zero reads: the header section and the EOF block; the handle's refusals; the result outlives its source ----
    t, reads, _at, _q = _single_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads[:3])
    rd0 = lc.reads(0, 2)
    ps0 = ctx.patterns(spm.ALGO_MYERS, [], k=1, both_strands=True)
    e = lc.bam(rd0, ps0, RNAME, 12_000)
    m = e.markdup()
    assert m.bytes() == e.bytes() == spm.bam_header(RNAME, 12_000) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert m.records() == b"" and len(m.lines()) == 0 and m.markdup_stats().n_records == 0 and m.device()[3] == 0
    b = lc.bam(rd, ps, RNAME, len(t["ref"]))
    out = ctypes.c_void_p(1)
    assert lib.spm_hip_bam_markdup(b._h, ctypes.byref(Opts(0, 0, 1)), ctypes.byref(out)) == INVALID and not out.value
    assert b"reserved" in lib.spm_hip_last_error(ctx._h)
    assert lib.spm_hip_bam_markdup(b._h, ctypes.byref(Opts(0, 1, 0)), ctypes.byref(out)) == INVALID and not out.value
    assert lib.spm_hip_bam_markdup(b._h, ctypes.byref(Opts(94, 0, 0)), ctypes.byref(out)) == INVALID and not out.value
    assert lib.spm_hip_bam_markdup(None, None, ctypes.byref(out)) == INVALID and lib.spm_hip_bam_markdup(b._h, None, None) == INVALID
    assert lib.spm_hip_bam_markdup(b._h, None, ctypes.byref(out)) == 0 and out.value   # NULL opts: the defaults
    st = spm.capi.BamMarkdupStats()
    assert lib.spm_hip_bam_markdup_stats(out, ctypes.byref(st)) == 0 and st.n_records == 3 and st.n_fragments == 3
    assert lib.spm_hip_bam_markdup_stats(b._h, ctypes.byref(st)) == INVALID and lib.spm_hip_bam_markdup_stats(out, None) == INVALID
    lib.spm_hip_bam_destroy(out)
    keep = b.markdup()
    raw_file = keep.bytes()
    for x in (b, m, e, ps0, rd0, rd, lc, ps, ref_text) + rest:
        x.close()
    d_file, n_file = keep.device()[:2]
    assert download(ctx, d_file, n_file, np.uint8).tobytes() == raw_file
    keep.close()
