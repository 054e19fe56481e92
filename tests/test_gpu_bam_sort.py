"""A BAM handle in coordinate order on the device: spm_hip_bam_sort against Python's stable sorted() over the records that
tests/bam_decode.py decodes from the unsorted file, under the rule of spm_hip.h written again in tests/bai_decode.py (sort_key).
The inputs are planted on a reference of 1.1 M symbols -- the smallest with a 2^20 border -- and on the paired inputs of
test_gpu_bam.py."""
import ctypes
import struct

import numpy as np
import pytest

import bai_decode
from bam_decode import at_voffset, bam_to_sam
from cpp_programs import download
from test_gpu_sam import _names, _rescue_reads
from test_jst_project import _make_tree
from test_pairs import MAX_TLEN, MIN_TLEN, _free_stretches, _planted_chain, _planted_pairs
from test_rescue import K, _chain_of
from test_sam import LINE
from test_strands import np_revcomp

gpu = pytest.mark.gpu
INVALID = -1
BORDERS = (1 << 14, 1 << 17, 1 << 20)
BLOCK_SIZES = (1, 7, 255, 256, 257, 1000, 0)
FLAGS = [(nm, m, sec) for nm in (False, True) for m in (False, True) for sec in (False, True)]
RNAME = "chr7"
_border = {}


def _border_reads():
    """the tree, the reads and {case: read index}: a few dozen reads of 30 .. 150 symbols"""
    if _border:
        return _border["t"], _border["reads"], _border["at"]
    t = _make_tree(7301, 1_100_000, 4, 6, 8)
    rng = np.random.default_rng(7302)
    ref = t["ref"]
    apos = t["alleles"]["pos"].astype(np.int64)
    for B in BORDERS:
        assert np.all((apos < B - 400) | (apos > B + 400)), B
    spots = iter(_free_stretches(t, 400, 24, first=30_000))
    a, b = next(spots) + 30, next(spots) + 30
    ref[b:b + 33] = ref[a:a + 33]                                   # two best loci
    reads, at = [], {}

    def add(name, r):
        at[name] = len(reads)
        reads.append(np.ascontiguousarray(r, np.uint8))

    x = next(spots) + 40                                            # read order is not coordinate order: the borders come last
    add("forward", ref[x:x + 40])
    add("reverse_same_pos", np_revcomp(ref[x:x + 40]))
    add("unmapped", rng.integers(0, 4, 33, dtype=np.uint8))
    for B in reversed(BORDERS):
        add(f"before{B}", ref[B - 150:B - 150 + 31 + B % 5])
        add(f"ends_at{B}", ref[B - 47:B])
        add(f"across{B}", ref[B - 60:B + 90])
        add(f"starts_at{B}", ref[B:B + 64])
        add(f"behind{B}", ref[B + 1:B + 36])
    y = next(spots) + 40
    add("twin1", ref[y:y + 35])
    add("twin2", ref[y:y + 35])
    add("two_best", ref[a:a + 33])
    add("reverse", np_revcomp(ref[next(spots) + 40:][:57]))
    for m in (30, 63, 64, 65, 97, 101, 126, 150, 33, 38, 77, 149):  # lengths that move the records through every alignment
        add(f"m{m}_{len(reads)}", ref[next(spots) + 17:][:m])
    _border.update(t=t, reads=reads, at=at)
    return t, reads, at


def _decoded(raw, D):
    text, stream, records, blocks = bam_to_sam(raw, D or 65280)
    return text, stream, records, blocks


def _check_sorted(ctx, spm, b, ref_len, D, seen=None):
    """b.sort() against Python's sorted() over the decoded records of b -> (the sorted Bam, its record stream, its records)"""
    Dv = D or 65280
    _t, in_stream, in_records, _b = _decoded(b.bytes(), D)
    in_lines = b.lines()
    items = bai_decode.intervals(in_records)
    order = sorted(range(len(items)), key=lambda i: bai_decode.sort_key(items[i]))   # (stable)
    s = b.sort()
    raw = s.bytes()
    text, stream, records, blocks = _decoded(raw, D)               # the file parses: every block, every record
    header = spm.sam_header(RNAME, ref_len, sorted=True)
    assert header.startswith(b"@HD\tVN:1.6\tSO:coordinate\n") and text[:len(header)] == header
    assert raw.startswith(spm.bam_header(RNAME, ref_len, D, sorted=True))
    assert [r[2] for r in records] == [in_records[i][2] for i in order]
    assert stream == b"".join(in_stream[in_records[i][0]:in_records[i][0] + in_records[i][1]] for i in order)
    assert s.records() == stream and len(s) == len(records) == len(b)
    got = s.lines()
    assert got.dtype == LINE
    assert got["offset"].tolist() == [o for o, _n, _l in records] and got["len"].tolist() == [n for _o, n, _l in records]
    assert int(got["len"].sum()) == len(stream) and (len(got) == 0 or got["offset"][0] == 0)
    for f in ("len", "read", "source", "flag", "mapq", "kind"):
        assert np.array_equal(got[f], in_lines[f][order]), f
    if seen is not None:                                            # the (source, destination) alignments the gather met
        seen |= set(zip((in_lines["offset"][order] % 4).tolist(), (got["offset"] % 4).tolist()))
    st, sst, bst = s.stats(), s.sort_stats(), b.stats()
    voff = s.voffsets()
    for i in range(len(got)):
        (block_size,) = struct.unpack("<i", at_voffset(blocks, int(voff[i]), 4))
        assert block_size == int(got["len"][i]) - 4, i
    n_blocks = (len(stream) + Dv - 1) // Dv
    assert (st.n_records, st.n_record_bytes, st.n_file_bytes, st.n_record_blocks) == (len(records), len(stream), len(raw), n_blocks)
    assert st.n_file_bytes == st.header_file_bytes + len(stream) + 31 * n_blocks + 28
    assert st.header_file_bytes == len(spm.bam_header(RNAME, ref_len, D, sorted=True))
    for c in ("n_reported", "n_secondary", "n_unmapped", "n_rescue_lines"):
        assert getattr(st, c) == getattr(bst, c), c
    assert (sst.n_records, sst.n_record_bytes) == (len(records), len(stream)) and sst.ms_host > 0 and sst.ms_total >= 0
    assert sst.key_bits == int(ref_len).bit_length() + 2
    # the views on the device; two calls; sorting a sorted handle
    d_file, n_file, d_rec, n_rec, d_lines, n_lines = s.device()
    assert (n_file, n_rec, n_lines) == (len(raw), len(stream), len(got))
    assert download(ctx, d_file, n_file, np.uint8).tobytes() == raw and download(ctx, d_rec, n_rec, np.uint8).tobytes() == stream
    assert download(ctx, d_lines, n_lines, LINE).tobytes() == got.tobytes()
    for again in (b.sort(), s.sort()):
        assert again.bytes() == raw and again.records() == stream and again.lines().tobytes() == got.tobytes()
        again.close()
    return s, stream, records


@gpu
def test_borders_ties_and_every_alignment(spm, ctx):
    t, reads, at = _border_reads()
    ref_len = len(t["ref"])
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    names = _names(len(reads))
    seen = set()
    kw = lambda nm, m, sec: dict(names=names if nm else None, cigar_m=m, secondary=sec)
    # ---- the cases are there, by the decoded records of the unsorted file ----
    b = lc.bam(rd, ps, RNAME, ref_len, **kw(False, False, True))
    _t, _s, in_records, _b = _decoded(b.bytes(), 0)
    items = bai_decode.intervals(in_records)
    primary = {}                                                    # read -> its first record (names are the read's index)
    for it, (_o, _n, line) in zip(items, in_records):
        primary.setdefault(int(line.split(b"\t")[0]), it)
    iv = lambda name: primary[at[name]][3:5]
    for B in BORDERS:
        assert iv(f"before{B}")[1] < B and iv(f"ends_at{B}")[1] == B and iv(f"starts_at{B}")[0] == B and iv(f"behind{B}")[0] == B + 1
        assert iv(f"across{B}")[0] < B < iv(f"across{B}")[1]
    f, r = primary[at["forward"]], primary[at["reverse_same_pos"]]
    assert f[3] == r[3] and not f[5] & 16 and r[5] & 16
    assert primary[at["twin1"]][2:5] == primary[at["twin2"]][2:5] and primary[at["twin1"]][5] == primary[at["twin2"]][5]
    assert primary[at["reverse"]][5] & 16 and not primary[at["unmapped"]][2] and primary[at["unmapped"]][5] & 4
    assert sum(1 for _o, _n, line in in_records if int(line.split(b"\t")[0]) == at["two_best"]) == 2
    assert sorted(range(len(items)), key=lambda i: bai_decode.sort_key(items[i])) != list(range(len(items)))
    b.close()
    # ---- every option set at the default block size ----
    for nm, m, sec in FLAGS:
        b = lc.bam(rd, ps, RNAME, ref_len, **kw(nm, m, sec))
        s, _stream, records = _check_sorted(ctx, spm, b, ref_len, 0, seen)
        assert len(records) >= len(reads)
        s.close()
        b.close()
    assert seen == {(x, y) for x in range(4) for y in range(4)}, sorted(seen)
    # ---- every block size: the record stream is the same ----
    for opt in (kw(True, True, True), kw(False, False, False)):
        first = None
        for D in BLOCK_SIZES:
            b = lc.bam(rd, ps, RNAME, ref_len, block_data=D, **opt)
            s, stream, _r = _check_sorted(ctx, spm, b, ref_len, D)
            first = stream if first is None else first
            assert stream == first, D
            s.close()
            b.close()
    for x in (rd, lc, ps, ref_text) + rest:
        x.close()


def _mates_stand_together(records):
    """a placed unmapped mate stands directly beside its mate: same name, same position"""
    lines = [l[:-1].split(b"\t") for _o, _n, l in records]
    n = 0
    for i, f in enumerate(lines):
        if int(f[1]) & 4 and f[2] != b"*":
            beside = [lines[j] for j in (i - 1, i + 1) if 0 <= j < len(lines)]
            assert any(g[0] == f[0] and g[3] == f[3] and not int(g[1]) & 4 for g in beside), (i, f[:4])
            n += 1
    return n


@gpu
def test_paired_inputs_with_pairs_and_with_rescues(spm, ctx):
    _t, reads, _classes = _planted_pairs()
    lc, rd, rest = _planted_chain(spm, ctx)
    ps = rest[1]
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    b = lc.bam(rd, ps, RNAME, 12_000, pairs=pr, names=_names(len(reads) // 2), secondary=True)
    s, _stream, records = _check_sorted(ctx, spm, b, 12_000, 0)
    assert _mates_stand_together(records) >= 1
    for x in (s, b, pr, rd, lc) + rest:
        x.close()
    t, reads, _planted = _rescue_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    for D in (0, 257):
        b = lc.bam(rd, ps, RNAME, 12_000, pairs=pr, rescues=rs, cigar_m=True, secondary=True, block_data=D)
        s, _stream, records = _check_sorted(ctx, spm, b, 12_000, D)
        assert _mates_stand_together(records) >= 1
        assert records[-1][2].split(b"\t")[2] == b"*"               # the pair without a position goes to the end
        s.close()
        b.close()
    for x in (rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_zero_reads_and_refusals(spm, ctx):
    t, reads, _at = _border_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads[:3])
    lib = spm.capi.lib()
    rd0 = lc.reads(0, 2)
    ps0 = ctx.patterns(spm.ALGO_MYERS, [], k=1, both_strands=True)
    e = lc.bam(rd0, ps0, RNAME, 12_000)
    s = e.sort()                                                    # zero records: the header section and the EOF block
    text, stream, records, _blocks = bam_to_sam(s.bytes())
    assert text == spm.sam_header(RNAME, 12_000, sorted=True) and stream == b"" and records == [] and len(s.lines()) == 0
    assert s.bytes() == spm.bam_header(RNAME, 12_000, sorted=True) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert s.stats().n_records == 0 and s.device()[3] == 0 and s.sort_stats().n_records == 0
    b = lc.bam(rd, ps, RNAME, len(t["ref"]))
    out = ctypes.c_void_p(1)
    assert lib.spm_hip_bam_sort(b._h, ctypes.byref(spm.capi.BamSortOpts(reserved=1)), ctypes.byref(out)) == INVALID and not out.value
    assert b"reserved" in lib.spm_hip_last_error(ctx._h)
    assert lib.spm_hip_bam_sort(None, None, ctypes.byref(out)) == INVALID and lib.spm_hip_bam_sort(b._h, None, None) == INVALID
    assert lib.spm_hip_bam_sort(b._h, None, ctypes.byref(out)) == 0 and out.value      # NULL opts: the defaults
    st = spm.capi.BamSortStats()
    assert lib.spm_hip_bam_sort_stats(out, ctypes.byref(st)) == 0 and st.n_records == 3
    assert lib.spm_hip_bam_sort_stats(b._h, ctypes.byref(st)) == INVALID                # no sort made this handle
    lib.spm_hip_bam_destroy(out)
    keep = b.sort()                                                 # the result outlives its source and every input
    raw = keep.bytes()
    for x in (b, s, e, ps0, rd0, rd, lc, ps, ref_text) + rest:
        x.close()
    d_file, n_file = keep.device()[:2]
    assert download(ctx, d_file, n_file, np.uint8).tobytes() == raw
    keep.close()
