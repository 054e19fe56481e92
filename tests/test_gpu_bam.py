"""BAM records in BGZF blocks on the device: spm_hip_jst_ref_loci_bam against spm_hip_jst_ref_loci_sam of the same inputs and
options.  The file is taken apart by tests/bam_decode.py -- a strict BGZF parser and a BAM-to-SAM renderer written from the
specification, sharing nothing with the C++ -- and the rendered text of EVERY record has to equal the SAM call's text (which
test_gpu_sam.py holds against its rule) byte for byte.  The inputs are the planted inputs of test_gpu_sam.py."""
import ctypes
import struct

import numpy as np
import pytest

from bam_decode import at_voffset, bam_to_sam
from cpp_programs import download
from test_gpu_sam import _names, _rescue_reads, _single_end_reads
from test_pairs import MAX_TLEN, MIN_TLEN, _chain, _planted_chain, _planted_pairs
from test_rescue import K, RESCUED, _chain_of
from test_sam import LINE

gpu = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
COUNTS = ("n_reported", "n_secondary", "n_unmapped", "n_rescue_lines")
REF_LEN = 12_000
# every input: with and without names, cigar_m and secondary, and once with MAPQ tables of the caller's
FLAGS = [(nm, m, sec) for nm in (False, True) for m in (False, True) for sec in (False, True)]
TABLES = dict(mapq_unique=(11, 12, 13, 14), mapq_multi=(21, 22, 23, 24))


def _check_bam(ctx, lc, rd, ps, ref_len=REF_LEN, block_data=0, rname="chr7", **kw):
    """one call against the SAM call of the same inputs -> (the Bam, the record stream)"""
    D = block_data or 65280
    s = lc.sam(rd, ps, rname, **kw)
    call = lambda: lc.bam(rd, ps, rname, ref_len, block_data=block_data, **kw)
    b = call()
    raw = b.bytes()
    text, stream, records, blocks = bam_to_sam(raw, D)             # every block and every record, none left out
    want = s.header(ref_len) + s.text()
    if text != want:
        have, lines = text.split(b"\n"), want.split(b"\n")
        raise AssertionError([(i, have[i] if i < len(have) else None, w) for i, w in enumerate(lines) if i >= len(have) or have[i] != w][:4])
    got, sam = b.lines(), s.lines()
    assert got.dtype == LINE and len(got) == len(sam) == len(records) == len(b)
    for f in ("read", "source", "flag", "mapq", "kind"):
        assert np.array_equal(got[f], sam[f]), f
    assert b.records() == stream
    # offset / len tile the stream and are the decoder's records; a record's virtual offset leads to its block_size
    assert got["offset"].tolist() == [o for o, _n, _l in records] and got["len"].tolist() == [n for _o, n, _l in records]
    assert int(got["len"].sum()) == len(stream) and (len(got) == 0 or got["offset"][0] == 0)
    st = b.stats()
    voff = b.voffsets()
    header_blocks = [x for x in blocks if x[0] < st.header_file_bytes]
    assert sum(len(p) + 31 for _o, p in header_blocks) == st.header_file_bytes
    for i in range(len(got)):
        (block_size,) = struct.unpack("<i", at_voffset(blocks, int(voff[i]), 4))
        assert block_size == int(got["len"][i]) - 4, i
    # the views on the device, two calls
    d_file, n_file, d_rec, n_rec, d_lines, n_lines = b.device()
    assert (n_file, n_rec, n_lines) == (len(raw), len(stream), len(got))
    assert download(ctx, d_file, n_file, np.uint8).tobytes() == raw and download(ctx, d_rec, n_rec, np.uint8).tobytes() == stream
    assert download(ctx, d_lines, n_lines, LINE).tobytes() == got.tobytes()
    again = call()
    assert again.bytes() == raw and again.records() == stream and again.lines().tobytes() == got.tobytes()
    again.close()
    ss = s.stats()
    assert {c: int(getattr(st, c)) for c in COUNTS} == {c: int(getattr(ss, c)) for c in COUNTS} and st.n_records == ss.n_lines
    n_blocks = (len(stream) + D - 1) // D
    assert (st.n_record_bytes, st.n_file_bytes, st.n_record_blocks) == (len(stream), len(raw), n_blocks)
    assert st.n_file_bytes == st.header_file_bytes + len(stream) + 31 * n_blocks + 28 and st.ms_host > 0 and st.ms_total >= 0
    s.close()
    return b, stream


@gpu
def test_single_end_stranded(spm, ctx):
    t, reads, at = _single_end_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    names = _names(len(reads))
    for nm, cigar_m, secondary in FLAGS:
        b, _s = _check_bam(ctx, lc, rd, ps, names=names if nm else None, cigar_m=cigar_m, secondary=secondary)
        b.close()
    b, _s = _check_bam(ctx, lc, rd, ps, rname="x|y@z", ref_len=2 ** 31 - 1, **TABLES)
    b.close()
    rd1 = lc.reads(2 * len(reads), 1)                              # the same loci as a plain set of 2n reads
    b, _s = _check_bam(ctx, lc, rd1, ps, secondary=True)
    for x in (b, rd1, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_paired_without_rescues(spm, ctx):
    _t, reads, _classes = _planted_pairs()
    lc, rd, rest = _planted_chain(spm, ctx)
    ps = rest[1]
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    names = _names(len(reads) // 2)
    for nm, cigar_m, secondary in FLAGS:
        b, _s = _check_bam(ctx, lc, rd, ps, pairs=pr, names=names if nm else None, cigar_m=cigar_m, secondary=secondary)
        b.close()
    b, _s = _check_bam(ctx, lc, rd, ps, pairs=pr, **TABLES)
    b.close()
    for x in (pr, rd, lc) + rest:
        x.close()


@gpu
def test_paired_with_rescues_and_block_borders(spm, ctx):
    t, reads, planted = _rescue_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    assert RESCUED in set(rs.view()[0]["status"].tolist())
    names = _names(len(reads) // 2)
    for nm, cigar_m, secondary in FLAGS:
        b, _s = _check_bam(ctx, lc, rd, ps, pairs=pr, rescues=rs, names=names if nm else None, cigar_m=cigar_m, secondary=secondary)
        b.close()
    b, _s = _check_bam(ctx, lc, rd, ps, pairs=pr, rescues=rs, **TABLES)
    b.close()
    rs40 = pr.rescue(lc, rd, ref_text, ps, 40, MIN_TLEN, MAX_TLEN)  # the 150-symbol mate: a transcript of more than 64 words
    assert int(rs40.view()[0]["cigar_len"].max()) > 64
    for cigar_m in (False, True):
        b, _s = _check_bam(ctx, lc, rd, ps, pairs=pr, rescues=rs40, cigar_m=cigar_m, secondary=True)
        b.close()
    # block borders: every record straddles blocks; the record stream is the same at every block size
    kw = dict(pairs=pr, rescues=rs, names=names, cigar_m=True, secondary=True)
    b, stream = _check_bam(ctx, lc, rd, ps, **kw)
    b.close()
    for D in (1, 7, 64, 255, 256, 257, 1000):
        b, s = _check_bam(ctx, lc, rd, ps, block_data=D, **kw)
        assert s == stream
        b.close()
    # a block size that divides the stream: the last block is full.  Of the four option sets one has a length with a divisor
    # in 2 .. 4000 unless all four lengths are primes or products of larger ones
    for opt in (kw, dict(kw, names=None), dict(kw, cigar_m=False), dict(kw, secondary=False)):
        b, full = _check_bam(ctx, lc, rd, ps, **opt)
        b.close()
        D = next((d for d in range(4000, 1, -1) if len(full) % d == 0), None)
        if D is not None:
            break
    assert D is not None, "no option set gives a record stream whose length has a divisor in 2 .. 4000"
    assert len(full) % D == 0 and D > 1
    b, s = _check_bam(ctx, lc, rd, ps, block_data=D, **opt)
    assert s == full and b.stats().n_record_blocks == len(full) // D
    for x in (b, rs40, rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_more_than_two_default_blocks(spm, ctx):
    t, _reads, _at = _single_end_reads()
    ref = t["ref"]
    rng = np.random.default_rng(1601)
    starts = rng.integers(0, len(ref) - 150, 560)            # about 450 would do if every read mapped
    reads = [np.ascontiguousarray(ref[s:s + 150]) for s in starts.tolist()]
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    b, stream = _check_bam(ctx, lc, rd, ps, secondary=True)
    assert b.stats().n_record_blocks >= 3 and len(stream) > 2 * 65280
    b.close()
    b, s = _check_bam(ctx, lc, rd, ps, secondary=True, block_data=4096)
    assert s == stream
    for x in (b, rd, lc, ps, ref_text) + rest:
        x.close()


@gpu
def test_refusals_and_edges(spm, ctx):
    t, reads, _planted = _rescue_reads()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    lib, capi = spm.capi.lib(), spm.capi
    err = lambda: lib.spm_hip_last_error(ctx._h)

    def call(ref_len=REF_LEN, block_data=0, reserved=0, no_opts=False, l=lc, r=rd, p=pr, **kw):
        opts = capi.BamOpts(sam=spm.sam_opts("chr7", **kw), ref_len=ref_len, block_data=block_data, reserved=reserved)
        out = ctypes.c_void_p(1)                                   # (a refusal leaves NULL behind)
        h = lambda v: v._h if v is not None else None
        rc = lib.spm_hip_jst_ref_loci_bam(h(l), h(r), h(p), None, ps._h, None if no_opts else ctypes.byref(opts), ctypes.byref(out))
        return rc, out

    def refused(word, code=INVALID, **kw):
        rc, out = call(**kw)
        assert rc == code and not out.value and word in err(), (rc, out.value, err())

    rc, out = call()                                               # the arguments of every refusal below, unchanged: accepted
    assert rc == 0 and out.value
    lib.spm_hip_bam_destroy(out)
    refused(b"ref_len is 0", ref_len=0)
    refused(b"2^31 - 1", code=UNSUPPORTED, ref_len=2 ** 31)
    refused(b"block_data", block_data=65281)
    refused(b"reserved", reserved=1)
    refused(b"NULL opts", no_opts=True)
    refused(b"NULL", r=None)                                       # what the SAM call refuses, with its codes
    refused(b"symbols", symbols="ACG")
    fewer = lc.reads(len(reads) - 2, 2)
    refused(b"pairs", r=fewer)
    fewer.close()
    assert lib.spm_hip_jst_ref_loci_bam(None, rd._h, pr._h, None, ps._h, None, ctypes.byref(ctypes.c_void_p())) == INVALID
    refused(b"disagree", ref_len=int(lc.view()["ref_end"].max()) - 1, secondary=True)   # a record that ends beyond the reference
    with pytest.raises(spm.SpmError, match="-1.*ref_len"):
        lc.bam(rd, ps, "chr7", 0, pairs=pr)
    # records corrupted in the device buffer: counted, not followed; nothing is written
    hip = ctypes.CDLL("libamdhip64.so")
    PAIR = spm.JST_PAIR_DTYPE
    d_pairs, n = pr.device()
    host = download(ctx, d_pairs, n, PAIR)
    broken = host.copy()
    broken["locus1"][int(np.nonzero(host["locus1"] != 0xFFFFFFFF)[0][0])] = len(lc.view()) + 5
    ctx.synchronize()
    assert hip.hipMemcpy(ctypes.c_void_p(d_pairs), broken.ctypes.data_as(ctypes.c_void_p), broken.nbytes, 1) == 0
    refused(b"disagree")
    assert hip.hipMemcpy(ctypes.c_void_p(d_pairs), host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1) == 0
    b, _s = _check_bam(ctx, lc, rd, ps, pairs=pr)                  # and after all of this the call answers as before
    b.close()
    assert lib.spm_hip_bam_view(None, None, None, None, None, None, None) == INVALID
    assert lib.spm_hip_bam_device(None, None, None, None, None, None, None) == INVALID and lib.spm_hip_bam_stats(None, None) == INVALID
    lib.spm_hip_bam_destroy(None)
    # zero reads: a header with no records; the result outlives every input
    rd0 = lc.reads(0, 2)
    ps0 = ctx.patterns(spm.ALGO_MYERS, [], k=1, both_strands=True)
    e = lc.bam(rd0, ps0, "chr7", REF_LEN)
    keep, _s = _check_bam(ctx, lc, rd, ps, pairs=pr, secondary=True)
    raw = keep.bytes()
    for x in (ps0, rd0, pr, rd, lc, ps, ref_text) + rest:
        x.close()
    text, stream, records, _blocks = bam_to_sam(e.bytes())
    assert text == spm.sam_header("chr7", REF_LEN) and stream == b"" and records == [] and len(e.lines()) == 0
    assert e.bytes() == spm.bam_header("chr7", REF_LEN) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert e.stats().n_records == 0 and e.stats().n_record_blocks == 0 and e.device()[3] == 0
    e.close()
    d_file, n_file = keep.device()[:2]
    assert download(ctx, d_file, n_file, np.uint8).tobytes() == raw
    keep.close()
