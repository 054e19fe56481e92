"""What the accessors of the four output handles share (csrc/output_handles.hpp): spm_sam, spm_bam (as written and sorted),
spm_bai and spm_bgzf (a deflated file) of one small chain.  The view is downloaded once and answers with the same pointers
afterwards, its bytes are what the device pointers of _device hold, asking for _device and _stats before the view or after it
makes no difference, and the handles can be destroyed in either order."""
import ctypes

import numpy as np
import pytest

from cpp_programs import download
from test_jst_project import _make_tree
from test_pairs import MAX_TLEN, MIN_TLEN, _free_stretches
from test_rescue import K, RESCUED, _chain_of, _diverge
from test_sam import LINE
from test_strands import np_revcomp

gpu = pytest.mark.gpu
RNAME = "chr7"
M, TLEN, BLOCK = 24, 140, 256


def _small_pairs():
    """a tree of 4 Ki bases and 8 pairs of 24-symbol reads: six proper pairs, one whose mate 2 is 4 substitutions away (found
    by the rescue alone: the search runs with k = 2), one of noise"""
    t = _make_tree(2201, 4096, 4, 6, 4)
    ref = t["ref"]
    rng = np.random.default_rng(2202)
    spots = _free_stretches(t, 240, 7)
    reads = []
    for x in spots[:6]:
        reads += [ref[x:x + M].copy(), np_revcomp(ref[x + TLEN - M:x + TLEN])]
    x = spots[6]
    reads += [ref[x:x + M].copy(), np_revcomp(_diverge(rng, ref[x + TLEN - M:x + TLEN]))]
    reads += [rng.integers(0, 4, M, dtype=np.uint8), rng.integers(0, 4, M, dtype=np.uint8)]
    return t, [np.ascontiguousarray(r, np.uint8) for r in reads]


def _address(p):
    return ctypes.cast(p, ctypes.c_void_p).value or 0


def _view(h):
    """[(host address, bytes)] of the handle's view"""
    if h._PREFIX == "sam":
        t, nb, rec, nl = h._view()
        return [(_address(t), nb), (_address(rec), nl * LINE.itemsize)]
    if h._PREFIX == "bam":
        f, nf, r, nr, rec, nl = h._view()
        return [(_address(f), nf), (_address(r), nr), (_address(rec), nl * LINE.itemsize)]
    return [h._span("view")]


def _device(h):
    """[(device address, bytes)] in the order of _view"""
    d = h.device()
    spans = [(d[i], d[i + 1]) for i in range(0, len(d), 2)]
    if h._PREFIX in ("sam", "bam"):
        spans[-1] = (spans[-1][0], spans[-1][1] * LINE.itemsize)
    return spans


def _check(ctx, h, view_first):
    """-> the bytes of the view"""
    if view_first:
        first = _view(h)
    dev, stats = _device(h), bytes(h.stats())
    if not view_first:
        first = _view(h)
    assert _view(h) == first and all(p and n for p, n in first)      # downloaded once: the same pointers and lengths
    assert _device(h) == dev and bytes(h.stats()) == stats          # and neither moves what the other calls answer
    assert [n for _p, n in dev] == [n for _p, n in first]
    got = [ctypes.string_at(p, n) for p, n in first]
    for (d, n), g in zip(dev, got):
        assert download(ctx, d, n, np.uint8).tobytes() == g
    return got


def _body(spm, ctx, view_first, reverse):
    t, reads = _small_pairs()
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    pr = lc.pairs(rd, MIN_TLEN, MAX_TLEN)
    rs = pr.rescue(lc, rd, ref_text, ps, K, MIN_TLEN, MAX_TLEN)
    assert rs.view()[0]["status"].tolist().count(RESCUED) == 1
    sam = lc.sam(rd, ps, RNAME, pairs=pr, rescues=rs)
    bam = lc.bam(rd, ps, RNAME, len(t["ref"]), pairs=pr, rescues=rs, block_data=BLOCK)
    srt = bam.sort()
    bai = srt.index()
    z = bam.deflate(block_data=BLOCK)
    st = bam.stats()
    assert (st.n_records, st.n_unmapped, st.n_rescue_lines) == (16, 2, 1) and st.n_record_blocks >= 3
    made = [sam, bam, srt, bai, z]
    got = [_check(ctx, h, view_first) for h in made]
    for h in reversed(made) if reverse else made:
        h.close()
    for x in (rs, pr, rd, lc, ps, ref_text) + rest:
        x.close()
    return got


@gpu
def test_views_device_pointers_and_destruction_order(spm, ctx):
    a = _body(spm, ctx, view_first=True, reverse=True)
    b = _body(spm, ctx, view_first=False, reverse=False)
    assert a == b
    sam_text, bam_file, sorted_file = a[0][0], a[1][0], a[2][0]
    assert sam_text.count(b"\n") == 16 and bam_file != sorted_file
