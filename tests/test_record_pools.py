"""What the handle classes of libspm_amd/engine.py share, without a device.  The four "records + CIGAR pool" results --
Alignments, JstAlignments, JstRefAlignments, JstRefLoci: the one CIGAR rendering on a hand-made pool, and that an object
without a handle releases nothing.  Every class over a C handle: close() releases the handle once, with the destroy call of its
own C type, and only while the context is open."""
import ctypes
import types

import numpy as np
import pytest

import libspm_amd as S

INS, DEL, EQ, X = S.capi.CIGAR_INS, S.capi.CIGAR_DEL, S.capi.CIGAR_EQ, S.capi.CIGAR_X
# "41=1X12=1I45=" (the docstring's), a one-word transcript behind it, and one with a deletion
POOL = np.array([41 << 4 | EQ, 1 << 4 | X, 12 << 4 | EQ, 1 << 4 | INS, 45 << 4 | EQ, 100 << 4 | EQ, 7 << 4 | EQ, 3 << 4 | DEL,
                 90 << 4 | EQ], dtype=np.uint32)
SLOTS = [(0, 5, "41=1X12=1I45="), (5, 1, "100="), (6, 3, "7=3D90="), (5, 0, "")]
CLASSES = [(S.Alignments, S.ALN_DTYPE), (S.JstAlignments, S.JST_ALN_DTYPE), (S.JstRefAlignments, S.JST_REF_ALN_DTYPE),
           (S.JstRefLoci, S.JST_REF_LOCUS_DTYPE)]


@pytest.mark.parametrize("cls,dtype", CLASSES, ids=[c.__name__ for c, _ in CLASSES])
def test_cigar_of_a_hand_made_pool_and_an_object_without_a_handle(cls, dtype, monkeypatch):
    def no_call():
        raise AssertionError("an object without a handle called into the library")

    monkeypatch.setattr(S.capi, "lib", no_call)
    recs = np.zeros(len(SLOTS), dtype=dtype)
    recs["cigar_off"] = [s[0] for s in SLOTS]
    recs["cigar_len"] = [s[1] for s in SLOTS]
    a = cls(None, None)
    assert [a.cigar(i, records=recs, ops=POOL) for i in range(len(SLOTS))] == [s[2] for s in SLOTS]
    assert a.cigar(-1, recs, POOL) == ""            # (positional, as the callers pass them)
    a.close()
    a.close()
    assert not a._h and a.ctx is None
    a.__del__()
    del a


# every class over a C handle: the prefix of its C type, and what its constructor takes behind (ctx, h).  Jst's constructor
# creates the tree, so its object is made without it.
HANDLES = [(S.Text, "text", (4,)), (S.PatternSet, "patterns", (S.ALGO_MYERS, 1)), (S.Hits, "hits", ()),
           (S.Alignments, "alns", ()), (S.Jst, "jst", None), (S.JstHits, "jst_hits", ()), (S.JstAlignments, "jst_alns", ()),
           (S.JstRefAlignments, "jst_ref_alns", ()), (S.JstRefLoci, "jst_ref_loci", ()), (S.JstReads, "jst_reads", ()),
           (S.JstPairs, "jst_pairs", ()), (S.JstRescues, "jst_rescues", ()), (S.Sam, "sam", ("chr1",)),
           (S.Bam, "bam", (65280,)), (S.Bgzf, "bgzf", ())]


class RecordingLib:
    """stands in for the loaded library: every function exists, does nothing and is written down with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name,) + args)


def _make(cls, extra, ctx, h):
    if extra is not None:
        return cls(ctx, h, *extra)
    obj = object.__new__(cls)
    obj.ctx, obj._h = ctx, h
    return obj


@pytest.mark.parametrize("cls,prefix,extra", HANDLES, ids=[c.__name__ for c, _, _ in HANDLES])
def test_close_releases_the_handle_once_and_only_under_an_open_context(cls, prefix, extra, monkeypatch):
    lib = RecordingLib()
    monkeypatch.setattr(S.capi, "lib", lambda: lib)
    assert cls._PREFIX == prefix
    # a handle and an open context: exactly the destroy call of the C type, once, with the handle
    a = _make(cls, extra, types.SimpleNamespace(_h=7), 1234)
    a.close()
    assert lib.calls == [(f"spm_hip_{prefix}_destroy", 1234)] and a._h is None
    a.close()
    a.__del__()
    assert len(lib.calls) == 1 and a._h is None
    # the context has been closed first: there is nothing left to release
    del lib.calls[:]
    b = _make(cls, extra, types.SimpleNamespace(_h=ctypes.c_void_p()), 1234)   # (what Context.close leaves)
    b.close()
    b.__del__()
    assert lib.calls == [] and b._h is None
    # no handle, no context
    c = _make(cls, extra, None, None)
    c.close()
    c.__del__()
    assert lib.calls == [] and c._h is None


def test_the_handle_classes_above_are_all_of_them():
    """every public class of the package but Context is one of HANDLES, and they share one close() and one __del__"""
    public = {c for c in vars(S).values() if isinstance(c, type) and c.__module__ == "libspm_amd.engine"} - {S.Context}
    assert public == {c for c, _, _ in HANDLES} and len({p for _, p, _ in HANDLES}) == 15
    assert len({c.close for c in public}) == 1 and len({c.__del__ for c in public}) == 1
