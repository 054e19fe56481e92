"""What the four "records + CIGAR pool" results of libspm_amd/engine.py share -- Alignments, JstAlignments, JstRefAlignments,
JstRefLoci -- without a device: the one CIGAR rendering on a hand-made pool, and that an object without a handle releases
nothing."""
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
