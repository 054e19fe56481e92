"""Reference side of the matcher state blobs (include/spm_hip.h, "matcher state"): a decoder and an encoder for the
documented record layout, the Myers DP column by the Sellers recurrence, and the Shift-Or register by its definition.

TEST INFRASTRUCTURE ONLY, like oracle.py.  Bit vectors are Python ints: bit j of VP / VN / R is row j of the needle.
A Myers record stands for the DP column D[0..|P|] after the symbols read so far: VP bit j set iff D[j+1] - D[j] = +1,
VN bit j set iff it is -1, score = D[|P|].  (D[0] is 0 in infix mode and the number of symbols read in prefix mode; the
record does not hold it, the deltas and the score imply it.)
"""
from __future__ import annotations

import numpy as np

from . import oracle as O

# spm_algo values of include/spm_hip.h
ALGO_SHIFTOR, ALGO_MYERS, ALGO_MYERS_PREFIX, ALGO_HORSPOOL = 0, 1, 2, 3


def is_myers(algo: int) -> bool:
    return algo in (ALGO_MYERS, ALGO_MYERS_PREFIX)


def n_words(algo: int, max_m: int) -> int:
    """Set-wide word count of every record: ceil(max|P| / 64) Myers, ceil(max|P| / 32) Shift-Or (at least 1)."""
    return max(1, (max_m + 63) // 64) if is_myers(algo) else max(1, (max_m + 31) // 32)


def stride(algo: int, max_m: int) -> int:
    nw = n_words(algo, max_m)
    return 8 + 16 * nw if is_myers(algo) else 8 + 4 * ((nw + 1) & ~1)


def _bits(words: np.ndarray) -> int:
    return int.from_bytes(np.ascontiguousarray(words).tobytes(), "little")


def _words(v: int, n: int, dtype) -> np.ndarray:
    size = np.dtype(dtype).itemsize
    return np.frombuffer(v.to_bytes(n * size, "little"), dtype=dtype)


def decode(blob: np.ndarray, algo: int, n_patterns: int, max_m: int) -> list[dict]:
    """Myers records -> {score, n_words, vp, vn}; Shift-Or records -> {n_words, pad, r} (all bits of the record)."""
    st, nw = stride(algo, max_m), n_words(algo, max_m)
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    assert len(b) >= st * n_patterns, (len(b), st, n_patterns)
    out = []
    for i in range(n_patterns):
        rec = b[st * i:st * (i + 1)]
        if is_myers(algo):
            out.append({"score": int(rec[0:4].view(np.int32)[0]), "n_words": int(rec[4:8].view(np.uint32)[0]),
                        "vp": _bits(rec[8:8 + 8 * nw].view(np.uint64)),
                        "vn": _bits(rec[8 + 8 * nw:8 + 16 * nw].view(np.uint64))})
        else:
            out.append({"n_words": int(rec[0:4].view(np.uint32)[0]), "pad": int(rec[4:8].view(np.uint32)[0]),
                        "r": _bits(rec[8:8 + 4 * nw].view(np.uint32))})
    return out


def encode(records: list[dict], algo: int, max_m: int) -> np.ndarray:
    """Inverse of decode (n_words is written as the set-wide value; Shift-Or's pad word and tail word as 0)."""
    st, nw = stride(algo, max_m), n_words(algo, max_m)
    out = np.zeros(st * max(1, len(records)), dtype=np.uint8)
    for i, r in enumerate(records):
        rec = out[st * i:st * (i + 1)]
        if is_myers(algo):
            rec[0:4] = np.frombuffer(np.int32(r["score"]).tobytes(), np.uint8)
            rec[4:8] = np.frombuffer(np.uint32(nw).tobytes(), np.uint8)
            rec[8:8 + 8 * nw] = np.frombuffer(_words(r["vp"], nw, np.uint64).tobytes(), np.uint8)
            rec[8 + 8 * nw:8 + 16 * nw] = np.frombuffer(_words(r["vn"], nw, np.uint64).tobytes(), np.uint8)
        else:
            rec[0:4] = np.frombuffer(np.uint32(nw).tobytes(), np.uint8)
            rec[8:8 + 4 * nw] = np.frombuffer(_words(r["r"], nw, np.uint32).tobytes(), np.uint8)
    return out


# ---- Myers: the DP column and its record ----
def initial_column(m: int) -> np.ndarray:
    return np.arange(m + 1, dtype=np.int32)


def record_from_column(col: np.ndarray) -> dict:
    d = np.diff(np.asarray(col, dtype=np.int64))
    assert np.all(np.abs(d) <= 1), "not a DP column"
    vp = _bits(np.packbits(d == 1, bitorder="little"))
    vn = _bits(np.packbits(d == -1, bitorder="little"))
    return {"score": int(col[-1]), "vp": vp, "vn": vn}


def column_from_record(rec: dict, m: int) -> np.ndarray:
    """D[0..m] from the deltas of rows 0..m-1 and score = D[m] (bits >= m are ignored)."""
    d = np.array([((rec["vp"] >> j) & 1) - ((rec["vn"] >> j) & 1) for j in range(m)], dtype=np.int64)
    col = np.empty(m + 1, dtype=np.int64)
    col[m] = rec["score"]
    col[:m] = rec["score"] - np.cumsum(d[::-1])[::-1]
    return col.astype(np.int32)


def sellers_column(text, pat, k: int, mode: int = O.INFIX, col: np.ndarray | None = None, text_offset: int = 0):
    """Sellers over `text` continuing from `col` (mutated in place; None = the empty-prefix column).  -> (hits, col)"""
    if col is None:
        col = initial_column(len(pat))
    hits = O.sellers(text, pat, k, mode=mode, col=col, text_offset=text_offset)
    return hits, col


def record_from_oracle(st, m: int) -> dict:
    """The fast oracle's state (oracle.MyersState, all blocks active) as a record: bits >= m cleared."""
    nb = int(st.n_blocks)
    assert int(st.active) == nb, "cut-off state: rows outside the band are not exact"
    mask = (1 << m) - 1
    vp = sum(int(st.vp[b]) << (64 * b) for b in range(nb)) & mask
    vn = sum(int(st.vn[b]) << (64 * b) for b in range(nb)) & mask
    return {"score": int(st.score[nb - 1]), "vp": vp, "vn": vn}


def oracle_from_record(rec: dict, m: int, k: int):
    """An oracle.MyersState (full width, for variant=1) that continues from the column of `rec`."""
    st = O.myers_state(m, k)
    col = column_from_record(rec, m)
    nb = int(st.n_blocks)
    for b in range(nb):
        st.vp[b] = (rec["vp"] >> (64 * b)) & ((1 << 64) - 1)
        st.vn[b] = (rec["vn"] >> (64 * b)) & ((1 << 64) - 1)
        st.score[b] = int(col[min(64 * (b + 1), m)])
    st.active = nb
    return st


# ---- Shift-Or: the register by definition ----
def shiftor_register(read: np.ndarray, pat: np.ndarray) -> int:
    """R after reading `read` (every symbol since the matcher was constructed): bit j (j < |P|) is clear exactly when
    P[0..j] equals the last j + 1 symbols read; bits >= |P| of the |P|-bit register are set."""
    m = len(pat)
    nw = (m + 31) // 32
    r = (1 << (32 * nw)) - 1
    read = np.asarray(read, dtype=np.uint8)
    pat = np.asarray(pat, dtype=np.uint8)
    for j in range(min(m, len(read))):
        if np.array_equal(read[len(read) - j - 1:], pat[:j + 1]):
            r &= ~(1 << j)
    return r


def shiftor_oracle_register(state: np.ndarray) -> int:
    """oracle.shiftor's state (uint32 words) as an int."""
    return _bits(np.asarray(state, dtype=np.uint32))


def shiftor_oracle_from_register(r: int, m: int) -> np.ndarray:
    return _words(r, (m + 31) // 32, np.uint32).copy()
