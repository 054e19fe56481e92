"""Thin object layer over the C ABI, used by tests, bench.py and the multi-GPU driver.

Names follow the reference's domain: a *haystack* (Text) is scanned for a set of *needles* (PatternSet); a scan
returns hit records (pos, pattern, score) -- what the reference's callback reads off the seqan2::Finder
(/root/reference/libspm/libspm/matcher/seqan_pattern_base.hpp:40-52).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


def _dtype(struct) -> np.dtype:
    """The numpy view of a record of the C ABI: capi's ctypes.Structure is the one statement of its layout."""
    return np.dtype(struct)


HIT_DTYPE = _dtype(capi.Hit)
ALN_DTYPE = _dtype(capi.Aln)
ALLELE_DTYPE = _dtype(capi.JstAllele)
JST_HIT_DTYPE = _dtype(capi.JstHit)
JST_ALN_DTYPE = _dtype(capi.JstAln)
JST_REF_ALN_DTYPE = _dtype(capi.JstRefAln)
JST_REF_LOCUS_DTYPE = _dtype(capi.JstRefLocus)
JST_READ_DTYPE = _dtype(capi.JstRead)
JST_PAIR_DTYPE = _dtype(capi.JstPair)
JST_RESCUE_DTYPE = _dtype(capi.JstRescue)
SAM_LINE_DTYPE = _dtype(capi.SamLine)
PILEUP_SITE_DTYPE = _dtype(capi.PileupSite)
PILEUP_PLANES = capi.PILEUP_PLANES
VARIANT_CALL_DTYPE = _dtype(capi.VariantCall)
_CIGAR_CHAR = {capi.CIGAR_INS: "I", capi.CIGAR_DEL: "D", capi.CIGAR_EQ: "=", capi.CIGAR_X: "X"}


def _check(rc, ctx_handle):
    if rc != 0:
        msg = capi.lib().spm_hip_last_error(ctx_handle)
        raise capi.SpmError(f"libspm_hip error {rc}: {msg.decode() if msg else ''}")


def _as_array(ptr, n, ctype, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    buf = (ctype * n).from_address(C.addressof(ptr.contents))
    return np.frombuffer(buf, dtype=dtype).copy()


def _size_then_fill(call, refuse=lambda rc: _check(rc, None)) -> bytes:
    """The bytes of a host-only call that writes into its caller's buffer: call(dst, cap, len) -> rc, once without a buffer,
    which answers E_OVERFLOW and the length, then with a buffer of that length.  refuse(rc) raises for any other first
    answer; where it returns (rc 0: there is nothing to write), the result is empty."""
    need = C.c_uint64()
    rc = call(None, 0, C.byref(need))
    if rc != capi.E_OVERFLOW:
        refuse(rc)
        return b""
    buf = C.create_string_buffer(need.value)
    _check(call(buf, need.value, C.byref(need)), None)
    return buf.raw[:need.value]


def _block_data(block_data) -> int:
    """the uncompressed bytes of a full BGZF block: 0 asks for the most a block may hold"""
    return int(block_data) or capi.BGZF_BLOCK_DATA


def _voffsets(stream_offsets, block_data, block_offset) -> np.ndarray:
    """BGZF virtual file offsets of bytes of the uncompressed stream: the file offset of the block that holds the byte << 16
    | the byte's offset in that block's data.  block_offset(i): the file offsets of the blocks i (an array)."""
    u = np.asarray(stream_offsets).astype(np.uint64)
    D = np.uint64(block_data)
    return (block_offset(u // D) << np.uint64(16)) | (u % D)


def _require_open(obj, method, whose, tree=True):
    """obj.<method> reads the needle set behind obj and, with tree, the tree: neither may have been closed.  An object
    that was given none has nothing to check."""
    needed = (obj._jst, obj._pats) if tree else (obj._pats,)
    if any(x is not None and not x._h for x in needed):
        what = "the tree or the needle set" if tree else "the needle set"
        raise capi.SpmError(f"{type(obj).__name__}.{method}: {what} of {whose} has been closed")


class _Handle:
    """An object of the C type spm_hip_<_PREFIX>_* and the context it was made in.  The calls that take the handle first go
    through _call and what is built on it; a method on a path that bench.py times spells its call out."""
    _PREFIX = None

    def __init__(self, ctx, h):
        self.ctx, self._h = ctx, h

    def _call(self, name, *args):
        _check(getattr(capi.lib(), f"spm_hip_{self._PREFIX}_{name}")(self._h, *args), self.ctx._h)

    def _stats(self, struct, name="stats"):
        s = struct()
        self._call(name, C.byref(s))
        return s

    def _span(self, name):
        """(pointer, count), both as int"""
        p, n = C.c_void_p(), C.c_uint64()
        self._call(name, C.byref(p), C.byref(n))
        return int(p.value or 0), int(n.value)

    def _new(self, name, *args) -> C.c_void_p:
        """the handle that a call puts into its last argument"""
        h = C.c_void_p()
        self._call(name, *args, C.byref(h))
        return h

    def close(self):
        if self._h:
            if self.ctx._h:  # the C objects point at their context: once it is gone there is nothing left to release
                getattr(capi.lib(), f"spm_hip_{self._PREFIX}_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        rc = capi.lib().spm_hip_init(device, C.c_void_p(stream) if stream else None, C.byref(self._h))
        if rc != 0:
            msg = capi.lib().spm_hip_last_error(None)
            raise capi.SpmError(f"spm_hip_init failed ({rc}): {msg.decode() if msg else ''}")
        self.device = device

    def synchronize(self):
        _check(capi.lib().spm_hip_synchronize(self._h), self._h)

    def close(self):
        if self._h:
            capi.lib().spm_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- haystacks ----
    def upload(self, ranks, sigma: int = 4) -> "Text":
        a = np.ascontiguousarray(ranks, dtype=np.uint8)
        h = C.c_void_p()
        _check(capi.lib().spm_hip_text_upload(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, sigma,
                                              C.byref(h)), self._h)
        return Text(self, h, sigma)

    def wrap(self, device_ptr: int, n: int, sigma: int = 4, keepalive=None) -> "Text":
        h = C.c_void_p()
        _check(capi.lib().spm_hip_text_wrap(self._h, C.c_void_p(device_ptr), n, sigma, C.byref(h)), self._h)
        t = Text(self, h, sigma)
        t._keepalive = keepalive
        return t

    def generate(self, seed: int, global_begin: int, n: int) -> "Text":
        h = C.c_void_p()
        _check(capi.lib().spm_hip_text_generate(self._h, seed, global_begin, n, C.byref(h)), self._h)
        return Text(self, h, 4)

    def generate_repeats(self, seed: int, global_begin: int, n: int, repeat_ppm: int) -> "Text":
        """Synthetic repeat-rich dna4 text (bench workload c3r; csrc/synth.hpp)."""
        h = C.c_void_p()
        _check(capi.lib().spm_hip_text_generate_repeats(self._h, seed, global_begin, n, repeat_ppm, C.byref(h)),
               self._h)
        return Text(self, h, 4)

    # ---- containers ----
    def _bgzf(self, frame, opts, device_ptr, n) -> "Bgzf":
        z = C.c_void_p()
        _check(frame(self._h, C.c_void_p(device_ptr), int(n), C.byref(opts), C.byref(z)), self._h)
        return Bgzf(self, z, block_data=_block_data(opts.block_data))

    def bgzf(self, device_ptr: int, n: int, *, block_data: int = 0, eof: bool = True) -> "Bgzf":
        """BGZF framing (stored blocks, nothing compressed) of n bytes at device_ptr, any alignment, on the device
        (spm_hip_bgzf_frame).  block_data: uncompressed bytes per block, 0 for 65280; eof: append the end-of-file block.  The
        source is read before the call returns."""
        return self._bgzf(capi.lib().spm_hip_bgzf_frame, bgzf_opts(block_data, eof), device_ptr, n)

    def bai(self, records: int, n_record_bytes: int, lines: int, n_lines: int, block_offsets: int, n_blocks: int,
            block_data: int = 0) -> "Bai":
        """The BAI index of a coordinate-sorted record stream in device memory (spm_hip_bai_build), the raw form of Bam.index():
        records / lines / block_offsets are device pointers to the uncompressed stream, its SAM_LINE_DTYPE records (offset and
        len are read) and the n_blocks + 1 file offsets of its blocks of block_data uncompressed bytes (0: 65280)."""
        z = C.c_void_p()
        _check(capi.lib().spm_hip_bai_build(self._h, C.c_void_p(records), int(n_record_bytes), C.c_void_p(lines), int(n_lines),
                                            C.c_void_p(block_offsets), int(n_blocks), int(block_data), C.byref(z)), self._h)
        return Bai(self, z)

    def bam_markdup(self, records: int, n_record_bytes: int, lines: int, n_lines: int, ref_len: int, dup_ptr: int,
                    min_qual: int = 0) -> capi.BamMarkdupStats:
        """Duplicate marks of a record stream in device memory (spm_hip_bam_markdup_records), the raw form of Bam.markdup():
        records / lines are device pointers to the uncompressed stream and its SAM_LINE_DTYPE records (offset, len and read are
        read), dup_ptr one to n_lines bytes that take 1 where the record is a duplicate.  min_qual: 0 for 15.  -> the counts."""
        opts, stats = bam_markdup_opts(min_qual), capi.BamMarkdupStats()
        _check(capi.lib().spm_hip_bam_markdup_records(self._h, C.c_void_p(records), int(n_record_bytes), C.c_void_p(lines), int(n_lines),
                                                      int(ref_len), C.byref(opts), C.c_void_p(dup_ptr), C.byref(stats)), self._h)
        return stats

    def bam_pileup(self, records: int, n_record_bytes: int, lines: int, n_lines: int, ref_len: int, begin: int = 0, end=None,
                   min_mapq: int = 0, min_baseq: int = 0, exclude_flags=None) -> "Pileup":
        """The pileup of a coordinate-sorted record stream in device memory (spm_hip_bam_pileup_records), the raw form of
        Bam.pileup(): records / lines are device pointers to the uncompressed stream and its SAM_LINE_DTYPE records (offset and len
        are read).  The other arguments are Bam.pileup's."""
        opts, h = pileup_opts(begin, end, min_mapq, min_baseq, exclude_flags), C.c_void_p()
        _check(capi.lib().spm_hip_bam_pileup_records(self._h, C.c_void_p(records), int(n_record_bytes), C.c_void_p(lines), int(n_lines),
                                                     int(ref_len), C.byref(opts), C.byref(h)), self._h)
        return Pileup(self, h, int(begin))

    def pileup_sites_vcf(self, sites: int, n_sites: int, rname, sample, ref_len: int, **opts) -> "Vcf":
        """Genotype calls and the VCF text of site records in device memory (spm_hip_pileup_sites_vcf_records), the raw form of
        PileupSites.vcf(): sites is a device pointer to n_sites PILEUP_SITE_DTYPE records in ascending pos.  opts: vcf_opts'."""
        o, h = vcf_opts(**opts), C.c_void_p()
        _check(capi.lib().spm_hip_pileup_sites_vcf_records(self._h, C.c_void_p(sites), int(n_sites), _name(rname), _name(sample),
                                                           int(ref_len), C.byref(o), C.byref(h)), self._h)
        return Vcf(self, h)

    def bgzf_deflate(self, device_ptr: int, n: int, *, block_data: int = 0, eof: bool = True, dynamic: bool = False) -> "Bgzf":
        """bgzf() with the blocks compressed on the device (spm_hip_bgzf_deflate: LZ77 matches and the fixed Huffman code per
        block; a block that would not shrink stays stored).  dynamic: a block may take a Huffman code of its own, built on the
        device (SPM_BGZF_DYNAMIC), where that is smaller.  The bytes are those of bgzf_deflate_host with the same arguments."""
        return self._bgzf(capi.lib().spm_hip_bgzf_deflate, bgzf_deflate_opts(block_data, eof, dynamic=dynamic), device_ptr, n)

    # ---- needles ----
    def patterns(self, algo: int, needles, k=0, sigma: int = 4, both_strands: bool = False) -> "PatternSet":
        """needles: a sequence of rank arrays, or -- reads of one length -- a 2-D uint8 array, one needle per row (what the C ABI
        takes anyway: ranks back to back + offsets; 100 000 rows cost a reshape instead of 100 000 Python objects).
        both_strands: the needles are n READS and the set holds 2n needles (spm_hip_patterns_create_stranded): pattern 2r is
        read r, pattern 2r + 1 its reverse complement, both with k[r]."""
        if isinstance(needles, np.ndarray) and needles.ndim == 2:
            mat = np.ascontiguousarray(needles, dtype=np.uint8)
            n_needles = mat.shape[0]
            offs = (np.arange(n_needles + 1, dtype=np.uint64) * mat.shape[1]).astype(np.uint32)
            cat = mat.reshape(-1) if mat.size else np.zeros(1, np.uint8)
            needles = mat          # (len() below)
        else:
            needles = [np.ascontiguousarray(p, dtype=np.uint8) for p in needles]
            offs = np.zeros(len(needles) + 1, dtype=np.uint32)
            if needles:
                offs[1:] = np.cumsum([len(p) for p in needles])
            cat = np.concatenate(needles) if needles and offs[-1] else np.zeros(1, np.uint8)
        if np.isscalar(k):
            ks = np.full(max(1, len(needles)), k, dtype=np.uint16)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uint16)
        h = C.c_void_p()
        create = capi.lib().spm_hip_patterns_create_stranded if both_strands else capi.lib().spm_hip_patterns_create
        _check(create(self._h, algo, cat.ctypes.data_as(C.POINTER(C.c_uint8)), offs.ctypes.data_as(C.POINTER(C.c_uint32)),
                      len(needles), ks.ctypes.data_as(C.POINTER(C.c_uint16)), sigma, C.byref(h)), self._h)
        return PatternSet(self, h, algo, (2 if both_strands else 1) * len(needles))


class Text(_Handle):
    _PREFIX = "text"

    def __init__(self, ctx, h, sigma):
        super().__init__(ctx, h)
        self.sigma = sigma
        self._keepalive = None

    def __len__(self):
        return int(capi.lib().spm_hip_text_length(self._h))

    @property
    def device_ptr(self) -> int:
        return int(capi.lib().spm_hip_text_device_ptr(self._h) or 0)

    def pack(self):
        """Build the optional 2-bit shadow (dna4 only): later seed-filter scans stream a quarter of the bytes."""
        _check(capi.lib().spm_hip_text_pack(self.ctx._h, self._h), self.ctx._h)
        return self

    @property
    def packed(self) -> bool:
        return bool(capi.lib().spm_hip_text_is_packed(self._h))

    def download(self, begin: int, n: int) -> np.ndarray:
        out = np.empty(n, dtype=np.uint8)
        _check(capi.lib().spm_hip_text_download(self.ctx._h, self._h, begin, n,
                                                out.ctypes.data_as(C.POINTER(C.c_uint8))), self.ctx._h)
        return out


class PatternSet(_Handle):
    _PREFIX = "patterns"

    def __init__(self, ctx, h, algo, n):
        super().__init__(ctx, h)
        self.algo, self.n = algo, n

    def __len__(self):
        """needles in the set: 2n for n reads on both strands"""
        return int(capi.lib().spm_hip_patterns_count(self._h))

    @property
    def strands(self) -> int:
        """2 for a set made with both_strands (read = pattern >> 1, strand = pattern & 1), else 1"""
        return int(capi.lib().spm_hip_patterns_strands(self._h))

    def needle(self, p: int) -> np.ndarray:
        """The ranks of needle p, from the set's host copy: SAM SEQ of a reverse-strand hit when p is odd in a stranded set."""
        n = C.c_uint32()
        capi.lib().spm_hip_patterns_needle(self._h, p, None, 0, C.byref(n))
        out = np.empty(n.value, dtype=np.uint8)
        rc = capi.lib().spm_hip_patterns_needle(self._h, p, out.ctypes.data_as(C.POINTER(C.c_uint8)), n.value, C.byref(n))
        if rc != 0:
            raise capi.SpmError(f"spm_hip_patterns_needle: no needle {p} in a set of {len(self)}")
        return out

    def window_size(self, p: int = 0) -> int:
        return int(capi.lib().spm_hip_patterns_window_size(self._h, p))

    @property
    def filterable(self) -> bool:
        return bool(capi.lib().spm_hip_patterns_filterable(self._h))

    def build_stats(self) -> capi.BuildStats:
        """What spm_hip_patterns_create spent where (host ms) and what it built (passes, keys, dense, anchors)."""
        return self._stats(capi.BuildStats, "build_stats")

    def state_stride(self) -> int:
        return int(capi.lib().spm_hip_patterns_state_stride(self._h))

    def initial_state(self) -> np.ndarray:
        st = np.zeros(self.state_stride() * max(1, self.n), dtype=np.uint8)
        self._call("state_init", st.ctypes.data)
        return st


class Hits(_Handle):
    _PREFIX = "hits"

    def __init__(self, ctx, h, text=None, pats=None):
        # the scan's haystack and needle set: align() reads both, so they live at least as long as the hits
        super().__init__(ctx, h)
        self._text, self._pats = text, pats

    def view(self) -> np.ndarray:
        """Hits sorted by (pattern, pos): per pattern, the order the reference's callback fires in."""
        rec = C.POINTER(capi.Hit)()
        n = C.c_uint64()
        _check(capi.lib().spm_hip_hits_view(self._h, C.byref(rec), C.byref(n)), self.ctx._h)
        if n.value == 0:
            return np.zeros(0, dtype=HIT_DTYPE)
        buf = (capi.Hit * n.value).from_address(C.addressof(rec.contents))
        return np.frombuffer(buf, dtype=HIT_DTYPE).copy()

    def device(self):
        p = C.c_void_p()
        n = C.c_uint64()
        _check(capi.lib().spm_hip_hits_device(self._h, C.byref(p), C.byref(n)), self.ctx._h)
        return int(p.value or 0), int(n.value)

    def copy_to(self, device_ptr: int, cap: int) -> int:
        """Async D2D copy of the hit records into a caller-owned device buffer; returns the hit count."""
        n = C.c_uint64()
        _check(capi.lib().spm_hip_hits_copy_device(self._h, C.c_void_p(device_ptr), cap, C.byref(n)), self.ctx._h)
        return int(n.value)

    def copy_fused(self, device_ptr: int, cap: int) -> int:
        """copy_to with a 16-byte {count, 0} header in front: the [count | records] buffer of dist.gather_hits_fused."""
        n = C.c_uint64()
        _check(capi.lib().spm_hip_hits_copy_fused(self._h, C.c_void_p(device_ptr), cap, C.byref(n)), self.ctx._h)
        return int(n.value)

    def copy_fused_device(self, device_ptr: int, cap: int) -> None:
        """copy_fused without the host knowing the count: header {count, status} written by a kernel from the scan's device
        counters (status != 0: the scan needs the host -- call view() / stats() and copy again).  No synchronisation."""
        _check(capi.lib().spm_hip_hits_copy_fused_device(self._h, C.c_void_p(device_ptr), cap), self.ctx._h)

    def align(self, begin_only: bool = False) -> "Alignments":
        """Begin + CIGAR transcript of every hit (spm_hip_hits_align); record i belongs to view() record i."""
        return Alignments(self.ctx, self._new("align", capi.ALIGN_BEGIN_ONLY if begin_only else 0))

    def select(self, loci: bool = True, window: int | None = None, best: int | None = None, strands: bool = False) -> "Hits":
        """A new, smaller Hits (spm_hip_hits_select): one record per locus (loci; window=None: every needle's own k) and,
        with best=s, only the records within s errors of their needle's minimum -- with strands=True (a set made with
        both_strands) of their READ's minimum over both strands.  Host AND device view of the result are sorted by
        (pattern, pos); it stays valid after this object is closed."""
        opts = _select_opts(loci, window, best, strands=strands)
        return Hits(self.ctx, self._new("select", C.byref(opts)), self._text, self._pats)

    def select_stats(self) -> capi.SelectStats:
        return self._stats(capi.SelectStats, "select_stats")

    def stats(self) -> capi.ScanStats:
        s = capi.ScanStats()
        _check(capi.lib().spm_hip_hits_stats(self._h, C.byref(s)), self.ctx._h)
        return s

    def checksum(self) -> int:
        return int(capi.lib().spm_hip_hits_checksum(self._h))


class _RecordPool(_Handle):
    """What the results made of records + a pool of CIGAR words (len << 4 | op) share: a view that hands out _REC records
    (numpy: _DTYPE) and the pool they point into.  The subclasses declare the three and keep what is their own."""
    _REC = _DTYPE = None

    def _raw(self):
        rec, ops = C.POINTER(self._REC)(), C.POINTER(C.c_uint32)()
        n, n_ops = C.c_uint64(), C.c_uint64()
        self._call("view", C.byref(rec), C.byref(n), C.byref(ops), C.byref(n_ops))
        return rec, n.value, ops, n_ops.value

    def __len__(self):
        return self._raw()[1]

    def view(self) -> np.ndarray:
        r = self._raw()
        return _as_array(r[0], r[1], self._REC, self._DTYPE)

    @property
    def ops(self) -> np.ndarray:
        r = self._raw()
        return _as_array(r[2], r[3], C.c_uint32, np.uint32)

    def _device(self):
        r, o = C.c_void_p(), C.c_void_p()
        n, n_ops = C.c_uint64(), C.c_uint64()
        self._call("device", C.byref(r), C.byref(n), C.byref(o), C.byref(n_ops))
        return int(r.value or 0), int(n.value), int(o.value or 0), int(n_ops.value)

    def _cigar(self, i, records, ops) -> str:
        r = (self.view() if records is None else records)[i]
        o = self.ops if ops is None else ops
        words = o[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])]
        return "".join(f"{int(w) >> 4}{_CIGAR_CHAR[int(w) & 15]}" for w in words)


class Alignments(_RecordPool):
    """Result of Hits.align(): ALN_DTYPE records in the order of Hits.view(), and the pool of CIGAR words
    (len << 4 | op) they point into."""
    _PREFIX, _REC, _DTYPE = "alns", capi.Aln, ALN_DTYPE

    def device(self):
        """(records, n, ops, n_ops): device pointers, records in device hit order."""
        return self._device()

    def cigar(self, i: int, records: np.ndarray | None = None, ops: np.ndarray | None = None) -> str:
        """SAM string of record i, e.g. "41=1X12=1I45=" (records / ops: views already fetched, to save the copies)."""
        return self._cigar(i, records, ops)

    def stats(self) -> capi.AlignStats:
        return self._stats(capi.AlignStats)


def scan(ctx: Context, text: Text, pats: PatternSet, begin: int = 0, end: int | None = None, *,
         engine: int = capi.ENGINE_AUTO, left_context: bool = False, pos_offset: int = 0, max_hits: int = 0,
         state_in: np.ndarray | None = None, want_state: bool = False, flags: int = 0):
    """One scan of text[begin:end) -- seqan_pattern_base::operator() for a whole needle set.

    Returns Hits, or (Hits, state_out) when want_state is set."""
    end = len(text) if end is None else end
    opts = capi.ScanOpts(engine=engine, left_context=1 if left_context else 0, pos_offset=pos_offset,
                         max_hits=max_hits, flags=flags, reserved=0)
    h = C.c_void_p()
    st_in = state_in.ctypes.data if state_in is not None else None
    st_out = None
    if want_state:
        st_out = np.zeros(pats.state_stride() * max(1, pats.n), dtype=np.uint8)
    _check(capi.lib().spm_hip_scan(ctx._h, text._h, begin, end, pats._h, C.byref(opts), st_in,
                                   st_out.ctypes.data if st_out is not None else None, C.byref(h)), ctx._h)
    hits = Hits(ctx, h, text, pats)
    return (hits, st_out) if want_state else hits


def _select_opts(loci, window, best, across=False, strands=False) -> capi.SelectOpts:
    flags = ((capi.SELECT_LOCI if loci else 0) | (capi.SELECT_BEST if best is not None else 0)
             | (capi.SELECT_ACROSS if across else 0) | (capi.SELECT_STRANDS if strands else 0))
    return capi.SelectOpts(flags=flags, window=capi.SELECT_WINDOW_K if window is None else int(window),
                           strata=0 if best is None else int(best), reserved=0)


def select_records(ctx: Context, device_ptr: int, n: int, pats: PatternSet | None = None, *, loci: bool = True,
                   window: int | None = None, best: int | None = None, strands: bool = False) -> Hits:
    """Hits.select() on a device buffer of n HIT_DTYPE records that no Hits owns -- what a gatherv delivers on the root
    (spm_hip_records_select).  pats may be None when window is explicit.  The result cannot be aligned.  strands: as
    Hits.select; without pats the records are taken by the index convention read = pattern >> 1."""
    opts = _select_opts(loci, window, best, strands=strands)
    h = C.c_void_p()
    _check(capi.lib().spm_hip_records_select(ctx._h, C.c_void_p(device_ptr), n, pats._h if pats is not None else None,
                                             C.byref(opts), C.byref(h)), ctx._h)
    return Hits(ctx, h, None, pats)


def scan_segments(ctx: Context, text: Text, pats: PatternSet, seg_offsets, *, engine: int = capi.ENGINE_AUTO,
                  max_hits: int = 0, flags: int = 0) -> Hits:
    """Scan a batch of independent haystacks stored back to back (segment s = text[off[s]:off[s+1]]) in one launch."""
    offs = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    opts = capi.ScanOpts(engine=engine, left_context=0, pos_offset=0, max_hits=max_hits, flags=flags, reserved=0)
    h = C.c_void_p()
    _check(capi.lib().spm_hip_scan_segments(ctx._h, text._h, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            len(offs) - 1, pats._h, C.byref(opts), C.byref(h)), ctx._h)
    return Hits(ctx, h, text, pats)


def synth_pattern(seed_text: int, seed_pat: int, n_total: int, p: int, L: int, kmax: int):
    out = np.empty(L, dtype=np.uint8)
    o = capi.lib().spm_hip_synth_pattern(seed_text, seed_pat, n_total, p, L, kmax,
                                         out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out, int(o)


def synth_repeat_pattern(seed_text: int, seed_pat: int, n_total: int, p: int, L: int, kmax: int, repeat_ppm: int,
                         across_every: int = 8):
    out = np.empty(L, dtype=np.uint8)
    o = capi.lib().spm_hip_synth_repeat_pattern(seed_text, seed_pat, n_total, p, L, kmax, repeat_ppm, across_every,
                                                out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out, int(o)


def synth_repeat_text(seed: int, repeat_ppm: int, begin: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    capi.lib().spm_hip_synth_repeat_text(seed, repeat_ppm, begin, n, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def synth_variants(seed_text: int, seed_var: int, ref_begin: int, n_ref: int, n_haplotypes: int):
    """The synthetic variants of config C5: (alleles, alt_pool, coverage) as numpy arrays."""
    na, npool = C.c_uint64(0), C.c_uint64(0)
    rc = capi.lib().spm_hip_jst_synth_variants(seed_text, seed_var, ref_begin, n_ref, n_haplotypes, None, C.byref(na),
                                               None, C.byref(npool), None)
    if rc != 0:
        raise capi.SpmError("spm_hip_jst_synth_variants: invalid argument")
    alleles = np.zeros(max(1, na.value), dtype=ALLELE_DTYPE)
    pool = np.zeros(max(1, npool.value), dtype=np.uint8)
    cov = np.zeros(max(1, na.value), dtype=np.uint64)
    rc = capi.lib().spm_hip_jst_synth_variants(seed_text, seed_var, ref_begin, n_ref, n_haplotypes,
                                               alleles.ctypes.data_as(C.POINTER(capi.JstAllele)), C.byref(na),
                                               pool.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(npool),
                                               cov.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise capi.SpmError("spm_hip_jst_synth_variants failed")
    return alleles[:na.value], pool[:npool.value], cov[:na.value]


class Jst(_Handle):
    """Journaled sequence tree in HBM: a reference Text + alleles + per-allele haplotype coverage."""
    _PREFIX = "jst"

    def __init__(self, ctx: Context, reference: Text, alleles, alt_pool, coverage, n_haplotypes: int):
        self.reference, self.n_haplotypes = reference, n_haplotypes
        al = np.ascontiguousarray(alleles, dtype=ALLELE_DTYPE)
        pool = np.ascontiguousarray(alt_pool, dtype=np.uint8)
        cw = (n_haplotypes + 63) // 64
        cov = np.ascontiguousarray(coverage, dtype=np.uint64).reshape(-1)
        if cov.size != len(al) * cw:
            raise ValueError("coverage must hold ceil(n_haplotypes / 64) words per allele")
        h = C.c_void_p()
        _check(capi.lib().spm_hip_jst_create(ctx._h, reference._h, al.ctypes.data_as(C.POINTER(capi.JstAllele)),
                                             len(al), pool.ctypes.data_as(C.POINTER(C.c_uint8)), pool.size,
                                             cov.ctypes.data_as(C.POINTER(C.c_uint64)), n_haplotypes, C.byref(h)),
               ctx._h)
        super().__init__(ctx, h)

    def haplotype_length(self, h: int) -> int:
        return int(capi.lib().spm_hip_jst_haplotype_length(self._h, h))

    def extract(self, h: int, begin: int, n: int) -> np.ndarray:
        out = np.empty(n, dtype=np.uint8)
        self._call("extract", h, begin, n, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out

    def index(self, window: int, block_len: int = 0, block_begin: int = 0, block_end: int = 0):
        self._call("index", window, block_len, block_begin, block_end)
        return self.stats()

    def stats(self) -> capi.JstStats:
        st = capi.JstStats()
        _check(capi.lib().spm_hip_jst_stats(self._h, C.byref(st)), self.ctx._h)
        return st

    def search_device(self, pats: PatternSet, *, engine: int = capi.ENGINE_AUTO, max_hits: int = 0,
                      alignable: bool = False) -> "JstHits":
        """One search over all haplotypes; the records stay in HBM (arrival order) until view()/copy_to().
        alignable: the result keeps the search's segment hits, so that JstHits.align() can align them."""
        opts = capi.ScanOpts(engine=engine, left_context=0, pos_offset=0, max_hits=max_hits,
                             flags=capi.SCAN_ALIGNABLE if alignable else 0, reserved=0)
        hh = C.c_void_p()
        _check(capi.lib().spm_hip_jst_search(self._h, pats._h, C.byref(opts), C.byref(hh)), self.ctx._h)
        return JstHits(self.ctx, hh, self, pats)

    def search(self, pats: PatternSet, *, engine: int = capi.ENGINE_AUTO, max_hits: int = 0) -> np.ndarray:
        """All hits over all haplotypes, sorted by (haplotype, pos, pattern): JST_HIT_DTYPE records."""
        h = self.search_device(pats, engine=engine, max_hits=max_hits)
        try:
            return h.view()
        finally:
            h.close()


class JstHits(_Handle):
    _PREFIX = "jst_hits"

    def __init__(self, ctx, h, jst=None, pats=None):
        # the search's tree and needle set: align() reads both, so they live at least as long as the hits
        super().__init__(ctx, h)
        self._jst, self._pats = jst, pats

    def __len__(self):
        return self.device()[1]

    def device(self):
        """(pointer, count) of the records in HBM: arrival order for a search, (haplotype, pattern, pos) order for a
        selection."""
        return self._span("device")

    def view(self) -> np.ndarray:
        rec = C.POINTER(capi.JstHit)()
        n = C.c_uint64(0)
        _check(capi.lib().spm_hip_jst_hits_view(self._h, C.byref(rec), C.byref(n)), self.ctx._h)
        if n.value == 0:
            return np.zeros(0, dtype=JST_HIT_DTYPE)
        buf = (capi.JstHit * n.value).from_address(C.addressof(rec.contents))
        return np.frombuffer(buf, dtype=JST_HIT_DTYPE).copy()

    def copy_to(self, device_ptr: int, cap: int) -> int:
        n = C.c_uint64(0)
        _check(capi.lib().spm_hip_jst_hits_copy_device(self._h, device_ptr, cap, C.byref(n)), self.ctx._h)
        return int(n.value)

    def align(self, begin_only: bool = False) -> "JstAlignments":
        """Begin + CIGAR transcript of every record (spm_hip_jst_hits_align), one alignment per segment hit shared by the
        haplotypes of its context; record i belongs to view() record i.  Needs search_device(..., alignable=True)."""
        _require_open(self, "align", "this search")
        a = self._new("align", capi.ALIGN_BEGIN_ONLY if begin_only else 0)
        return JstAlignments(self.ctx, a, self._jst, self._pats)

    def align_selected(self, begin_only: bool = False) -> "JstAlignments":
        """Begin + CIGAR transcript of the records this SELECTION kept (spm_hip_jst_selection_align): the kept records are
        located in the tree's index, their distinct segment hits aligned once and shared.  Record i of the result's view()
        belongs to view() record i of this selection, and record i of its device() to record i of this selection's
        device(), in (haplotype, pattern, pos) order.  The search need not have been alignable and may be closed; the tree
        and the needle set must be open, and the tree not indexed again since the search."""
        _require_open(self, "align_selected", "this selection")
        a = C.c_void_p()
        _check(capi.lib().spm_hip_jst_selection_align(self._h, capi.ALIGN_BEGIN_ONLY if begin_only else 0, C.byref(a)),
               self.ctx._h)
        return JstAlignments(self.ctx, a, self._jst, self._pats)

    def select(self, loci: bool = True, window: int | None = None, best: int | None = None,
               across: bool = False, strands: bool = False) -> "JstHits":
        """A new, smaller JstHits (spm_hip_jst_hits_select): one record per locus of every haplotype (loci; window=None:
        every needle's own k) and, with best=s, only the records within s errors of the minimum of their (haplotype,
        needle) -- with across=True, of their needle on all haplotypes.  The device view of the result is sorted by
        (haplotype, pattern, pos), its host view as every view(); it stays valid after this object is closed.  align()
        does not take it; align_selected() aligns the records it kept.  strands=True (a set made with both_strands): the
        minimum is taken per READ = pattern >> 1 over both strands."""
        _require_open(self, "select", "these hits", tree=False)
        opts = _select_opts(loci, window, best, across, strands)
        return JstHits(self.ctx, self._new("select", C.byref(opts)), self._jst, self._pats)

    def select_stats(self) -> capi.SelectStats:
        return self._stats(capi.SelectStats, "select_stats")


def select_jst_records(ctx: Context, device_ptr: int, n: int, pats: PatternSet | None = None, *, loci: bool = True,
                       window: int | None = None, best: int | None = None, across: bool = False,
                       strands: bool = False) -> JstHits:
    """JstHits.select() on a device buffer of n JST_HIT_DTYPE records that no JstHits owns -- what a gatherv of the block
    shards delivers on the root (spm_hip_jst_records_select).  pats may be None when window is explicit."""
    opts = _select_opts(loci, window, best, across, strands)
    h = C.c_void_p()
    _check(capi.lib().spm_hip_jst_records_select(ctx._h, C.c_void_p(device_ptr), n, pats._h if pats is not None else None,
                                                 C.byref(opts), C.byref(h)), ctx._h)
    return JstHits(ctx, h, None, pats)


class JstAlignments(_RecordPool):
    """Result of JstHits.align(): JST_ALN_DTYPE records in the order of JstHits.view(), and the pool of CIGAR words
    (len << 4 | op) they point into -- one transcript per segment hit, shared by the haplotypes of its context."""
    _PREFIX, _REC, _DTYPE = "jst_alns", capi.JstAln, JST_ALN_DTYPE

    def __init__(self, ctx, h, jst=None, pats=None):
        # the tree and the needle set behind these alignments: project() reads both
        super().__init__(ctx, h)
        self._jst, self._pats = jst, pats

    def device(self):
        """(records, n, ops, n_ops): device pointers.  From JstHits.align(): records in the arrival order of the alignment
        fan-out.  From JstHits.align_selected(): record i matched to record i of the selection's device()."""
        return self._device()

    def cigar(self, i: int, records: np.ndarray | None = None, ops: np.ndarray | None = None) -> str:
        """SAM string of record i (records / ops: views already fetched, to save the copies)."""
        return self._cigar(i, records, ops)

    def stats(self) -> capi.JstAlignStats:
        return self._stats(capi.JstAlignStats)

    def project(self) -> "JstRefAlignments":
        """These alignments in REFERENCE coordinates (spm_hip_jst_alns_project): ref_begin, ref_end, ref_score and a
        transcript against the reference, computed once per shared transcript slot.  Record i of the result's view()
        belongs to view() record i, record i of its device() to device() record i.  Not for begin_only alignments; the
        tree and the needle set must be open, and the tree not indexed again since the search."""
        _require_open(self, "project", "these alignments")
        return JstRefAlignments(self.ctx, self._new("project", 0), self._jst, self._pats)


class JstRefAlignments(_RecordPool):
    """Result of JstAlignments.project(): JST_REF_ALN_DTYPE records matched to the source's records, and the pool of CIGAR
    words (len << 4 | op) against the reference -- one transcript per distinct transcript slot of the source."""
    _PREFIX, _REC, _DTYPE = "jst_ref_alns", capi.JstRefAln, JST_REF_ALN_DTYPE

    def __init__(self, ctx, h, jst=None, pats=None):
        # the tree and the needle set behind these records: normalize() reads the reference text and the needles
        super().__init__(ctx, h)
        self._jst, self._pats = jst, pats

    def device(self):
        """(records, n, ops, n_ops): device pointers; record i matched to record i of the source's device()."""
        return self._device()

    def cigar(self, i: int, records: np.ndarray | None = None, ops: np.ndarray | None = None) -> str:
        """SAM string of record i (records / ops: views already fetched, to save the copies)."""
        return self._cigar(i, records, ops)

    def stats(self) -> capi.JstProjectStats:
        return self._stats(capi.JstProjectStats)

    def normalize(self) -> "JstRefAlignments":
        """These records with every indel at its leftmost equivalent place (spm_hip_jst_ref_alns_normalize): the same
        records in the same order, every field but cigar_off / cigar_len unchanged, one transcript per distinct slot.
        collapse() of the result merges the haplotypes that differ only in which copy of a repeat an indel touches.  The
        tree and the needle set must be open during the call (the tree may have been indexed again); the result stays
        valid after they and this object are closed."""
        _require_open(self, "normalize", "these alignments")
        return JstRefAlignments(self.ctx, self._new("normalize", 0), self._jst, self._pats)

    def normalize_stats(self) -> capi.JstNormalizeStats:
        """Stage times and counts of the normalize() call that made this object (an error for any other)."""
        return self._stats(capi.JstNormalizeStats, "normalize_stats")

    def collapse(self) -> "JstRefLoci":
        """One record per distinct reference alignment (spm_hip_jst_ref_alns_collapse): records that agree in needle,
        reference range and transcript are merged; the result carries the haplotypes that support each locus and their
        haplotype distances.  Reads only these records and their pool: tree and needle set may be closed, and the result
        stays valid after this object is closed."""
        return JstRefLoci(self.ctx, self._new("collapse", 0))


def _or_null(obj):
    """the handle of an optional argument"""
    return obj._h if obj is not None else None


class JstRefLoci(_RecordPool):
    """Result of JstRefAlignments.collapse(): JST_REF_LOCUS_DTYPE records in (pattern, ref_begin, ref_end, ref_score,
    cigar_len, transcript words) order, one transcript per locus in `ops`, and per locus the distinct haplotypes that
    support it (`members`, ascending) with the smallest haplotype distance each has there (`member_scores`)."""
    _PREFIX, _REC, _DTYPE = "jst_ref_loci", capi.JstRefLocus, JST_REF_LOCUS_DTYPE

    def _raw(self):
        rec = C.POINTER(capi.JstRefLocus)()
        ops, mem = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        msc = C.POINTER(C.c_int32)()
        n, n_ops, n_mem = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("view", C.byref(rec), C.byref(n), C.byref(ops), C.byref(n_ops), C.byref(mem), C.byref(msc), C.byref(n_mem))
        return rec, n.value, ops, n_ops.value, mem, msc, n_mem.value

    @property
    def members(self) -> np.ndarray:
        r = self._raw()
        return _as_array(r[4], r[6], C.c_uint32, np.uint32)

    @property
    def member_scores(self) -> np.ndarray:
        r = self._raw()
        return _as_array(r[5], r[6], C.c_int32, np.int32)

    @property
    def locus_of(self) -> np.ndarray:
        """locus_of[i]: the locus of record i of the source's view()"""
        m = C.POINTER(C.c_uint32)()
        n = C.c_uint64()
        self._call("map", C.byref(m), None, C.byref(n))
        return _as_array(m, n.value, C.c_uint32, np.uint32)

    def cigar(self, i: int, records: np.ndarray | None = None, ops: np.ndarray | None = None) -> str:
        """SAM string of locus i (records / ops: views already fetched, to save the copies)."""
        return self._cigar(i, records, ops)

    def haplotypes(self, i: int, records: np.ndarray | None = None):
        """(haplotypes, scores) of locus i"""
        r = (self.view() if records is None else records)[i]
        lo, hi = int(r["member_off"]), int(r["member_off"]) + int(r["n_haplotypes"])
        return self.members[lo:hi], self.member_scores[lo:hi]

    def device(self):
        """dict of device pointers and counts: records, n, ops, n_ops, members, member_scores, n_members, and locus_of
        (matched to the source's device() records) with n_alns."""
        r, o, m, s, mp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, n_ops, n_mem, n_alns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("device", C.byref(r), C.byref(n), C.byref(o), C.byref(n_ops), C.byref(m), C.byref(s), C.byref(n_mem))
        self._call("map", None, C.byref(mp), C.byref(n_alns))
        return {"records": int(r.value or 0), "n": int(n.value), "ops": int(o.value or 0), "n_ops": int(n_ops.value),
                "members": int(m.value or 0), "member_scores": int(s.value or 0), "n_members": int(n_mem.value),
                "locus_of": int(mp.value or 0), "n_alns": int(n_alns.value)}

    def stats(self) -> capi.JstCollapseStats:
        return self._stats(capi.JstCollapseStats)

    def reads(self, n_reads: int, strands: int = 1) -> "JstReads":
        """One JST_READ_DTYPE record per read 0 .. n_reads - 1 (spm_hip_jst_ref_loci_reads): where its loci stand, how many
        it has on which strand, its primary locus -- the smallest (score, locus index) -- and how many loci share the best
        and the next stratum.  strands=2: the loci stem from a set made with both_strands (read = pattern >> 1).  The result
        stays valid after this object is closed."""
        return JstReads(self.ctx, self._new("reads", strands, n_reads, 0))

    def pairs(self, reads: "JstReads", min_tlen: int, max_tlen: int) -> "JstPairs":
        """One JST_PAIR_DTYPE record per pair of mates -- reads 2p and 2p + 1 of `reads`, this object's reads(n, strands=2)
        (spm_hip_jst_ref_loci_pairs): the best concordant combination of a forward locus of one mate and a reverse locus
        of the other with min_tlen <= fragment length <= max_tlen, how many there are, the SAM TLEN and FLAGs; without one,
        the mates' own primaries.  The result stays valid after this object and `reads` are closed."""
        opts = capi.JstPairOpts(min_tlen=int(min_tlen), max_tlen=int(max_tlen), flags=0, reserved=0)
        return JstPairs(self.ctx, self._new("pairs", reads._h, C.byref(opts)))

    def sam(self, reads: "JstReads", patterns: "PatternSet", rname: str, *, pairs: "JstPairs | None" = None,
            rescues: "JstRescues | None" = None, names=None, symbols: str = "ACGT", cigar_m: bool = False, secondary: bool = False,
            mapq_unique=None, mapq_multi=None) -> "Sam":
        """SAM lines of these loci (spm_hip_jst_ref_loci_sam), written on the device: per read its reported line and, with
        secondary, one line per other locus.  reads: this object's reads(); patterns: the needle set behind the loci; pairs
        (and rescues): paired-end mode, reads 2p and 2p + 1 are mates.  names: one per read (paired: per pair), str or bytes;
        None prints the index.  mapq_unique / mapq_multi: four values each; None (both): the default tables.  The result
        stays valid after every input is closed.  (With base qualities and the MD tag: sam_ex.)"""
        return self.sam_ex(reads, patterns, rname, pairs=pairs, rescues=rescues, names=names, symbols=symbols, cigar_m=cigar_m,
                           secondary=secondary, mapq_unique=mapq_unique, mapq_multi=mapq_multi)

    def sam_ex(self, reads: "JstReads", patterns: "PatternSet", rname: str, *, qualities=None, md: bool = False,
               reference: "Text | None" = None, pairs: "JstPairs | None" = None, rescues: "JstRescues | None" = None, names=None,
               symbols: str = "ACGT", cigar_m: bool = False, secondary: bool = False, mapq_unique=None, mapq_multi=None) -> "Sam":
        """sam() with base qualities and the MD tag (spm_hip_jst_ref_loci_sam_ex).  qualities: Phred values 0 .. 93 as sequenced,
        a 2-D uint8 array with one row per read or a sequence of arrays, printed as QUAL (back to front on a reverse line);
        md with reference, the resident ranks the loci were projected against: an MD:Z: tag behind NM on every line with a
        CIGAR.  With none of the three: the bytes of sam()."""
        opts = sam_opts(rname, symbols, cigar_m=cigar_m, secondary=secondary, mapq_unique=mapq_unique, mapq_multi=mapq_multi)
        keep = _set_names(opts, names)
        extras, keep_q = sam_extras(qualities, md, reference)
        s = self._new("sam_ex", reads._h, _or_null(pairs), _or_null(rescues), patterns._h, C.byref(opts), _ref_or_null(extras))
        del keep, keep_q
        return Sam(self.ctx, s, rname)

    def bam(self, reads: "JstReads", patterns: "PatternSet", rname: str, ref_len: int, *, pairs: "JstPairs | None" = None,
            rescues: "JstRescues | None" = None, names=None, symbols: str = "ACGT", cigar_m: bool = False, secondary: bool = False,
            mapq_unique=None, mapq_multi=None, block_data: int = 0) -> "Bam":
        """The alignments of sam() as a complete BAM file in device memory (spm_hip_jst_ref_loci_bam): header, records in BGZF
        blocks of block_data uncompressed bytes (0: 65280; stored, nothing is compressed), EOF block.  ref_len: the length of
        the reference, 1 .. 2^31 - 1.  Every other argument as for sam().  The result stays valid after every input is closed.
        (With base qualities and the MD tag: bam_ex.)"""
        return self.bam_ex(reads, patterns, rname, ref_len, pairs=pairs, rescues=rescues, names=names, symbols=symbols, cigar_m=cigar_m,
                           secondary=secondary, mapq_unique=mapq_unique, mapq_multi=mapq_multi, block_data=block_data)

    def bam_ex(self, reads: "JstReads", patterns: "PatternSet", rname: str, ref_len: int, *, qualities=None, md: bool = False,
               reference: "Text | None" = None, pairs: "JstPairs | None" = None, rescues: "JstRescues | None" = None, names=None,
               symbols: str = "ACGT", cigar_m: bool = False, secondary: bool = False, mapq_unique=None, mapq_multi=None,
               block_data: int = 0) -> "Bam":
        """bam() with base qualities and the MD tag (spm_hip_jst_ref_loci_bam_ex): qualities, md and reference as for sam_ex();
        the reference has ref_len symbols."""
        opts = capi.BamOpts(sam=sam_opts(rname, symbols, cigar_m=cigar_m, secondary=secondary, mapq_unique=mapq_unique,
                                         mapq_multi=mapq_multi), ref_len=int(ref_len), block_data=int(block_data), reserved=0)
        keep = _set_names(opts.sam, names)
        extras, keep_q = sam_extras(qualities, md, reference)
        b = self._new("bam_ex", reads._h, _or_null(pairs), _or_null(rescues), patterns._h, C.byref(opts), _ref_or_null(extras))
        del keep, keep_q
        return Bam(self.ctx, b, _block_data(block_data))


def _ref_or_null(struct):
    """an optional struct argument by reference"""
    return C.byref(struct) if struct is not None else None


def sam_extras(qualities=None, md: bool = False, reference: "Text | None" = None):
    """spm_sam_extras of JstRefLoci.sam() / bam() -> (the struct, or None when nothing is asked for; what has to stay alive
    across the call).  qualities: a 2-D uint8 array, one row per read, or a sequence of arrays, back to back in read order."""
    if qualities is None and not md and reference is None:
        return None, None
    cat = None
    if qualities is not None:
        if isinstance(qualities, np.ndarray) and qualities.ndim == 2:
            cat = np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
        else:
            rows = [np.ascontiguousarray(q, dtype=np.uint8).reshape(-1) for q in qualities]
            cat = np.concatenate(rows) if rows else np.zeros(0, np.uint8)
    extras = capi.SamExtras(qual=cat.ctypes.data if cat is not None and cat.size else None, n_qual=cat.size if cat is not None else 0,
                            reference=_or_null(reference), flags=capi.SAM_MD if md else 0, reserved=0)
    return extras, cat


def sam_md(words, ref_ranks, ref_begin: int, symbols: str = "ACGT") -> str:
    """The MD string of one transcript (words: len << 4 | op) whose first reference position is ref_begin, by the serial host
    rendering of the device's rule (spm_hip_sam_md).  Needs no device."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    ref = np.ascontiguousarray(ref_ranks, dtype=np.uint8)
    sym = symbols.encode() if isinstance(symbols, str) else bytes(symbols)
    wp = w.ctypes.data_as(C.POINTER(C.c_uint32)) if w.size else None
    rp = (ref if ref.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8))

    def refuse(rc):
        raise capi.SpmError(f"libspm_hip error {rc}: spm_hip_sam_md: the transcript leaves the reference [0, {ref.size})")

    return _size_then_fill(lambda buf, cap, need: capi.lib().spm_hip_sam_md(wp, w.size, rp, ref.size, int(ref_begin), sym, buf, cap, need),
                           refuse).decode()


def _set_names(opts: "capi.SamOpts", names):
    """names (str or bytes, or None) into opts -> what has to stay alive across the call"""
    if names is None:
        return None
    raw = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in raw], dtype=np.uint64)
    blob = C.create_string_buffer(b"".join(raw), int(off[-1]) + 1)
    opts.names, opts.name_off, opts.n_names = C.addressof(blob), off.ctypes.data, len(raw)
    return blob, off


def sam_opts(rname, symbols: str = "ACGT", *, cigar_m: bool = False, secondary: bool = False, mapq_unique=None,
             mapq_multi=None) -> capi.SamOpts:
    """spm_sam_opts without names.  mapq_unique, mapq_multi: both None for the default tables, else both given."""
    if (mapq_unique is None) != (mapq_multi is None):
        raise ValueError("mapq_unique and mapq_multi: give both tables or neither")
    enc = lambda x: x.encode() if isinstance(x, str) else bytes(x)
    opts = capi.SamOpts(rname=enc(rname), symbols=enc(symbols), n_names=0, mapq_defaults=1 if mapq_unique is None else 0,
                        flags=(capi.SAM_CIGAR_M if cigar_m else 0) | (capi.SAM_SECONDARY if secondary else 0), reserved=0)
    if mapq_unique is not None:
        opts.mapq_unique = (C.c_uint8 * 4)(*[int(x) for x in mapq_unique])
        opts.mapq_multi = (C.c_uint8 * 4)(*[int(x) for x in mapq_multi])
    return opts


def sam_mapq(n_best: int, n_next: int, mapq_unique=None, mapq_multi=None) -> int:
    """The MAPQ of (n_best, n_next) under the given tables (None: the defaults).  Needs no device."""
    opts = sam_opts("x", mapq_unique=mapq_unique, mapq_multi=mapq_multi)
    return int(capi.lib().spm_hip_sam_mapq(C.byref(opts), min(int(n_best), 0xFFFFFFFF), min(int(n_next), 0xFFFFFFFF)))


def sam_header(rname, ref_len: int, sorted: bool = False) -> bytes:
    """The @HD and @SQ lines (spm_hip_sam_header; sorted: spm_hip_sam_header_sorted, SO:coordinate).  Needs no device."""
    rname = rname.encode() if isinstance(rname, str) else bytes(rname)
    call = capi.lib().spm_hip_sam_header_sorted if sorted else capi.lib().spm_hip_sam_header

    def refuse(rc):
        raise capi.SpmError(f"libspm_hip error {rc}: spm_hip_sam_header refused rname {rname!r}")

    return _size_then_fill(lambda buf, cap, need: call(rname, int(ref_len), buf, cap, need), refuse)


class Sam(_Handle):
    """Result of JstRefLoci.sam(): the SAM text and one SAM_LINE_DTYPE record per line, in line order."""
    _PREFIX = "sam"

    def __init__(self, ctx, h, rname):
        super().__init__(ctx, h)
        self.rname = rname

    def _view(self):
        t, rec = C.c_void_p(), C.POINTER(capi.SamLine)()
        nb, nl = C.c_uint64(), C.c_uint64()
        self._call("view", C.byref(t), C.byref(nb), C.byref(rec), C.byref(nl))
        return t, nb.value, rec, nl.value

    def __len__(self):
        return self.device()[3]

    def text(self) -> bytes:
        t, nb, _rec, _nl = self._view()
        return C.string_at(t, nb) if nb else b""

    def lines(self) -> np.ndarray:
        _t, _nb, rec, nl = self._view()
        return _as_array(rec, nl, capi.SamLine, SAM_LINE_DTYPE)

    def device(self):
        """(text, n_bytes, lines, n_lines): device pointers and counts"""
        t, rec = C.c_void_p(), C.c_void_p()
        nb, nl = C.c_uint64(), C.c_uint64()
        self._call("device", C.byref(t), C.byref(nb), C.byref(rec), C.byref(nl))
        return int(t.value or 0), int(nb.value), int(rec.value or 0), int(nl.value)

    def stats(self) -> capi.SamStats:
        return self._stats(capi.SamStats)

    def header(self, ref_len: int) -> bytes:
        return sam_header(self.rname, ref_len)

    def _bgzf(self, frame, frame_host, ref_len, block_data, eof, **how) -> "Bgzf":
        text, n_bytes, _lines, _n = self.device()
        z = frame(text, n_bytes, block_data=block_data, eof=eof, **how)
        if ref_len is not None:
            z.prefix = frame_host(self.header(ref_len), block_data, eof=False, **how)
        return z

    def bgzf(self, ref_len: int | None = None, *, block_data: int = 0, eof: bool = True) -> "Bgzf":
        """The text, framed where it lies in device memory (Context.bgzf).  With ref_len the header is framed on the host, as
        blocks of its own in front: bytes() is a .sam.gz."""
        return self._bgzf(self.ctx.bgzf, bgzf_frame_host, ref_len, block_data, eof)

    def bgzf_deflate(self, ref_len: int | None = None, *, block_data: int = 0, eof: bool = True, dynamic: bool = False) -> "Bgzf":
        """bgzf() with the blocks compressed (Context.bgzf_deflate); the header's blocks come from the host deflater."""
        return self._bgzf(self.ctx.bgzf_deflate, bgzf_deflate_host, ref_len, block_data, eof, dynamic=dynamic)


def bam_header(rname, ref_len: int, block_data: int = 0, sorted: bool = False) -> bytes:
    """The framed header section of a BAM file (spm_hip_bam_header; sorted: spm_hip_bam_header_sorted).  Needs no device."""
    rname = rname.encode() if isinstance(rname, str) else bytes(rname)
    call = capi.lib().spm_hip_bam_header_sorted if sorted else capi.lib().spm_hip_bam_header
    return _size_then_fill(lambda buf, cap, need: call(rname, int(ref_len), int(block_data), buf, cap, need),
                           lambda rc: _check(rc if rc else -1, None))


def bai_build_host(records, lines, block_offsets, block_data: int = 0) -> bytes:
    """The BAI index of a coordinate-sorted record stream by the serial host builder (spm_hip_bai_build_host): records the
    uncompressed stream, lines its SAM_LINE_DTYPE records, block_offsets the n_blocks + 1 file offsets of its blocks of
    block_data uncompressed bytes (0: 65280).  Needs no device."""
    records = bytes(records)
    lines = np.ascontiguousarray(lines, dtype=SAM_LINE_DTYPE)
    offs = np.ascontiguousarray(block_offsets, dtype=np.uint64)
    src = C.create_string_buffer(records, len(records) + 1)
    return _size_then_fill(lambda dst, cap, need: capi.lib().spm_hip_bai_build_host(
        src, len(records), lines.ctypes.data, len(lines), offs.ctypes.data, max(len(offs), 1) - 1, int(block_data), dst, cap, need))


def bam_markdup_opts(min_qual: int = 0) -> capi.BamMarkdupOpts:
    return capi.BamMarkdupOpts(min_qual=int(min_qual), flags=0, reserved=0)


def bam_markdup_host(records, lines, ref_len: int, min_qual: int = 0) -> np.ndarray:
    """dup[i] = 1 where record i is a duplicate, by the serial host builder (spm_hip_bam_markdup_host): records the uncompressed
    stream, lines its SAM_LINE_DTYPE records.  Needs no device."""
    records = bytes(records)
    lines = np.ascontiguousarray(lines, dtype=SAM_LINE_DTYPE)
    src = C.create_string_buffer(records, len(records) + 1)
    dup = np.zeros(len(lines), dtype=np.uint8)
    opts = bam_markdup_opts(min_qual)
    _check(capi.lib().spm_hip_bam_markdup_host(src, len(records), lines.ctypes.data, len(lines), int(ref_len), C.byref(opts),
                                               dup.ctypes.data), None)
    return dup


def pileup_opts(begin: int = 0, end=None, min_mapq: int = 0, min_baseq: int = 0, exclude_flags=None) -> capi.PileupOpts:
    """end None (or 0): the reference's length; exclude_flags None (or 0): 0x704, and 0x4 is always excluded"""
    return capi.PileupOpts(begin=int(begin), end=int(end or 0), exclude_flags=int(exclude_flags or 0), min_mapq=int(min_mapq),
                           min_baseq=int(min_baseq), reserved0=0, flags=0, reserved1=0)


def pileup_site_opts(min_depth: int = 1, min_alt: int = 2, min_alt_permille: int = 200) -> capi.PileupSiteOpts:
    return capi.PileupSiteOpts(min_depth=int(min_depth), min_alt=int(min_alt), min_alt_permille=int(min_alt_permille), flags=0)


def bam_pileup_host(records, lines, ref_len: int, begin: int = 0, end=None, min_mapq: int = 0, min_baseq: int = 0,
                    exclude_flags=None) -> np.ndarray:
    """The (8, end - begin) uint32 counts of a coordinate-sorted record stream by the serial host builder
    (spm_hip_bam_pileup_host), the planes in the order PILEUP_PLANES: records the uncompressed stream, lines its SAM_LINE_DTYPE
    records.  Needs no device."""
    records = bytes(records)
    lines = np.ascontiguousarray(lines, dtype=SAM_LINE_DTYPE)
    src = C.create_string_buffer(records, len(records) + 1)
    opts = pileup_opts(begin, end, min_mapq, min_baseq, exclude_flags)
    n = max((int(end) if end else int(ref_len)) - int(begin), 0)
    counts = np.zeros((len(PILEUP_PLANES), n), dtype=np.uint32)
    _check(capi.lib().spm_hip_bam_pileup_host(src, len(records), lines.ctypes.data, len(lines), int(ref_len), C.byref(opts),
                                              counts.ctypes.data), None)
    return counts


def pileup_sites_host(counts, begin: int, ref_ranks, min_depth: int = 1, min_alt: int = 2, min_alt_permille: int = 200) -> np.ndarray:
    """The PILEUP_SITE_DTYPE records of an (8, n) pileup that begins at `begin`, against the ranks of the whole reference, by the
    serial host builder (spm_hip_pileup_sites_host).  Needs no device."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    ref = np.ascontiguousarray(ref_ranks, dtype=np.uint8)
    assert counts.ndim == 2 and counts.shape[0] == len(PILEUP_PLANES)
    n = counts.shape[1]
    opts, need = pileup_site_opts(min_depth, min_alt, min_alt_permille), C.c_uint64()
    out = np.zeros(n, dtype=PILEUP_SITE_DTYPE)
    _check(capi.lib().spm_hip_pileup_sites_host(counts.ctypes.data, int(begin), n, ref.ctypes.data, len(ref), C.byref(opts),
                                                out.ctypes.data, n, C.byref(need)), None)
    return out[:need.value].copy()


class Pileup(_Handle):
    """Result of Bam.pileup() and Context.bam_pileup(): the eight count planes of a region in device memory, plane-major.  (Made by
    those two calls only, so the package does not export the name; it is libspm_amd.engine.Pileup.)"""
    _PREFIX = "pileup"

    def __init__(self, ctx, h, begin: int = 0):
        super().__init__(ctx, h)
        self.begin = begin

    def __len__(self):
        return self.device()[1]

    def counts(self) -> np.ndarray:
        """(8, n) uint32, the planes in the order PILEUP_PLANES; column j is reference position begin + j"""
        p, n = self._span("view")
        if n == 0:
            return np.zeros((len(PILEUP_PLANES), 0), dtype=np.uint32)
        buf = (C.c_uint32 * (len(PILEUP_PLANES) * n)).from_address(p)
        return np.frombuffer(buf, dtype=np.uint32).reshape(len(PILEUP_PLANES), n).copy()

    def depth(self) -> np.ndarray:
        """A + C + G + T + N + DEL per position"""
        return self.counts()[:6].sum(axis=0, dtype=np.uint32)

    def device(self):
        """(counts, n_positions): device pointer and count"""
        return self._span("device")

    def stats(self) -> capi.PileupStats:
        return self._stats(capi.PileupStats)

    def sites(self, reference: "Text", min_depth: int = 1, min_alt: int = 2, min_alt_permille: int = 200) -> np.ndarray:
        """The columns that depart from the resident reference (spm_hip_pileup_sites; the rule is in spm_hip.h), in position
        order, as PILEUP_SITE_DTYPE records.  reference: the dna4 Text of ranks that sam_extras takes."""
        s = self.site_records(reference, min_depth, min_alt, min_alt_permille)
        try:
            return s.view()
        finally:
            s.close()

    def site_records(self, reference: "Text", min_depth: int = 1, min_alt: int = 2, min_alt_permille: int = 200) -> "PileupSites":
        """sites() as an object that keeps the records in device memory: .view() is what sites() returns, .vcf() genotypes them"""
        opts = pileup_site_opts(min_depth, min_alt, min_alt_permille)
        return PileupSites(self.ctx, self._new("sites", reference._h, C.byref(opts)))


class PileupSites(_Handle):
    """Result of Pileup.site_records(): the site records of a pileup in device memory, in position order.  (Made by that call
    only, so the package does not export the name; it is libspm_amd.engine.PileupSites.)"""
    _PREFIX = "pileup_sites"

    def __len__(self):
        return self.device()[1]

    def view(self) -> np.ndarray:
        rec, n = C.POINTER(capi.PileupSite)(), C.c_uint64()
        self._call("view", C.byref(rec), C.byref(n))
        return _as_array(rec, n.value, capi.PileupSite, PILEUP_SITE_DTYPE)

    def device(self):
        """(sites, n): device pointer and count"""
        return self._span("device")

    def vcf(self, rname, sample, ref_len: int, **opts) -> "Vcf":
        """Genotype calls for these sites and the VCF text of the variant ones, on the device (spm_hip_pileup_sites_vcf; the rule
        is in spm_hip.h): one sample, SNV alleles.  opts: vcf_opts' (ploidy, the three costs, the two priors, min_qual)."""
        o = vcf_opts(**opts)
        return Vcf(self.ctx, self._new("vcf", _name(rname), _name(sample), int(ref_len), C.byref(o)))


_PileupSites = PileupSites


def _name(s) -> bytes:
    return s.encode() if isinstance(s, str) else bytes(s)


def vcf_opts(ploidy: int = 2, cost_match: int = 0, cost_het: int = 0, cost_miss: int = 0, prior_het: int = 0, prior_hom_alt: int = 0,
             min_qual: int = 20) -> capi.VcfOpts:
    """the three costs all 0: 44, 3039, 24771; the two priors both 0: 30000, 33010 (milli-Phred); min_qual in Phred, as given"""
    return capi.VcfOpts(ploidy=int(ploidy), cost_match=int(cost_match), cost_het=int(cost_het), cost_miss=int(cost_miss),
                        prior_het=int(prior_het), prior_hom_alt=int(prior_hom_alt), min_qual=int(min_qual), flags=0, reserved0=0,
                        reserved1=0)


def vcf_header(rname, sample, ref_len: int) -> bytes:
    """The meta lines and the #CHROM line of the files Vcf.text() gives (spm_hip_vcf_header).  Needs no device."""
    rname, sample = _name(rname), _name(sample)
    return _size_then_fill(lambda buf, cap, need: capi.lib().spm_hip_vcf_header(rname, sample, int(ref_len), buf, cap, need))


def pileup_sites_calls_host(sites, **opts) -> np.ndarray:
    """The VARIANT_CALL_DTYPE records of PILEUP_SITE_DTYPE records by the serial host builder (spm_hip_pileup_sites_calls_host);
    offset and len stay 0, they belong to a text.  opts: vcf_opts'.  Needs no device."""
    sites = np.ascontiguousarray(sites, dtype=PILEUP_SITE_DTYPE)
    o, calls = vcf_opts(**opts), np.zeros(len(sites), dtype=VARIANT_CALL_DTYPE)
    _check(capi.lib().spm_hip_pileup_sites_calls_host(sites.ctypes.data, len(sites), C.byref(o), calls.ctypes.data), None)
    return calls


def pileup_sites_vcf_host(sites, rname, sample, ref_len: int, **opts) -> bytes:
    """The VCF file of PILEUP_SITE_DTYPE records by the serial host builder (spm_hip_pileup_sites_vcf_host): the bytes of
    Vcf.text().  opts: vcf_opts'.  Needs no device."""
    sites = np.ascontiguousarray(sites, dtype=PILEUP_SITE_DTYPE)
    o, rname, sample = vcf_opts(**opts), _name(rname), _name(sample)
    return _size_then_fill(lambda buf, cap, need: capi.lib().spm_hip_pileup_sites_vcf_host(
        sites.ctypes.data, len(sites), rname, sample, int(ref_len), C.byref(o), buf, cap, need))


class Vcf(_Handle):
    """Result of PileupSites.vcf() and Context.pileup_sites_vcf(): a VCF file and one VARIANT_CALL_DTYPE record per site, in
    device memory.  (Made by those two calls only, so the package does not export the name; it is libspm_amd.engine.Vcf.)"""
    _PREFIX = "vcf"

    def _view(self):
        t, rec = C.c_void_p(), C.POINTER(capi.VariantCall)()
        nb, nc = C.c_uint64(), C.c_uint64()
        self._call("view", C.byref(t), C.byref(nb), C.byref(rec), C.byref(nc))
        return t, nb.value, rec, nc.value

    def __len__(self):
        return self.device()[3]

    def text(self) -> bytes:
        """the file: header, then one line per site whose best genotype is not ref/ref"""
        t, nb, _rec, _nc = self._view()
        return C.string_at(t, nb) if nb else b""

    def calls(self) -> np.ndarray:
        """one record per site; text()[offset:offset + len] is the site's line"""
        _t, _nb, rec, nc = self._view()
        return _as_array(rec, nc, capi.VariantCall, VARIANT_CALL_DTYPE)

    def device(self):
        """(text, n_bytes, calls, n_calls): device pointers and counts"""
        t, rec = C.c_void_p(), C.c_void_p()
        nb, nc = C.c_uint64(), C.c_uint64()
        self._call("device", C.byref(t), C.byref(nb), C.byref(rec), C.byref(nc))
        return int(t.value or 0), int(nb.value), int(rec.value or 0), int(nc.value)

    def stats(self) -> capi.VcfStats:
        return self._stats(capi.VcfStats)

    def bgzf(self, *, block_data: int = 0, eof: bool = True) -> "Bgzf":
        """The file framed where it lies in device memory (Context.bgzf): bytes() is a .vcf.gz of stored blocks."""
        text, n_bytes, _calls, _n = self.device()
        return self.ctx.bgzf(text, n_bytes, block_data=block_data, eof=eof)

    def bgzf_deflate(self, *, block_data: int = 0, eof: bool = True, dynamic: bool = False) -> "Bgzf":
        """bgzf() with the blocks compressed on the device (Context.bgzf_deflate): bytes() is a .vcf.gz."""
        text, n_bytes, _calls, _n = self.device()
        return self.ctx.bgzf_deflate(text, n_bytes, block_data=block_data, eof=eof, dynamic=dynamic)


class Bam(_Handle):
    """Result of JstRefLoci.bam(): the file, the uncompressed record stream and one SAM_LINE_DTYPE record per BAM record
    (offset / len: the record in the stream), in record order."""
    _PREFIX = "bam"

    def __init__(self, ctx, h, block_data):
        super().__init__(ctx, h)
        self.block_data = block_data

    def _view(self):
        f, r, rec = C.c_void_p(), C.c_void_p(), C.POINTER(capi.SamLine)()
        nf, nr, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("view", C.byref(f), C.byref(nf), C.byref(r), C.byref(nr), C.byref(rec), C.byref(nl))
        return f, nf.value, r, nr.value, rec, nl.value

    def __len__(self):
        return self.device()[5]

    def bytes(self) -> bytes:
        f, nf, _r, _nr, _rec, _nl = self._view()
        return C.string_at(f, nf) if nf else b""

    def records(self) -> bytes:
        _f, _nf, r, nr, _rec, _nl = self._view()
        return C.string_at(r, nr) if nr else b""

    def lines(self) -> np.ndarray:
        _f, _nf, _r, _nr, rec, nl = self._view()
        return _as_array(rec, nl, capi.SamLine, SAM_LINE_DTYPE)

    def voffsets(self) -> np.ndarray:
        """the BGZF virtual file offset of every record"""
        first, block = np.uint64(self.stats().header_file_bytes), np.uint64(self.block_data + 31)  # stored blocks, no gaps
        return _voffsets(self.lines()["offset"], self.block_data, lambda i: first + i * block)

    def deflate(self, block_data: int = 0, eof: bool = True, *, dynamic: bool = False) -> "Bgzf":
        """The file with its blocks compressed (spm_hip_bam_deflate): the header section deflated on the host, the record
        stream on the device where it lies, in blocks of block_data uncompressed bytes.  block_offsets() are the record
        blocks' file offsets; voffsets(self.lines()["offset"]) the records' virtual offsets.  dynamic: as in
        Context.bgzf_deflate, for the header's blocks too."""
        opts = bgzf_deflate_opts(block_data, eof, dynamic=dynamic)
        return Bgzf(self.ctx, self._new("deflate", C.byref(opts)), block_data=_block_data(block_data))

    def sort(self) -> "Bam":
        """A new Bam with these records in coordinate order (spm_hip_bam_sort): reference position, forward before reverse,
        ties in this object's order, records without a position last; the header says SO:coordinate.  What index() takes."""
        opts = capi.BamSortOpts(reserved=0)
        return Bam(self.ctx, self._new("sort", C.byref(opts)), self.block_data)

    def sort_stats(self) -> capi.BamSortStats:
        """the stage times of the sort() that made this object"""
        return self._stats(capi.BamSortStats, "sort_stats")

    def markdup(self, min_qual: int = 0) -> "Bam":
        """A new Bam whose duplicate reads and pairs carry FLAG 0x400 (spm_hip_bam_markdup; the rule is in spm_hip.h): the same
        records in the same order, one bit per record apart.  min_qual: the lowest base quality that counts towards a record's
        score, 0 for 15."""
        opts = bam_markdup_opts(min_qual)
        return Bam(self.ctx, self._new("markdup", C.byref(opts)), self.block_data)

    def markdup_stats(self) -> capi.BamMarkdupStats:
        """the stage times and counts of the markdup() that made this object"""
        return self._stats(capi.BamMarkdupStats, "markdup_stats")

    def pileup(self, begin: int = 0, end=None, min_mapq: int = 0, min_baseq: int = 0, exclude_flags=None) -> "Pileup":
        """The per-base pileup of this coordinate-sorted object over [begin, end) (spm_hip_bam_pileup; the rule is in spm_hip.h):
        how many records show A, C, G, T, another symbol, a deletion, an insertion behind the position or a base below
        min_baseq.  end None: the reference's length.  exclude_flags None: 0x704, so the duplicates markdup() marked stay out;
        0x4 is always excluded.  Records with a MAPQ below min_mapq stay out.  An unsorted object is refused."""
        opts = pileup_opts(begin, end, min_mapq, min_baseq, exclude_flags)
        return Pileup(self.ctx, self._new("pileup", C.byref(opts)), int(begin))

    def index(self, deflated: "Bgzf | None" = None) -> "Bai":
        """The BAI index of this coordinate-sorted file (spm_hip_bam_index), or, with deflated = self.deflate(block_data) in
        blocks of this object's block_data, of that file.  An unsorted object is refused."""
        return Bai(self.ctx, self._new("index", _or_null(deflated)))

    def device(self):
        """(file, n_file, records, n_record_bytes, lines, n_lines): device pointers and counts"""
        f, r, rec = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nf, nr, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("device", C.byref(f), C.byref(nf), C.byref(r), C.byref(nr), C.byref(rec), C.byref(nl))
        return int(f.value or 0), int(nf.value), int(r.value or 0), int(nr.value), int(rec.value or 0), int(nl.value)

    def stats(self) -> capi.BamStats:
        return self._stats(capi.BamStats)


class Bai(_Handle):
    """Result of Bam.index() and Context.bai(): the bytes of a .bai file in device memory.  (Made by those two calls only, so the
    package does not export the name; it is libspm_amd.engine.Bai.)"""
    _PREFIX = "bai"

    def bytes(self) -> bytes:
        p, n = self._span("view")
        return C.string_at(p, n) if n else b""

    def device(self):
        """(bytes, n): device pointer and count"""
        return self._span("device")

    def stats(self) -> capi.BaiStats:
        return self._stats(capi.BaiStats)


def bgzf_opts(block_data: int = 0, eof: bool = True) -> capi.BgzfOpts:
    return capi.BgzfOpts(block_data=int(block_data), flags=capi.BGZF_EOF if eof else 0, reserved=0)


def bgzf_frame_host(data, block_data: int = 0, eof: bool = True) -> bytes:
    """The container of Context.bgzf by the serial host framer (spm_hip_bgzf_frame_host).  Needs no device."""
    data = bytes(data)
    opts = bgzf_opts(block_data, eof)
    src = C.create_string_buffer(data, len(data) + 1)
    # (no data and no end-of-file block: the size call answers 0 with a length of 0, and that is the result)
    return _size_then_fill(lambda dst, cap, need: capi.lib().spm_hip_bgzf_frame_host(src, len(data), C.byref(opts), dst, cap, need))


def bgzf_deflate_opts(block_data: int = 0, eof: bool = True, *, dynamic: bool = False) -> capi.BgzfDeflateOpts:
    flags = (capi.BGZF_EOF if eof else 0) | (capi.BGZF_DYNAMIC if dynamic else 0)
    return capi.BgzfDeflateOpts(block_data=int(block_data), flags=flags, level=1, reserved=0)


def bgzf_deflate_host(data, block_data: int = 0, eof: bool = True, *, dynamic: bool = False) -> bytes:
    """The bytes of Context.bgzf_deflate by the serial host deflater (spm_hip_bgzf_deflate_host).  Needs no device."""
    data = bytes(data)
    opts = bgzf_deflate_opts(block_data, eof, dynamic=dynamic)
    cap = C.c_uint64()
    _check(capi.lib().spm_hip_bgzf_deflate_bound(len(data), C.byref(opts), C.byref(cap)), None)
    src = C.create_string_buffer(data, len(data) + 1)
    dst = C.create_string_buffer(cap.value + 1)
    need = C.c_uint64()
    _check(capi.lib().spm_hip_bgzf_deflate_host(src, len(data), C.byref(opts), dst, cap.value, C.byref(need)), None)
    return dst.raw[:need.value]


class Bgzf(_Handle):
    """Result of Context.bgzf() / Sam.bgzf(), their bgzf_deflate() and Bam.deflate(): BGZF blocks in device memory.  prefix: bytes
    framed on the host that belong in front of them (Sam.bgzf with ref_len: the header's blocks); bytes() has them, device()
    is the device part alone.  block_data: the uncompressed bytes of a full block."""
    _PREFIX = "bgzf"

    def __init__(self, ctx, h, prefix: bytes = b"", block_data: int = capi.BGZF_BLOCK_DATA):
        super().__init__(ctx, h)
        self.prefix, self.block_data = prefix, block_data

    def block_offsets(self) -> np.ndarray:
        """n_blocks + 1 offsets into bytes(): of every data block of the device part, then their end (spm_hip_bgzf_blocks)"""
        p, n = C.POINTER(C.c_uint64)(), C.c_uint64()
        self._call("blocks", C.byref(p), C.byref(n))
        return np.ctypeslib.as_array(p, shape=(n.value + 1,)).astype(np.uint64) + np.uint64(len(self.prefix))

    def block_offsets_device(self):
        """(offsets, n_blocks): the same offsets on the device, without the prefix's length"""
        return self._span("blocks_device")

    def voffsets(self, stream_offsets) -> np.ndarray:
        """the BGZF virtual file offset of the bytes at these offsets of the uncompressed stream"""
        return _voffsets(stream_offsets, self.block_data, lambda i: self.block_offsets()[i.astype(np.int64)])

    def deflate_stats(self) -> capi.BgzfDeflateStats:
        return self._stats(capi.BgzfDeflateStats, "deflate_stats")

    def block_types(self) -> tuple:
        """(stored, fixed, dynamic): how many data blocks of the device part took each form (spm_hip_bgzf_block_types)"""
        n = (C.c_uint64 * 3)()
        self._call("block_types", n)
        return int(n[0]), int(n[1]), int(n[2])

    def bytes(self) -> bytes:
        p, n = self._span("view")
        return self.prefix + (C.string_at(p, n) if n else b"")

    def device(self):
        """(bytes, n): device pointer and count"""
        return self._span("device")

    def stats(self) -> capi.BgzfStats:
        return self._stats(capi.BgzfStats)


class JstReads(_Handle):
    """Result of JstRefLoci.reads(): one JST_READ_DTYPE record per read, in read order, in both views."""
    _PREFIX = "jst_reads"

    def __len__(self):
        return self.device()[1]

    def view(self) -> np.ndarray:
        rec, n = C.POINTER(capi.JstRead)(), C.c_uint64()
        self._call("view", C.byref(rec), C.byref(n))
        return _as_array(rec, n.value, capi.JstRead, JST_READ_DTYPE)

    def device(self):
        """(pointer, count) of the records in HBM"""
        return self._span("device")

    def stats(self) -> capi.JstReadsStats:
        return self._stats(capi.JstReadsStats)


class JstPairs(_Handle):
    """Result of JstRefLoci.pairs(): one JST_PAIR_DTYPE record per pair of mates, in pair order, in both views."""
    _PREFIX = "jst_pairs"

    def __len__(self):
        return self.device()[1]

    def view(self) -> np.ndarray:
        rec, n = C.POINTER(capi.JstPair)(), C.c_uint64()
        self._call("view", C.byref(rec), C.byref(n))
        return _as_array(rec, n.value, capi.JstPair, JST_PAIR_DTYPE)

    def device(self):
        """(pointer, count) of the records in HBM"""
        return self._span("device")

    def stats(self) -> capi.JstPairsStats:
        return self._stats(capi.JstPairsStats)

    def rescue(self, loci: "JstRefLoci", reads: "JstReads", reference: "Text", patterns: "PatternSet", k: int, min_tlen: int,
               max_tlen: int) -> "JstRescues":
        """Mate rescue (spm_hip_jst_pairs_rescue): for every pair here without a proper combination, one job per mapped
        mate -- the other mate, on the opposite strand, searched with at most k edits in the stretch of `reference` the
        fragment bounds allow beside that mate's locus, and aligned as Hits.align() aligns.  loci, reads: what these pairs
        were made from; patterns: the both_strands Myers set behind them.  One JST_RESCUE_DTYPE record per job, ordered by
        (pair, mate rescued).  The result stays valid after every input is closed."""
        opts = capi.JstRescueOpts(min_tlen=int(min_tlen), max_tlen=int(max_tlen), k=int(k), flags=0, reserved=0)
        r = C.c_void_p()
        _check(capi.lib().spm_hip_jst_pairs_rescue(loci._h, reads._h, self._h, reference._h, patterns._h, C.byref(opts),
                                                   C.byref(r)), self.ctx._h)
        return JstRescues(self.ctx, r)


class JstRescues(_RecordPool):
    """Result of JstPairs.rescue(): one JST_RESCUE_DTYPE record per job, ordered by (pair, mate rescued), and the pool of
    CIGAR words (len << 4 | op) the found ones point into."""
    _PREFIX, _REC, _DTYPE = "jst_rescues", capi.JstRescue, JST_RESCUE_DTYPE

    def view(self):
        """(records, ops)"""
        r = self._raw()
        return _as_array(r[0], r[1], self._REC, self._DTYPE), _as_array(r[2], r[3], C.c_uint32, np.uint32)

    def device(self):
        """(records, n, ops, n_ops): device pointers"""
        return self._device()

    def cigar(self, i: int) -> str:
        records, ops = self.view()
        return self._cigar(i, records, ops)

    def stats(self) -> capi.JstRescuesStats:
        return self._stats(capi.JstRescuesStats)
