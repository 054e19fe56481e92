/*
 * spm_hip.h -- C ABI of the MI355X-native online pattern-matching engine (libspm_hip.so).
 *
 * This is the drop-in boundary for libspm's matcher hot path.  The reference has no FFI for this path:
 * its boundary is the header-only C++ template API
 *     spm::{horspool,shiftor,myers,restorable_*}_matcher::operator()(haystack, callback)
 *         /root/reference/libspm/libspm/matcher/seqan_pattern_base.hpp:40-52
 * so the entry points below are what a binding for that call operator needs: build the pattern tables once
 * (the matcher constructors), hand over a haystack of 1-byte ranks, run one scan, read back the hits in the
 * order the callback would have seen them.  include/libspm/ holds the C++ mirror of the reference API that
 * marshals to these calls; INTEGRATION.md shows the binding from the reference side.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every function returns 0 on success and a
 * negative spm_status on failure; spm_hip_last_error() gives the message.  Nothing throws across the ABI.
 * Handles are opaque and owned by the library.  Not thread-safe per context; contexts are independent.
 */
#ifndef SPM_HIP_H
#define SPM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spm_ctx spm_ctx;           /* one device + one HIP stream */
typedef struct spm_text spm_text;         /* haystack resident in HBM, one uint8 rank per symbol */
typedef struct spm_patterns spm_patterns; /* compiled needle set: Peq / mask tables, seed index */
typedef struct spm_hits spm_hits;         /* result of one scan */
typedef struct spm_jst spm_jst;           /* journaled sequence tree: reference + alleles + coverage, resident in HBM */
typedef struct spm_jst_hits spm_jst_hits; /* result of one search over all haplotypes */

enum spm_status {
    SPM_OK = 0,
    SPM_E_INVALID = -1,     /* bad argument */
    SPM_E_HIP = -2,         /* HIP runtime error (message has the hipError string) */
    SPM_E_NOMEM = -3,
    SPM_E_UNSUPPORTED = -4, /* e.g. needle longer than SPM_MAX_NEEDLE */
    SPM_E_OVERFLOW = -5,    /* hit buffer too small; see spm_scan_opts.max_hits */
    SPM_E_PEER = -6         /* multi-GPU exchange: another rank reported an error; nothing was sent or received */
};

/* Which reference matcher a pattern set stands for. */
enum spm_algo {
    SPM_ALGO_SHIFTOR = 0,      /* spm::shiftor_matcher   matcher/shiftor_matcher.hpp:20-41  -> begin positions */
    SPM_ALGO_MYERS = 1,        /* spm::myers_matcher     matcher/myers_matcher.hpp:19-54    -> (end, distance) */
    SPM_ALGO_MYERS_PREFIX = 2, /* spm::restorable_myers_prefix_matcher  matcher/myers_prefix_matcher_restorable.hpp:117-160 */
    SPM_ALGO_HORSPOOL = 3      /* spm::horspool_matcher  matcher/horspool_matcher.hpp:20-41 -> begin positions
                                  (same hit set as Shift-Or: every occurrence) */
};

enum spm_engine {
    SPM_ENGINE_AUTO = 0,  /* seed filter when the pattern set admits one, else brute force */
    SPM_ENGINE_BRUTE = 1, /* one lane per pattern, every text symbol through the recurrence */
    SPM_ENGINE_FILTER = 2 /* lossless pigeonhole seed filter + bit-vector verification */
};

#define SPM_MAX_NEEDLE 2048u

/* One hit record, 16 bytes.  Replaces what the reference's callback reads off the seqan2::Finder:
 *   Myers:  pos = seqan2::endPosition(finder)   (exclusive end; test/api/libspm/matcher/myers_matcher_test.cpp:49-51)
 *           score = edit distance of that end position (the pattern state's `errors`)
 *   exact:  pos = seqan2::beginPosition(finder) (test/api/libspm/matcher/horspool_matcher_test.cpp:48-50), score = 0
 * `pattern` = index into the pattern set.  Positions are relative to text[0] plus spm_scan_opts.pos_offset. */
typedef struct spm_hit {
    uint64_t pos;
    uint32_t pattern;
    int32_t score;
} spm_hit;

typedef struct spm_scan_opts {
    uint32_t engine;       /* spm_engine */
    uint32_t left_context; /* 0: text[begin] is the first symbol of the haystack (cold start, the reference's
                              operator() semantics).  1: the symbols before `begin` belong to the same haystack
                              and may be read as warm-up, so the hits equal those of a scan of the whole text
                              whose last symbol lies in [begin,end) -- the shard rule of SURVEY.md 8(e). */
    uint64_t pos_offset;   /* added to every reported position (global coordinate of text[0]) */
    uint64_t max_hits;     /* capacity of the hit buffer; 0 = library default */
    uint32_t flags;        /* SPM_SCAN_* bits.  (The host view spm_hip_hits_view is always sorted by (pattern, pos);
                              the device view is in arrival order.) */
    uint32_t reserved;
} spm_scan_opts;

#define SPM_SCAN_IGNORE_PACKED 1u /* do not use the text's 2-bit shadow even if it has one */
/* Deferred completion.  spm_hip_scan normally returns when it KNOWS the scan is complete: it reads the device counters
 * back once (one host synchronisation), because a list that proved too small means another attempt.  With this flag a
 * whole (unsegmented), stateless scan through the seed filter returns as soon as its kernels are enqueued; the counters are
 * read at the first accessor that needs the hit count (view, device, copy_device, copy_fused, stats, destroy), and a scan
 * that does need attention -- a list overflowed, a span gave up, or an EARLIER deferred scan left the context's band table
 * in a state this one could not trust -- is repeated there, synchronously, retries and fallbacks included.  The text and
 * the needle set must stay alive until then.  Stateful and segmented scans and the brute-force engine ignore the flag.
 * With spm_hip_hits_copy_fused_device a step of a scan loop has no host synchronisation at all: the GPU never waits for
 * the host between steps (the status word of its header says whether the host has to look). */
#define SPM_SCAN_DEFER 2u
/* Only spm_hip_jst_search looks at this bit (it never reaches a scan): the result keeps the search's segment hits -- the
 * hits in context coordinates, before the fan-out -- until it is destroyed, so that spm_hip_jst_hits_align can align
 * them.  Without it a search holds what it always held and spm_hip_jst_hits_align refuses its hits (a selection of them
 * is aligned by spm_hip_jst_selection_align, which needs no segment hits). */
#define SPM_SCAN_ALIGNABLE 4u

/* Per-scan device timings, HIP events on the context's stream (ms). */
typedef struct spm_scan_stats {
    float ms_total;
    float ms_main;        /* the dominant kernel: brute-force scan, or the seed filter */
    float ms_verify;      /* filter engine: bit-vector verification of the candidates */
    uint32_t engine_used; /* spm_engine actually run */
    uint32_t fell_back;   /* 1 if the filter engine gave up on the WHOLE scan and the brute engine re-ran it (dedupe set or
                             overflow list exhausted, or a segmented scan overflowed); see fallback_spans for the usual,
                             span-local form */
    uint64_t n_candidates;
    uint64_t n_hits;
    uint32_t main_launches;
    uint32_t n_bands;     /* filter engine: what was actually verified -- diagonal bands after candidate merging (sets with
                             k >= 8), else the candidates whose whole seed matches the text */
    uint32_t fallback_spans;   /* filter engine: spans of the text whose seed hits exceeded their budget (repeat-rich
                                  stretches); only those were scanned again by the brute-force kernel */
    uint32_t span_symbols;     /* filter engine: text symbols per span of the streaming launch of the last pass (the unit
                                  the waves draw work in: span borders are where a window's symbols come from two
                                  dequeues); 0 for the brute engine */
    uint64_t fallback_symbols; /* how many text symbols the re-scan of the fallback_spans covered */
} spm_scan_stats;

/* ---- context -------------------------------------------------------------------------------------- */
/* stream: a hipStream_t to run on (e.g. torch's current stream), or NULL to create a private one. */
int spm_hip_init(int device, void *stream, spm_ctx **out);
void spm_hip_destroy(spm_ctx *ctx);
const char *spm_hip_last_error(const spm_ctx *ctx); /* ctx may be NULL: error of the failed spm_hip_init */
int spm_hip_synchronize(spm_ctx *ctx);

/* ---- haystack: replaces spm::make_seqan_container(views::all(haystack)), seqan_pattern_base.hpp:44-45 ----
 * sigma = alphabet size (4 dna4, 5 dna5, 15 dna15; seqan/alphabet.hpp:100-105); symbols are ranks < sigma. */
int spm_hip_text_upload(spm_ctx *ctx, const uint8_t *ranks, uint64_t n, uint32_t sigma, spm_text **out);
/* Borrow a device buffer (16-byte aligned) that the caller keeps alive, e.g. a torch uint8 tensor.  The buffer is read
 * once (at HBM speed) to check that every symbol is a rank < sigma; SPM_E_INVALID otherwise -- the same contract as
 * spm_hip_text_upload.  The caller must not change it while the handle lives. */
int spm_hip_text_wrap(spm_ctx *ctx, const void *device_ranks, uint64_t n, uint32_t sigma, spm_text **out);
/* Synthetic uniform dna4 text generated in HBM: base(i) of SURVEY.md 8(d) for i in [global_begin, +n). */
int spm_hip_text_generate(spm_ctx *ctx, uint64_t seed, uint64_t global_begin, uint64_t n, spm_text **out);
/* Synthetic repeat-rich dna4 text (bench workload c3r): the uniform text above with `repeat_ppm` parts per million of
 * its bases inside tandem-repeat / low-complexity stretches of 16..256 bases (libspm_amd/csrc/synth.hpp says exactly
 * how).  spm_hip_synth_repeat_text regenerates any slice on the host; spm_hip_synth_repeat_pattern cuts needle p from
 * it at a uniformly random position, and every `across_every`-th one (0: none) across a stretch on purpose. */
int spm_hip_text_generate_repeats(spm_ctx *ctx, uint64_t seed, uint64_t global_begin, uint64_t n, uint32_t repeat_ppm,
                                  spm_text **out);
/* Optional: build a 2-bit shadow of a dna4 haystack (16 symbols per uint32, +25 % HBM).  Later seed-filter scans of
 * this text stream the shadow instead of the 1-byte ranks -- a quarter of the HBM traffic -- and return identical hits;
 * verification and the brute-force engine keep reading the original ranks.  Meant for a reference that is scanned
 * against many needle batches.  SPM_E_INVALID if the text holds a symbol >= 4 or is not dna4.
 * spm_scan_opts.flags & SPM_SCAN_IGNORE_PACKED makes a scan read the 1-byte text anyway. */
int spm_hip_text_pack(spm_ctx *ctx, spm_text *text);
int spm_hip_text_is_packed(const spm_text *text);
int spm_hip_text_download(spm_ctx *ctx, const spm_text *text, uint64_t begin, uint64_t n, uint8_t *out);
uint64_t spm_hip_text_length(const spm_text *text);
const void *spm_hip_text_device_ptr(const spm_text *text);
void spm_hip_text_destroy(spm_text *text);

/* ---- needles: replaces the matcher constructors (myers_matcher.hpp:40-43, shiftor_matcher.hpp:38-40,
 * horspool_matcher.hpp:38-40, myers_matcher_restorable.hpp:132).  ranks_concat holds the needles back to back,
 * needle p = ranks_concat[offsets[p] .. offsets[p+1]).  k[p] = max_error_count of needle p (NULL = all 0;
 * ignored by the exact matchers). */
int spm_hip_patterns_create(spm_ctx *ctx, int algo, const uint8_t *ranks_concat, const uint32_t *offsets,
                            uint32_t n_patterns, const uint16_t *k, uint32_t sigma, spm_patterns **out);
void spm_hip_patterns_destroy(spm_patterns *p);
/* spm::window_size (seqan_pattern_base.hpp:97-99, myers_matcher.hpp:51-53): |P| exact, |P|+k Myers, 0 if empty. */
uint64_t spm_hip_patterns_window_size(const spm_patterns *p, uint32_t pattern);
/* 1 if the set admits the lossless seed filter (dna4, every needle long enough for its k). */
int spm_hip_patterns_filterable(const spm_patterns *p);

/* ---- stranded needle sets: n reads searched on both strands ---------------------------------------------------------
 * The arguments of spm_hip_patterns_create, read as n_reads READS.  The result is an ordinary set of 2 * n_reads needles:
 * pattern 2r is read r, pattern 2r + 1 its reverse complement, both with k[r].  The interleaving is the contract --
 * read = pattern >> 1, strand = pattern & 1 -- and every other call (window_size, state blobs, scan, segments, the pan-genome
 * search, align, project, normalise, collapse) sees nothing but 2n needles.  The CIGAR of the reverse-complement needle
 * against the forward text is what SAM stores for a reverse-strand read.
 *   * Complement by rank: dna4 ACGT 3 - r; dna5 ACGNT {4,2,1,3,0}; dna15 ABCDGHKMNRSTVWY {11,12,4,5,2,3,7,6,8,14,10,0,1,13,9}.
 *     A rank >= sigma (it matches nothing) is kept as it is, at its mirrored place.  Any other sigma: SPM_E_UNSUPPORTED.
 *   * 2 * n_reads, or twice the summed lengths, above 2^32 - 1: SPM_E_UNSUPPORTED, decided before any allocation.
 *   * All four algo values are accepted. */
int spm_hip_patterns_create_stranded(spm_ctx *ctx, int algo, const uint8_t *ranks_concat, const uint32_t *offsets,
                                     uint32_t n_reads, const uint16_t *k, uint32_t sigma, spm_patterns **out);
uint32_t spm_hip_patterns_strands(const spm_patterns *p);   /* 1, or 2 for a stranded set */
uint32_t spm_hip_patterns_count(const spm_patterns *p);     /* needles in the set (2 * n_reads when stranded) */
/* The symbols of needle `pattern`, copied from the set's host copy: SAM SEQ of a reverse-strand hit.  Any set.  *len is
 * always written (0 for a pattern outside the set, which is SPM_E_INVALID); cap < *len is SPM_E_INVALID and copies nothing. */
int spm_hip_patterns_needle(const spm_patterns *p, uint32_t pattern, uint8_t *out, uint32_t cap, uint32_t *len);

/* What spm_hip_patterns_create spent where (host wall clock, ms) and what it built.  The reference's constructors are
 * O(|P|) per needle (myers_matcher.hpp:40-43); a set of 100 000 needles is built by `threads` host threads here
 * (SPM_HIP_BUILD_THREADS; default: the hardware concurrency, at most 16). */
typedef struct spm_build_stats {
    float ms_total;
    float ms_tables;  /* match-mask tables of the bit-vector engines */
    float ms_index;   /* seed index of the filter engine */
    float ms_upload;  /* the device allocation + the host-to-device stream of every table (pinned chunks) */
    uint32_t threads;
    uint32_t passes;            /* passes of the seed filter over the text per scan (0: brute-force engine only) */
    uint32_t dense;             /* 1: the one dense pass (presence bits in LDS + fingerprint buckets in L2) */
    uint32_t anchor_sixteenths; /* sixteenths of all text windows that are looked up, summed over the passes */
    uint64_t keys;              /* indexed windows */
    uint32_t stride, key_len;
    uint64_t bytes_device;      /* the set's one device allocation (every table, 256-byte aligned) */
} spm_build_stats;
int spm_hip_patterns_build_stats(const spm_patterns *p, spm_build_stats *out);

/* ---- matcher state: replaces capture()/restore() (myers_matcher_restorable.hpp:57-63,136-142;
 * shiftor_matcher_restorable.hpp:44-50).  A state blob holds one record per pattern, each
 * spm_hip_patterns_state_stride() bytes:
 *   Myers:    int32 score; uint32 n_words; uint64 vp[n_words]; uint64 vn[n_words]
 *   Shift-Or: uint32 n_words; uint32 pad;  uint32 r[n_words]   (stride rounded up to a multiple of 8 bytes)
 * n_words is set-wide, the same in every record: ceil(max|P| / 64) Myers, ceil(max|P| / 32) Shift-Or, max over the set.
 * Bit j of vp / vn / r is row j of the needle.  Myers: the DP column after the symbols read, vp bit j set iff
 * D[j+1] - D[j] = +1, vn bit j iff it is -1, score = D[|P|].  Shift-Or: r bit j clear iff P[0..j] equals the last j+1
 * symbols read.  Bits at or above the needle's own |P| are zero (vp, vn) or set (r) on output and ignored on input.
 * spm_hip_patterns_state_init writes the constructor-time state (vp bits of rows below |P| set, vn = 0, score = |P|;
 * r = ~0). */
size_t spm_hip_patterns_state_stride(const spm_patterns *p);
int spm_hip_patterns_state_init(const spm_patterns *p, void *state);

/* ---- scan: replaces seqan_pattern_base::operator()(haystack, callback), seqan_pattern_base.hpp:40-52 ----
 * Scans text[begin,end).  state_in == NULL: fresh matcher (non-restorable semantics).  state_in != NULL:
 * continue from that state (restorable semantics, myers_matcher_restorable.hpp:72-82); state_out (may alias
 * state_in, may be NULL) receives the state after the last symbol.  With state_in, left_context changes nothing;
 * without it and with left_context = 1, state_out is the state after text[0, end). */
int spm_hip_scan(spm_ctx *ctx, const spm_text *text, uint64_t begin, uint64_t end, const spm_patterns *patterns,
                 const spm_scan_opts *opts, const void *state_in, void *state_out, spm_hits **out);

/* Batch of independent haystacks stored back to back in one text: haystack s = text[seg_offsets[s], seg_offsets[s+1])
 * (n_segments + 1 ascending host offsets).  Each one is scanned as seqan_pattern_base::operator() would scan it on its
 * own -- cold start at its first symbol, no hit spans two haystacks -- in ONE launch.  Positions are reported relative to
 * text[0]; the caller maps them to (segment, local position).  Used by the journaled-sequence traversal, whose
 * variant contexts are thousands of short haystacks. */
int spm_hip_scan_segments(spm_ctx *ctx, const spm_text *text, const uint64_t *seg_offsets, uint64_t n_segments,
                          const spm_patterns *patterns, const spm_scan_opts *opts, spm_hits **out);

/* ---- hits ------------------------------------------------------------------------------------------ */
/* Host view, sorted by (pattern, pos): per pattern this is the order the reference's callback fires in. */
int spm_hip_hits_view(spm_hits *hits, const spm_hit **records, uint64_t *n);
/* Device view (arrival order, not sorted): pointer to n spm_hit records in HBM, for an RCCL gather. */
int spm_hip_hits_device(spm_hits *hits, const void **device_records, uint64_t *n);
/* Copy the first min(n, cap) records into a caller-owned device buffer (e.g. a torch tensor that an RCCL
 * send/recv will read), asynchronously on the context's stream.  *n receives the number of hits. */
int spm_hip_hits_copy_device(spm_hits *hits, void *device_dst, uint64_t cap, uint64_t *n);
/* The same with a 16-byte header {n as uint64, 0} in front of the records: device_dst (16-byte aligned) holds cap + 1
 * records' worth of bytes; one kernel writes header and records.
 * This is the fixed-size [count | records] buffer one ncclAllGather per scan exchanges (libspm_amd.dist.gather_hits_fused):
 * the count is written from the host value the library already has, no second call from the caller. */
int spm_hip_hits_copy_fused(spm_hits *hits, void *device_dst, uint64_t cap, uint64_t *n);
/* The same without the host knowing the count: a kernel reads the scan's counters on the device and writes the header
 * {n as uint64, status as uint64} and the first min(n, cap) records.  status 0: the records are the scan's final result;
 * nonzero: the scan needs the host's attention (a list overflowed, spans gave up) -- call an accessor (which completes
 * the scan) and copy again.  Does not synchronise; completes nothing. */
int spm_hip_hits_copy_fused_device(spm_hits *hits, void *device_dst, uint64_t cap);
int spm_hip_hits_stats(const spm_hits *hits, spm_scan_stats *out);
/* order-independent checksum: sum over hits of mix64(pos ^ pattern<<40 ^ score<<58), SURVEY.md 8(d) */
uint64_t spm_hip_hits_checksum(spm_hits *hits);
void spm_hip_hits_destroy(spm_hits *hits);

/* ---- begins and alignments of hits: what seqan2's findBegin adds to a Myers finder ----------------------------------
 * A Myers hit is (end e, distance d).  Its begin is the LARGEST b in [lo, e] with ED(P, text[b, e)) = d -- the shortest
 * text span, the begin a backward scan from e reaches first.  lo is the first symbol the scan let an alignment use:
 * spm_hip_scan's `begin` (left_context = 0), 0 (left_context = 1), or the start of the hit's segment
 * (spm_hip_scan_segments).  ED is unit-cost edit distance over ranks; a needle rank >= sigma matches nothing.
 * The transcript is one optimal global alignment of P against text[b, e) with exactly d edits, as BAM-style CIGAR words
 * len << 4 | op, the needle being the query and the text the reference: SPM_CIGAR_EQ (match), SPM_CIGAR_X (mismatch),
 * SPM_CIGAR_INS (a needle symbol only), SPM_CIGAR_DEL (a text symbol only); adjacent equal ops are merged.
 * Tie order: walking back from (|P|, e - b), a diagonal step (= or X) is taken whenever it is optimal, else an
 * insertion, else a deletion.  The result depends only on (P, text, e, d): bit-identical across runs and engines.
 * Exact sets (Shift-Or, Horspool): begin = pos, end = pos + |P|, CIGAR |P|=.
 * Not supported (SPM_E_UNSUPPORTED): MYERS_PREFIX sets, stateful scans (state_in != NULL).  The hits of a
 * journaled-sequence search have an entry point of their own, spm_hip_jst_hits_align below.
 * The scan's text and needle set must still be alive. */
typedef struct spm_aln {
    uint64_t begin;       /* b + pos_offset (exact sets: pos) */
    uint64_t end;         /* the hit's pos (Myers) / pos + |P| (exact) */
    uint32_t pattern;
    int32_t score;        /* the hit's distance */
    uint32_t cigar_off;   /* first word of this record's transcript in the ops pool */
    uint32_t cigar_len;   /* words; 0 with SPM_ALIGN_BEGIN_ONLY */
} spm_aln;
typedef struct spm_alns spm_alns;

enum spm_cigar_op { SPM_CIGAR_INS = 1, SPM_CIGAR_DEL = 2, SPM_CIGAR_EQ = 7, SPM_CIGAR_X = 8 };
#define SPM_ALIGN_BEGIN_ONLY 1u /* begins only: skip the transcript stage (cigar_len = 0, empty ops pool) */

/* Device timings (ms, HIP events) and how the hits were split over the kernel classes. */
typedef struct spm_align_stats {
    float ms_total;        /* both stages */
    float ms_begin;        /* stage A: backward bit-vector scan to the begin */
    float ms_cigar;        /* stage B: banded DP + traceback */
    float ms_host;         /* wall clock of the whole call, host side included */
    uint64_t n_alns;
    uint64_t n_ops;        /* CIGAR words in the pool (sum of 2 score + 1 over the hits) */
    uint32_t begin_lane;        /* stage A, one lane per hit (|P| <= 256) */
    uint32_t begin_wave;        /* stage A, one wave per hit, a 64-bit word per lane */
    uint32_t cigar_lane;        /* stage B, one lane per hit, traceback in LDS (slots <= 1 KiB) */
    uint32_t cigar_wave;        /* stage B, one wave per hit, traceback in LDS (slots <= 64 KiB) */
    uint32_t cigar_wave_global; /* stage B, one wave per hit, traceback in a global scratch slice */
    uint32_t reserved[3];
} spm_align_stats;

/* Align every hit.  Records follow the hits: host view record i belongs to spm_hip_hits_view record i (order
 * (pattern, pos)), device record i to device hit i.  cigar_off is the exclusive prefix sum of 2 score + 1 in host order.
 * A deferred scan is completed first; an overflowed scan returns its SPM_E_OVERFLOW. */
int spm_hip_hits_align(spm_hits *hits, uint32_t flags, spm_alns **out);
int spm_hip_alns_view(spm_alns *a, const spm_aln **records, uint64_t *n, const uint32_t **ops, uint64_t *n_ops);
/* Device view: records in device hit order and the ops pool, in HBM, owned by the handle. */
int spm_hip_alns_device(spm_alns *a, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops);
int spm_hip_alns_stats(const spm_alns *a, spm_align_stats *out);
void spm_hip_alns_destroy(spm_alns *a);

/* ---- selection of hits: one record per locus, the best error stratum per needle, on the device -------------------------
 * A Myers scan reports EVERY end position whose distance is <= k, so one occurrence comes back as a cluster of neighbouring
 * ends.  A selection turns the records of a scan into a new, smaller spm_hits.  For a record r = (pos, pattern, score):
 *   SPM_SELECT_LOCI   r is kept iff there is no other record r' of the same pattern -- and, in a segmented scan, of the same
 *                     segment -- with |pos' - pos| <= w and (score', pos') < (score, pos) lexicographically.
 *                     w = spm_select_opts.window; SPM_SELECT_WINDOW_K: the needle's own k (0 for exact sets, whose k the
 *                     matchers ignore); window = 0 keeps everything.  Suppression is strict: a record dominated by a record
 *                     that is itself dominated is still dropped.  The rule depends only on the SET of records, so the
 *                     result is bit-identical across engines, runs and arrival orders.  Any two kept records of one pattern
 *                     (and segment) are more than w apart; of a plateau of equal scores the leftmost survives.
 *                     Segment of a record, p = pos - pos_offset: Myers seg_off[s] < p <= seg_off[s+1]; exact sets
 *                     seg_off[s] <= p < seg_off[s+1].
 *   SPM_SELECT_BEST   applied after LOCI: r is kept iff score <= min_score(pattern) + spm_select_opts.strata, the minimum
 *                     taken over that pattern's INPUT records, over the whole result (not per segment).  LOCI never removes
 *                     a pattern's minimum -- the leftmost minimal record inside its window always survives -- so the minimum
 *                     before LOCI is the minimum after it.
 *   SPM_SELECT_STRANDS  with BEST, for stranded needle sets (spm_hip_patterns_create_stranded): the minimum is taken per READ =
 *                     pattern >> 1, over the input records of both its patterns.  "A perfect forward hit beats a 3-error
 *                     reverse hit elsewhere."  LOCI is unchanged: records of different patterns never see each other, so a
 *                     palindromic read yields two records per place, and both stay.  Without BEST: SPM_E_INVALID.  With a
 *                     needle set at hand (the scan's, or patterns != NULL) that is not stranded: SPM_E_INVALID; a raw buffer
 *                     with patterns == NULL is taken by the index convention.  Order, views, stats, re-selection: as ever.
 *   neither flag      a sorted copy.
 * The result is a new spm_hits with a hit block of its own.  BOTH its host view and its device view are in (pattern, pos)
 * order (positions compare as in spm_hip_hits_view) -- the one device view with a defined order.  It copies the source's
 * alignment context (text, needle set, pos_offset, left context, segment table, statefulness): spm_hip_hits_align accepts
 * it and refuses exactly what it refuses on the source.  It stays valid after the source is destroyed; text and needle set
 * must stay alive, as for any hits.  spm_hip_hits_stats on it returns the source's scan statistics with n_hits set to the
 * selected count.  Every other accessor (view, device, copies, checksum, gatherv) takes it unchanged.
 * Exact sets and MYERS_PREFIX sets go through the same rule (exact: score 0).  Stateful scans can be selected.  A deferred
 * source is completed first; an overflowed source returns its SPM_E_OVERFLOW.  SPM_E_UNSUPPORTED, decided on the host before
 * any launch: more than 2^32 - 1 records; bits(n_patterns) + bits(largest position) above 64.  Unknown flag bits, a nonzero
 * reserved field or a NULL opts: SPM_E_INVALID.
 * LOCI and BEST are not shard-local -- a locus can straddle a shard boundary, the best stratum is global -- so under the
 * sharding of the multi-GPU exchange below the order is: gatherv first, spm_hip_records_select on the root second. */
#define SPM_SELECT_LOCI 1u
#define SPM_SELECT_BEST 2u
#define SPM_SELECT_STRANDS 8u   /* with SPM_SELECT_BEST: the minimum is taken per READ = pattern >> 1, over both strands */
#define SPM_SELECT_WINDOW_K 0xFFFFFFFFu
typedef struct spm_select_opts {
    uint32_t flags;    /* SPM_SELECT_* */
    uint32_t window;   /* LOCI: w, or SPM_SELECT_WINDOW_K */
    uint32_t strata;   /* BEST: strata kept above the needle's minimum (0: the best stratum only) */
    uint32_t reserved; /* 0 */
} spm_select_opts;
typedef struct spm_select_stats {
    float ms_total;    /* device: order + select (HIP events) */
    float ms_order;    /* keys + radix sort of (key, index) pairs */
    float ms_select;   /* selection, scan of the keep flags, compaction */
    float ms_host;     /* wall clock of the whole call (the first selection of a process loads the unit's code object) */
    uint64_t n_in;     /* records of the source */
    uint64_t n_loci;   /* records LOCI kept (n_in without the flag) */
    uint64_t n_out;    /* records of the result */
    uint32_t key_bits; /* bits of the sort key the radix passes covered */
    uint32_t reserved;
} spm_select_stats;
int spm_hip_hits_select(spm_hits *hits, const spm_select_opts *opts, spm_hits **out);
/* The same on a device buffer of n spm_hit records that no spm_hits owns -- what spm_hip_gatherv_hits delivers on the root.
 * patterns: the needle set the records belong to; may be NULL if window is explicit.  The records are taken as they are:
 * positions of one buffer share one coordinate system, there is no segment table.  (The host reads the range of the
 * positions back before it plans the sort: one synchronisation more than spm_hip_hits_select.)  The result carries no
 * alignment context: spm_hip_hits_align returns SPM_E_INVALID on it, spm_hip_hits_stats zeros but for n_hits. */
int spm_hip_records_select(spm_ctx *ctx, const void *device_records, uint64_t n, const spm_patterns *patterns,
                           const spm_select_opts *opts, spm_hits **out);
/* SPM_E_INVALID on a result no selection made */
int spm_hip_hits_select_stats(const spm_hits *hits, spm_select_stats *out);

/* ---- journaled-sequence (pan-genome) search, config C5 ----------------------------------------------------
 * The reference only designs the journaled sequence (specs/journaled_sequence_class_diagram.drawio:7-298) and gives the
 * matcher-side hooks a traverser needs (spm::window_size / capture / restore, matcher/concept.hpp:26-161).  The
 * contract implemented here is SURVEY.md 8(f)-2: the hit set equals the union over haplotypes of a linear scan of each
 * materialised haplotype, reported as (haplotype, position in haplotype coordinates).
 *
 * Device-side scheme: the reference axis is cut into blocks; (block, haplotype) pairs whose haplotype-local sequence
 * plus window-1 symbols of left context are byte-identical are found by an exact allele-set signature, one
 * representative of each is spelled out into a context buffer, the buffer is scanned as independent segments by the
 * same kernels as spm_hip_scan_segments, and every hit is fanned out to the haplotypes sharing its context.
 *
 * Alleles: sorted by `pos` (ties keep the given order); allele i replaces reference[pos, pos + ref_len) by
 * alt_pool[alt_off, alt_off + alt_len).  coverage: n_alleles x ceil(n_haplotypes / 64) words, bit h of row i set iff
 * haplotype h carries allele i.  Two alleles that overlap on the reference (pos_j < pos_i + ref_len_i for i < j) must
 * have disjoint coverage (multi-allelic sites); otherwise SPM_E_UNSUPPORTED.  At most 65 535 haplotypes; contexts are
 * shared among the haplotypes of one group of 1024. */
typedef struct spm_jst_allele {
    uint64_t pos;
    uint32_t ref_len;
    uint32_t alt_len;
    uint64_t alt_off;
} spm_jst_allele;

typedef struct spm_jst_hit {
    uint64_t pos;       /* what the matcher reports (Myers: exclusive end; exact: begin), haplotype coordinates */
    uint32_t haplotype;
    uint32_t pattern;
    int32_t score;
    uint32_t reserved;
} spm_jst_hit;

typedef struct spm_jst_stats {
    uint64_t haplotype_symbols; /* sum of haplotype lengths over the indexed blocks: what per-haplotype scans read */
    uint64_t context_symbols;   /* symbols laid out in the context buffer (what the device streams per search) */
    uint64_t contexts;          /* non-empty (block, haplotype) pairs */
    uint64_t unique_contexts;
    uint64_t n_blocks;
    uint32_t block_len;
    uint32_t window;
    float ms_index;             /* build of the context index (once per window size) */
    float ms_scan;              /* last search: segment scan incl. verification */
    float ms_main;              /* last search: the scan's main kernel(s) (seed filter / brute force) */
    float ms_verify;            /* last search: verification of the filter's candidates */
    float ms_fanout;            /* last search: hit fan-out to haplotypes */
    uint32_t engine_used;
    uint32_t main_launches;
    uint32_t fell_back;         /* last search: 1 if the seed filter overflowed and the brute engine re-ran the scan */
    uint64_t segment_hits;      /* last search: hits in context coordinates, before the fan-out */
    uint64_t candidates;        /* last search: seed-filter candidates */
    uint64_t bands;             /* last search: diagonal bands verified after candidate merging (0: not merged) */
} spm_jst_stats;

/* `reference` must stay alive as long as the tree (it is not copied). */
int spm_hip_jst_create(spm_ctx *ctx, const spm_text *reference, const spm_jst_allele *alleles, uint64_t n_alleles,
                       const uint8_t *alt_pool, uint64_t alt_pool_len, const uint64_t *coverage,
                       uint32_t n_haplotypes, spm_jst **out);
void spm_hip_jst_destroy(spm_jst *jst);
uint64_t spm_hip_jst_haplotype_length(const spm_jst *jst, uint32_t haplotype);
/* Symbols [begin, begin + n) of haplotype h (host walk over the allele table; for needles and tests). */
int spm_hip_jst_extract(spm_jst *jst, uint32_t haplotype, uint64_t begin, uint64_t n, uint8_t *out);
/* Build the context index for needle sets whose spm::window_size is <= window.  block_len = reference positions per
 * block (0 = library default); only blocks [block_begin, block_end) are indexed (block_end = 0: all) -- the shard of
 * one GPU when a tree is searched by several, SURVEY.md 8(e). */
int spm_hip_jst_index(spm_jst *jst, uint32_t window, uint32_t block_len, uint64_t block_begin, uint64_t block_end);
int spm_hip_jst_search(spm_jst *jst, const spm_patterns *patterns, const spm_scan_opts *opts, spm_jst_hits **out);
int spm_hip_jst_stats(const spm_jst *jst, spm_jst_stats *out);
/* Host view sorted by (haplotype, pos, pattern); device view in arrival order (for an RCCL gather). */
int spm_hip_jst_hits_view(spm_jst_hits *hits, const spm_jst_hit **records, uint64_t *n);
int spm_hip_jst_hits_device(spm_jst_hits *hits, const void **device_records, uint64_t *n);
/* Copy the first min(n, cap) records into a caller-owned device buffer, asynchronously on the context's stream. */
int spm_hip_jst_hits_copy_device(spm_jst_hits *hits, void *device_dst, uint64_t cap, uint64_t *n);
void spm_hip_jst_hits_destroy(spm_jst_hits *hits);

/* ---- begins and alignments of pan-genome hits: spm_hip_hits_align for the result of spm_hip_jst_search -------------
 * The haplotypes that share a context share it byte for byte, window - 1 symbols of left context included, and begin and
 * transcript depend only on (P, text, end, distance).  So ONE alignment per segment hit, computed in the context buffer by
 * the kernels of spm_hip_hits_align (lo = the start of the hit's context), serves every haplotype of that context; a
 * fan-out kernel writes one record per (haplotype, hit) with the haplotype's coordinates.
 *   * The search must have been made with spm_scan_opts.flags & SPM_SCAN_ALIGNABLE, else SPM_E_INVALID.  Tree and needle
 *     set must still be alive, and the tree must not have been indexed again since the search (spm_hip_jst_index frees
 *     the context buffer the alignment reads): SPM_E_INVALID otherwise.  MYERS_PREFIX sets cannot be searched at all.
 *   * Host view: record i belongs to record i of spm_hip_jst_hits_view (order (haplotype, pos, pattern)).  The device
 *     view is in the arrival order of this call's fan-out and is NOT matched to spm_hip_jst_hits_device; every record
 *     names its own (haplotype, end, pattern, score).
 *   * begin is the largest b >= 0 OF THAT HAPLOTYPE with ED(P, hap[b, end)) = score, the transcript the one the tie order
 *     above gives for P against hap[b, end): exactly what spm_hip_scan + spm_hip_hits_align return on the materialised
 *     haplotype.  (A context starts at the haplotype's first symbol or carries window - 1 >= |P| + k - 1 symbols of left
 *     context, a reported hit ends on an owned symbol, and an alignment with d <= k edits spans at most |P| + d symbols:
 *     its begin cannot lie left of the context.)
 *   * Records of haplotypes that share a context share one transcript: the same cigar_off / cigar_len.  The pool holds
 *     one slot of 2 score + 1 words per aligned segment hit, in the order (pattern, position in the context buffer).
 *   * Two calls on the same hits give byte-identical host views (records and pool).
 *   * Exact sets: begin = pos, end = pos + |P|, transcript |P|=. */
typedef struct spm_jst_aln {      /* 40 bytes */
    uint64_t begin;               /* haplotype coordinates; exact sets: pos */
    uint64_t end;                 /* the hit's pos (Myers) / pos + |P| (exact) */
    uint32_t haplotype;
    uint32_t pattern;
    int32_t score;
    uint32_t cigar_off;           /* first word of the transcript in the ops pool */
    uint32_t cigar_len;           /* 0 with SPM_ALIGN_BEGIN_ONLY */
    uint32_t reserved;
} spm_jst_aln;
typedef struct spm_jst_alns spm_jst_alns;

typedef struct spm_jst_align_stats { /* 80 bytes */
    float ms_total;        /* device: stage A + stage B + fan-out (HIP events) */
    float ms_begin;        /* stage A over the segment hits */
    float ms_cigar;        /* stage B over the segment hits */
    float ms_fanout;       /* the alignment fan-out */
    float ms_host;         /* wall clock of the whole call, host side included */
    float ms_worklist;     /* ... of which: reading the segment hits back and building the work list on the host */
    uint64_t n_alns;         /* records = the search's hit count */
    uint64_t n_segment_alns; /* alignments actually computed (segment hits that end on an owned symbol) */
    uint64_t n_ops;          /* CIGAR words in the pool (sum of 2 score + 1 over the segment alignments) */
    uint32_t begin_lane, begin_wave, cigar_lane, cigar_wave, cigar_wave_global; /* as in spm_align_stats */
    uint32_t reserved[3];
} spm_jst_align_stats;

/* flags: SPM_ALIGN_BEGIN_ONLY */
int spm_hip_jst_hits_align(spm_jst_hits *hits, uint32_t flags, spm_jst_alns **out);
int spm_hip_jst_alns_view(spm_jst_alns *a, const spm_jst_aln **records, uint64_t *n, const uint32_t **ops, uint64_t *n_ops);
int spm_hip_jst_alns_device(spm_jst_alns *a, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops);
int spm_hip_jst_alns_stats(const spm_jst_alns *a, spm_jst_align_stats *out);
void spm_hip_jst_alns_destroy(spm_jst_alns *a);

/* ---- begins and alignments of the records a SELECTION kept (spm_hip_jst_hits_select below) ---------------------------
 * A read mapper wants begin and CIGAR of the loci it kept, not of every record.  A selection keeps no map from its records
 * back to the search's segment hits, but the search's fan-out is a bijection from (segment hit that ends on an owned symbol,
 * member haplotype of its context) to haplotype record, and it is inverted per kept record from the tables of the index:
 * the block of the haplotype that owns the record's last symbol, that cell's context, where the context starts in the
 * haplotype -- hence the segment hit in the context buffer.  Kept records of haplotypes that share a context land on the
 * same segment hit; the DISTINCT ones are aligned once by the kernels of spm_hip_hits_align, then gathered.
 *   * Accepted: the result of spm_hip_jst_hits_select whose source chain ends, through any number of selections, at a result
 *     of spm_hip_jst_search.  Any select flags, SPM_SELECT_ACROSS included.  The search need NOT have been made with
 *     SPM_SCAN_ALIGNABLE, and the selection's source may already be destroyed.  Tree and needle set must still be alive, and
 *     the tree must not have been indexed again since the search (spm_hip_jst_index frees the context buffer the alignment
 *     reads): SPM_E_INVALID otherwise.
 *   * Refused with SPM_E_INVALID and a message that says why: a result of spm_hip_jst_records_select (it names no tree, and
 *     its records may stem from several block shards); a search's own result (use spm_hip_jst_hits_align, or a selection
 *     without flags, which is a sorted copy); unknown flag bits; NULL arguments.
 *   * One spm_jst_aln per record of the selection, n_alns = its count.  begin, end and transcript are exactly those
 *     spm_hip_jst_hits_align defines: begin is the largest b >= 0 OF THAT HAPLOTYPE with ED(P, hap[b, end)) = score, the
 *     transcript the one the tie order above gives for P against hap[b, end).  (A context starts at the haplotype's first
 *     symbol or carries window - 1 >= |P| + k - 1 symbols of left context, a reported hit ends on an owned symbol, and an
 *     alignment with d <= k edits spans at most |P| + d symbols: its begin cannot lie left of the context.)  The record for
 *     (haplotype, pattern, end, score) has the same begin and the same transcript words as that record of
 *     spm_hip_jst_hits_align on an alignable search over the same tree and set; pool offsets differ.
 *   * DEVICE view: record i belongs to record i of the selection's device view, in (haplotype, pattern, pos) order -- the
 *     first device view of alignments with a defined order.  Host view: record i belongs to record i of
 *     spm_hip_jst_hits_view of the selection.
 *   * The pool holds one slot of 2 score + 1 words per DISTINCT segment hit among the kept records, in the order (pattern,
 *     position in the context buffer).  Records that map to the same segment hit share cigar_off / cigar_len.  Two calls
 *     give byte-identical host views (records and pool).
 *   * Exact sets: begin = pos, end = pos + |P|, transcript |P|= (the last symbol of such a hit is pos + |P| - 1).
 *   * A record that cannot be located -- its last symbol lies outside the indexed blocks, its cell owns nothing, its mapped
 *     position falls outside its context or into the left context -- fails the whole call with SPM_E_INVALID and the count;
 *     nothing is aligned.  The detection is a device counter read back with the count of distinct hits, never a fault: every
 *     table index is tested against the table's size before it is read.
 *   * SPM_E_UNSUPPORTED, decided on the host: bits(n_patterns - 1) + bits(context symbols) above 64 (before any launch); a
 *     pool that would exceed 2^32 words (once the distinct hits are known, before anything is aligned).
 *   * An empty selection: an empty result and SPM_OK.
 *   * The result is an ordinary spm_jst_alns: view, device, stats and destroy take it unchanged.  In its spm_jst_align_stats
 *     n_segment_alns counts the distinct segment hits aligned, ms_fanout is the device time of locate + order + gather, and
 *     ms_worklist the host part (work list of the distinct hits; download and sort of the host view).
 * flags: SPM_ALIGN_BEGIN_ONLY */
int spm_hip_jst_selection_align(spm_jst_hits *selection, uint32_t flags, spm_jst_alns **out);

/* ---- pan-genome alignments in reference coordinates: SAM POS, CIGAR and NM of what the two calls above return -------------
 * spm_hip_jst_hits_align and spm_hip_jst_selection_align end at begin, end and a transcript in the coordinates of ONE
 * haplotype.  This call projects them through the alleles that haplotype carries onto the reference of the tree.
 *
 * Journal of haplotype h.  The carried alleles are applied in table order.  A carried allele (pos p, ref_len r, alt a[0..al))
 * pairs its first min(r, al) alt symbols with the reference positions p .. p + min - 1.  If al > r the remaining al - r alt
 * symbols are INSERTED: they have no reference position, and their ANCHOR is p + min(r, al).  If r > al the reference positions
 * p + al .. p + r - 1 are DELETED.  Every other haplotype symbol is paired with the reference position it was copied from.
 *
 * Projection of a record (h, begin, end, transcript of P against hap[begin, end)).  Walk the transcript with a haplotype
 * cursor x = begin and a needle cursor i = 0:
 *     transcript column | hap[x] paired with rho                          | hap[x] inserted
 *     = / X             | = if P[i] == ref[rho], else X; consumes rho     | I
 *     D                 | D; consumes rho                                 | nothing
 *     I                 | I                                               | I
 * Before every column that consumes a reference position rho, except the first such column, rho - rho_prev - 1 D columns are
 * emitted: the reference positions a carried allele deleted between the two.  Nothing else ever emits them, so leading and
 * trailing deleted stretches are not part of the alignment.
 *   * Adjacent equal ops are merged; words are len << 4 | op with the SPM_CIGAR_* values above.
 *   * ref_begin is the first consumed rho, ref_end the last consumed rho plus 1.
 *   * If no column consumes a reference position the alignment lies wholly inside one inserted stretch: the transcript is
 *     |P| I, and ref_begin = ref_end = the anchor of hap[begin].
 *   * ref_score is the number of X, I and D symbols of the projected transcript (SAM NM); score stays the haplotype distance.
 *   * = / X compare ranks, as everywhere else (dna5 / dna15 included).
 * It follows that the projected transcript consumes exactly P and ref[ref_begin, ref_end).
 * Example, ref = AACCGGTTAACC, one carried allele each (every haplotype transcript is a single = run):
 *     SNP at pos 5, G->T                     CGTT  = hap[3,7)   2=1X1=     [3,7)  ref_score 1
 *     deletion at pos 4, ref_len 2           CCTT  = hap[2,6)   2=2D2=     [2,8)  2
 *     insertion at pos 4, ref_len 0, alt TTT CTTTG = hap[3,8)   1=3I1=     [3,5)  3
 *     the same insertion                     TT    = hap[4,6)   2I         [4,4)  2
 *     replacement at pos 4, GG->TAC          CTACT = hap[3,8)   1=2X1I1=   [3,7)  3
 *
 *   * Accepted: the result of spm_hip_jst_hits_align or of spm_hip_jst_selection_align, Myers and exact sets.  Tree and
 *     needle set must still be alive.
 *   * Refused with SPM_E_INVALID and a message that says why: alignments made with SPM_ALIGN_BEGIN_ONLY (there is no
 *     transcript to project); a tree that has been indexed again since the search (the rule of the align calls: the tables
 *     the projection walks belong to an index generation); unknown flag bits; NULL arguments.
 *   * Host view: record i belongs to record i of spm_hip_jst_alns_view of the source.  Device view: record i belongs to
 *     record i of spm_hip_jst_alns_device of the source.  Two calls give byte-identical host views (records and pool).
 *   * Records that share a transcript slot share a context, hence the alleles over it: the projection is computed once per
 *     distinct source slot.  Two source records with equal cigar_off get equal cigar_off, ref_begin, ref_end and ref_score.
 *     The pool holds one projected transcript per distinct source slot, in source pool order.
 *   * A record that cannot be projected -- a transcript outside the source pool, a begin outside its haplotype, a
 *     transcript that does not consume its needle -- fails the whole call with SPM_E_INVALID; the detection is a device
 *     counter, never a fault: every table index is tested against the table's size before it is read.
 *   * More than 2^32 - 1 pool words: SPM_E_UNSUPPORTED, decided once the words are counted and before any is written.
 *   * No records: an empty result and SPM_OK.
 * flags: must be 0 */
typedef struct spm_jst_ref_aln {  /* 40 bytes */
    uint64_t ref_begin;           /* reference coordinates; inside an insertion: the anchor */
    uint64_t ref_end;
    uint32_t haplotype;
    uint32_t pattern;
    int32_t score;                /* the haplotype distance, as in the source record */
    int32_t ref_score;            /* X + I + D symbols of the projected transcript */
    uint32_t cigar_off;           /* first word of the projected transcript in the ops pool of this result */
    uint32_t cigar_len;
} spm_jst_ref_aln;
typedef struct spm_jst_ref_alns spm_jst_ref_alns;

typedef struct spm_jst_project_stats { /* 64 bytes */
    float ms_total;            /* device: the four stages below (HIP events) */
    float ms_representatives;  /* one representative record per distinct source slot, slots numbered in pool order */
    float ms_count;            /* the projection with a counting sink, and the offsets of the projected transcripts */
    float ms_emit;             /* the projection with a writing sink */
    float ms_gather;           /* one record per source record */
    float ms_host;             /* wall clock of the whole call, host view included */
    uint64_t n_alns;             /* records = the source's count */
    uint64_t n_projected;        /* distinct slots projected */
    uint64_t n_ops;              /* words in the projected pool */
    uint64_t n_inside_insertion; /* slots whose alignment lies wholly inside an inserted stretch (ref_begin == ref_end) */
    uint64_t n_changed;          /* slots whose projected words differ from their haplotype words */
} spm_jst_project_stats;

int spm_hip_jst_alns_project(spm_jst_alns *a, uint32_t flags, spm_jst_ref_alns **out);
int spm_hip_jst_ref_alns_view(spm_jst_ref_alns *a, const spm_jst_ref_aln **records, uint64_t *n, const uint32_t **ops,
                              uint64_t *n_ops);
int spm_hip_jst_ref_alns_device(spm_jst_ref_alns *a, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops);
int spm_hip_jst_ref_alns_stats(const spm_jst_ref_alns *a, spm_jst_project_stats *out);
void spm_hip_jst_ref_alns_destroy(spm_jst_ref_alns *a);

/* ---- projected alignments collapsed to one record per locus: what a mapper prints ---------------------------------------
 * spm_hip_jst_alns_project returns one record per (haplotype, needle) hit: a read that maps to one place of the reference
 * comes back once per haplotype.  This call merges the records that say the same thing about the reference and keeps, per
 * merged record, the haplotypes that support it and their haplotype distances.
 *
 * Locus.  Two source records belong to the same locus iff they have equal pattern, ref_begin and ref_end and equal projected
 * transcripts: the same cigar_len and the same words.  (ref_score is a function of the words.)  Haplotype, haplotype distance
 * and slot do not enter: haplotypes whose contexts differ by an allele elsewhere in the block have distinct slots and may
 * have identical projections, so the question is one about CONTENT and is decided by comparing the words.
 * Order of the loci, in the host view and in the device view alike: ascending (pattern, ref_begin, ref_end, ref_score,
 * cigar_len), then the transcripts compared word by word as uint32.  The order is total on loci and reads only content.
 * Record.  score is the smallest haplotype distance among the source records of the locus, n_records their number.  The ops
 * pool holds exactly one transcript per locus, in locus order: cigar_off is the exclusive prefix sum of cigar_len.
 * Members.  Two parallel pools, haplotype (uint32) and score (int32).  members[member_off .. member_off + n_haplotypes) are
 * the DISTINCT haplotypes among the source records of the locus, ascending, each with the smallest score it has in that
 * locus.  member_off is the exclusive prefix sum of n_haplotypes.
 * Map.  locus_of[i] is the locus of source record i: the host map belongs to spm_hip_jst_ref_alns_view of the source, the
 * device map to spm_hip_jst_ref_alns_device of the source (the two views of a projection may differ in order).
 * The result is a function of the SET of source records only: records, the three pools and the host map are byte-identical
 * across engines, block lengths, arrival orders and runs.
 *
 * Worked cases.
 *  1. Same range, different transcripts.  ref = GATTCGCAAAAGTCCATG, one allele deletes the A at position 10; haplotype 0
 *     carries it, haplotype 1 does not.  Needle TTCGCAAAGTCCA, k = 1.  Haplotype 0: distance 0, projected 8=1D5=, [2,16),
 *     NM 1.  Haplotype 1: distance 1, projected 5=1D8=, [2,16), NM 1.  TWO loci, in this order (the word 5= is smaller than
 *     8=).  Left-normalisation of indels would merge them; it is not part of this call.  spm_hip_jst_ref_alns_normalize
 *     (below) is that stage: on its result this call gives ONE locus, 5=1D8=.
 *  2. One haplotype twice.  ref = GATTCGCATGTCCATG, one allele inserts G at position 8, carried by haplotype 0.  Needle
 *     ATTCGCA, k = 1.  The hit ending at 8 is 7= with distance 0; the hit ending at 9 is 7=1D with distance 1, and its D
 *     falls on the inserted symbol and projects to nothing.  Both records project to 7=, [1,8): ONE locus, n_records 2,
 *     n_haplotypes 1, member score 0.
 *  3. One member score per haplotype.  A read cut across a carried SNP: the carrier has distance 0, a non-carrier distance 1,
 *     both project to the same ...1X...: one locus, score 0, members (carrier, 0), (other, 1).
 *  4. Inside an insertion.  Alignments wholly inside one inserted stretch (ref_begin == ref_end, transcript |P| I) say nothing
 *     about WHERE in the stretch they lie: they merge whenever pattern and anchor agree.
 *
 *   * Accepted: any result of spm_hip_jst_alns_project (of a search's alignments or of a selection's; Myers and exact sets).
 *     The call reads only the projected records and their pool: tree and needle set need NOT be alive.  The result stays
 *     valid after the source is destroyed.
 *   * SPM_E_INVALID with a message: unknown flag bits, NULL arguments.
 *   * SPM_E_UNSUPPORTED, decided on the host before any launch: bits(n_patterns - 1) + bits(reference length) above 64.
 *   * A record whose transcript lies outside the source pool, or that disagrees with the record that represents its slot,
 *     fails the whole call with SPM_E_INVALID; the detection is a device counter, never a fault: every table index is tested
 *     against the table's size before it is read.
 *   * No records: an empty result and SPM_OK.
 * flags: must be 0 */
typedef struct spm_jst_ref_locus {  /* 48 bytes */
    uint64_t ref_begin;             /* reference coordinates; inside an insertion: the anchor */
    uint64_t ref_end;
    uint32_t pattern;
    int32_t ref_score;              /* X + I + D symbols of the transcript (SAM NM) */
    int32_t score;                  /* the smallest haplotype distance among the source records */
    uint32_t n_records;             /* source records merged */
    uint32_t cigar_off;             /* first word of the transcript in the ops pool of this result */
    uint32_t cigar_len;
    uint32_t member_off;            /* first member in the two member pools */
    uint32_t n_haplotypes;          /* distinct haplotypes among the source records */
} spm_jst_ref_locus;
typedef struct spm_jst_ref_loci spm_jst_ref_loci;

typedef struct spm_jst_collapse_stats { /* 80 bytes */
    float ms_total;            /* device: the four stages below (HIP events) */
    float ms_slots;            /* one representative record per distinct source slot */
    float ms_order;            /* slots sorted by (pattern, ref_begin), the rule inside every group, the locus of every slot */
    float ms_records;          /* records sorted by (locus, haplotype), the member heads */
    float ms_emit;             /* loci, transcripts, members */
    float ms_host;             /* wall clock of the whole call, host view included */
    uint64_t n_alns;           /* source records */
    uint64_t n_slots;          /* distinct source slots */
    uint64_t n_loci;
    uint64_t n_members;
    uint64_t n_ops;            /* words in the pool of this result */
    uint64_t n_multi_slot;     /* loci that merge more than one slot */
    uint64_t max_run;          /* longest run of slots with equal (pattern, ref_begin, ref_end, ref_score, cigar_len): the
                                  comparison of words is quadratic in it */
} spm_jst_collapse_stats;

int spm_hip_jst_ref_alns_collapse(spm_jst_ref_alns *a, uint32_t flags, spm_jst_ref_loci **out);
/* every pointer but records and n may be NULL */
int spm_hip_jst_ref_loci_view(spm_jst_ref_loci *l, const spm_jst_ref_locus **records, uint64_t *n, const uint32_t **ops,
                              uint64_t *n_ops, const uint32_t **members, const int32_t **member_scores, uint64_t *n_members);
int spm_hip_jst_ref_loci_device(spm_jst_ref_loci *l, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops,
                                const void **members, const void **member_scores, uint64_t *n_members);
/* locus_of: n_alns uint32 each; host_map or device_map may be NULL */
int spm_hip_jst_ref_loci_map(spm_jst_ref_loci *l, const uint32_t **host_map, const void **device_map, uint64_t *n_alns);
int spm_hip_jst_ref_loci_stats(const spm_jst_ref_loci *l, spm_jst_collapse_stats *out);
void spm_hip_jst_ref_loci_destroy(spm_jst_ref_loci *l);

/* ---- the loci of every read: what a mapper reports per read ----------------------------------------------------------------
 * One spm_jst_read per read 0 .. n_reads - 1, in read order, from the loci of a collapse.  strands says how patterns name
 * reads: read = pattern / strands (2: a stranded set, forward = pattern 2r; 1: a plain set, every locus is forward).  The loci
 * of a read are contiguous in the loci order, forward before reverse, leftmost first, and the PRIMARY locus is the one with
 * the smallest (score, locus index).  MAPQ is a policy over (n_best, n_next): spm_hip_jst_ref_loci_sam applies it.
 * The result is a pure function of the loci records: byte-identical across runs, host and device view alike.  It outlives
 * the loci handle.
 *   * SPM_E_INVALID: strands not 1 or 2, flags != 0, NULL arguments, strands * n_reads above 2^32 - 1.
 *   * A locus whose pattern is >= strands * n_reads (or whose score is negative) is COUNTED on the device and fails the whole
 *     call with SPM_E_INVALID, never a fault.
 *   * No loci: every read unmapped.  n_reads == 0: an empty result.  Both SPM_OK. */
typedef struct spm_jst_read {        /* 32 bytes */
    uint32_t first_locus;            /* index of the read's first locus in the loci order; no loci: where it would stand */
    uint32_t n_loci;                 /* loci of the read, both strands (they are contiguous: patterns strands * r ..) */
    uint32_t n_forward;              /* of those, on pattern strands * r */
    uint32_t primary;                /* the locus with the smallest (score, locus index); 0xFFFFFFFF: unmapped */
    int32_t best;                    /* its score (haplotype distance); -1 unmapped */
    int32_t best_ref_score;          /* its ref_score (SAM NM); -1 unmapped */
    uint32_t n_best;                 /* loci of the read with score == best */
    uint32_t n_next;                 /* ... with score == best + 1 */
} spm_jst_read;
typedef struct spm_jst_reads spm_jst_reads;
typedef struct spm_jst_reads_stats { /* 48 bytes */
    float ms_total;                  /* device: the three passes (HIP events) */
    float ms_host;                   /* wall clock of the whole call, host view included */
    uint64_t n_reads;
    uint64_t n_loci;
    uint64_t n_mapped;               /* reads with at least one locus */
    uint64_t n_unique;               /* reads with n_best == 1 */
    uint64_t n_multi;                /* reads with n_best > 1 */
} spm_jst_reads_stats;
int spm_hip_jst_ref_loci_reads(spm_jst_ref_loci *l, uint32_t strands, uint32_t n_reads, uint32_t flags, spm_jst_reads **out);
int spm_hip_jst_reads_view(spm_jst_reads *r, const spm_jst_read **records, uint64_t *n);
int spm_hip_jst_reads_device(spm_jst_reads *r, const void **records, uint64_t *n);
int spm_hip_jst_reads_stats(const spm_jst_reads *r, spm_jst_reads_stats *out);
void spm_hip_jst_reads_destroy(spm_jst_reads *r);

/* ---- the mates of paired-end reads: one proper pair per read pair --------------------------------------------------------------
 * One spm_jst_pair per pair p = 0 .. n_reads / 2 - 1, in pair order, from the loci of a collapse and their read summary made
 * with strands == 2.  Reads 2p (mate 1) and 2p + 1 (mate 2) are the mates of pair p: the loci of the pair are the contiguous
 * patterns 4p (mate 1 forward), 4p + 1 (mate 1 reverse), 4p + 2 (mate 2 forward), 4p + 3 (mate 2 reverse), and each of the
 * four sub-runs is ascending in ref_begin.  The forward loci of a read are its first n_forward loci, its reverse loci the rest.
 *
 * Concordance (FR orientation only).  Forward locus a of one mate and reverse locus b of the OTHER mate are concordant iff
 *     a.ref_begin <= b.ref_begin,  a.ref_end <= b.ref_end  and  min_tlen <= b.ref_end - a.ref_begin <= max_tlen.
 * Both directions count: mate 1 forward with mate 2 reverse, and mate 2 forward with mate 1 reverse.  A locus inside an
 * insertion (ref_begin == ref_end, the anchor) takes part as it is.
 * The best pair is the minimum of (a.score + b.score, index of a, index of b) over the concordant combinations; the sum is
 * taken in 64 bits.  n_pairs counts the concordant combinations, n_best those whose sum equals the best, n_next those whose
 * sum equals the best + 1; all three are accumulated in 64 bits and clamped to 0xFFFFFFFF in the record.
 * No concordant combination: locus1 and locus2 are the mates' own primaries from the read summary (0xFFFFFFFF: unmapped),
 * tlen is 0, best is -1, the counts are 0.  MAPQ is a policy over (n_best, n_next): spm_hip_jst_ref_loci_sam applies it.
 * flag1 / flag2 are the SAM FLAG of the two primary lines:
 *     0x1 always   0x2 proper pair   0x4 this mate has no locus   0x8 the other mate has no locus
 *     0x10 this mate's reported locus is a reverse pattern   0x20 the other mate's is   0x40 mate 1 / 0x80 mate 2
 * No secondary or supplementary bits are emitted.
 * The result is a pure function of the loci and opts: byte-identical across runs, host and device view alike.  It outlives
 * both source handles.
 *
 * Worked cases, reads of 30 symbols, min_tlen 100, max_tlen 300.
 *  1. The pair of the primaries is not the primary pair.  Mate 1 has one forward locus [1000,1030), score 0.  Mate 2 has the
 *     reverse loci [1170,1200) with score 1 and [7000,7030) with score 0: its own primary is the distant copy.  Only the first
 *     is concordant (fragment 200): locus2 is the locus at 1170, tlen +200, best 1, n_pairs 1, n_best 1, flag1 0x63, flag2 0x93.
 *  2. Mate 1 on the reverse strand.  Mate 2 forward at [500,530), mate 1 reverse at [720,750): tlen -250 (mate 2's line: +250),
 *     flag1 0x53, flag2 0xA3.
 *  3. Bounds and shapes.  a = [1000,1030) forward: b = [1070,1100) gives 100, concordant; [1069,1099) gives 99, not;
 *     [1270,1300) gives 300, concordant; [1271,1301) gives 301, not.  b = [990,1120) begins left of a (a dovetail) and
 *     a = [1000,1200), b = [1050,1150) ends right of b (a containment): neither is concordant.  Two forward loci of one mate
 *     and two reverse loci of the other, same strand on both mates, or only one mate mapped: never a proper pair; the record
 *     carries the primaries, tlen 0, and flags without 0x2.
 *
 *   * SPM_E_INVALID with a message: NULL arguments; unknown flag bits or a nonzero reserved; min_tlen == 0, min_tlen >
 *     max_tlen, max_tlen > 2^31 - 1; a reads handle of another context, one not made with strands == 2, one with an odd
 *     number of reads, one made from a different number of loci.
 *   * Everything else about the agreement of the two handles is tested on the device before it is used as an index -- the run
 *     of a read lies inside the loci, the patterns at the head and the tail of its sub-runs name the read, its primary lies
 *     inside the run, every locus lies in the run of its own read -- and a concordant combination whose score sum does not fit
 *     in 31 bits is unusable: either is COUNTED and fails the whole call with SPM_E_INVALID, never a fault.
 *   * Zero reads: an empty result.  No loci: every pair unmapped, flag1 0x4D, flag2 0x8D.  Both SPM_OK. */
typedef struct spm_jst_pair_opts {   /* 16 bytes */
    uint32_t min_tlen, max_tlen;     /* 1 <= min_tlen <= max_tlen <= 2^31 - 1 */
    uint32_t flags;                  /* must be 0 (FR orientation) */
    uint32_t reserved;               /* must be 0 */
} spm_jst_pair_opts;
typedef struct spm_jst_pair {        /* 32 bytes */
    uint32_t locus1, locus2;         /* locus reported for mate 1 / mate 2; 0xFFFFFFFF: unmapped */
    int32_t tlen;                    /* SAM TLEN of mate 1 (mate 2: its negative): + (b.ref_end - a.ref_begin) when mate 1 is
                                        the forward locus, - when it is the reverse one; 0 when not a proper pair */
    int32_t best;                    /* score sum of the best concordant pair; -1: none */
    uint32_t n_pairs, n_best, n_next;
    uint16_t flag1, flag2;           /* SAM FLAG of the two primary lines */
} spm_jst_pair;
typedef struct spm_jst_pairs spm_jst_pairs;
typedef struct spm_jst_pairs_stats { /* 72 bytes */
    float ms_total;                  /* device: the three passes (HIP events) */
    float ms_host;                   /* wall clock of the whole call, host view included */
    uint64_t n_pairs;                /* read pairs */
    uint64_t n_proper;               /* pairs with a concordant combination */
    uint64_t n_unique;               /* ... with n_best == 1 */
    uint64_t n_multi;                /* ... with n_best > 1 */
    uint64_t n_discordant;           /* both mates mapped, not proper */
    uint64_t n_one_mate;             /* exactly one mate mapped */
    uint64_t n_unmapped;             /* neither */
    uint64_t max_window;             /* the longest partner window any forward locus walked: the walk is linear in it */
} spm_jst_pairs_stats;
int spm_hip_jst_ref_loci_pairs(spm_jst_ref_loci *l, spm_jst_reads *r, const spm_jst_pair_opts *opts, spm_jst_pairs **out);
int spm_hip_jst_pairs_view(spm_jst_pairs *p, const spm_jst_pair **records, uint64_t *n);
int spm_hip_jst_pairs_device(spm_jst_pairs *p, const void **records, uint64_t *n);
int spm_hip_jst_pairs_stats(const spm_jst_pairs *p, spm_jst_pairs_stats *out);
void spm_hip_jst_pairs_destroy(spm_jst_pairs *p);

/* ---- mate rescue: a missing mate re-aligned beside its partner -------------------------------------------------------------
 * A pair whose record lacks 0x2 gives one JOB per mapped mate: one-mate pairs one, discordant pairs two; proper pairs and
 * pairs with no mate mapped none.  The ANCHOR A of a job is the locus the pair record reports for that mate (locus1 / locus2,
 * its primary; only the primary is used).  The job looks for the OTHER mate Y on the opposite strand: needle
 *     q = 4 pair + 2 (mate of Y) + (1 - strand bit of A's pattern)
 * of `patterns`, the stranded Myers set that produced the loci.  Jobs -- and records -- are ordered by (pair, mate rescued).
 * Window and ends, N the length of `reference`, ends exclusive as ref_end is:
 *     A forward:  lo = A.ref_begin,                    window [lo, min(lo + max_tlen, N)),
 *                 ends e in [max(lo + min_tlen, A.ref_end), min(lo + max_tlen, N)]
 *     A reverse:  lo = max(0, A.ref_end - max_tlen),   window [lo, A.ref_end),   ends e in (lo, A.ref_end]
 * No alignment begins left of lo (the lo of spm_hip_hits_align); an empty range finds nothing.
 * Search: unit-cost semi-global edit distance of q in the window (a needle rank >= sigma matches nothing).  d(e) is the
 * distance of the best alignment that ends at e and begins at or right of lo; the candidate is the minimum of (d, e) over
 * the admissible ends with d <= k.  A needle of m <= k symbols is not searched: status NONE, counted in n_short (and in
 * n_none).  Needles above 256 symbols: SPM_E_UNSUPPORTED.
 * Alignment: begin and transcript of (q, e, d, lo) are those of spm_hip_hits_align over `reference` -- the largest begin;
 * diagonal, then I, then D -- computed by the same kernels.
 * Classification: the concordance predicate of the pairing on (A, rescued alignment), POST HOC.  A forward anchor's
 * candidate is concordant by construction.  A reverse anchor's candidate can fail on its begin -- it begins right of A's
 * begin (a dovetail), or the fragment is shorter than min_tlen: it is kept with its alignment, status NOT_CONCORDANT, tlen 0,
 * and NO second-best end is tried.
 * Limits.  The search is against the REFERENCE, not the haplotypes: a mate that carries non-reference alleles pays for them
 * in edits, and k has to cover that; score is a reference distance (SAM NM), not a haplotype distance, and is never mixed
 * with the anchor's score.  FR orientation only (no RF, no FF).  MAPQ: see spm_hip_jst_ref_loci_sam.
 * flag is the SAM FLAG of the rescued mate's line: 0x1; 0x2 when RESCUED; 0x4 when NONE; 0x10 the needle is a reverse
 * pattern (not for NONE); 0x20 the anchor is; 0x40 / 0x80 the rescued mate is mate 1 / mate 2.
 * The result is a pure function of its inputs: byte-identical across runs, host and device view alike.  It outlives all
 * five inputs.
 *
 * Worked cases, reads of 30 symbols, min_tlen 100, max_tlen 300, N = 10000.
 *  1. Mate 1 forward at [1000,1030), mate 2 unmapped: one job, needle 4p + 3, window [1000,1300), ends 1100 .. 1300.  The best
 *     end is 1200 with 4 edits, its begin 1170: RESCUED, tlen +200, flag 0x93.
 *  2. Mate 2 reverse at [720,750), mate 1 unmapped: needle 4p + 0, window [450,750), ends 451 .. 750.  Candidate [500,530):
 *     RESCUED, tlen +250, flag 0x63.  Candidate [700,730): 50 < min_tlen, NOT_CONCORDANT, tlen 0, flag 0x61.  Candidate
 *     [725,750) with min_tlen 20: it begins right of 720 (a dovetail), NOT_CONCORDANT.
 *  3. Clipping.  A forward at [9800,9830): window [9800,10000), ends 9900 .. 10000.  A forward at [9950,9980): ends 10050 ..
 *     are beyond N: nothing is found.  A reverse at [170,200): lo = 0, ends 1 .. 200.
 *  4. A discordant pair (both mapped): two jobs, the first rescues mate 1 (anchor locus2), the second mate 2 (anchor locus1).
 *
 *   * SPM_E_INVALID with a message, decided on the host before any launch: NULL arguments; nonzero flags or reserved;
 *     min_tlen == 0, min_tlen > max_tlen, max_tlen > 2^31 - 1; handles of different contexts; a reads handle not made with
 *     strands == 2; pairs->n != reads->n / 2; a reads handle made from a different number of loci; a needle set that is not a
 *     stranded Myers set with n == 2 n_reads; a text sigma other than the set's.
 *   * SPM_E_UNSUPPORTED, likewise: a MYERS_PREFIX set; a needle above 256 symbols.
 *   * A pair record that disagrees with the read summary, the loci or the reference -- an index outside the loci, a pattern
 *     that does not name the mate and the strand the flags state, ref_end > N, a locus that is not the read's primary -- is
 *     COUNTED on the device, each test before the value is used as an index, and fails the call with SPM_E_INVALID.
 *   * Zero pairs, or zero jobs: an empty result and SPM_OK. */
typedef struct spm_jst_rescue_opts { /* 20 bytes */
    uint32_t min_tlen, max_tlen;     /* 1 <= min_tlen <= max_tlen <= 2^31 - 1: the rule of the pairing */
    uint32_t k;                      /* the most edits a rescued mate may have against the reference */
    uint32_t flags;                  /* must be 0 */
    uint32_t reserved;               /* must be 0 */
} spm_jst_rescue_opts;
enum spm_rescue_status { SPM_RESCUE_RESCUED = 0, SPM_RESCUE_NONE = 1, SPM_RESCUE_NOT_CONCORDANT = 2 };
typedef struct spm_jst_rescue {      /* 48 bytes */
    uint64_t ref_begin, ref_end;     /* the rescued alignment; 0, 0 for NONE */
    uint32_t pair;
    uint32_t pattern;                /* the needle that was aligned */
    uint32_t anchor;                 /* the anchor's locus index */
    int32_t score;                   /* edits against the reference; -1 for NONE */
    uint32_t cigar_off, cigar_len;   /* into this result's ops pool: cigar_off is the exclusive prefix sum of 2 score + 1 over
                                        the found jobs in job order; 0, 0 for NONE */
    int32_t tlen;                    /* SAM TLEN of mate 1 as the pairing defines it; 0 unless RESCUED */
    uint16_t flag;                   /* SAM FLAG of the rescued mate's line */
    uint16_t status;                 /* spm_rescue_status */
} spm_jst_rescue;
typedef struct spm_jst_rescues spm_jst_rescues;
typedef struct spm_jst_rescues_stats { /* 80 bytes */
    float ms_total;                  /* device: the four stages below (HIP events) */
    float ms_jobs;                   /* the job list */
    float ms_search;                 /* the bounded search, one wave per job */
    float ms_align;                  /* begins and transcripts of the found jobs */
    float ms_emit;                   /* classification and records */
    float ms_host;                   /* wall clock of the whole call */
    uint64_t n_pairs;
    uint64_t n_jobs;                 /* = n_rescued + n_none + n_not_concordant */
    uint64_t n_rescued;
    uint64_t n_none;
    uint64_t n_not_concordant;
    uint64_t n_short;                /* of n_none: needles of m <= k symbols, not searched */
    uint64_t max_window;             /* the longest window of any job */
} spm_jst_rescues_stats;
int spm_hip_jst_pairs_rescue(spm_jst_ref_loci *loci, spm_jst_reads *reads, spm_jst_pairs *pairs, const spm_text *reference,
                             const spm_patterns *patterns, const spm_jst_rescue_opts *opts, spm_jst_rescues **out);
/* ops and n_ops may be NULL */
int spm_hip_jst_rescues_view(spm_jst_rescues *r, const spm_jst_rescue **records, uint64_t *n, const uint32_t **ops,
                             uint64_t *n_ops);
int spm_hip_jst_rescues_device(spm_jst_rescues *r, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops);
int spm_hip_jst_rescues_stats(const spm_jst_rescues *r, spm_jst_rescues_stats *out);
void spm_hip_jst_rescues_destroy(spm_jst_rescues *r);

/* ---- SAM lines and MAPQ: what a mapper's user takes away -------------------------------------------------------------------
 * One call turns (loci, read summary, optionally pairs and rescues, needle set) into SAM text in HBM plus one fixed-size
 * spm_sam_line per line.  Lines are ordered by read; within a read the REPORTED line comes first, then (with
 * SPM_SAM_SECONDARY) its secondary lines in locus order.  Single-end: pairs == NULL, the reads handle may have strands 1 or 2.
 * Paired: reads 2p and 2p + 1 are the mates of pair p, strands == 2.
 *
 * MAPQ is a policy over (n_best, n_next), given by two tables of the opts:
 *     mapq(n_best, n_next) = 0                               for n_best == 0
 *                            mapq_unique[min(n_next, 3)]     for n_best == 1
 *                            mapq_multi[min(n_best, 5) - 2]  otherwise
 * (the counts arrive clamped to 0xFFFFFFFF; min takes care of that).  With mapq_defaults != 0 the tables of the opts are not
 * read: mapq_multi = {3, 1, 1, 0}, which is floor(-10 log10(1 - 1/n)) for n = 2, 3, 4, >= 5, and mapq_unique = {60, 40, 30,
 * 20}, which is a CONVENTION, not a derivation: a unique best placement is the surer the fewer placements stand one edit
 * behind it, and these four numbers say so in the range mappers commonly print.  They are the caller's to override.
 * Which counts a line uses.  Single-end: the read's.  Mates of a proper pair: the pair record's, on both lines.  Mates of a
 * pair that is neither proper nor rescued: each mate's own read counts.  A rescued pair: both lines take the ANCHOR read's
 * counts (the rescued mate was searched only beside the anchor: its placement is as sure as the anchor's).  Unmapped lines:
 * MAPQ 0.  Secondary lines: 255 (SAM: unavailable).
 *
 * Which line a read reports, in paired mode with rescues.  Only records with status RESCUED are used.  A discordant pair can
 * have two: the one with the smaller score is used, on a tie the first in record order (it rescues mate 1).  The rescued
 * mate's reported line is the rescue alignment: ref_begin, ref_end, score as NM, its transcript in the rescues' pool, flag as
 * the record has it.  The anchor's line is its locus with flag (pair flag | 0x2) & ~0x8 and 0x20 set iff the rescue's flag has
 * 0x10.  Both carry the rescue's tlen (negated on mate 2's line, as the pairing defines).  Without a used rescue the lines
 * are locus1 / locus2 with flag1 / flag2 and the pair's tlen.
 * Mate fields.  Both mates have a reported line: RNEXT "=", PNEXT the mate's POS.  This mate mapped, the other not: "=", own
 * POS, TLEN 0.  This mate unmapped, the other mapped: RNAME and POS are the mate's, RNEXT "=", PNEXT the mate's POS, MAPQ 0,
 * CIGAR "*".  Neither: "* 0 0 * * 0 0".  Single-end: RNEXT "*", PNEXT 0, TLEN 0.
 * Secondary lines (SPM_SAM_SECONDARY).  Every locus of the read that is not its reported line, in locus order; for a mate
 * whose line came from a rescue that is all of its loci.  FLAG 0x100, 0x10 for a reverse pattern; paired also 0x1, 0x40 or
 * 0x80, 0x20 iff the mate's reported line is reverse, 0x8 iff the mate has none; never 0x2.  TLEN 0, mate fields as above (a
 * secondary's "own POS" is its own), SEQ "*".
 * Fields of a mapped line.  QNAME: the caller's name (one per read, paired: one per pair, shared by the mates), without
 * names the decimal index of the read / pair.  FLAG.  RNAME of the opts.  POS = ref_begin + 1.  MAPQ.  CIGAR: the words as
 * <len><op> with I D = X; with SPM_SAM_CIGAR_M maximal runs of adjacent = / X words become one M of the summed length.  SEQ:
 * the needle locus.pattern through `symbols` (sigma characters; a rank >= sigma prints N) -- the reverse pattern already is
 * the reverse complement, which is what SAM wants.  QUAL "*".  Tags in this order: NM:i:<ref_score> XH:i:<score, the haplotype
 * distance> XN:i:<n_haplotypes>, and on reported lines X0:i:<n_best> X1:i:<n_next>, the counts the MAPQ used.  A rescued
 * mate's line has NM:i:<score> XR:i:1 X0 X1.  An unmapped line has SEQ = the forward read and no tags.  (QUAL other than "*", and an MD tag: spm_hip_jst_ref_loci_sam_ex below.)  A locus inside an
 * insertion (ref_begin == ref_end, all I) is printed as it is.  Every line ends in \n.
 *
 * Worked cases (rname "chr", default tables, no names).
 *  1. Single-end read 7, primary locus [99,131) on pattern 15 (reverse), words 20= 1X 11=, ref_score 1, score 0, 2 haplotypes,
 *     n_best 1, n_next 1:   7 16 chr 100 40 20=1X11= * 0 0 <SEQ> * NM:i:1 XH:i:0 XN:i:2 X0:i:1 X1:i:1   (CIGAR_M: 32M).
 *  2. Case 1 of the pairing (flag1 0x63, flag2 0x93, tlen +200, loci [1000,1030) and [1170,1200), n_best 1, n_next 0), pair 0:
 *     0 99 chr 1001 60 30= = 1171 200 ...   and   0 147 chr 1171 60 30= = 1001 -200 ...
 *  3. Case 1 of the rescue (mate 1 at [1000,1030), flag1 0x49; mate 2 rescued at [1170,1200), 4 edits, flag 0x93, tlen +200; the
 *     anchor read has n_best 2):  anchor flag (0x49 | 0x2) & ~0x8 | 0x20 = 0x63, both MAPQ 3, and mate 2's line ends in
 *     NM:i:4 XR:i:1 X0:i:2 X1:i:0.
 *  4. One mate only (flag1 0x49, flag2 0x85, mate 1 at [500,530)):  0 73 chr 501 60 30= = 501 0 ...   and
 *     0 133 chr 501 0 * = 501 0 <SEQ> *.
 *
 *   * SPM_E_INVALID with a message, decided on the host before any launch: NULL arguments; unknown flags, a nonzero
 *     reserved, a mapq_defaults above 1; rescues without pairs; handles of different contexts; a reads handle made from
 *     another number of loci; pairs with a reads handle whose strands is not 2, or whose count is not reads / 2; a needle set
 *     whose n is not strands x n_reads; strlen(symbols) != the set's sigma;
 *     an rname or a name that is empty, longer than 254 bytes or contains a byte outside '!' .. '~' ('@' is allowed, "*"
 *     alone is not); n_names not the number of reads (single-end) / pairs (paired); names without name_off or the other way
 *     round; a name_off that does not ascend from 0.
 *   * SPM_E_UNSUPPORTED, likewise: a MYERS_PREFIX set; reads + (with SPM_SAM_SECONDARY) loci above 2^32 - 1, the bound on
 *     the number of lines.
 *   * Everything else about the agreement of the inputs is tested on the device before a value is used as an index: the run
 *     of a read lies inside the loci and names the read, a pair's loci lie in the runs of its mates, rescue records are
 *     ordered by (pair, mate rescued), a rescue names a pair inside the pairs and an anchor that is that pair's locus, a
 *     transcript lies inside its pool, the query length of a transcript (= + X + I) equals the needle's length.  A failure is
 *     COUNTED and fails the call with SPM_E_INVALID, never a fault.
 *   * Zero reads: an empty result and SPM_OK.
 * The result is a pure function of its inputs: byte-identical across runs, host and device view equal.  It outlives all
 * inputs (the strings of the opts are copied). */
#define SPM_SAM_CIGAR_M 1u      /* = and X words print as M, adjacent ones merged */
#define SPM_SAM_SECONDARY 2u    /* a line for every locus that is not its read's reported line */
typedef struct spm_sam_opts {       /* 64 bytes */
    const char *rname;              /* NUL-terminated */
    const char *symbols;            /* NUL-terminated, sigma characters: the letter of every rank */
    const char *names;              /* the names back to back, or NULL: decimal indices */
    const uint64_t *name_off;       /* n_names + 1 offsets into names, name_off[0] == 0; NULL with names == NULL */
    uint64_t n_names;               /* reads (single-end) or pairs (paired); 0 with names == NULL */
    uint8_t mapq_unique[4];         /* n_best == 1: by min(n_next, 3) */
    uint8_t mapq_multi[4];          /* n_best >= 2: by min(n_best, 5) - 2 */
    uint32_t mapq_defaults;         /* 1: use the default tables, the two above are not read; 0: use them */
    uint32_t flags;                 /* SPM_SAM_* */
    uint64_t reserved;              /* must be 0 */
} spm_sam_opts;
enum spm_sam_kind { SPM_SAM_UNMAPPED = 0, SPM_SAM_LOCUS = 1, SPM_SAM_RESCUE = 2, SPM_SAM_SECONDARY_LINE = 3 };
typedef struct spm_sam_line {       /* 24 bytes: what a BAM writer needs of a line besides the pools */
    uint64_t offset;                /* first byte of the line in the text */
    uint32_t len;                   /* bytes, the \n included */
    uint32_t read;
    uint32_t source;                /* locus index (LOCUS, SECONDARY_LINE), rescue index (RESCUE), 0xFFFFFFFF (UNMAPPED) */
    uint16_t flag;
    uint8_t mapq;
    uint8_t kind;                   /* spm_sam_kind */
} spm_sam_line;
typedef struct spm_sam spm_sam;
typedef struct spm_sam_stats {      /* 72 bytes */
    float ms_total;                 /* device: the four stages below (HIP events) */
    float ms_lines;                 /* first rescue of every pair, the reported lines, the line records */
    float ms_measure;               /* the length of every line, the offsets */
    float ms_write;                 /* the text, one wave per line */
    float ms_stats;                 /* offsets into the records, the counts */
    float ms_host;                  /* wall clock of the whole call (the views are downloaded when first asked for) */
    uint64_t n_lines;               /* = n_reported + n_secondary + n_unmapped */
    uint64_t n_bytes;
    uint64_t n_reported;            /* lines of kind LOCUS or RESCUE */
    uint64_t n_secondary;
    uint64_t n_unmapped;
    uint64_t n_rescue_lines;        /* of n_reported: kind RESCUE */
} spm_sam_stats;
int spm_hip_jst_ref_loci_sam(spm_jst_ref_loci *loci, spm_jst_reads *reads, spm_jst_pairs *pairs /* NULL: single-end */,
                             spm_jst_rescues *rescues /* NULL; needs pairs */, const spm_patterns *patterns,
                             const spm_sam_opts *opts, spm_sam **out);
/* text is NOT NUL-terminated; every pointer may be NULL */
int spm_hip_sam_view(spm_sam *s, const char **text, uint64_t *n_bytes, const spm_sam_line **lines, uint64_t *n_lines);
int spm_hip_sam_device(spm_sam *s, const void **text, uint64_t *n_bytes, const void **lines, uint64_t *n_lines);
int spm_hip_sam_stats(const spm_sam *s, spm_sam_stats *out);
void spm_hip_sam_destroy(spm_sam *s);
/* host only, no device needed.  The header: "@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:<rname>\tLN:<ref_len>\n", not NUL-terminated.
 * *len is what it needs; cap too small: SPM_E_OVERFLOW and nothing is written.  A bad rname: SPM_E_INVALID. */
int spm_hip_sam_header(const char *rname, uint64_t ref_len, char *buf, uint64_t cap, uint64_t *len);
/* the MAPQ of (n_best, n_next) under the tables of opts (only the three mapq members are read); -1: NULL opts or
 * mapq_defaults above 1 */
int spm_hip_sam_mapq(const spm_sam_opts *opts, uint32_t n_best, uint32_t n_next);

/* ---- base qualities and the MD tag: what makes the lines usable by a variant caller without the reference at hand ----------
 * spm_hip_jst_ref_loci_sam_ex and spm_hip_jst_ref_loci_bam_ex are the two calls above and below with one more argument.
 * extras == NULL, or an all-zero extras, gives the bytes of the call without it; the results are the same handles.
 *
 * QUAL.  qual holds Phred values 0 .. 93, the reads back to back in READ order, each as sequenced (forward): read r owns
 * qual[q_off[r] .. q_off[r] + m[strands * r]) with q_off the exclusive sum of the read lengths.  They are copied in the call.
 * A line whose SEQ is the forward read prints them in order; a line whose SEQ is the reverse complement (pattern & 1 in a
 * stranded set, a rescue with flag 0x10) prints them back to front; an unmapped line prints them forward, beside its forward
 * SEQ; a secondary line (SEQ "*") keeps QUAL "*", and l_seq 0 in BAM.  The text gets value + 33, a BAM record the value.  A
 * one-base read with Phred 9 prints "*", which a reader takes for "no qualities": the ambiguity is the SAM specification's own
 * and is left as it is.
 *
 * MD (SPM_SAM_MD, with the resident reference ranks).  Every line that prints a CIGAR carries MD:Z: directly behind NM:i:
 * (kinds LOCUS, RESCUE, SECONDARY_LINE).  The string is computed from the transcript's words as they are; SPM_SAM_CIGAR_M does
 * not change it.  With c the count of matched reference positions, 0 at first, and a reference cursor that starts at ref_begin:
 *     = of length L   c += L
 *     I               nothing: it does not end a match run
 *     X of length L   for each of its L positions: print c, the reference letter, c = 0 (adjacent mismatches are separated by 0)
 *     D of length L   print c, '^', the L reference letters, c = 0
 *     at the end      print c
 * A reference letter is symbols[rank], N for a rank >= sigma.  The result matches [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*.  In BAM the
 * tag is 4d 44 5a, the string, 00.
 * Worked cases (symbols "ACGT"):
 *     20= 1X 11=             G at the X          20G11
 *     5= 2X 3= 2D 1X 4=      AC / GT / A         5A0C3^GT0A4
 *     3X                     ACG                 0A0C0G0
 *     4= 2I 4=                                   8
 *     all I (a locus inside an insertion)        0
 *
 *   * SPM_E_INVALID with a message that names the member, decided on the host before any launch: unknown flags or a nonzero
 *     reserved; SPM_SAM_MD without a reference, or a reference without SPM_SAM_MD; a reference of another context, or whose
 *     sigma is not the needle set's; qual without n_qual or the other way round; n_qual not the sum of the read lengths; a
 *     value above 93; the BAM call only: a reference whose length is not ref_len.
 *   * Counted on the device like every other disagreement, failing the call with SPM_E_INVALID and nothing written: a mapped
 *     line whose [ref_begin, ref_end), or what its transcript spans, does not lie inside the reference; an X column whose
 *     reference rank equals the read's rank there (the reference is not the one the loci were projected against). */
#define SPM_SAM_MD 1u
typedef struct spm_sam_extras {     /* 32 bytes */
    const uint8_t *qual;            /* host: Phred values 0 .. 93; NULL: QUAL "*" / ff */
    uint64_t n_qual;                /* the sum of the read lengths; 0 with qual == NULL */
    const spm_text *reference;      /* the resident reference ranks; needed with SPM_SAM_MD, else NULL */
    uint32_t flags;                 /* SPM_SAM_MD */
    uint32_t reserved;              /* must be 0 */
} spm_sam_extras;
int spm_hip_jst_ref_loci_sam_ex(spm_jst_ref_loci *loci, spm_jst_reads *reads, spm_jst_pairs *pairs /* NULL: single-end */,
                                spm_jst_rescues *rescues /* NULL; needs pairs */, const spm_patterns *patterns,
                                const spm_sam_opts *opts, const spm_sam_extras *extras /* NULL: none */, spm_sam **out);
/* host only, no device needed.  The MD string of one transcript of n_words words whose first reference position is ref_begin,
 * by the serial rendering of the same rule; not NUL-terminated.  *len is what it needs; cap too small: SPM_E_OVERFLOW and
 * nothing is written.  SPM_E_INVALID: a NULL argument (words may be NULL with n_words 0), or a transcript that leaves
 * [0, ref_len). */
int spm_hip_sam_md(const uint32_t *words, uint32_t n_words, const uint8_t *ref_ranks, uint64_t ref_len, uint64_t ref_begin,
                   const char *symbols, char *buf, uint64_t cap, uint64_t *len);

/* ---- BGZF framing of a device buffer: what makes SAM text in HBM a .sam.gz that samtools and tabix read --------------------
 * One call frames n bytes at device_src (any alignment, owned by no handle; read before the call returns) into BGZF blocks in
 * a new device buffer.  Every block is one gzip member with one STORED deflate block -- the uncompressed BGZF that `samtools
 * view -u` writes; nothing is compressed.  A block of d data bytes is d + 31 bytes:
 *     1f 8b 08 04 | MTIME 00 00 00 00 | XFL 00 | OS ff | XLEN 06 00 | 42 43 02 00 | BSIZE = d + 30, u16       18 bytes
 *     01 (BFINAL, BTYPE 00) | LEN = d, u16 | NLEN = ~d, u16                                                   5 bytes
 *     the data                                                                                                d bytes
 *     CRC32 of the data, u32 | ISIZE = d, u32                                                                 8 bytes
 * all little-endian.  With D = block_data, blocks 0 .. nb - 2 hold D bytes and the last one the rest; there is no empty data
 * block: n == 0 gives no block at all.  SPM_BGZF_EOF appends the 28 bytes of the end-of-file block,
 *     1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00.
 * The byte at uncompressed offset u lies at file offset (u / D) * (D + 31) + 23 + u % D, its BGZF virtual offset is
 * ((u / D) * (D + 31)) << 16 | (u % D).  CRC32 is the standard one (reflected 0xEDB88320, initial value and final xor ~0;
 * crc32("123456789") = 0xCBF43926).
 * Worked case, the 6 bytes "abcdef", block_data 4, SPM_BGZF_EOF: 35 + 33 + 28 = 96 bytes,
 *     1f8b08040000000000ff0600424302002200 01 0400 fbff 61626364 11cd82ed 04000000
 *     1f8b08040000000000ff0600424302002000 01 0200 fdff 6566     704982fd 02000000   and the EOF block.
 *
 *   * SPM_E_INVALID with a message, decided on the host before any launch: NULL ctx, opts or out; NULL device_src with n > 0;
 *     block_data above 65280; flag bits other than SPM_BGZF_EOF; a nonzero reserved.
 *   * SPM_E_UNSUPPORTED, likewise: more than 2^31 - 2 blocks (the host-only calls: a framed size beyond 64 bits).
 *   * n == 0: SPM_OK with the EOF block, or with nothing (the views are NULL, 0).
 * The result is a pure function of the bytes and the opts: equal to spm_hip_bgzf_frame_host of the same bytes, host and device
 * view equal.  It outlives the source. */
#define SPM_BGZF_EOF 1u             /* append the end-of-file block */
#define SPM_BGZF_DYNAMIC 4u         /* the deflate calls only: a block may take a Huffman code of its own (see there) */
#define SPM_BGZF_BLOCK_DATA 65280u  /* the default and the most a block holds: htslib's 0xff00 */
typedef struct spm_bgzf_opts {      /* 16 bytes */
    uint32_t block_data;            /* uncompressed bytes per block, 1 .. 65280; 0: 65280 */
    uint32_t flags;                 /* SPM_BGZF_* */
    uint64_t reserved;              /* must be 0 */
} spm_bgzf_opts;
typedef struct spm_bgzf spm_bgzf;
typedef struct spm_bgzf_stats {     /* 32 bytes */
    float ms_frame;                 /* device: the frame stage (HIP events) */
    float ms_host;                  /* wall clock of the whole call (the view is downloaded when first asked for) */
    uint64_t n_in;
    uint64_t n_out;                 /* = n_in + 31 * n_blocks (+ 28 with SPM_BGZF_EOF) */
    uint64_t n_blocks;              /* data blocks; the EOF block is not counted */
} spm_bgzf_stats;
int spm_hip_bgzf_frame(spm_ctx *ctx, const void *device_src, uint64_t n, const spm_bgzf_opts *opts, spm_bgzf **out);
/* every pointer may be NULL */
int spm_hip_bgzf_view(spm_bgzf *z, const void **bytes, uint64_t *n);
int spm_hip_bgzf_device(spm_bgzf *z, const void **bytes, uint64_t *n);
int spm_hip_bgzf_stats(const spm_bgzf *z, spm_bgzf_stats *out);
void spm_hip_bgzf_destroy(spm_bgzf *z);
/* host only, no device needed.  The same container by a serial framer over the same geometry and CRC functions.  *len is what
 * it needs; cap too small: SPM_E_OVERFLOW and nothing is written.  The opts are checked as above. */
int spm_hip_bgzf_frame_host(const void *src, uint64_t n, const spm_bgzf_opts *opts, void *dst, uint64_t cap, uint64_t *len);
int spm_hip_bgzf_framed_size(uint64_t n, const spm_bgzf_opts *opts, uint64_t *len);

/* ---- BGZF blocks with real deflate: LZ77 matches and the fixed Huffman code, per block, on the device -------------------
 * spm_hip_bgzf_deflate is spm_hip_bgzf_frame with the blocks compressed: the same container (BC field, BSIZE = total - 1,
 * CRC32, ISIZE, the same split of n bytes into blocks of block_data, the same EOF block), and the payload of a block is ONE
 * deflate block with BFINAL 1 -- fixed Huffman (BTYPE 01) if that is strictly smaller than the stored form (d + 5 bytes), else
 * the stored block (BTYPE 00) spm_hip_bgzf_frame writes.  So no block is longer than d + 31 and no file longer than the
 * stored file, and BSIZE always fits.  What `samtools view -b` writes, where spm_hip_bgzf_frame is `-u`.
 *
 * The token rule (the output is a pure function of the bytes and the opts: spm_hip_bgzf_deflate_host gives the same bytes):
 *   * Lane t of 256 owns the positions [t c, min((t + 1) c, d)) of a block, c = max(64, ceil(d / 256)).  No token crosses a
 *     chunk border; a match's source lies anywhere earlier in the block and may overlap its target.
 *   * Two candidates per position i.  Near: i - 1.  Far: the largest j with hash4(j) == hash4(i) among the positions of earlier
 *     segments of 256 positions, hash4 = (the four bytes at the position as a little-endian word * 2654435761 mod 2^32) >> 18;
 *     positions with fewer than four bytes behind them in the block have no far candidate and are not hashed.
 *   * Greedy, left to right: at i both candidates are extended, no further than 258 symbols, the chunk's end, or (far) a
 *     distance of 32768.  The longer wins, the near one on a tie.  A match if its length is >= 4, or >= 3 at distance 1; else
 *     the literal.
 *   * Bits: 1 (BFINAL), 1 0 (BTYPE 01), the lanes' tokens in lane order in the RFC 1951 fixed code, the end-of-block code
 *     (seven zeros), zero padding to the byte.
 * Worked cases, block_data 0, SPM_BGZF_EOF (each inflated with zlib; the EOF block follows):
 *   the 6 bytes "abcdef" (six literals, 58 bits), 34 bytes where the stored block takes 37:
 *                                     1f8b08040000000000ff0600424302002100 4b4c4a4e494d0300 ef398e4b 06000000
 *   300 bytes 'a' (lane 0: literal, match 63 at 1; lanes 1 .. 3: match 64 at 1; lane 4: match 44 at 1; 93 bits), 38 bytes:
 *                                     1f8b08040000000000ff0600424302002500 4ba410500a28059402520000 09199789 2c010000
 * A record at offset u of the uncompressed stream has the BGZF virtual offset offsets[u / D] << 16 | u % D, with the offsets
 * of spm_hip_bgzf_blocks.
 *
 * SPM_BGZF_DYNAMIC lets a block take a Huffman code of its own (BTYPE 10), built on the device by the workgroup that parses
 * the block.  The tokens are the same; only their coding may change.  Without the flag every call gives the bytes above.
 * With it, per block of d bytes (again a pure function of the bytes and the opts, and again spm_hip_bgzf_deflate_host's):
 *   1. Counts: the literal/length symbols 0 .. 285 of the block's tokens, symbol 256 once; the distance symbols 0 .. 29.  An
 *      alphabet with fewer than two symbols in use gives count 1 to its lowest-numbered unused symbols until it has two (zlib's
 *      device), so every code the block transmits is complete.
 *   2. Code lengths: an optimal length-limited prefix code, lengths <= 15 (<= 7 for the code-length code): the sum of count x
 *      length is minimal.  Which optimal code: package-merge over the symbols in use sorted by (count, symbol); a level's list
 *      is the symbols merged with the pairwise sums of the level below (an odd last item dropped), a symbol in front of a sum
 *      of equal weight; the first 2n - 2 items of the last level are taken, and the items their sums are made of.  So a symbol
 *      with a larger count never has a longer code, and of two with equal counts the lower-numbered never the shorter one.
 *      Codes are assigned canonically (RFC 1951 3.2.2).
 *   3. Header: HLIT and HDIST from the highest symbol with a nonzero length.  The HLIT + 257 + HDIST + 1 lengths are ONE
 *      sequence (a run may cross from the literal/length part into the distance part), run-length coded greedily from the
 *      left: a run of zeros of 3 or more takes symbol 18 (11 .. 138) or 17 (3 .. 10), each as long as it can be; a run of a
 *      nonzero length is sent once, then by symbol 16 (3 .. 6) while 3 or more remain; what is left goes as plain lengths.
 *      Steps 1 and 2 (limit 7) over the counts of these 19 symbols; HCLEN from the last nonzero entry in the RFC's permuted
 *      order, at least 4.
 *   4. Bits: 1 (BFINAL), 0 1 (BTYPE 10), HLIT in 5 bits, HDIST in 5, HCLEN in 4, 3 bits per code-length code length, the coded
 *      sequence with its extra bits, the lanes' tokens in lane order with their extra bits, the code of symbol 256, zero
 *      padding to the byte.
 *   5. Choice: with s = d + 5, f the fixed payload's bytes and y the dynamic payload's: stored if neither f nor y is below s;
 *      else the smaller of f and y, fixed when they are equal.  So no block is longer than without the flag.
 * Worked cases, block_data 0, no EOF block:
 *   "ab" 20 times (40 literals; lengths: 'a' 2, 'b' 1, 256 2; distance symbols 0 and 1 padded in with length 1; HLIT 0,
 *   HDIST 1, HCLEN 14; 105 bits in front of the first token, 167 in all), 47 bytes where the fixed form takes 68:
 *       1f8b08040000000000ff0600424302002e00 05c181000000008020d6f387b89224499224499264 135ad4bc 28000000
 *   1000 bytes 'a' (lane 0: literal, match 63 at 1; lanes 1 .. 14: match 64 at 1; lane 15: match 40 at 1; HLIT 20, HDIST 1,
 *   HCLEN 14), 53 bytes where the fixed form takes 59:
 *       1f8b08040000000000ff0600424302003400 a5c1010d000000c2a0acf62f61856fc090524a29a594524a29551d 03da389a e8030000
 *   The 6 bytes "abcdef", a block of one byte and the 300 bytes 'a' above keep their fixed form: the dynamic header alone
 *   outweighs them.
 *
 *   * SPM_E_INVALID with a message, decided on the host before any launch: NULL ctx, opts or out; NULL device_src with n > 0;
 *     block_data above 65280; flag bits other than SPM_BGZF_EOF and SPM_BGZF_DYNAMIC (2 stays refused); a level other
 *     than 1; a nonzero reserved.
 *   * SPM_E_UNSUPPORTED, likewise: more than 2^31 - 2 blocks.
 *   * n == 0: SPM_OK with the EOF block, or with nothing.
 * The result is a spm_bgzf: view, device, stats (n_out the real size) and destroy work on it.  It outlives the source. */
typedef struct spm_bgzf_deflate_opts { /* 16 bytes */
    uint32_t block_data;            /* uncompressed bytes per block, 1 .. 65280; 0: 65280 */
    uint32_t flags;                 /* SPM_BGZF_EOF, SPM_BGZF_DYNAMIC */
    uint32_t level;                 /* must be 1: the greedy parse */
    uint32_t reserved;              /* must be 0 */
} spm_bgzf_deflate_opts;
typedef struct spm_bgzf_deflate_stats { /* 72 bytes */
    float ms_parse;                 /* device (HIP events): candidates, parse, bits and CRC of every block */
    float ms_scan;                  /* device: the blocks' file offsets */
    float ms_place;                 /* device: the blocks at their place, the EOF block */
    float ms_host;                  /* wall clock of the whole call */
    uint64_t n_in;
    uint64_t n_out;                 /* the file's bytes, prefix and EOF block included */
    uint64_t n_blocks;              /* data blocks of the device part */
    uint64_t n_stored_blocks;       /* of them, those that did not shrink */
    uint64_t n_matches;             /* tokens of the blocks that were not stored */
    uint64_t n_literals;
    uint64_t n_prefix_bytes;        /* bytes in front of the first data block (spm_hip_bam_deflate: the header's blocks) */
} spm_bgzf_deflate_stats;
int spm_hip_bgzf_deflate(spm_ctx *ctx, const void *device_src, uint64_t n, const spm_bgzf_deflate_opts *opts, spm_bgzf **out);
/* n_blocks + 1 file offsets: of every data block, then the end of the data blocks.  On the host (made when first asked for)
 * and on the device.  Also for a handle of spm_hip_bgzf_frame, where they are b * (D + 31).  Every out pointer may be NULL. */
int spm_hip_bgzf_blocks(spm_bgzf *z, const uint64_t **offsets, uint64_t *n_blocks);
int spm_hip_bgzf_blocks_device(spm_bgzf *z, const void **offsets, uint64_t *n_blocks);
/* of a handle of spm_hip_bgzf_frame: every block stored, no tokens, ms_place the frame stage */
int spm_hip_bgzf_deflate_stats(const spm_bgzf *z, spm_bgzf_deflate_stats *out);
/* the handle's data blocks that came out stored (n[0]), fixed (n[1]) and dynamic (n[2]); they sum to n_blocks.  Of a handle
 * of spm_hip_bgzf_frame every block is stored.  A NULL argument: SPM_E_INVALID. */
int spm_hip_bgzf_block_types(const spm_bgzf *z, uint64_t n[3]);
/* host only, no device needed: the same bytes by the serial rendering of the same rule.  *len is what it needs
 * (spm_hip_bgzf_deflate_bound is enough: the stored size, with SPM_BGZF_DYNAMIC too); cap too small: SPM_E_OVERFLOW and nothing is written. */
int spm_hip_bgzf_deflate_host(const void *src, uint64_t n, const spm_bgzf_deflate_opts *opts, void *dst, uint64_t cap, uint64_t *len);
int spm_hip_bgzf_deflate_bound(uint64_t n, const spm_bgzf_deflate_opts *opts, uint64_t *len);

/* ---- BAM records in BGZF blocks: the same alignments as spm_hip_jst_ref_loci_sam, as the file its users store ---------------
 * One call turns (loci, read summary, optionally pairs and rescues, needle set) into a complete BAM file in HBM: the header
 * section (framed on the host into blocks of its own, so that records start at a block border, as htslib writes them), the
 * record stream framed by the kernel of spm_hip_bgzf_frame, the EOF block.  Which records exist, in which order, with which
 * FLAG, MAPQ, mate fields and counts is the rule of spm_hip_jst_ref_loci_sam, line for line: record i is line i, and
 * `samtools view -h` of the file prints spm_hip_sam_header + that call's text, with XN X0 X1 typed as unsigned.
 * The handle has three views, each on the host (downloaded when first asked for) and on the device: the file; the
 * uncompressed record stream; one spm_sam_line per record whose offset / len locate the record (len = block_size + 4) in that
 * stream.  The record at stream offset u has the BGZF virtual file offset
 *     (header_file_bytes + (u / D) * (D + 31)) << 16 | (u % D)            D = block_data, 65280 by default
 * which is what a .bai or .csi would be built from (none is written).
 *
 * A record is little-endian; block_size counts what follows it:
 *     block_size i32 | refID i32 | pos i32 | l_read_name u8 | mapq u8 | bin u16 | n_cigar_op u16 | flag u16 | l_seq u32 |
 *     next_refID i32 | next_pos i32 | tlen i32 | read_name NUL-terminated | cigar u32[n_cigar_op] | seq u8[(l_seq+1)/2] |
 *     qual u8[l_seq] | tags
 * refID: RNAME printed 0, "*" -1.  pos: POS - 1 (POS 0: -1).  next_refID: "=" 0, "*" -1.  next_pos: PNEXT - 1.  read_name: the
 * QNAME bytes, l_read_name counts the NUL.  cigar: the transcript's words as they are (len << 4 | op with I 1, D 2, = 7, X 8 is
 * BAM's encoding); with SPM_SAM_CIGAR_M every maximal run of = / X words is one word sum << 4 | 0 and n_cigar_op counts items; a
 * line with CIGAR "*" has n_cigar_op 0.  seq: two symbols per byte, the first in the high nibble, the code of a letter its place
 * in "=ACMGRSVTWYHKDBN" in either case, any other letter or a rank >= sigma 15; a secondary (SEQ "*") has l_seq 0; with odd l_seq
 * the last low nibble is 0.  qual: l_seq bytes ff, or with the qualities of spm_sam_extras the values themselves.  bin: the specification's reg2bin(pos, pos + max(span, 1)) with span the
 * reference symbols of the transcript (= X D), 0 on an unmapped record -- a locus inside an insertion takes end = pos + 1; pos -1
 * gives 4680.  tags, in the text's order, SEVEN BYTES EACH whatever the value, on purpose (a record's length does not depend on
 * its values): NM XH XR are type i (int32), XN X0 X1 type I (uint32: the counts arrive clamped to 0xFFFFFFFF).  The one
 * exception is MD (SPM_SAM_MD of spm_sam_extras), type Z, directly behind NM: 4d 44 5a, the string, 00 -- the first tag whose
 * length depends on its values.  An unmapped record has none.
 *
 * Worked records (the worked SAM cases above; rname "chr", default tables, no names), in hex, fields separated by spaces:
 *  1. Case 1 (read 7 reverse at [99,131), words 20= 1X 11=, MAPQ 40) with a SEQ of 32 A, without SPM_SAM_CIGAR_M, 133 bytes:
 *       81000000 00000000 63000000 02 28 4912 0300 1000 20000000 ffffffff ffffffff 00000000 3700
 *       47010000 18000000 b7000000  11 x 16  ff x 32  4e4d69 01000000  584869 00000000  584e49 02000000  583049 01000000
 *       583149 01000000          and with SPM_SAM_CIGAR_M, 125 bytes:  79000000 ... 0100 1000 ... 3700  00020000  11 x 16 ...
 *  2. The unmapped mate of case 4 (flag 133 beside a mate at POS 501) with the SEQ ACG, 43 bytes:
 *       27000000 00000000 f4010000 02 00 4912 0000 8500 03000000 00000000 f4010000 00000000 3000  1240  ffffff
 *  3. A secondary of pair 0's mate 2 at [7000,7004), words 4=, flag 401, mate at POS 1001, 1 haplotype, 63 bytes:
 *       3b000000 00000000 581b0000 02 ff 4912 0100 9101 00000000 00000000 e8030000 00000000 3000  47000000
 *       4e4d69 00000000  584869 00000000  584e49 01000000
 *
 *   * Everything spm_hip_jst_ref_loci_sam refuses, with the same codes; the sam member of the opts is that call's opts.
 *   * SPM_E_INVALID: ref_len == 0; block_data above 65280; a nonzero reserved.  SPM_E_UNSUPPORTED: ref_len above 2^31 - 1; more
 *     than 2^31 - 2 record blocks.
 *     Where several refusals apply to one call, which of them is reported is not specified.
 *   * Counted on the device like every other disagreement of the inputs, and failing the call with SPM_E_INVALID and nothing
 *     written: a record of more than 65535 CIGAR items; an item of length 0, or a merged run above 2^28 - 1; a mapped record
 *     that ends beyond ref_len.
 *   * Zero reads: the header section and the EOF block, which is a valid empty BAM.
 * A pure function of its inputs: byte-identical across runs, host and device views equal.  It outlives all inputs. */
typedef struct spm_bam_opts {       /* 80 bytes */
    spm_sam_opts sam;               /* as for spm_hip_jst_ref_loci_sam: the same flags, the same MAPQ tables */
    uint64_t ref_len;               /* 1 .. 2^31 - 1: l_ref and the @SQ line's LN */
    uint32_t block_data;            /* as in spm_bgzf_opts */
    uint32_t reserved;              /* must be 0 */
} spm_bam_opts;
typedef struct spm_bam spm_bam;
typedef struct spm_bam_stats {      /* 104 bytes */
    float ms_total;                 /* device: the five stages below (HIP events) */
    float ms_lines;                 /* shared with spm_hip_jst_ref_loci_sam */
    float ms_measure;               /* the length and shape of every record, the offsets */
    float ms_write;                 /* the record stream, one wave per record */
    float ms_frame;                 /* the record stream into BGZF blocks behind the header section, the EOF block */
    float ms_stats;                 /* offsets into the line records, the counts */
    float ms_host;                  /* wall clock of the whole call (the views are downloaded when first asked for) */
    uint32_t reserved;
    uint64_t n_records;             /* = n_reported + n_secondary + n_unmapped */
    uint64_t n_record_bytes;        /* the uncompressed record stream */
    uint64_t n_file_bytes;          /* = header_file_bytes + n_record_bytes + 31 * n_record_blocks + 28 */
    uint64_t header_file_bytes;     /* the framed header section: where the first record block starts */
    uint64_t n_record_blocks;
    uint64_t n_reported;            /* as in spm_sam_stats */
    uint64_t n_secondary;
    uint64_t n_unmapped;
    uint64_t n_rescue_lines;
} spm_bam_stats;
int spm_hip_jst_ref_loci_bam(spm_jst_ref_loci *loci, spm_jst_reads *reads, spm_jst_pairs *pairs /* NULL: single-end */,
                             spm_jst_rescues *rescues /* NULL; needs pairs */, const spm_patterns *patterns,
                             const spm_bam_opts *opts, spm_bam **out);
/* the same with base qualities and the MD tag (spm_sam_extras above; its reference has ref_len symbols) */
int spm_hip_jst_ref_loci_bam_ex(spm_jst_ref_loci *loci, spm_jst_reads *reads, spm_jst_pairs *pairs /* NULL: single-end */,
                                spm_jst_rescues *rescues /* NULL; needs pairs */, const spm_patterns *patterns,
                                const spm_bam_opts *opts, const spm_sam_extras *extras /* NULL: none */, spm_bam **out);
/* every pointer may be NULL */
int spm_hip_bam_view(spm_bam *b, const void **file, uint64_t *n_file, const void **records, uint64_t *n_record_bytes,
                     const spm_sam_line **lines, uint64_t *n_lines);
int spm_hip_bam_device(spm_bam *b, const void **file, uint64_t *n_file, const void **records, uint64_t *n_record_bytes,
                       const void **lines, uint64_t *n_lines);
int spm_hip_bam_stats(const spm_bam *b, spm_bam_stats *out);
void spm_hip_bam_destroy(spm_bam *b);
/* host only, no device needed.  The FRAMED header section: "BAM\1", l_text, the bytes of spm_hip_sam_header, n_ref = 1, l_name,
 * the name with its NUL, l_ref, in BGZF blocks of block_data (0: 65280) without an EOF block.  *len is what it needs; cap too
 * small: SPM_E_OVERFLOW and nothing is written.  rname, ref_len and block_data are checked as above. */
int spm_hip_bam_header(const char *rname, uint64_t ref_len, uint32_t block_data, void *buf, uint64_t cap, uint64_t *len);
/* The file of a BAM handle with its blocks deflated (spm_hip_bgzf_deflate's rule and refusals; b NULL: SPM_E_INVALID): the
 * plain header section deflated on the host into blocks of its own, the handle's device record stream deflated by the kernels
 * behind it, the EOF block with SPM_BGZF_EOF.  The result's view and device hold the whole file; the offsets of
 * spm_hip_bgzf_blocks are absolute file offsets of the record blocks, n_prefix_bytes is where the first one starts.  The
 * result needs the BAM handle no longer once the call returns. */
int spm_hip_bam_deflate(spm_bam *b, const spm_bgzf_deflate_opts *opts, spm_bgzf **out);

/* ---- coordinate-sorted BAM and its BAI index: what a variant caller, a pile-up and `samtools view chr:a-b` need -----------
 * spm_hip_bam_sort returns a NEW spm_bam with the records of b in coordinate order: view, device, stats, destroy,
 * spm_hip_bam_deflate and this call again work on it unchanged.  Its header section says SO:coordinate
 * (spm_hip_sam_header_sorted / spm_hip_bam_header_sorted are the host-only siblings of the header calls, which keep their
 * bytes), its line records are those of b, permuted, with their new offset.  The counts and byte totals of its spm_bam_stats
 * are the new file's; the stage times of the call are spm_hip_bam_sort_stats' (SPM_E_INVALID on a handle no sort made).
 * The order: refID as unsigned (0, then -1), then pos, then forward before reverse (flag 0x10); ties keep the order of b.  A
 * placed unmapped mate (refID 0, pos the mate's) therefore stands beside its mate; records with refID -1 go to the end.
 * Sorting a sorted handle gives byte-identical views.  Zero records: the header section and the EOF block.
 *   * SPM_E_INVALID: NULL b or out; a nonzero reserved (opts may be NULL).  SPM_E_UNSUPPORTED: more than 2^32 - 1 records
 *     (cannot occur today).  A handle whose line records do not name records of its stream (they always do) fails with
 *     SPM_E_INVALID after one read-back, and nothing is returned.
 *
 * spm_hip_bam_index builds the BAI (SAM specification 5.2) of the handle's own stored file, or, with `deflated` the result of
 * spm_hip_bam_deflate(b, ...) in blocks of the same block_data, of that file; spm_hip_bai_build is the raw form over any
 * device record stream, its spm_sam_line records (offset / len), and the n_blocks + 1 file offsets of its blocks;
 * spm_hip_bai_build_host the same bytes by a serial walk on the host, no device needed.  The rule:
 *   * A record's interval is [pos, pos + max(span, 1)), span the reference symbols of its CIGAR (M D N = X); pos + 1 with
 *     flag 0x4 or without CIGAR -- what the writer binned it with.  Its bin is the record's bin field.
 *   * The virtual offset of stream offset u is offsets[u / D] << 16 | u % D.  A record begins at that of its offset and ends
 *     at that of offset + len: a record that ends on a block border ends at the next block's first byte, the stream's last
 *     one possibly at the EOF block.
 *   * The file: "BAI\1", n_ref = 1, n_bin, the bins, n_intv, the linear index, n_no_coor (always written), little-endian.
 *   * A bin's chunks are the maximal runs of CONSECUTIVE records in file order that carry the bin: (begin of the first,
 *     end of the last).  Bins in ascending number, a bin's chunks in file order, not merged further (htslib also merges
 *     chunks that meet in one block; a reader finds the same records either way).
 *   * If the reference has a record, the pseudo-bin 37450 comes last and counts in n_bin: (begin of the first placed record,
 *     end of the last), (n_mapped, n_unmapped) = the records with refID >= 0 without / with flag 0x4.
 *   * n_intv = ((max end - 1) >> 14) + 1 over the placed records; ioffset[w] the smallest begin among the records that
 *     overlap window w, an empty window taking the value of the next one to its right that is not.
 *   * n_no_coor: the records with refID -1.
 * Worked cases.  No records: 24 bytes,  42414901 01000000 00000000 00000000 0000000000000000.
 * Four records of one name byte and at most one CIGAR word, block_data 100, stored blocks from file offset 0 (offsets 0, 131,
 * 226):  42 bytes at 0, pos 100, 50M (bin 4681);  42 at 42, pos 16380, 10M (crosses 2^14: bin 585);  42 at 84, pos 16390, 10M,
 * reverse (bin 4682, ends in block 1 at byte 26);  38 at 126, refID -1.  152 bytes:
 *     42414901 01000000 04000000
 *     49020000 01000000 2a00000000000000 5400000000000000
 *     49120000 01000000 0000000000000000 2a00000000000000
 *     4a120000 01000000 5400000000000000 1a00830000000000
 *     4a920000 02000000 0000000000000000 1a00830000000000 0300000000000000 0000000000000000
 *     02000000 0000000000000000 2a00000000000000
 *     0100000000000000
 *   * SPM_E_INVALID, decided on the host: NULL b, ctx or out; NULL buffers with nonzero counts; block_data above 65280 (0:
 *     65280); n_blocks that is not what n_record_bytes in blocks of block_data give; records without lines or lines without
 *     records; a `deflated` of another context, input length or block size.  SPM_E_UNSUPPORTED: more than 2^32 - 1 records.
 *   * Counted on the device, tested before a value is used as an index, and failing the call with SPM_E_INVALID and nothing
 *     written: a record out of coordinate order (key(i) < key(i - 1)); a line that leaves the stream or does not start
 *     where the one before it ended (the first at 0, the last ending the stream); a block_size that is not len - 4; a name
 *     and CIGAR that leave the record; a refID other than 0 and -1; a placed record with pos < 0, an end beyond 2^29 (the
 *     reach of a BAI) or a bin field beyond 37448.
 * One read-back brings the counts, which give the size, and the error counter.  A pure function of its inputs: host and
 * device builder agree byte for byte (min into the linear index does not depend on order). */
typedef struct spm_bam_sort_opts {  /* 8 bytes */
    uint64_t reserved;              /* must be 0 */
} spm_bam_sort_opts;
typedef struct spm_bam_sort_stats { /* 48 bytes */
    float ms_total;                 /* device: the five stages below (HIP events) */
    float ms_keys;                  /* the key fields of every record out of the stream */
    float ms_sort;                  /* the stable radix sort of (key, record index) over key_bits */
    float ms_place;                 /* the new offsets, the permuted line records */
    float ms_gather;                /* the records to their new place, one wave per record */
    float ms_frame;                 /* the new stream into BGZF blocks behind the new header section, the EOF block */
    float ms_host;                  /* wall clock of the whole call */
    uint32_t key_bits;              /* what ref_len needs, the strand bit and the refID bit */
    uint64_t n_records;
    uint64_t n_record_bytes;
} spm_bam_sort_stats;
int spm_hip_bam_sort(spm_bam *b, const spm_bam_sort_opts *opts /* NULL: defaults */, spm_bam **out);
int spm_hip_bam_sort_stats(const spm_bam *b, spm_bam_sort_stats *out);
/* host only: spm_hip_sam_header / spm_hip_bam_header with "SO:coordinate" */
int spm_hip_sam_header_sorted(const char *rname, uint64_t ref_len, char *buf, uint64_t cap, uint64_t *len);
int spm_hip_bam_header_sorted(const char *rname, uint64_t ref_len, uint32_t block_data, void *buf, uint64_t cap, uint64_t *len);
typedef struct spm_bai spm_bai;
typedef struct spm_bai_stats {      /* 80 bytes */
    float ms_total;                 /* device: the four stages below (HIP events) */
    float ms_records;               /* every record's item, the order test, the linear index's minima, the counts */
    float ms_chunks;                /* runs into chunks, the chunks ordered by bin */
    float ms_bins;                  /* bin heads, the byte offsets */
    float ms_write;                 /* the back-fill of the linear index, the bytes */
    float ms_host;                  /* wall clock of the whole call */
    uint64_t n_bins;                /* the file's n_bin: the pseudo-bin is counted */
    uint64_t n_chunks;              /* of the bins that hold records */
    uint64_t n_intv;
    uint64_t n_mapped;
    uint64_t n_unmapped;
    uint64_t n_no_coor;
    uint64_t n_bytes;
} spm_bai_stats;
int spm_hip_bam_index(spm_bam *b, spm_bgzf *deflated /* NULL: the handle's own stored file */, spm_bai **out);
int spm_hip_bai_build(spm_ctx *ctx, const void *device_records, uint64_t n_record_bytes, const void *device_lines, uint64_t n_lines,
                      const void *device_block_offsets, uint64_t n_blocks, uint32_t block_data, spm_bai **out);
int spm_hip_bai_build_host(const void *records, uint64_t n_record_bytes, const spm_sam_line *lines, uint64_t n_lines,
                           const uint64_t *block_offsets, uint64_t n_blocks, uint32_t block_data, void *dst, uint64_t cap, uint64_t *len);
/* every pointer may be NULL */
int spm_hip_bai_view(spm_bai *z, const void **bytes, uint64_t *n);
int spm_hip_bai_device(spm_bai *z, const void **bytes, uint64_t *n);
int spm_hip_bai_stats(const spm_bai *z, spm_bai_stats *out);
void spm_hip_bai_destroy(spm_bai *z);

/* ---- duplicate reads and pairs marked with FLAG 0x400: the step between "sort" and "index" (samtools markdup, Picard) ------
 * spm_hip_bam_markdup returns a NEW spm_bam that differs from b in bit 0x400 of every record's flag (one byte per record, at
 * record offset 19, and the flag of the record's line) and in the CRC32 of the re-framed blocks, nothing else: the header
 * section with its SO:, record order, offsets and lengths, rname, ref_len, block_data, sorted and the sort stats are b's.
 * view, device, stats, destroy, spm_hip_bam_deflate, spm_hip_bam_sort, spm_hip_bam_index and this call again work on it
 * unchanged; the stage times and counts of the call are spm_hip_bam_markdup_stats'.  spm_hip_bam_markdup_records is the raw
 * form over any device record stream and its spm_sam_line records (offset, len, read): dup[i] = 1 iff record i is a duplicate;
 * spm_hip_bam_markdup_host the same bytes by a serial walk on the host (maps, no sort), no device needed.  The rule, a
 * function of the record stream and the line records alone:
 *   * Which records take part.  Read r's PRIMARY RECORD is the one line with lines.read == r whose record's flag has neither
 *     0x100 nor 0x800; mates are reads 2p and 2p + 1.  r is PLACED if its primary record exists and lacks 0x4.  Secondary and
 *     unmapped records never take part: their 0x400 comes out clear.
 *   * The 5' end (u, s) of a placed read: s is flag 0x10; u = pos on the forward strand, u = end - 1 on the reverse strand,
 *     end = pos + max(span, 1) with span the reference symbols of the CIGAR (M D N = X), the record's end in the BAI rule.
 *     CIGAR items S and H are refused (the writers make none): unclipped ends are out of scope.
 *   * A placed read is a PAIR END if its primary flag has 0x1, read r ^ 1 is placed and that read's primary flag has 0x1;
 *     any other placed read is a FRAGMENT.
 *   * The score of a record is the sum of its qual bytes v with min_qual <= v <= 93, clamped to 2^24 - 1: the ff fill scores
 *     0.  A pair's score is the sum of its two mates' scores.
 *   * Pairs.  The key of pair p is its two ends ordered by (u, s): (u_lo, s_lo, u_hi, s_hi).  Which mate is the lower end is
 *     NOT part of the key -- a fixed choice: Picard tells F1F2 from F2F1, this rule does not.  Among pairs of equal key the one
 *     with the highest score stays, ties going to the lowest p; every other pair of that key is a duplicate, on BOTH primary
 *     records.
 *   * Fragments.  A fragment whose (u, s) is an end of ANY pair is a duplicate, whether or not that pair is one itself.  Among
 *     the remaining fragments of equal (u, s) the highest score stays, ties going to the lowest r; the others are duplicates.
 *   * An incoming 0x400 is ignored and recomputed: marking a marked handle is byte-identical.  Nothing depends on record
 *     order: sort-then-mark and mark-then-sort have byte-identical views.
 * Worked cases (ref_len 10000, refID 0, no qualities; POS as SAM prints it):
 *     read 0   FLAG 0   POS 101  40=   (100, +)   stays
 *     read 1   FLAG 0   POS 101  30=   (100, +)   duplicate of 0
 *     read 2   FLAG 16  POS 112  30=   (140, -)   stays
 *     read 3   FLAG 16  POS 102  40=   (140, -)   duplicate of 2, although POS differs
 *     read 4   FLAG 16  POS 101  40=   (139, -)   stays
 *     reads 6, 7     a pair  (1000, +) / (1199, -)   stay
 *     reads 8, 9     a pair  (1000, +) / (1199, -)   pair 4 is a duplicate, both records
 *     reads 10, 11   a pair  (1000, +) / (1299, -)   stay
 *     read 12  its mate 13 unmapped  (1000, +)     duplicate: a pair end sits there
 *     read 13  flag 0x4, placed beside 12          unchanged
 *   If read 1 carries 30 values of Phred 30 and read 0 40 values of Phred 10 (below the default min_qual), read 0 is the duplicate.
 *   * SPM_E_INVALID, decided on the host before any launch: NULL arguments (opts and stats may be NULL); nonzero flags or
 *     reserved; min_qual above 93; buffers without counts or counts without buffers.  SPM_E_UNSUPPORTED: more than 2^32 - 1
 *     records; ref_len >= 2^30 (a pair key needs 2 * bits(ref_len) + 2 bits of the 64 the sort takes, and a BAI reaches 2^29).
 *   * Counted on the device, each test before a value is used as an index, brought back with the counts in ONE read-back,
 *     and failing the call with SPM_E_INVALID, nothing returned or written, never a fault: a line that leaves the stream; a
 *     block_size that is not len - 4; a name or CIGAR that leaves the record; an l_seq whose seq and qual leave the record;
 *     lines.read >= n_lines; two primary records of one read; a placed primary record with a refID other than 0, pos < 0,
 *     end > ref_len or a CIGAR item S or H.
 *   * Zero records: the header section and the EOF block.
 * A pure function of its inputs: host and device agree byte for byte across runs; the result outlives b. */
typedef struct spm_bam_markdup_opts {  /* 16 bytes */
    uint32_t min_qual;              /* 0: 15; above 93: SPM_E_INVALID */
    uint32_t flags;                 /* must be 0 */
    uint64_t reserved;              /* must be 0 */
} spm_bam_markdup_opts;
typedef struct spm_bam_markdup_stats { /* 88 bytes */
    float ms_total;                 /* device: the five stages below (HIP events) */
    float ms_keys;                  /* primary records claimed; 5' end and score of every placed one, one wave per record */
    float ms_sort;                  /* pairs, then ends: by inverted score, then stably by key */
    float ms_mark;                  /* "my key is my left neighbour's" by read, then by line; the counts */
    float ms_write;                 /* the stream copied, one byte per record, the line records (0 in the raw form) */
    float ms_frame;                 /* the stream into BGZF blocks behind the header section (0 in the raw form) */
    float ms_host;                  /* wall clock of the whole call */
    uint32_t reserved;
    uint64_t n_records;
    uint64_t n_pairs;
    uint64_t n_fragments;
    uint64_t n_dup_pairs;
    uint64_t n_dup_fragments;
    uint64_t n_dup_records;         /* 2 n_dup_pairs + n_dup_fragments */
    uint64_t n_fragments_beside_pairs; /* of n_dup_fragments: a pair end sits at their (u, s) */
} spm_bam_markdup_stats;
int spm_hip_bam_markdup(spm_bam *b, const spm_bam_markdup_opts *opts /* NULL: defaults */, spm_bam **out);
/* SPM_E_INVALID on a handle no markdup made */
int spm_hip_bam_markdup_stats(const spm_bam *b, spm_bam_markdup_stats *out);
/* dup is a caller-owned device buffer of n_lines bytes, written behind the read-back */
int spm_hip_bam_markdup_records(spm_ctx *ctx, const void *device_records, uint64_t n_record_bytes, const void *device_lines,
                                uint64_t n_lines, uint64_t ref_len, const spm_bam_markdup_opts *opts /* NULL: defaults */,
                                void *device_dup, spm_bam_markdup_stats *stats /* NULL */);
int spm_hip_bam_markdup_host(const void *records, uint64_t n_record_bytes, const spm_sam_line *lines, uint64_t n_lines,
                             uint64_t ref_len, const spm_bam_markdup_opts *opts /* NULL: defaults */, uint8_t *dup);

/* ---- the per-base pileup of a coordinate-sorted BAM handle, and its variant sites (samtools depth / mpileup, the candidate
 * step of a variant caller): the first consumer of the sorted, duplicate-marked stream ---------------------------------------
 * spm_hip_bam_pileup counts, for every reference position of a region [begin, end), how many records show A, C, G, T, another
 * symbol, a deletion, an insertion behind the position, or a base below the quality threshold: counts[plane * n + (pos -
 * begin)], n = end - begin, uint32, plane-major, the planes in the order SPM_PILEUP_A .. SPM_PILEUP_LOWQ.  The handle form
 * works on any spm_bam whose records are in coordinate order (an unsorted one is refused by the order test, not by a flag); on
 * a handle out of spm_hip_bam_markdup the duplicates are left out by the default exclude_flags.  spm_hip_bam_pileup_records is
 * the raw form over any device record stream and its spm_sam_line records (offset and len are read), spm_hip_bam_pileup_host
 * the same counts by a serial walk on the host, no device needed.  The rule, a function of the stream, the line records
 * (offset, len), ref_len, the region and the options alone:
 *   * Which records take part: flag lacks 0x4, flag & exclude_flags == 0, mapq >= min_mapq, at least one CIGAR item.  Any
 *     other record is skipped, not refused.
 *   * The walk.  r = pos, q = 0; for each CIGAR item (op, len):
 *       M = X (0 7 8)   for j < len, column r + j: the quality byte qual[q + j] below min_baseq adds 1 to LOWQ; otherwise the
 *                       4-bit SEQ code at q + j adds 1 to its plane (1 A, 2 C, 4 G, 8 T, any other code N).  r += len, q += len.
 *                       A quality of ff (absent) passes every threshold, as in htslib.
 *       D (2)           1 to DEL at r .. r + len - 1; r += len.
 *       N (3)           r += len; nothing is counted.
 *       I (1)           1 to INS at column r - 1 if r > pos (a leading insertion is dropped); q += len.
 *       S (4)           q += len.      H P (5 6)   nothing.
 *     Only columns inside [begin, end) are counted.  A record's end is pos + max(span, 1), the BAI rule.
 *   * Overlapping mates of a pair are counted twice, once per record, as samtools depth counts them.
 *   * Depth is A + C + G + T + N + DEL.  INS and LOWQ are outside it.
 * Worked table (ref_len 1000, refID 0, min_baseq 0, forward records; POS 0-based; qualities ff unless given):
 *      0   10   4M           ACGT      A@10 C@11 G@12 T@13
 *      1   10   2=1X1=       ACNT      A@10 C@11 N@12 T@13
 *      2   11   2M2D2M       CGAA      C@11 G@12 DEL@13,14 A@15 A@16
 *      3   12   2M3N2M       GTCC      G@12 T@13, nothing at 14..16, C@17 C@18
 *      4   12   2I3M         TTGTA     the leading I is dropped: G@12 T@13 A@14
 *      5   12   2S1I3M       AATGTA    S, then I with r == pos, dropped: G@12 T@13 A@14
 *      6   13   2M2I2M       TAGGAC    T@13 A@14 INS@14 A@15 C@16
 *      7   13   3M2S         TAACC     T@13 A@14 A@15
 *      8   14   2H3M1P2M3H   AACAC     A@14 A@15 C@16 A@17 C@18
 *      9   15   3M           ACG, qual 0 20 ff   A@15 C@16 G@17; min_baseq 1: LOWQ@15 C@16 G@17; min_baseq 93: LOWQ@15,16 G@17
 *     10   15   3M flag 0x400   AAA    nothing by default; A@15,16,17 with exclude_flags 0x4
 *     11   unplaced, flag 0x4          nothing
 *   * SPM_E_INVALID, decided on the host before any launch: NULL arguments (opts may be NULL); nonzero flags or reserved
 *     fields; min_baseq above 93; begin > end or end > ref_len (end 0: ref_len); buffers without counts or counts without
 *     buffers.  SPM_E_UNSUPPORTED: more than 2^32 - 1 records; ref_len above 2^31.
 *   * Counted on the device in one counter, each test before a value is used as an index, brought back in ONE read-back, and
 *     failing the call with SPM_E_INVALID, nothing returned or written, never a fault: a line that leaves the stream; a
 *     block_size that is not len - 4; a name, CIGAR, SEQ or QUAL that leaves the record; a record that takes part with a
 *     refID other than 0, pos < 0 or end > ref_len, a CIGAR op code above 8, or a CIGAR query length that is not l_seq (SEQ *
 *     beside a CIGAR, what a secondary line of spm_hip_jst_ref_loci_bam carries: leave 0x100 in exclude_flags); records
 *     out of coordinate order (pos descending among the records of refID 0, or a record of refID 0 behind one of another
 *     refID).  The order is a precondition, as it is for samtools mpileup and for spm_hip_bai_build; the host builder refuses
 *     the same inputs.
 *   * Zero records give all-zero counts, an empty region a view of length 0.
 * A pure function of its inputs: integer adds commute, host and device agree byte for byte across runs; the result outlives b.
 *
 * spm_hip_pileup_sites compares a finished pileup with the resident reference (a dna4 spm_text of ranks, the handle
 * spm_sam_extras.reference takes; shorter than the pileup's end, another sigma or another context: SPM_E_INVALID) and returns,
 * in position order, the columns with depth >= min_depth, alt >= min_alt and 1000 * alt >= min_alt_permille * depth, where
 * alt = depth - counts[plane of the reference base] + INS (a reference rank above 3 takes plane N).  A site's counts[4] are the
 * four base planes A C G T: N + DEL is depth less their sum, and INS is alt - (depth - counts[ref]).  spm_hip_pileup_sites_host
 * is the serial twin over host arrays: cap records at dst, *n the number of sites, SPM_E_OVERFLOW with *n set when cap is too small. */
enum { SPM_PILEUP_A = 0, SPM_PILEUP_C, SPM_PILEUP_G, SPM_PILEUP_T, SPM_PILEUP_N, SPM_PILEUP_DEL, SPM_PILEUP_INS, SPM_PILEUP_LOWQ,
       SPM_PILEUP_PLANES };
typedef struct spm_pileup_opts {   /* 32 bytes */
    uint64_t begin, end;           /* end 0: ref_len; begin <= end <= ref_len else SPM_E_INVALID */
    uint32_t exclude_flags;        /* 0: 0x704 (UNMAP | SECONDARY | QCFAIL | DUP); 0x4 is always excluded */
    uint8_t  min_mapq, min_baseq;  /* min_baseq above 93: SPM_E_INVALID */
    uint16_t reserved0;            /* must be 0 */
    uint32_t flags, reserved1;     /* must be 0 */
} spm_pileup_opts;
typedef struct spm_pileup_stats {  /* 88 bytes */
    float ms_total;                /* device: the four stages below (HIP events) */
    float ms_records;              /* every record read and tested, the order test, pos and end */
    float ms_scan;                 /* the running maximum of end */
    float ms_tiles;                /* one workgroup per tile: the counters in LDS, the plane segments stored */
    float ms_summary;              /* n_covered, sum_depth, max_depth, n_evidence from the finished planes */
    float ms_host;                 /* wall clock of the whole call */
    uint32_t tile_positions;       /* positions per tile of this build (not part of the ABI's promises) */
    uint32_t reserved;
    uint64_t n_records;
    uint64_t n_taking_part;
    uint64_t n_evidence;           /* the sum of all planes */
    uint64_t n_covered;            /* positions with depth > 0 */
    uint64_t sum_depth;
    uint64_t max_depth;
    uint64_t n_tile_visits;        /* records walked by tiles, a record once per tile it reaches into: the scheme's redundancy */
} spm_pileup_stats;
typedef struct spm_pileup_site {   /* 32 bytes */
    uint32_t pos;
    uint32_t depth;
    uint32_t alt;
    uint32_t counts[4];            /* the base planes A C G T */
    uint8_t ref;                   /* the reference rank at pos */
    uint8_t reserved[3];
} spm_pileup_site;
typedef struct spm_pileup_site_opts { /* 16 bytes */
    uint32_t min_depth, min_alt, min_alt_permille; /* NULL opts: 1, 2, 200 */
    uint32_t flags;                /* must be 0 */
} spm_pileup_site_opts;
typedef struct spm_pileup spm_pileup;
typedef struct spm_pileup_sites spm_pileup_sites;
int spm_hip_bam_pileup(spm_bam *b, const spm_pileup_opts *opts /* NULL: defaults */, spm_pileup **out);
int spm_hip_bam_pileup_records(spm_ctx *ctx, const void *device_records, uint64_t n_record_bytes, const void *device_lines,
                               uint64_t n_lines, uint64_t ref_len, const spm_pileup_opts *opts /* NULL: defaults */, spm_pileup **out);
/* counts: 8 * (end - begin) values, written only when the call succeeds */
int spm_hip_bam_pileup_host(const void *records, uint64_t n_record_bytes, const spm_sam_line *lines, uint64_t n_lines,
                            uint64_t ref_len, const spm_pileup_opts *opts /* NULL: defaults */, uint32_t *counts);
/* the host view is downloaded when first asked for; n_positions = end - begin; every out pointer may be NULL */
int spm_hip_pileup_view(spm_pileup *p, const uint32_t **counts, uint64_t *n_positions);
int spm_hip_pileup_device(spm_pileup *p, const void **counts, uint64_t *n_positions);
int spm_hip_pileup_stats(const spm_pileup *p, spm_pileup_stats *out);
void spm_hip_pileup_destroy(spm_pileup *p);
int spm_hip_pileup_sites(spm_pileup *p, const spm_text *reference, const spm_pileup_site_opts *opts /* NULL: defaults */,
                         spm_pileup_sites **out);
int spm_hip_pileup_sites_view(spm_pileup_sites *s, const spm_pileup_site **sites, uint64_t *n);
int spm_hip_pileup_sites_device(spm_pileup_sites *s, const void **sites, uint64_t *n);
void spm_hip_pileup_sites_destroy(spm_pileup_sites *s);
int spm_hip_pileup_sites_host(const uint32_t *counts, uint64_t begin, uint64_t n_positions, const uint8_t *ref_ranks, uint64_t ref_len,
                              const spm_pileup_site_opts *opts /* NULL: defaults */, spm_pileup_site *dst, uint64_t cap, uint64_t *n);

/* ---- genotype calls for pileup sites and the VCF text of the variant ones (one sample, SNV alleles): the end of the chain ----
 * spm_hip_pileup_sites_vcf genotypes every site record of a spm_pileup_sites handle and writes, on the device, a complete VCF
 * file: the header of spm_hip_vcf_header, then one line per site whose best genotype is not ref/ref, in site order.
 * spm_hip_pileup_sites_vcf_records is the raw form over any device array of spm_pileup_site records; the two host twins give the
 * same call records and the same bytes by a serial loop, no device needed.  The rule is integer arithmetic throughout (its
 * functions are in libspm_amd/csrc/pileup_vcf_core.hpp, one source for host and device), so both sides agree byte for byte:
 *   * Options (spm_vcf_opts; NULL: the defaults).  ploidy 1 or 2 (0: 2).  cost_match, cost_het, cost_miss: what one read base
 *     costs, in milli-Phred (1/1000 of -10 log10), when it agrees with a homozygous genotype, with one allele of a heterozygous
 *     one, with no allele; all three 0: 44, 3039, 24771, which are round(-10000 log10 p) for p = 1 - e, (1 - e) / 2 + e / 6 and
 *     e / 3 at e = 0.01.  prior_het, prior_hom_alt, milli-Phred, both 0: 30000 and 33010 (theta = 1e-3 and theta / 2): ref/ref
 *     pays nothing, ref/alt prior_het, alt/alt prior_hom_alt, alt1/alt2 2 * prior_het; with ploidy 1 a non-reference genotype
 *     pays prior_hom_alt.  min_qual, Phred: FILTER is PASS at or above it, LowQual below (NULL opts: 20; with opts the value as
 *     given, so 0 passes every line).  A cost or prior above 1 000 000, a ploidy above 2, nonzero flags or reserved fields:
 *     SPM_E_INVALID.
 *   * A site whose ref rank is above 3 gets no call: status SPM_CALL_REF_N, no line.
 *   * The alleles are the ranks A C G T; a genotype is a pair a <= b (10 of them; with ploidy 1 the 4 with a == b).  In uint64
 *       cost(g) = sum over x of counts[x] * c(x, g) + prior(g),   c = cost_match if a == b == x, cost_het if a != b and x is a or b,
 *     cost_miss otherwise.  Only counts[4] and ref are read of the evidence: N, DEL and INS take no part.  Counts up to 2^32 - 1
 *     do not overflow.
 *   * The best genotype has the least cost; ties go to the one that comes first in VCF genotype order (0,0) (0,1) (1,1) (0,2)
 *     (1,2) (2,2) (0,3) ... over (the reference rank, then the other ranks ascending).
 *   * Best is ref/ref: status SPM_CALL_REF, a record and no line.  Otherwise SPM_CALL_VARIANT: ALT lists the non-reference
 *     alleles of the best genotype by ascending rank (one or two), GT indexes into REF, ALT.
 *   * PL, over the kept alleles in VCF genotype order F(j, k) = k (k + 1) / 2 + j: min((cost(g) - cost(best) + 500) / 1000,
 *     2^31 - 1); 3 or 6 values with ploidy 2, 2 with ploidy 1.  QUAL is the PL of ref/ref, GQ = min(99, second-smallest PL), AD
 *     the counts of the kept alleles, DP the site's depth.
 *   * The line, tabs between the fields and one \n behind:
 *       CHROM POS . REF ALT QUAL FILTER DP=<depth> GT:AD:GQ:PL <gt>:<ad,..>:<gq>:<pl,..>
 *     POS is 1-based, the separator inside GT is '/'.
 * Worked table (reference A, defaults, ploidy 2):
 *     counts A,C,G,T   depth   tail of the line
 *     10,10,0,0        20      A C 157 PASS DP=20 GT:AD:GQ:PL 0/1:10,10:99:157,0,190
 *     0,0,3,0          3       A G 41 PASS DP=3 GT:AD:GQ:PL 1/1:0,3:6:41,6,0
 *     0,8,0,8          16      A C,T 288 PASS DP=16 GT:AD:GQ:PL 1/2:0,8,8:99:288,144,123,144,0,123
 *     19,1,0,0         20      no line: ref/ref wins (25607 against 90780 for A/C)
 *   The first row: AA = 10 * 44 + 10 * 24771 = 248150, AC = 20 * 3039 + 30000 = 90780, CC = 248150 + 33010 = 281160; the
 *   differences 157370 and 190380 give the PLs 157 and 190.
 * The header (spm_hip_vcf_header, host only; *len / SPM_E_OVERFLOW as spm_hip_sam_header has them; rname under that call's rule,
 * sample 1 .. 254 bytes of '!' .. '~'), these bytes, \t a tab, every line ended by \n:
 *     ##fileformat=VCFv4.2
 *     ##contig=<ID=<rname>,length=<ref_len>>
 *     ##FILTER=<ID=LowQual,Description="QUAL below the threshold">
 *     ##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth: A + C + G + T + N + DEL">
 *     ##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">
 *     ##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Base counts of the REF and ALT alleles">
 *     ##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">
 *     ##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype costs">
 *     #CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t<sample>
 * The handle has two views, each on the host (downloaded when first asked for) and on the device: the text, and one 32-byte
 * spm_variant_call per site (offset and len: the site's line in the text; len 0 where there is none, offset then where the next
 * line starts).  Refused with SPM_E_INVALID and a message, nothing returned: NULL arguments (opts may be NULL; sites may be NULL
 * with n_sites 0), what the options list above, a bad rname or sample, and -- counted on the device in the pass that makes the
 * calls and read back once -- sites whose pos is not strictly ascending or reaches ref_len.  SPM_E_UNSUPPORTED: more than
 * 2^32 - 1 sites, a ref_len above 2^32 - 1 (a site's pos is 32 bits), or, on the device, a text of 2^32 bytes or more (its
 * line offsets are 32 bits).  Zero sites give the header
 * alone.  Out of scope: indel alleles (the pileup keeps no inserted sequence), several samples, a tabix index, BCF, per-base
 * quality likelihoods (a site has counts only), overlap resolution of mates. */
enum { SPM_CALL_REF = 0, SPM_CALL_VARIANT = 1, SPM_CALL_REF_N = 2 };
typedef struct spm_vcf_opts {      /* 40 bytes */
    uint32_t ploidy;               /* 1 or 2; 0: 2 */
    uint32_t cost_match, cost_het, cost_miss; /* all 0: 44, 3039, 24771 */
    uint32_t prior_het, prior_hom_alt;        /* both 0: 30000, 33010 */
    uint32_t min_qual;             /* as given; NULL opts: 20 */
    uint32_t flags;                /* must be 0 */
    uint32_t reserved0, reserved1; /* must be 0 */
} spm_vcf_opts;
typedef struct spm_variant_call {  /* 32 bytes */
    uint32_t pos;                  /* 0-based, the site's */
    uint32_t depth;                /* the site's: DP */
    uint32_t qual;                 /* the PL of ref/ref; 0 without a call */
    uint32_t len;                  /* bytes of the line; 0: the site has none */
    uint64_t offset;               /* of the line in the text, the header included */
    uint8_t status;                /* SPM_CALL_REF, SPM_CALL_VARIANT, SPM_CALL_REF_N */
    uint8_t gq;                    /* 0 where the site has no line */
    uint8_t gt[2];                /* the best genotype as allele ranks, gt[0] <= gt[1]; ploidy 1: both the same */
    uint8_t n_alt;                 /* 0 .. 2 */
    uint8_t alt[2];                /* the ALT ranks, ascending; 0 where unused */
    uint8_t reserved;
} spm_variant_call;
typedef struct spm_vcf_stats {     /* 80 bytes */
    float ms_total;                /* device: the three stages below (HIP events) */
    float ms_call;                 /* every site genotyped: call record, line length, order test, counters */
    float ms_scan;                 /* the exclusive sum of the line lengths */
    float ms_write;                /* the lines formatted in LDS and stored, the header copied in front */
    float ms_host;                 /* wall clock of the whole call */
    uint32_t group_sites;          /* sites per workgroup of the write stage of this build (not part of the ABI's promises) */
    uint64_t n_sites;
    uint64_t n_variant;            /* lines */
    uint64_t n_ref;                /* best genotype ref/ref */
    uint64_t n_ref_n;              /* reference rank above 3: no call */
    uint64_t n_low_qual;           /* lines with FILTER LowQual */
    uint64_t n_header_bytes;
    uint64_t n_text_bytes;         /* header and lines */
} spm_vcf_stats;
typedef struct spm_vcf spm_vcf;
int spm_hip_pileup_sites_vcf(spm_pileup_sites *s, const char *rname, const char *sample, uint64_t ref_len,
                             const spm_vcf_opts *opts /* NULL: defaults */, spm_vcf **out);
int spm_hip_pileup_sites_vcf_records(spm_ctx *ctx, const void *device_sites, uint64_t n_sites, const char *rname, const char *sample,
                                     uint64_t ref_len, const spm_vcf_opts *opts /* NULL: defaults */, spm_vcf **out);
/* the host views are downloaded when first asked for; every out pointer may be NULL */
int spm_hip_vcf_view(spm_vcf *v, const char **text, uint64_t *n_bytes, const spm_variant_call **calls, uint64_t *n_calls);
int spm_hip_vcf_device(spm_vcf *v, const void **text, uint64_t *n_bytes, const void **calls, uint64_t *n_calls);
int spm_hip_vcf_stats(const spm_vcf *v, spm_vcf_stats *out);
void spm_hip_vcf_destroy(spm_vcf *v);
/* calls: n records, written only when the call succeeds; offset and len stay 0, they belong to a text and this call makes
 * none.  Sites whose pos is not strictly ascending: SPM_E_INVALID */
int spm_hip_pileup_sites_calls_host(const spm_pileup_site *sites, uint64_t n, const spm_vcf_opts *opts /* NULL: defaults */,
                                    spm_variant_call *calls);
/* the whole file into dst: *len its length, SPM_E_OVERFLOW with *len set when cap is too small */
int spm_hip_pileup_sites_vcf_host(const spm_pileup_site *sites, uint64_t n, const char *rname, const char *sample, uint64_t ref_len,
                                  const spm_vcf_opts *opts /* NULL: defaults */, char *dst, uint64_t cap, uint64_t *len);
int spm_hip_vcf_header(const char *rname, const char *sample, uint64_t ref_len, char *buf, uint64_t cap, uint64_t *len);

/* ---- projected alignments with every indel at its leftmost equivalent place ---------------------------------------------
 * Two haplotypes may differ only in WHICH copy of a homopolymer or tandem repeat an indel removes or adds.  They project to
 * different transcripts over the same reference range, and spm_hip_jst_ref_alns_collapse, which decides on content, keeps
 * them apart.  This call returns the records of a projection with every transcript LEFT-NORMALISED, in a form the collapse
 * (and view, device, destroy and this call again) takes unchanged.  No other call changes its output.
 *
 * The rule.  Per record: the needle P, ref[ref_begin, ref_end) and the transcript as columns c_0 .. c_{n-1} (a word
 * len << 4 | op is len columns).  A GAP RUN is a maximal stretch of consecutive columns of one gap op (I or D); adjacent words
 * of one op are one run.  For the run in columns [c, c + L) let i be the number of needle symbols the columns before c
 * consume and r be ref_begin plus the number of reference positions they consume.  One STEP LEFT is allowed iff
 *     c >= 2             (the column on the run's left is not column 0: the first column of a transcript never moves, and a
 *                         run never becomes a leading gap),
 *     column c - 1 is =, and
 *     P[i - 1] == P[i + L - 1] for an I run, ref[r - 1] == ref[r + L - 1] for a D run (ranks are compared, as everywhere).
 * The step turns columns [c - 1, c - 1 + L) into the gap and column c - 1 + L into =.  If the run's new left neighbour is a
 * run of the SAME op the two are one run from then on: c becomes that run's first column, L grows, and stepping goes on with
 * the joined run.  A left neighbour that is X or the other gap op stops the run.  Runs are treated left to right; a run is
 * finished when no step is allowed, then comes the next run on its right.  Adjacent equal ops are merged into words exactly
 * as the projection merges them (a run above 2^28 - 1 columns is full words and then the rest).
 * It follows that
 *   * ref_begin, ref_end, ref_score, score, haplotype and pattern are unchanged, and so is the number of =, X, I and D columns;
 *   * the result consumes exactly P and ref[ref_begin, ref_end), and every = / X column is still true;
 *   * normalising a normalised transcript changes nothing;
 *   * the result depends only on (P, ref, ref_begin, words);
 *   * a transcript wholly inside an insertion (|P| I) is unchanged;
 *   * the word count grows by at most one word per gap run -- result words <= 2 x source words -- and may shrink, when runs
 *     join or a passed = run is used up.
 * Worked cases (ref, needle, ref_begin: source -> result).
 *  1. GATTCGCAAAAGTCCATG, TTCGCAAAGTCCA, 2: 8=1D5= -> 5=1D8= (and 6=1D7=, 5=1D8= give the same): collapse case 1, whose two
 *     haplotypes now agree.
 *  2. GGAC (ACT)x5 GGTC, AC (ACT)x4 GG, 2: one unit deleted in any of the five places -> 2=3D14=.  A tandem repeat of unit 3.
 *  3. GATCCGT, ATCCCG, 1: 4=1I1= or 3=1I2= -> 2=1I3=.  An insertion.
 *  4. GACGTCGTA, ACGTCGTCGTA, 1: 7=3I1= -> 1=3I7=.  The run stops with one column on its left.
 *  5. CAAAAG, AAAG, 1: 3=1D1= -> 1=1D3=.  The first column is pinned.
 *  6. CAAAAAAG, AAAAG, 1: 2=1D1=1D2=, 1=1D2=1D2= and 4=2D1= -> 1=2D4=.  Two runs join and go on as one.
 *  7. GACGTTA, ACGATTA, 1: 3=1X1I2= unchanged.  An X stops a run.
 *
 *   * Accepted: any result of spm_hip_jst_alns_project or of this call.  The call reads the reference text of the tree and
 *     the needles of the set behind the projection: both must be alive DURING the call.  The result outlives them and its
 *     source.  A tree indexed again since the search is accepted: the reference text belongs to no index generation.
 *   * Record i of the host view belongs to record i of the source's host view, record i of the device view to record i of
 *     the source's device view.  Every field but cigar_off / cigar_len equals the source's.  The pool holds one transcript per
 *     distinct source slot, in source pool order; equal source cigar_off gives equal result cigar_off.  Two calls give
 *     byte-identical host views.
 *   * spm_hip_jst_ref_alns_stats on the result answers the counts (n_alns, n_projected = slots, n_ops = words of this pool)
 *     with zero times; spm_hip_jst_ref_alns_normalize_stats on a handle this call did not make is SPM_E_INVALID.
 *   * SPM_E_INVALID with a message: NULL arguments, unknown flag bits, a handle that names no tree.
 *   * A slot whose transcript lies outside the source pool, whose words do not consume exactly its needle and its reference
 *     range, or whose range lies outside the reference is COUNTED on the device and fails the whole call with SPM_E_INVALID,
 *     never a fault: every needle, reference and pool index is tested against its size before it is read.
 *   * More than 2^32 - 1 result words: SPM_E_UNSUPPORTED, decided before any result word is written.
 *   * No records: an empty result and SPM_OK.
 * flags: must be 0 */
typedef struct spm_jst_normalize_stats { /* 96 bytes */
    float ms_total;            /* device: the five stages below (HIP events) */
    float ms_slots;            /* one representative record per distinct source slot */
    float ms_normalize;        /* the rule, one lane per slot */
    float ms_offsets;          /* where every slot's words go; their total */
    float ms_gather;           /* one record per source record */
    float ms_compact;          /* the slots' words into the pool */
    float ms_host;             /* wall clock of the whole call, host view included */
    float reserved;
    uint64_t n_alns;           /* records = the source's count */
    uint64_t n_slots;          /* distinct source slots */
    uint64_t n_ops_in;         /* words of the source's pool */
    uint64_t n_ops;            /* words of this pool */
    uint64_t n_changed;        /* slots whose words differ from the source's */
    uint64_t n_steps;          /* steps left, summed over all runs of all slots */
    uint64_t n_joined;         /* joins of two runs */
    uint64_t n_pinned;         /* stops that only the first-column rule caused (a run that joins another may stop twice) */
} spm_jst_normalize_stats;

int spm_hip_jst_ref_alns_normalize(spm_jst_ref_alns *a, uint32_t flags, spm_jst_ref_alns **out);
int spm_hip_jst_ref_alns_normalize_stats(const spm_jst_ref_alns *a, spm_jst_normalize_stats *out);

/* ---- selection of pan-genome hits: one record per haplotype locus, the best stratum per (haplotype, needle) -------------
 * spm_hip_hits_select for the 24-byte records of spm_hip_jst_search.  The locus is (haplotype, pattern).  For a record
 * r = (haplotype, pos, pattern, score):
 *   SPM_SELECT_LOCI    r is dropped iff another record r' has the same haplotype and the same pattern, |pos' - pos| <= w and
 *                      (score', pos') < (score, pos) lexicographically.  w as in spm_hip_hits_select (window, or with
 *                      SPM_SELECT_WINDOW_K the needle's own k, 0 for exact sets; w = 0 keeps everything).  Suppression is
 *                      strict: a dominated record still dominates.  Records of different haplotypes never see each other,
 *                      and there is no segment notion: haplotype coordinates are one range per haplotype.
 *   SPM_SELECT_BEST    applied after LOCI: r is kept iff score <= min + strata, min taken over the INPUT records of the same
 *                      (haplotype, pattern) ...
 *   SPM_SELECT_ACROSS  ... or, with this flag, over the input records of the same pattern on ALL haplotypes ("the best place
 *                      of this read anywhere in the pan-genome").  ACROSS without BEST is SPM_E_INVALID.
 *   SPM_SELECT_STRANDS with BEST: the minimum's pattern becomes the READ = pattern >> 1 -- over (haplotype, read), or with
 *                      ACROSS over the read on all haplotypes.  Refusals as in spm_hip_hits_select (the strands of a search's
 *                      needle set are remembered by its result and by every selection of it).  LOCI is unchanged.
 *   neither flag       a sorted copy.
 * Without ACROSS the records of haplotype h in the result are exactly what spm_hip_scan + spm_hip_hits_select with the same
 * opts return on the materialised haplotype h.  The rule reads only the SET of records: the result is bit-identical across
 * engines, block lengths, runs and arrival orders.
 * The result is a new spm_jst_hits with a buffer of its own; it stays valid after the source is destroyed (the needle set
 * must stay alive if the result is selected again with SPM_SELECT_WINDOW_K).  Its DEVICE view is in (haplotype, pattern,
 * pos) order -- the one device view of pan-genome hits with a defined order; its host view is in the order of every
 * spm_hip_jst_hits_view, (haplotype, pos, pattern, score).  copy_device, gatherv_jst_hits and destroy take it unchanged, and
 * it may be selected again.  spm_hip_jst_hits_align does NOT take it, whatever the source was (SPM_E_INVALID): it keeps no
 * map back to the search's segment hits.  The records it kept are aligned by spm_hip_jst_selection_align above, which
 * locates them in the tree's index; for that a selection of a search's hits remembers the tree and its index generation.
 * Decided on the host before any launch: SPM_E_UNSUPPORTED for more than 2^32 - 1 records, or
 * bits(n_haplotypes - 1) + bits(n_patterns - 1) + bits(largest position) above 64 (for a tree the position bound is the
 * reference length plus all inserted symbols), or SPM_SELECT_ACROSS on records that name a pattern index of 2^24 or above
 * (only a raw buffer without a needle set can); SPM_E_INVALID for unknown flag bits, a nonzero reserved field or NULL opts.
 * No records: an empty result and SPM_OK.  spm_hip_hits_select and spm_hip_records_select refuse SPM_SELECT_ACROSS. */
#define SPM_SELECT_ACROSS 4u   /* pan-genome selections only, with SPM_SELECT_BEST */
int spm_hip_jst_hits_select(spm_jst_hits *hits, const spm_select_opts *opts, spm_jst_hits **out);
/* The same on a device buffer of n spm_jst_hit records (8-byte aligned) that no handle owns -- what spm_hip_gatherv_jst_hits
 * delivers on the root.  A locus can straddle the block shards of several GPUs and the best stratum is global, so under
 * sharding the order is: gatherv first, select on the root second.  patterns may be NULL if the window is explicit
 * (SPM_SELECT_WINDOW_K without a set: SPM_E_INVALID).  (haplotype, pattern, pos) must be unique in the buffer; the search
 * guarantees that.  The ranges of haplotype, pattern and position are read off the buffer by a reduction kernel and one
 * small read-back before the sort is planned. */
int spm_hip_jst_records_select(spm_ctx *ctx, const void *device_records, uint64_t n, const spm_patterns *patterns,
                               const spm_select_opts *opts, spm_jst_hits **out);
/* n_in, n_loci, n_out, key_bits and the order / select / host times; SPM_E_INVALID on a result no selection made */
int spm_hip_jst_hits_select_stats(const spm_jst_hits *hits, spm_select_stats *out);

/* Synthetic variants of config C5: one SNP per 1000 reference bases, one indel of length 1..50 per
 * 10 000, each carried by a random non-empty subset of n_haplotypes <= 64; the reference is the synthetic text of
 * `seed_text`.  Call with alleles == NULL to get the counts (*n_alleles, *alt_pool_len) first.  Host side. */
int spm_hip_jst_synth_variants(uint64_t seed_text, uint64_t seed_var, uint64_t ref_begin, uint64_t n_ref,
                               uint32_t n_haplotypes, spm_jst_allele *alleles, uint64_t *n_alleles, uint8_t *alt_pool,
                               uint64_t *alt_pool_len, uint64_t *coverage);

/* ---- multi-GPU exchange: the gatherv of hit records to one rank over RCCL (xGMI), SURVEY.md 8(e) -------------------
 * One process per GPU; the path shards by text position (spm_scan_opts.left_context / pos_offset) and needs no
 * data-path collective.  The single exchange step is this gatherv (RCCL has none of its own: one ncclAllGather of the
 * per-rank counts, then grouped ncclSend / ncclRecv).  librccl.so is opened when the first communicator is made.
 *   rank 0:      spm_hip_comm_unique_id(id)  -> hand the 128 bytes to the other ranks (MPI, a file, a socket ...)
 *   every rank:  spm_hip_comm_init(ctx, id, rank, world, &comm)
 *   per scan:    spm_hip_gatherv_hits(comm, hits, 0, &records, &n, counts)
 * Records arrive in rank order (= ascending shard order); on the root *device_records points at n_total records in HBM
 * (owned by the communicator, valid until its next gatherv), elsewhere it is NULL.  counts may be NULL. */
typedef struct spm_comm spm_comm;
int spm_hip_comm_unique_id(void *id128);
int spm_hip_comm_init(spm_ctx *ctx, const void *unique_id128, int rank, int world, spm_comm **out);
void spm_hip_comm_destroy(spm_comm *comm);
int spm_hip_gatherv_hits(spm_comm *comm, spm_hits *local, int root, const void **device_records, uint64_t *n_total,
                         uint64_t *counts);
int spm_hip_gatherv_jst_hits(spm_comm *comm, spm_jst_hits *local, int root, const void **device_records,
                             uint64_t *n_total, uint64_t *counts);
/* host arithmetic of the gatherv: byte offset of every rank's records in the root's buffer, offsets[world] = total */
int spm_hip_gatherv_plan(const uint64_t *counts, uint32_t world, uint32_t record_bytes, uint64_t *offsets);
/* Failure is collective: a rank whose local result is unusable (e.g. SPM_E_OVERFLOW of its scan), a root that cannot hold
 * the records, counts that overflow the offsets -- all ranks learn of it in an exchange every rank takes part in and return
 * an error (the failing rank its own, the others SPM_E_PEER) BEFORE any send or receive is posted; nobody is left waiting.
 * Host-only self-check of that protocol over an in-process loopback of `world` threads (no GPU, no RCCL): scenario 0 clean,
 * 1 rank `victim` has a local error, 2 the root cannot reserve its buffer, 3 the counts overflow, 4 no rank has records.
 * detail[world] (may be NULL) receives the status every rank returned.  SPM_OK iff all ranks behaved as promised and
 * nothing hung. */
int spm_hip_comm_selftest(int world, int root, int scenario, int victim, uint32_t record_bytes, uint64_t seed, int *detail);

/* ---- synthetic needles of the benchmark configs (host side) -------------------------- */
uint64_t spm_hip_synth_pattern(uint64_t seed_text, uint64_t seed_pat, uint64_t n_total, uint32_t p, uint32_t L,
                               uint32_t kmax, uint8_t *out);
uint64_t spm_hip_synth_repeat_pattern(uint64_t seed_text, uint64_t seed_pat, uint64_t n_total, uint32_t p, uint32_t L,
                                      uint32_t kmax, uint32_t repeat_ppm, uint32_t across_every, uint8_t *out);
void spm_hip_synth_repeat_text(uint64_t seed, uint32_t repeat_ppm, uint64_t begin, uint64_t n, uint8_t *out);
uint64_t spm_hip_mix64(uint64_t z);

/* Host-only self-check of the seed index (no device, no context): builds the level-1 / level-2 tables exactly as
 * spm_hip_patterns_create does and verifies what the filter's losslessness rests on -- every indexed 16-symbol window of
 * every seed is found at both levels, every needle sits in exactly one pass (anchored sets: every seed has its one key
 * in one pass, beginning with an anchor dimer of that pass), the stride fits every seed.
 * stats[8] = {passes, stride, keys, windows checked, windows missing, level-1 false positives, trials,
 *            hash variant | anchor dimers per pass << 8 (0: unanchored)}.
 * Returns SPM_OK iff nothing is missing. */
int spm_hip_host_selftest(int algo, const uint8_t *ranks_concat, const uint32_t *offsets, uint32_t n_patterns,
                          const uint16_t *k, uint32_t sigma, uint64_t *stats);

const char *spm_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPM_HIP_H */
