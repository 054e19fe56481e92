// internal.hpp -- what the translation units of libspm_hip.so share: the compiled needle set, the arguments of one scan, and
// the entry points of the engines.  (patterns.hip: needle sets; text.hip: context + haystacks; scan.hip: the scan driver;
// scan_brute.hip / scan_filter.hip: the engines, the seed filter's kernels in filter_stream / filter_dense / filter_resolve /
// filter_verify.hip (filter_launch.hpp); hits.hip: results; align.hip: alignments of hits; select.hip: selection of hits;
// device_order.hip: the pair sort of the drivers that order records (device_order.hpp); jst.hip: journaled sequences, with
// jst_align.hip, jst_ref.hip, jst_reads.hip and jst_sam.hip behind it (map in jst.hpp) and jst_select.hip beside it;
// bgzf.hip: BGZF framing and deflate; bam_index.hip: the sorted BAM, its BAI index and its duplicate marks (the handles of both
// and of jst_sam.hip: output_handles.hpp); comm.hip: the multi-GPU exchange.)
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "common.hpp"
#include "index_types.hpp"

using namespace spm_hip;

// ----------------------------------------------------------------------------------------------------
// pattern set
// ----------------------------------------------------------------------------------------------------
struct spm_patterns : spm_hip::seed_index // (the seed index: passes, entries, seed layout -- index_types.hpp)
{
    spm_ctx *ctx = nullptr;
    int algo = 0;
    uint32_t n = 0;
    uint32_t strands = 1; // 2: made by spm_hip_patterns_create_stranded -- pattern 2r is read r, 2r + 1 its reverse complement
    uint32_t sigma = 4;
    std::vector<uint8_t> ranks;
    std::vector<uint32_t> offsets;
    std::vector<int32_t> m, k; // padded to n_groups*64
    uint32_t n_groups = 0;
    uint32_t max_m = 0;
    uint32_t max_window = 0;
    uint32_t max_k = 0;
    uint32_t NW = 1;   // 32-bit words per needle in the brute kernels (power of two)
    bool is_myers() const { return algo == SPM_ALGO_MYERS || algo == SPM_ALGO_MYERS_PREFIX; }
    // device
    void *d_arena = nullptr;   // the set's one device allocation: every d_* table below points into it (patterns.hip)
    uint32_t *d_peq = nullptr; // [group][sigma+1][NW][64], needles top-aligned
    uint32_t *d_peq_bot = nullptr; // Myers only: same shape, needles bottom-aligned (cut-off kernel)
    uint32_t *d_peq_verify = nullptr; // exact matchers: Myers-style match masks (top-aligned) for the verify kernel;
                                      // for Myers sets verification reads d_peq itself
    uint32_t *d_hp0 = nullptr; // prefix: [group][NW][64]
    int32_t *d_m = nullptr;
    int32_t *d_k = nullptr;
    mutable uint64_t cand_hint = 0; // most candidates a filter scan of this set has produced so far
    uint8_t *d_surplus = nullptr;   // per needle: seeds - k (candidate merging); nullptr = no needle has k >= kMergeMinK
    uint8_t *d_ranks = nullptr;     // filterable sets: the needles' symbols, back to back (whole-seed check of a candidate)
    uint32_t *d_offsets = nullptr;  // ... and where each needle starts
    uint32_t *d_needle_pk = nullptr;  // dna4 sets: the needles 2 bits per symbol, 16 per word (piece count of a candidate)
    uint32_t *d_pk_offsets = nullptr; // ... and the first word of each
    uint16_t *d_seed_q = nullptr;
    pass_entry *d_pass_tab = nullptr; // the passes' key directories, for resolve_kernel
    uint4 *d_entries = nullptr;
    mutable uint64_t hit_hint = 0;    // most hits a filter scan of this set has reported so far (sizes the dedupe set)
    mutable bool scanned = false;     // the hints come from at least one completed filter scan
    mutable int exact_whole = -1;     // 1: k = 0 and every needle is its own single seed (decided at the first scan)
    mutable uint64_t band_hint = 0;   // ... and band-list slots it drew (sizes the verification grid)
    spm_build_stats build{};          // what spm_hip_patterns_create spent where
    // alignment tables, built at the first spm_hip_hits_align of the set (align.hip): one allocation holding the reversed
    // needles' 64-bit match masks [sigma][words] per needle, their word offsets, the needle ranks and their offsets
    mutable void *d_align = nullptr;
    mutable const uint64_t *d_al_rpeq = nullptr;
    mutable const uint32_t *d_al_rpeq_off = nullptr;
    mutable const uint8_t *d_al_ranks = nullptr;
    mutable const uint32_t *d_al_offsets = nullptr;
};

using clk = std::chrono::steady_clock;
inline float ms_since(clk::time_point t) { return std::chrono::duration<float, std::milli>(clk::now() - t).count(); }
// the three events of a selection -> the times of spm_select_stats, once (`timed`: they are still to be read)
inline hipError_t select_stats_close(bool &timed, hipEvent_t begin, hipEvent_t ordered, hipEvent_t end, spm_select_stats &s)
{
    const hipError_t e = timed ? hipEventSynchronize(end) : hipSuccess;
    if (!timed || e != hipSuccess)
        return e;
    hipEventElapsedTime(&s.ms_total, begin, end);
    hipEventElapsedTime(&s.ms_order, begin, ordered);
    hipEventElapsedTime(&s.ms_select, ordered, end);
    timed = false;
    return hipSuccess;
}

inline bool spm_trace_on() { return trace_on(); } // (host_util.hpp)


// every knob of a scan, read from the environment in ONE place, once per C-ABI call that scans.  Each one is set by a test:
// to reach a rare path that some input also takes by default, or to pick the path a test compares against.
struct scan_tuning
{
    int cand_cap = 0;
    int brute_cutoff = 1;
    int verify_wave_min_words = 8;
    int span_budget = 0;
    int verify_runs = 1;
    int verify_runs_min_bands = 65536;
    int band_cap = 0;
    static scan_tuning from_env()
    {
        scan_tuning T;
        T.cand_cap = env_int("SPM_HIP_FILTER_CAND_CAP", 0);
        T.brute_cutoff = env_int("SPM_HIP_BRUTE_CUTOFF", 1);
        T.verify_wave_min_words = env_int("SPM_HIP_VERIFY_WAVE_MIN_WORDS", 8);
        T.span_budget = env_int("SPM_HIP_FILTER_SPAN_BUDGET", 0);
        T.verify_runs = env_int("SPM_HIP_VERIFY_RUNS", 1);
        T.verify_runs_min_bands = env_int("SPM_HIP_VERIFY_RUNS_MIN_BANDS", 65536);
        T.band_cap = env_int("SPM_HIP_FILTER_BAND_CAP", 0);
        return T;
    }
};

struct scan_args // what the caller asked for: const for the whole call
{
    spm_ctx *ctx;
    const spm_text *text;
    uint64_t begin, end, ctx_begin; // owned end positions of the filter engine's share, and where its haystack begins
    const spm_patterns *ps;
    spm_scan_opts opts;
    spm_hits *hits;
    scan_tuning tune;                        // the environment's knobs, as this call found them
    const uint64_t *seg_offsets = nullptr; // host; n_segments + 1 entries
    uint64_t n_segments = 0;
    const uint64_t *d_seg_offsets = nullptr; // the same table already resident on the device (journaled-sequence index)
    const uint32_t *d_seg_owned = nullptr;   // optional per-segment offset of the first wanted end symbol (filter engine)
};

struct scan_state // what scan_impl owns between the attempts and passes of one call
{
    retry_state retry;
    filter_result filt;                           // of the latest filter run
    const uint64_t *segs = nullptr;               // segmented scans: the table on the host (host_segments, scan.hip)
    std::vector<uint64_t> seg_host;               // ... fetched once per call when only the device table was given
    const std::vector<uint64_t> *tiles = nullptr; // brute pass over an explicit tile table {scan_lo, own_lo, own_hi}
};

// ---- state blobs: ABI state <-> the kernels' [group][rows][64] layout (patterns.hip) ----
void state_to_internal(const spm_patterns *p, const void *state, std::vector<uint32_t> &out);
void state_from_internal(const spm_patterns *p, const std::vector<uint32_t> &in, void *state);
// ---- haystack allocation (text.hip) ----
int text_alloc(spm_ctx *ctx, uint64_t n, uint32_t sigma, spm_text **out);
// ---- the engines ----
int ensure_scratch(spm_ctx *ctx, size_t bytes);
// one brute-force pass; `report` = false suppresses hits (state-only pass)   (scan_brute.hip)
int run_brute(const scan_args &A, const scan_state &S, uint64_t begin, uint64_t end, uint64_t ctx_begin,
              const uint32_t *d_state_in, uint32_t *d_state_out, bool report, bool single_tile);
// the seed filter's launches for one scan: streaming pass(es), resolve, verification   (scan_filter.hip)
int run_filter(const scan_args &A, const retry_state &R, filter_result &out);
// after_launch: work the caller wants on the stream right behind the filter scan's kernels, before the host reads the
// counters (the pan-genome search's fan-out); spm_hits::hook_final tells whether it saw the final hit list.   (scan.hip)
int scan_impl(spm_ctx *ctx, const spm_text *text, uint64_t begin, uint64_t end, const spm_patterns *patterns,
              const spm_scan_opts *opts_in, const void *state_in, void *state_out, const uint64_t *seg_offsets,
              uint64_t n_segments, spm_hits **out, const uint64_t *d_seg_offsets = nullptr,
              const uint32_t *d_seg_owned = nullptr, const std::function<int(spm_hits *)> *after_launch = nullptr);

// ---- alignment of Myers hits (align.hip): the work list, the kernel classes, stage A and stage B.  Shared by
// spm_hip_hits_align (hits of a scan) and, through jst_align_segments (jst_hits_align.hpp), by spm_hip_jst_hits_align (segment hits of
// a journaled-sequence search) and spm_hip_jst_selection_align (the distinct segment hits of a selection's records). ----
struct align_work
{
    const spm_patterns *ps = nullptr;
    const spm_text *text = nullptr;
    uint64_t pos_offset = 0;          // hits[i].pos - pos_offset = the hit's end in text coordinates
    const spm_hit *hits = nullptr;    // host copies; record i of d_recs belongs to hits[i]
    uint64_t n = 0;
    const uint64_t *lo = nullptr;     // per hit: the first text symbol its alignment may use
    const uint32_t *cig_off = nullptr; // per hit: first word of its transcript in the pool
    bool begin_only = false;
    spm_aln *d_recs = nullptr;        // [n], allocated by the caller
    uint32_t *d_ops = nullptr;        // [n_ops]
    uint64_t n_ops = 0;               // 0 with begin_only
    spm_aln *h_recs = nullptr;        // optional: where the records are copied back to
    uint32_t *h_ops = nullptr;        // optional: ... and the pool
    const char *who = "";             // the C-ABI call, for messages
};
int align_run(spm_ctx *ctx, const align_work &W, spm_align_stats &stats);
// builds, once per set, the alignment tables of spm_patterns (d_al_*): the projection reads the needle ranks among them
int spm_align_tables(const spm_patterns *ps);

// ---- the out-parameters of a "records + CIGAR pool" result: what the _view (host pointers) and _device (R = W = S = void)
// entry points of spm_alns, spm_jst_alns, spm_jst_ref_alns and spm_jst_ref_loci hand out.  records and n are required;
// every other out-parameter is filled where the caller asked for it. ----
template <class R, class W = uint32_t, class S = int32_t> struct pool_src
{
    const R *recs;
    uint64_t n;
    const W *ops;
    uint64_t n_ops;
    const W *members = nullptr; // loci only: the haplotypes that support each locus ...
    const S *member_scores = nullptr; // ... and their distances
    uint64_t n_members = 0;
};
template <class R, class W, class S>
int pool_out(const pool_src<R, W, S> &src, const R **records, uint64_t *n, const W **ops, uint64_t *n_ops,
             const W **members = nullptr, const S **member_scores = nullptr, uint64_t *n_members = nullptr)
{
    if (!records || !n)
        return SPM_E_INVALID;
    *records = src.recs;
    *n = src.n;
    if (ops)
        *ops = src.ops;
    if (n_ops)
        *n_ops = src.n_ops;
    if (members)
        *members = src.members;
    if (member_scores)
        *member_scores = src.member_scores;
    if (n_members)
        *n_members = src.n_members;
    return SPM_OK;
}

// Every translation unit with kernels is a code object of its own, loaded by the HIP runtime at the first launch out of
// it (~1-3 ms each).  spm_hip_init loads them all, so that the first scan of a process does not pay for it.
void spm_warm_text_kernels();
void spm_warm_brute_kernels();
void spm_warm_filter_kernels();
void spm_warm_hits_kernels();
void spm_warm_jst_kernels();
void spm_warm_align_kernels();
void spm_warm_bgzf_kernels();
#pragma GCC visibility push(hidden) // (the units behind the tree, and the pair sort: calls inside the library, like filter_launch.hpp's)
void spm_warm_jst_align_kernels();
void spm_warm_jst_ref_kernels();
void spm_warm_jst_reads_kernels();
void spm_warm_jst_sam_kernels();
void spm_warm_bam_index_kernels();
void spm_warm_bam_pileup_kernels();
void spm_warm_pileup_vcf_kernels();
void spm_warm_device_order_kernels(spm_ctx *ctx); // (hipcub's kernels have no name to ask for: it sorts one pair in ctx's scratch)
#pragma GCC visibility pop

// ---- the frame stage of BGZF (bgzf.hip) on the context's stream: n bytes at d_src into d_dst, which has room for
// bgzf_framed_size(n, D, eof) bytes (bgzf_core.hpp) ----
hipError_t bgzf_frame_enqueue(spm_ctx *ctx, const void *d_src, uint64_t n, uint32_t D, bool eof, void *d_dst);
// ---- the deflate stages (bgzf.hip): n bytes at d_src as deflated blocks behind `prefix`, bytes that are blocks already, into a
// new handle whose offsets count from the prefix's first byte.  The opts have passed spm_hip_bgzf_deflate's checks. ----
int bgzf_deflate_run(const char *who, spm_ctx *ctx, const void *d_src, uint64_t n, const spm_bgzf_deflate_opts *opts,
                     const std::vector<uint8_t> &prefix, spm_bgzf **out);

// ---- the header section of a BAM file before its framing (jst_bam.hpp), for the call that writes one and for spm_hip_bam_sort
// (bam_index.hpp), which writes it again with SO:coordinate; the blocks' offsets of a spm_bgzf handle made ready on the host
// and, with on_device, on the device (bgzf.hip), for spm_hip_bam_index over a deflated file ----
#pragma GCC visibility push(hidden)
int bam_plain_header(const char *who, spm_ctx *ctx, const char *rname, uint64_t ref_len, bool sorted, std::vector<uint8_t> &h);
int bgzf_offsets_ready(spm_bgzf *z, bool on_device);
#pragma GCC visibility pop

// deferred scans (SPM_SCAN_DEFER): read the counters back, and repeat the scan if it needs attention   (scan.hip)
int spm_complete_deferred(spm_hits *h);
