// jst_select.hip -- selection of pan-genome hits behind the C ABI: spm_hip_jst_hits_select, spm_hip_jst_records_select,
// spm_hip_jst_hits_select_stats.  The host side of jst_select.hpp: plan (select_plan.hpp: plan_jst_select), lay the scratch
// out (scratch_layout.hpp), enqueue keys -> sort -> loci -> [group numbers -> minima] -> scan -> compact on the context's
// stream, read the two counts back (the one synchronisation; sort, scans and read-back are device_order.hpp's), hand out a
// new spm_jst_hits with a buffer of exactly the kept records.
// MI355X only; no CPU path exists in this library: if HIP fails the call fails.
#include "internal.hpp"
#include "device_order.hpp"
#include "jst_select.hpp"
#include "scratch_layout.hpp"

namespace
{

struct jsel_source // what the two entry points know about their records
{
    const spm_jst_hit *d_recs = nullptr;
    uint64_t n = 0;
    uint64_t n_hap = 1, n_patterns = 1, max_pos = 0;
    const spm_patterns *ps = nullptr; // may be null (records)
    uint32_t strands = 0;             // of the needle set the records stem from (0: no set is known)
    spm_jst *jst = nullptr;           // the tree and index generation of the search the records stem from (records: none):
    uint64_t generation = 0;          // what spm_hip_jst_selection_align locates the kept records in
};

constexpr uint64_t kJselAcrossPatterns = 1ull << 24; // entries of the per-pattern minima of SPM_SELECT_ACROSS, at most (64 MiB)

int jsel_run(spm_ctx *ctx, const jsel_source &S, const jst_select_plan &plan, uint32_t strata, spm_jst_hits *R)
{
    const uint32_t n = (uint32_t)S.n;
    R->sel.n_in = S.n;
    R->sel.key_bits = plan.key_bits;
    for (hipEvent_t &e : R->sel_ev)
        SPM_HIP_CHECK(ctx, hipEventCreate(&e));
    SPM_HIP_CHECK(ctx, hipEventRecord(R->sel_ev[0], ctx->stream));
    if (n == 0) {
        SPM_HIP_CHECK(ctx, hipEventRecord(R->sel_ev[1], ctx->stream));
        SPM_HIP_CHECK(ctx, hipEventRecord(R->sel_ev[2], ctx->stream));
        return SPM_OK;
    }
    const bool numbered = plan.best && !plan.across; // minima indexed by group number: at most n groups
    const uint64_t n_min = plan.min_slots;

    // the scratch: keys and indices twice (the sort's in and out), scores in arrival and in sorted order, flags, offsets,
    // group numbers, minima, counts, the compacted records (their count is known only after the read-back)
    using flag_op = sel_flag_op<jst_select_params>;
    jst_select_params P{};
    size_t sort_bytes = 0, scan_bytes = 0, head_bytes = 0;
    SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, n, plan.key_bits, &sort_bytes));
    SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(flag_op{P}), n, &scan_bytes));
    SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(jsel_head_op{nullptr}), n, &head_bytes));
    const size_t tmp_bytes = std::max(sort_bytes, std::max(scan_bytes, head_bytes));
    unsigned long long *keys_in = nullptr, *d_out = nullptr; // (d_out: the kept records as 8-byte words, three each)
    uint32_t *idx_in = nullptr, *offs = nullptr, *gid = nullptr;
    int32_t *score_in = nullptr;
    uint8_t *tmp = nullptr;
    scratch_layout L;
    L.take(keys_in, n);
    L.take(P.keys, n);
    L.take(idx_in, n);
    L.take(P.idx, n);
    L.take(score_in, n);
    L.take(P.score, n);
    L.take(P.keep, n);
    L.take(P.head, n);
    L.take(offs, n);
    L.take(gid, numbered ? n : 0);
    L.take(P.minima, n_min);
    L.take(P.counts, 2);
    L.take(tmp, tmp_bytes);
    L.take(d_out, 3 * (size_t)n);
    SPM_TRY(ensure_scratch(ctx, L.bytes()));
    L.bind(ctx->d_scratch);

    P.recs = reinterpret_cast<const unsigned long long *>(S.d_recs);
    P.score_in = score_in;
    P.n = n;
    P.pos_bits = plan.pos_bits;
    P.pos_mask = plan.pos_bits >= 64 ? ~0ull : (1ull << plan.pos_bits) - 1;
    P.pat_mask = plan.pat_bits >= 32 ? 0xFFFFFFFFu : (1u << plan.pat_bits) - 1;
    P.loci = plan.loci;
    P.best = plan.best;
    P.across = plan.across;
    P.shift = plan.strands ? 1u : 0u;
    P.window = plan.window;
    P.k_tab = plan.window == SPM_SELECT_WINDOW_K && S.ps ? S.ps->d_k : nullptr; // (WINDOW_K: the set is alive, jsel_make)
    P.halo = plan.halo;
    P.strata = strata;
    P.gid = numbered ? gid : nullptr;
    if (!plan.best)
        P.minima = nullptr;
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, 16, ctx->stream));
    if (plan.best)
        SPM_HIP_CHECK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(P.minima), 0x7FFFFFFF, n_min, ctx->stream));

    // order
    SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_select_keys_kernel, n, P.recs, keys_in, idx_in, score_in, n, plan.pos_bits, plan.pat_bits));
    SPM_HIP_CHECK(ctx, sort_pairs(ctx, tmp, tmp_bytes, keys_in, P.keys, idx_in, P.idx, n, plan.key_bits));
    SPM_HIP_CHECK(ctx, hipEventRecord(R->sel_ev[1], ctx->stream));

    // select
    SPM_HIP_CHECK(ctx, launch_1d<kSelTile>(ctx, jst_select_loci_kernel, n, P));
    if (plan.best) {
        if (numbered)
            SPM_HIP_CHECK(ctx, exclusive_sum(ctx, tmp, tmp_bytes, counted<uint32_t>(jsel_head_op{P.head}), gid, n));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_select_minima_kernel, n, P));
    }
    SPM_HIP_CHECK(ctx, exclusive_sum(ctx, tmp, tmp_bytes, counted<uint32_t>(flag_op{P}), offs, n));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_select_compact_kernel, n, P, offs, d_out));
    SPM_HIP_CHECK(ctx, hipEventRecord(R->sel_ev[2], ctx->stream));

    // the one read-back: how many records LOCI kept, how many the result has
    SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, 2));
    const unsigned long long *c = ctx->h_counters;
    R->sel.n_loci = c[0];
    R->sel.n_out = c[1];
    if (c[1] > S.n) {
        SPM_SET_ERR(ctx, "pan-genome selection: the compaction counted %llu records out of %llu", c[1], (unsigned long long)S.n);
        return SPM_E_HIP;
    }
    // the result's own buffer, of the kept count; the copy is ordered before any later use of the scratch on this stream
    R->cap = std::max<uint64_t>(c[1], 1);
    SPM_HIP_CHECK(ctx, hipMalloc(&R->d, R->cap * sizeof(spm_jst_hit)));
    if (c[1])
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->d, d_out, c[1] * sizeof(spm_jst_hit), hipMemcpyDeviceToDevice, ctx->stream));
    R->n = c[1];
    return SPM_OK;
}

// opts -> plan -> result
int jsel_make(spm_ctx *ctx, const jsel_source &S, const spm_select_opts *opts, const char *who, clk::time_point t_call,
              spm_jst_hits **out)
{
    // the needle set is read only for the needles' own windows: with an explicit window it may be gone by now (spm_hip.h)
    const bool use_set = S.ps && (opts->flags & SPM_SELECT_LOCI) && opts->window == SPM_SELECT_WINDOW_K;
    const bool myers = use_set && S.ps->is_myers();
    const jst_select_plan plan =
        plan_jst_select(*opts, S.n, S.n_hap, S.n_patterns, S.max_pos, S.ps != nullptr, myers, use_set ? S.ps->max_k : 0);
    if (plan.status != SPM_OK) {
        SPM_SET_ERR(ctx, "%s: %s", who, plan.why);
        return plan.status;
    }
    if (plan.strands && S.strands != 0 && S.strands != 2) {
        // (a raw buffer without a set is taken by the index convention: read = pattern >> 1)
        SPM_SET_ERR(ctx, "%s: SPM_SELECT_STRANDS on a needle set that spm_hip_patterns_create_stranded did not make", who);
        return SPM_E_INVALID;
    }
    if (plan.across && S.n_patterns > kJselAcrossPatterns) {
        // (ACROSS keeps one minimum per pattern index; only a raw buffer without a set can name indices this large)
        SPM_SET_ERR(ctx, "%s: SPM_SELECT_ACROSS takes pattern indices below 2^24, the records name %llu", who,
                    (unsigned long long)(S.n_patterns - 1));
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_hits, void (*)(spm_jst_hits *)> R(new spm_jst_hits, spm_hip_jst_hits_destroy);
    R->ctx = ctx;
    R->selected = true; // (spm_hip_jst_hits_align refuses it, whatever the source was: spm_hip_jst_selection_align takes it)
    R->patterns = S.ps;
    R->jst = S.jst;
    R->generation = S.generation;
    R->pat_strands = S.strands;
    R->sel_n_hap = S.n_hap;
    R->sel_n_patterns = S.n_patterns;
    R->sel_max_pos = S.max_pos;
    SPM_TRY(jsel_run(ctx, S, plan, opts->strata, R.get()));
    if (!plan.loci)
        R->sel.n_loci = R->sel.n_in;
    R->sel_timed = true;
    R->sel.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] %s: %llu records -> %llu loci -> %llu kept; key %u bits (%u + %u + %u), halo %u; host %.3f ms\n",
                who, (unsigned long long)R->sel.n_in, (unsigned long long)R->sel.n_loci, (unsigned long long)R->sel.n_out,
                plan.key_bits, plan.hap_bits, plan.pat_bits, plan.pos_bits, plan.halo, R->sel.ms_host);
    *out = R.release();
    return SPM_OK;
}

} // namespace

extern "C" int spm_hip_jst_hits_select(spm_jst_hits *h, const spm_select_opts *opts, spm_jst_hits **out)
{
    if (!h || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = h->ctx;
    if (!opts) {
        SPM_SET_ERR(ctx, "spm_hip_jst_hits_select: opts is NULL");
        return SPM_E_INVALID;
    }
    const auto t_call = clk::now();
    jsel_source S;
    S.d_recs = h->d;
    S.n = h->n;
    S.ps = h->patterns;
    S.jst = h->jst;
    S.generation = h->generation;
    S.strands = h->pat_strands;
    S.n_hap = std::max<uint64_t>(h->sel_n_hap, 1);
    S.n_patterns = std::max<uint64_t>(h->sel_n_patterns, 1);
    S.max_pos = h->sel_max_pos;
    return jsel_make(ctx, S, opts, "spm_hip_jst_hits_select", t_call, out);
}

extern "C" int spm_hip_jst_records_select(spm_ctx *ctx, const void *device_records, uint64_t n, const spm_patterns *patterns,
                                          const spm_select_opts *opts, spm_jst_hits **out)
{
    if (!ctx || !out || (n && !device_records) || ((uintptr_t)device_records & 7)) {
        SPM_SET_ERR(ctx, "spm_hip_jst_records_select: invalid argument (the records must be 8-byte aligned)");
        return SPM_E_INVALID;
    }
    if (!opts) {
        SPM_SET_ERR(ctx, "spm_hip_jst_records_select: opts is NULL");
        return SPM_E_INVALID;
    }
    const auto t_call = clk::now();
    jsel_source S;
    S.d_recs = static_cast<const spm_jst_hit *>(device_records);
    S.n = n;
    S.ps = patterns;
    S.strands = patterns ? patterns->strands : 0;
    S.n_patterns = patterns ? std::max<uint64_t>(patterns->n, 1) : 1;
    {
        // refuse what the plan refuses whatever the records hold, before anything is launched
        const jst_select_plan early = plan_jst_select(*opts, n, 1, 1, 0, patterns != nullptr, patterns && patterns->is_myers(), 0);
        if (early.status != SPM_OK) {
            SPM_SET_ERR(ctx, "spm_hip_jst_records_select: %s", early.why);
            return early.status;
        }
    }
    if (n) {
        // the ranges of haplotype, pattern and position in the buffer: the host plans the sort key from them
        SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        SPM_TRY(ensure_scratch(ctx, 256));
        unsigned long long *d_rng = static_cast<unsigned long long *>(ctx->d_scratch);
        unsigned long long *c = ctx->h_counters;
        SPM_HIP_CHECK(ctx, hipMemsetAsync(d_rng, 0, 24, ctx->stream));
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 8);
        hipLaunchKernelGGL(jst_select_range_kernel, dim3(grid), dim3(256), 0, ctx->stream,
                           static_cast<const unsigned long long *>(device_records), (uint32_t)n, d_rng);
        SPM_HIP_CHECK(ctx, hipGetLastError());
        SPM_HIP_CHECK(ctx, read_counts(ctx, d_rng, 3));
        const uint64_t max_hap = c[0], max_pat = c[1], max_pos = c[2];
        if (patterns && max_pat >= std::max<uint64_t>(patterns->n, 1)) {
            SPM_SET_ERR(ctx, "spm_hip_jst_records_select: a record names pattern %llu, outside the set of %u",
                        (unsigned long long)max_pat, patterns->n);
            return SPM_E_INVALID;
        }
        if (!patterns)
            S.n_patterns = max_pat + 1;
        S.n_hap = max_hap + 1;
        S.max_pos = max_pos;
    }
    return jsel_make(ctx, S, opts, "spm_hip_jst_records_select", t_call, out);
}

extern "C" int spm_hip_jst_hits_select_stats(const spm_jst_hits *hc, spm_select_stats *out)
{
    if (!hc || !out)
        return SPM_E_INVALID;
    spm_jst_hits *h = const_cast<spm_jst_hits *>(hc);
    if (!h->selected) {
        SPM_SET_ERR(h->ctx, "spm_hip_jst_hits_select_stats: no selection made these hits");
        return SPM_E_INVALID;
    }
    SPM_HIP_CHECK(h->ctx, select_stats_close(h->sel_timed, h->sel_ev[0], h->sel_ev[1], h->sel_ev[2], h->sel));
    *out = h->sel;
    return SPM_OK;
}
