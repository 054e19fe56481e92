// select.hip -- selection of hits behind the C ABI: spm_hip_hits_select, spm_hip_records_select, spm_hip_hits_select_stats.
// The host side of select.hpp: plan (select_plan.hpp), lay the scratch out (scratch_layout.hpp), enqueue keys -> sort -> loci
// -> scan -> compact on the context's stream, read the two counts back (the one synchronisation; device_order.hpp has the
// sort, the scan and the read-back), hand out a new spm_hits.
// MI355X only; no CPU path exists in this library: if HIP fails the call fails.
#include "internal.hpp"
#include "device_order.hpp"
#include "scratch_layout.hpp"
#include "select.hpp"

namespace
{

// a hit block for `cap` records: recycled from the context's pool, or new (the counters cleared either way)
int select_acquire(spm_ctx *ctx, spm_hits *H)
{
    for (size_t i = 0; i < ctx->pool.size(); ++i)
        if (ctx->pool[i].cap == H->cap) {
            static_cast<hits_block &>(*H) = ctx->pool[i];
            ctx->pool.erase(ctx->pool.begin() + i);
            if (!H->zeroed)
                SPM_HIP_CHECK(ctx, hipMemsetAsync(H->d_count, 0, kCntBlock * sizeof(unsigned long long), ctx->stream));
            return SPM_OK;
        }
    SPM_HIP_CHECK(ctx, hipMalloc(&H->d_hits, std::max<uint64_t>(H->cap, 1) * sizeof(spm_hit)));
    SPM_HIP_CHECK(ctx, hipMalloc(&H->d_count, kCntBlock * sizeof(unsigned long long)));
    for (int i = 0; i < 4; ++i)
        SPM_HIP_CHECK(ctx, hipEventCreate(&H->ev[i]));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(H->d_count, 0, kCntBlock * sizeof(unsigned long long), ctx->stream));
    return SPM_OK;
}

struct select_source // what the two entry points know about their records
{
    const spm_hit *d_recs = nullptr;
    uint64_t n = 0;
    uint64_t n_patterns = 1;
    uint64_t bias = 0, max_rel = 0;      // pos - bias lies in [0, max_rel]
    const spm_patterns *ps = nullptr;    // may be null (records)
    const std::vector<uint64_t> *segs = nullptr;
    uint64_t pos_offset = 0;
    uint64_t cap = 0;                    // capacity of the result's hit block
};

int select_run(spm_ctx *ctx, const select_source &S, const select_plan &plan, uint32_t strata, spm_hits *H)
{
    const uint32_t n = (uint32_t)S.n;
    H->sel.n_in = S.n;
    H->sel.key_bits = plan.key_bits;
    SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[0], ctx->stream));
    if (n == 0) {
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[1], ctx->stream));
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[2], ctx->stream));
        return SPM_OK;
    }
    const uint64_t n_segs = S.segs && S.segs->size() > 1 ? S.segs->size() - 1 : 0;

    // the scratch: keys and indices twice (the sort's in and out), flags, scores, offsets, minima, segment table, counts
    using flag_op = sel_flag_op<select_params>;
    select_params P{};
    size_t sort_bytes = 0, scan_bytes = 0;
    SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, n, plan.key_bits, &sort_bytes));
    SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(flag_op{P}), n, &scan_bytes));
    const size_t tmp_bytes = std::max(sort_bytes, scan_bytes);
    unsigned long long *keys_in = nullptr, *d_segs = nullptr;
    uint32_t *idx_in = nullptr, *offs = nullptr;
    uint8_t *tmp = nullptr;
    scratch_layout L;
    L.take(keys_in, n);
    L.take(P.keys, n);
    L.take(idx_in, n);
    L.take(P.idx, n);
    L.take(P.keep, n);
    L.take(P.score, n);
    L.take(offs, n);
    L.take(P.minima, plan.min_slots);
    L.take(d_segs, n_segs ? n_segs + 1 : 0);
    L.take(P.counts, 2);
    L.take(tmp, tmp_bytes);
    SPM_TRY(ensure_scratch(ctx, L.bytes()));
    L.bind(ctx->d_scratch);

    P.recs = S.d_recs;
    P.n = n;
    P.pos_bits = plan.pos_bits;
    P.pos_mask = plan.pos_bits >= 64 ? ~0ull : (1ull << plan.pos_bits) - 1;
    P.bias = S.bias;
    P.loci = plan.loci;
    P.best = plan.best;
    P.shift = plan.strands ? 1u : 0u;
    P.window = plan.window;
    P.k_tab = plan.window == SPM_SELECT_WINDOW_K && S.ps ? S.ps->d_k : nullptr;
    P.halo = plan.halo;
    P.strata = strata;
    if (!plan.best)
        P.minima = nullptr;
    if (n_segs) {
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_segs, S.segs->data(), (n_segs + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        P.segs = d_segs;
        P.n_segs = n_segs;
        P.seg_bias = S.bias - S.pos_offset;
        P.seg_myers = S.ps && S.ps->is_myers() ? 1u : 0u;
    }
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, 16, ctx->stream));
    if (plan.best)
        SPM_HIP_CHECK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(P.minima), 0x7FFFFFFF, plan.min_slots, ctx->stream));

    // order
    SPM_HIP_CHECK(ctx, launch_1d(ctx, select_keys_kernel, n, S.d_recs, keys_in, idx_in, n, plan.pos_bits, S.bias));
    SPM_HIP_CHECK(ctx, sort_pairs(ctx, tmp, tmp_bytes, keys_in, P.keys, idx_in, P.idx, n, plan.key_bits));
    SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[1], ctx->stream));

    // select
    SPM_HIP_CHECK(ctx, launch_1d<kSelTile>(ctx, select_loci_kernel, n, P));
    SPM_HIP_CHECK(ctx, exclusive_sum(ctx, tmp, tmp_bytes, counted<uint32_t>(flag_op{P}), offs, n));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, select_compact_kernel, n, P, offs, H->d_hits, H->d_count + kCntHits));
    SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[2], ctx->stream));

    // the one read-back: how many records LOCI kept, how many the result has
    SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, 2));
    const unsigned long long *c = ctx->h_counters;
    H->sel.n_loci = c[0];
    H->sel.n_out = c[1];
    H->n = c[1];
    return SPM_OK;
}

// opts -> plan -> result; `fill` copies what the result inherits from its source
int select_make(spm_ctx *ctx, const select_source &S, const spm_select_opts *opts, const char *who, clk::time_point t_call,
                const std::function<void(spm_hits *)> &fill, spm_hits **out)
{
    const bool myers = S.ps && S.ps->is_myers();
    const select_plan plan = plan_select(*opts, S.n, S.n_patterns, S.max_rel, S.ps != nullptr, myers, S.ps ? S.ps->max_k : 0);
    if (plan.status != SPM_OK) {
        SPM_SET_ERR(ctx, "%s: %s", who, plan.why);
        return plan.status;
    }
    if (plan.strands && S.ps && S.ps->strands != 2) {
        // (a raw buffer without a set is taken by the index convention: read = pattern >> 1)
        SPM_SET_ERR(ctx, "%s: SPM_SELECT_STRANDS on a needle set that spm_hip_patterns_create_stranded did not make", who);
        return SPM_E_INVALID;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_hits, void (*)(spm_hits *)> H(new spm_hits, spm_hip_hits_destroy);
    H->ctx = ctx;
    H->cap = S.cap;
    SPM_TRY(select_acquire(ctx, H.get()));
    fill(H.get());
    H->selected = true;
    H->timed = false; // (ev[0..2] are the selection's; the scan statistics are the source's, copied)
    H->counted = true;
    H->n = 0;
    H->sel = spm_select_stats{};
    SPM_TRY(select_run(ctx, S, plan, opts->strata, H.get()));
    if (!plan.loci)
        H->sel.n_loci = H->sel.n_in;
    H->sel_timed = true;
    H->sel.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] %s: %llu records -> %llu loci -> %llu kept; key %u bits, halo %u; host %.3f ms\n", who,
                (unsigned long long)H->sel.n_in, (unsigned long long)H->sel.n_loci, (unsigned long long)H->sel.n_out,
                plan.key_bits, plan.halo, H->sel.ms_host);
    *out = H.release();
    return SPM_OK;
}

} // namespace

extern "C" int spm_hip_hits_select(spm_hits *h, const spm_select_opts *opts, spm_hits **out)
{
    if (!h || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = h->ctx;
    if (!opts) {
        SPM_SET_ERR(ctx, "spm_hip_hits_select: opts is NULL");
        return SPM_E_INVALID;
    }
    const auto t_call = clk::now();
    const void *d_recs = nullptr;
    uint64_t n = 0;
    const int rc = spm_hip_hits_device(h, &d_recs, &n); // (completes a deferred scan; SPM_E_OVERFLOW for an overflowed one)
    if (rc != SPM_OK)
        return rc;
    const spm_patterns *ps = h->al_patterns;
    if (h->al_device_segs) {
        SPM_SET_ERR(ctx, "spm_hip_hits_select: the segment hits of a journaled-sequence search cannot be selected (not supported)");
        return SPM_E_UNSUPPORTED;
    }
    select_source S;
    S.d_recs = static_cast<const spm_hit *>(d_recs);
    S.n = n;
    S.ps = ps;
    S.cap = h->cap;
    S.pos_offset = h->al_pos_offset;
    S.segs = h->al_segs.empty() ? nullptr : &h->al_segs;
    if (h->sel_records) {
        // a selection of a selection of raw records: positions as the first selection found them
        S.n_patterns = h->sel_n_patterns;
        S.bias = h->sel_bias;
        S.max_rel = h->sel_max_rel;
    } else {
        if (!ps || !h->al_text) {
            SPM_SET_ERR(ctx, "spm_hip_hits_select: these hits do not come from spm_hip_scan / spm_hip_scan_segments");
            return SPM_E_INVALID;
        }
        // positions: pos_offset + [0, |text|]; the begin of an exact occurrence that a restored state completes lies up to
        // max|P| - 1 symbols in front of its chunk (spm_hip_hits_view compares positions as signed for the same reason)
        const uint64_t before = h->al_stateful && !ps->is_myers() ? ps->max_m : 0;
        S.n_patterns = std::max<uint64_t>(ps->n, 1);
        S.bias = h->al_pos_offset - before;
        S.max_rel = h->al_text->n + before;
    }
    spm_scan_stats st{};
    if (!h->sel_records)
        (void)spm_hip_hits_stats(h, &st);
    return select_make(ctx, S, opts, "spm_hip_hits_select", t_call,
                       [&](spm_hits *H) {
                           H->stats = st;
                           H->al_text = h->al_text;
                           H->al_patterns = h->al_patterns;
                           H->al_lo = h->al_lo;
                           H->al_pos_offset = h->al_pos_offset;
                           H->al_stateful = h->al_stateful;
                           H->al_segs = h->al_segs;
                           H->sel_records = h->sel_records;
                           H->sel_n_patterns = h->sel_n_patterns;
                           H->sel_bias = h->sel_bias;
                           H->sel_max_rel = h->sel_max_rel;
                       },
                       out);
}

extern "C" int spm_hip_records_select(spm_ctx *ctx, const void *device_records, uint64_t n, const spm_patterns *patterns,
                                      const spm_select_opts *opts, spm_hits **out)
{
    if (!ctx || !out || (n && !device_records) || ((uintptr_t)device_records & 15)) {
        SPM_SET_ERR(ctx, "spm_hip_records_select: invalid argument (the records must be 16-byte aligned)");
        return SPM_E_INVALID;
    }
    if (!opts) {
        SPM_SET_ERR(ctx, "spm_hip_records_select: opts is NULL");
        return SPM_E_INVALID;
    }
    const auto t_call = clk::now();
    select_source S;
    S.d_recs = static_cast<const spm_hit *>(device_records);
    S.n = n;
    S.ps = patterns;
    S.n_patterns = patterns ? std::max<uint64_t>(patterns->n, 1) : 1;
    S.cap = std::max<uint64_t>(n, 1ull << 20); // (the default capacity of a scan: such a block is likely in the pool)
    {
        // refuse what the plan refuses whatever the records hold, before anything is launched
        const select_plan early = plan_select(*opts, n, 1, 0, patterns != nullptr, patterns && patterns->is_myers(), 0);
        if (early.status != SPM_OK) {
            SPM_SET_ERR(ctx, "spm_hip_records_select: %s", early.why);
            return early.status;
        }
    }
    if (n) {
        // the range of the positions and patterns in the buffer: the host plans the sort key from it
        SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        SPM_TRY(ensure_scratch(ctx, 256));
        unsigned long long *d_rng = static_cast<unsigned long long *>(ctx->d_scratch);
        const unsigned long long init[3] = {~0ull, 0ull, 0ull};
        unsigned long long *c = ctx->h_counters;
        memcpy(c, init, sizeof(init));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_rng, c, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 8);
        hipLaunchKernelGGL(select_range_kernel, dim3(grid), dim3(256), 0, ctx->stream, S.d_recs, (uint32_t)n, d_rng);
        SPM_HIP_CHECK(ctx, hipGetLastError());
        SPM_HIP_CHECK(ctx, read_counts(ctx, d_rng, 3));
        const uint64_t lo = c[0] ^ (1ull << 63), hi = c[1] ^ (1ull << 63), max_pat = c[2];
        if (patterns && max_pat >= std::max<uint64_t>(patterns->n, 1)) {
            SPM_SET_ERR(ctx, "spm_hip_records_select: a record names pattern %llu, outside the set of %u",
                        (unsigned long long)max_pat, patterns->n);
            return SPM_E_INVALID;
        }
        if (!patterns)
            S.n_patterns = max_pat + 1;
        S.bias = lo;
        S.max_rel = hi - lo;
    }
    return select_make(ctx, S, opts, "spm_hip_records_select", t_call,
                       [&](spm_hits *H) {
                           H->sel_records = true;
                           H->sel_n_patterns = S.n_patterns;
                           H->sel_bias = S.bias;
                           H->sel_max_rel = S.max_rel;
                           H->al_patterns = patterns; // (the window table of a later selection; align refuses sel_records)
                       },
                       out);
}

extern "C" int spm_hip_hits_select_stats(const spm_hits *hc, spm_select_stats *out)
{
    if (!hc || !out)
        return SPM_E_INVALID;
    spm_hits *h = const_cast<spm_hits *>(hc);
    if (!h->selected) {
        SPM_SET_ERR(h->ctx, "spm_hip_hits_select_stats: no selection made these hits");
        return SPM_E_INVALID;
    }
    SPM_HIP_CHECK(h->ctx, select_stats_close(h->sel_timed, h->ev[0], h->ev[1], h->ev[2], h->sel));
    *out = h->sel;
    return SPM_OK;
}
