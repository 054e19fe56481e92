// scan.hip -- the scan driver behind spm_hip_scan / spm_hip_scan_segments: what seqan_pattern_base::operator() does
// (/root/reference/libspm/libspm/matcher/seqan_pattern_base.hpp:40-71) -- choose the engine, run it, handle overflow and fallbacks.
// MI355X only; no CPU scan path exists in this library: if HIP fails the call fails.
#include "internal.hpp"
#include "filter_shared.hpp"

int ensure_scratch(spm_ctx *ctx, size_t bytes)
{
    if (ctx->scratch_bytes >= bytes)
        return SPM_OK;
    const auto t0 = clk::now();
    if (ctx->d_scratch) {
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        SPM_HIP_CHECK(ctx, hipFree(ctx->d_scratch));
        ctx->d_scratch = nullptr;
        ctx->scratch_bytes = 0;
    }
    // what a scan needs follows what earlier scans counted, and those counts wobble by a few per cent from run to run (slots
    // are drawn in chunks): a quarter of headroom, so that a text with millions of candidates does not pay for a new multi-GB
    // allocation (hundreds of ms) every few scans
    size_t want = bytes + bytes / 4;
    hipError_t e = hipMalloc(&ctx->d_scratch, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        want = bytes;
        SPM_HIP_CHECK(ctx, hipMalloc(&ctx->d_scratch, want));
    }
    ctx->scratch_bytes = want;
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] scratch (survivor / band lists, dedupe set) grows to %.1f MiB: %.2f ms\n", want / 1048576.0, ms_since(t0));
    return SPM_OK;
}

extern "C" int spm_hip_scan(spm_ctx *ctx, const spm_text *text, uint64_t begin, uint64_t end,
                            const spm_patterns *patterns, const spm_scan_opts *opts_in, const void *state_in,
                            void *state_out, spm_hits **out)
{
    return scan_impl(ctx, text, begin, end, patterns, opts_in, state_in, state_out, nullptr, 0, out);
}

extern "C" int spm_hip_scan_segments(spm_ctx *ctx, const spm_text *text, const uint64_t *seg_offsets,
                                     uint64_t n_segments, const spm_patterns *patterns, const spm_scan_opts *opts_in,
                                     spm_hits **out)
{
    if (!ctx || !text || !seg_offsets || n_segments == 0) {
        SPM_SET_ERR(ctx, "spm_hip_scan_segments: invalid argument");
        return SPM_E_INVALID;
    }
    for (uint64_t s = 0; s < n_segments; ++s)
        if (seg_offsets[s + 1] < seg_offsets[s] || seg_offsets[s + 1] > text->n) {
            SPM_SET_ERR(ctx, "spm_hip_scan_segments: offsets must ascend and stay inside the text");
            return SPM_E_INVALID;
        }
    spm_scan_opts o{};
    if (opts_in)
        o = *opts_in;
    o.left_context = 0;
    return scan_impl(ctx, text, seg_offsets[0], seg_offsets[n_segments], patterns, &o, nullptr, nullptr, seg_offsets,
                     n_segments, out);
}

namespace
{
// the hit buffer, the counter block (cleared) and the events of this scan: recycled from an earlier scan, or new
int acquire_hits(spm_ctx *ctx, spm_hits *H)
{
    // recycle the buffers of an earlier scan (hipMalloc/hipEventCreate per scan cost ~0.2 ms)
    for (size_t i = 0; i < ctx->pool.size(); ++i)
        if (ctx->pool[i].cap == H->cap) {
            static_cast<hits_block &>(*H) = ctx->pool[i];
            ctx->pool.erase(ctx->pool.begin() + i);
            if (!H->zeroed) // (a recycled block was cleared when it went back to the pool, off this scan's critical path)
                SPM_HIP_CHECK(ctx, hipMemsetAsync(H->d_count, 0, kCntBlock * sizeof(unsigned long long), ctx->stream));
            return SPM_OK;
        }
    const auto ta = clk::now();
    SPM_HIP_CHECK(ctx, hipMalloc(&H->d_hits, std::max<uint64_t>(H->cap, 1) * sizeof(spm_hit)));
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] a new hit buffer (%llu records): %.2f ms\n", (unsigned long long)H->cap, ms_since(ta));
    SPM_HIP_CHECK(ctx, hipMalloc(&H->d_count, kCntBlock * sizeof(unsigned long long)));
    for (int i = 0; i < 4; ++i)
        SPM_HIP_CHECK(ctx, hipEventCreate(&H->ev[i]));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(H->d_count, 0, kCntBlock * sizeof(unsigned long long), ctx->stream));
    return SPM_OK;
}

// Filter or brute force.  Restorable scans (myers_matcher_restorable.hpp:72-82: the chunk continues from the restored
// state): only the first window_size - 1 symbols of a chunk can complete an occurrence that began before it: those are
// scanned by the brute-force kernel from the state; from there on every occurrence lies inside the chunk, so the seed
// filter takes the rest with the chunk as its haystack.  The state after the last symbol comes from the last 2 max|P|
// symbols.  Short chunks stay with the brute-force kernel (unless the caller asks for the filter).
int choose_engine(spm_ctx *ctx, const spm_patterns *patterns, const spm_scan_opts &opts, uint64_t range, bool stateful,
                  bool segmented, uint64_t state_prefix, bool &use_filter)
{
    const bool want_filter = opts.engine == SPM_ENGINE_FILTER || (opts.engine == SPM_ENGINE_AUTO && !patterns->fidx.empty());
    if (opts.engine == SPM_ENGINE_FILTER && patterns->fidx.empty()) {
        SPM_SET_ERR(ctx, "spm_hip_scan: the seed filter does not apply to this needle set");
        return SPM_E_UNSUPPORTED;
    }
    use_filter = want_filter && patterns->n > 0 && range > 0;
    if (stateful && use_filter &&
        (segmented || range <= state_prefix || (opts.engine != SPM_ENGINE_FILTER && range < (1u << 18))))
        use_filter = false;
    if (opts.engine == SPM_ENGINE_FILTER && !use_filter && patterns->n > 0 && range > 0) {
        SPM_SET_ERR(ctx, "spm_hip_scan: the seed filter does not apply to this stateful scan (chunk shorter than a window)");
        return SPM_E_UNSUPPORTED;
    }
    return SPM_OK;
}

void take_stats(spm_hits *h, const unsigned long long *c)
{
    h->stats.n_candidates = c[kCntPairs];
    h->stats.n_bands = (uint32_t)std::min<unsigned long long>(c[kCntBandsVerified], 0xFFFFFFFFull);
}

struct scan_call // one scan_impl call: the request, what was decided about it, the state of its attempts; and its steps
{
    const scan_args &A;
    spm_ctx *ctx;
    const spm_patterns *ps;
    spm_hits *H;
    uint64_t begin, end; // the caller's range (A.begin .. A.end: the filter engine's share of it)
    const void *state_in;
    void *state_out;
    bool has_state, stateful, segmented;
    uint64_t state_prefix, tail_begin; // symbols of a chunk that can complete an occurrence begun before it; first symbol
                                       // of a state-only pass that ends at `end`
    const std::function<int(spm_hits *)> *after_launch;
    scan_state S{};

    // a scan with nothing to report and nothing to compute: the events, and the state handed through
    int finish_trivial()
    {
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[1], ctx->stream));
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[2], ctx->stream));
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[3], ctx->stream));
        H->stats.engine_used = SPM_ENGINE_BRUTE;
        if (state_in && state_out && state_out != state_in)
            memcpy(state_out, state_in, spm_hip_patterns_state_stride(ps) * ps->n);
        else if (state_out && !state_in)
            spm_hip_patterns_state_init(ps, state_out);
        return SPM_OK;
    }

    // clear the counter block for another attempt and (usually) forget the launches of the one that is discarded
    int clear_counters(bool forget_launches = true)
    {
        SPM_HIP_CHECK(ctx, hipMemsetAsync(H->d_count, 0, kCntBlock * sizeof(unsigned long long), ctx->stream));
        if (forget_launches)
            H->stats.main_launches = 0;
        return SPM_OK;
    }

    // segmented scans: the segment table on the host -- the caller's, or fetched from the device once per call
    int host_segments()
    {
        if (S.segs || !A.d_seg_offsets)
            return SPM_OK;
        S.seg_host.resize(A.n_segments + 1);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(S.seg_host.data(), A.d_seg_offsets, (A.n_segments + 1) * sizeof(uint64_t),
                                          hipMemcpyDeviceToHost, ctx->stream));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        S.segs = S.seg_host.data();
        return SPM_OK;
    }

    // deferred completion: the counters travel to this result's own pinned block; nobody waits for them now
    int defer_completion()
    {
        if (!H->h_c)
            SPM_HIP_CHECK(ctx, hipHostMalloc(&H->h_c, kCntBlock * sizeof(unsigned long long), hipHostMallocDefault));
        if (!H->ev_done)
            SPM_HIP_CHECK(ctx, hipEventCreateWithFlags(&H->ev_done, hipEventDisableTiming));
        // (the copy itself is enqueued by whoever asks first: spm_hip_hits_copy_fused_device lets its kernel write the
        // counters to the pinned block -- no launch of its own --, anything else enqueues it in spm_complete_deferred)
        H->pending = true;
        H->c_on_the_way = false;
        H->d_count_cleared = false;
        // Sets that go through the band table: the host cannot know yet whether this scan gave every slot back.
        // It assumes so; if the band list or the table overflowed, the device remembers (resolve_params::
        // table_poison), later scans declare themselves void until the host -- completing this one -- has emptied
        // the table, and are repeated when they are completed in turn.
        ctx->band_dirty = false;
        H->d_text = A.text;
        H->d_patterns = ps;
        H->d_begin = begin;
        H->d_end = end;
        H->d_opts = A.opts;
        return SPM_OK;
    }

    // ---- span-local fallback: only the spans that gave up are scanned again, by the brute-force kernel ----
    int span_fallback(unsigned long long *c)
    {
        const uint64_t n_ovf = c[kCntSpansGaveUp];
        std::vector<uint64_t> ov(2 * n_ovf);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(ov.data(), S.filt.d_ovf, ov.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        const fallback_plan F = plan_fallback(ov.data(), n_ovf, A.begin, end, ps->max_window, (uint64_t)ctx->n_cu, ps->n_groups);
        if (segmented) // every segment is a haystack of its own: the tiles follow the segment table
            SPM_TRY(host_segments());
        std::vector<uint64_t> tab;
        fallback_tiles(F, A.ctx_begin, segmented ? S.segs : nullptr, A.n_segments, tab);
        H->stats.fallback_spans = (uint32_t)std::min<uint64_t>(n_ovf, 0xFFFFFFFFu);
        if (!tab.empty()) {
            if (tab.size() / 3 > 0xFFFFFFFFull) {
                SPM_SET_ERR(ctx, "span-local fallback: too many tiles");
                return SPM_E_UNSUPPORTED;
            }
            S.tiles = &tab;
            const int rc = run_brute(A, S, begin, end, A.ctx_begin, nullptr, nullptr, true, false);
            S.tiles = nullptr;
            SPM_TRY(rc);
            H->stats.main_launches--; // (run_brute counts itself as a main launch: ms_main stays the filter's)
            SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[3], ctx->stream)); // the re-scan counts as verification time
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(c, H->d_count, kCntReadBackRescan * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        }
        H->stats.fallback_symbols = F.total;
        return SPM_OK;
    }

    // ---- the filter engine's attempts: run, maybe defer, maybe hook, read counters, ask the policy, act.  On return the
    // hit list is final, or the scan was deferred, or use_filter is false: the whole range again, brute force ----
    int filter_attempts(bool &use_filter, bool &deferred)
    {
        unsigned long long *c = ctx->h_counters;
        // (further rounds: the dedupe set was left out, or too small for the re-scan's hits)
        for (int round = 0, attempt = 0; round < 3;) {
            SPM_TRY(run_filter(A, S.retry, S.filt));
            H->cand_cap = S.filt.cand_cap;
            H->band_cap = S.filt.band_cap;
            if ((A.opts.flags & SPM_SCAN_DEFER) && round == 0 && attempt == 0 && !stateful && !segmented && !after_launch) {
                deferred = true;
                return defer_completion();
            }
            if (after_launch && !stateful)
                SPM_TRY((*after_launch)(H));
            // the overflow checks need the counters: one small D2H copy
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(c, H->d_count, kCntReadBack * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            if (c[kCntVoid] == 0)
                ctx->band_dirty = false; // every band was consumed: the table is empty again
            scan_decision d = decide_scan(c, S.filt, H->cap, S.retry, attempt, A.tune.cand_cap);
            if (d.what == scan_outcome::more_room) {
                if (spm_trace_on())
                    fprintf(stderr, "[spm_hip] scan attempt %d starts over:%s%s%s (survivor slots drawn %llu of %llu, band slots %llu of %llu, "
                                    "overflow flags %llu, spans that gave up %llu)\n",
                            attempt, d.more_surv ? " survivor list too small" : "", d.more_bands ? " band list too small" : "",
                            d.more_seen ? " dedupe set too small" : "", c[kCntSurvSlots], (unsigned long long)H->cand_cap,
                            c[kCntBandSlots], (unsigned long long)H->band_cap, c[kCntVoid], c[kCntSpansGaveUp]);
                S.retry = d.next;
                ++attempt;
                SPM_TRY(clear_counters());
                continue;
            }
            take_stats(H, c);
            if (scan_clean(c, H->cand_cap))
                raise_hints(*ps, c);
            const bool rescan = d.what == scan_outcome::span_fallback;
            if (rescan) {
                SPM_TRY(span_fallback(c));
                d = decide_scan(c, S.filt, H->cap, S.retry, attempt, A.tune.cand_cap, true);
            }
            S.retry = d.next;
            switch (d.what) {
            case scan_outcome::brute_fallback:
                H->stats.fell_back = 1;
                use_filter = false;
                return clear_counters(false);
            case scan_outcome::with_seen:
            case scan_outcome::with_full_seen: // a new round
                SPM_TRY(clear_counters());
                ++round;
                attempt = 0;
                continue;
            case scan_outcome::final_hits:
            case scan_outcome::caller_overflow:
                H->n = c[kCntHits];
                H->counted = true;
                if (!rescan && d.what == scan_outcome::final_hits && after_launch && !stateful) { // nothing was added to the hit list after the caller's work ran on it
                    H->hook_final = true;
                    H->fan_count = c[kCntFanOut];
                }
                return SPM_OK;
            case scan_outcome::more_room: // (both handled above, and never decided after the re-scan)
            case scan_outcome::span_fallback:
                return SPM_E_INVALID;
            }
        }
        return SPM_OK;
    }

    // the states of a stateful scan on the device, in the kernels' layout (freed on every return path): state_in goes up
    dev_scratch state_mem;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    size_t st_words = 0;
    std::vector<uint32_t> h_in;
    int state_open()
    {
        if (!stateful)
            return SPM_OK;
        st_words = (size_t)ps->n_groups * (ps->is_myers() ? 2 * ps->NW + 1 : ps->NW) * 64;
        SPM_HIP_CHECK(ctx, state_mem.alloc(&d_in, st_words * 4 * 2));
        d_out = d_in + st_words;
        if (has_state) {
            state_to_internal(ps, state_in, h_in);
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_in, h_in.data(), st_words * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        return SPM_OK;
    }
    // ... and the state after the last symbol comes back: from a state-only pass that starts at tail_begin, unless `have`
    int state_close(bool have, bool aside)
    {
        if (state_out && !have) {
            SPM_TRY(run_brute(A, S, tail_begin, end, tail_begin, has_state && tail_begin == begin ? d_in : nullptr, d_out, false, true));
            H->stats.main_launches -= aside ? 1 : 0;
        }
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[3], ctx->stream));
        std::vector<uint32_t> h_out(state_out ? st_words : 0);
        if (state_out)
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(h_out.data(), d_out, st_words * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (d_in) // (h_in is a host temporary; d_in is freed on return)
            SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (state_out)
            state_from_internal(ps, h_out, state_out);
        return SPM_OK;
    }

    // ---- the brute-force kernel's share of a filtered chunk: its first window - 1 symbols, and the exit state ----
    int stateful_remainder()
    {
        SPM_TRY(state_open());
        if (has_state) {
            SPM_TRY(run_brute(A, S, begin, begin + state_prefix, begin, d_in, nullptr, true, true));
            H->stats.main_launches--; // (ms_main stays the filter's)
            H->counted = false;       // more hits may have arrived
        }
        return state_close(false, true);
    }

    // ---- the brute-force engine: the whole range in one launch, plus a state-only pass where the exit state needs one ----
    int brute_engine()
    {
        H->stats.engine_used = SPM_ENGINE_BRUTE;
        H->stats.span_symbols = 0; // (no streaming launch, or one whose scan is being replaced)
        SPM_TRY(state_open());
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[1], ctx->stream));
        const uint64_t range = end - begin;
        // A scan that must hand back an exact state and fits one tile does both in one pass, unless that pass starts too
        // late: a single tile cold-starts max_window - 1 symbols before begin, or at ctx_begin (a prefix set's always).
        const bool prefix = ps->algo == SPM_ALGO_MYERS_PREFIX;
        const uint64_t warm = ps->max_window > 0 ? ps->max_window - 1 : 0;
        const uint64_t pass_begin = begin - std::min(warm, begin - A.ctx_begin);
        const bool one_pass_state = state_out && (prefix || (range <= (1u << 16) && (has_state || pass_begin <= tail_begin)));
        SPM_TRY(host_segments()); // (a device-resident segment table: the fallback of the journaled-sequence search)
        SPM_TRY(run_brute(A, S, begin, end, A.ctx_begin, has_state ? d_in : nullptr, one_pass_state ? d_out : nullptr, true,
                          one_pass_state));
        SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[2], ctx->stream));
        return state_close(one_pass_state, false);
    }

    void trace(clk::time_point t_call) const
    {
        spm_scan_stats st{}; // (costs one event synchronisation: diagnostics only)
        spm_hip_hits_stats(H, &st);
        fprintf(stderr, "[spm_hip] scan [%llu, %llu)%s: engine %s%s, %u main launch(es); %.3f ms (main %.3f, verification %.3f); "
                        "%llu seed-checked pairs, %u bands, %llu hits%s; host %.3f ms\n",
                (unsigned long long)begin, (unsigned long long)end, segmented ? " segmented" : "",
                st.engine_used == SPM_ENGINE_FILTER ? (ps->filter_dense ? "filter (dense pass)" : "filter") : "brute",
                st.fell_back ? " after a whole-scan fallback" : "", st.main_launches, st.ms_total, st.ms_main, st.ms_verify,
                (unsigned long long)st.n_candidates, st.n_bands, (unsigned long long)st.n_hits,
                st.fallback_spans ? " (spans re-scanned by the brute-force kernel)" : "", ms_since(t_call));
    }
};

} // namespace

int scan_impl(spm_ctx *ctx, const spm_text *text, uint64_t begin, uint64_t end, const spm_patterns *patterns,
              const spm_scan_opts *opts_in, const void *state_in, void *state_out, const uint64_t *seg_offsets,
              uint64_t n_segments, spm_hits **out, const uint64_t *d_seg_offsets, const uint32_t *d_seg_owned,
              const std::function<int(spm_hits *)> *after_launch)
{
    if (!ctx || !text || !patterns || !out || begin > end || end > text->n) {
        SPM_SET_ERR(ctx, "spm_hip_scan: invalid argument");
        return SPM_E_INVALID;
    }
    if (patterns->sigma != text->sigma) {
        SPM_SET_ERR(ctx, "spm_hip_scan: text sigma %u != pattern sigma %u", text->sigma, patterns->sigma);
        return SPM_E_INVALID;
    }
    spm_scan_opts opts{};
    if (opts_in)
        opts = *opts_in;
    const auto t_call = clk::now();
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));

    std::unique_ptr<spm_hits, void (*)(spm_hits *)> H(new spm_hits, spm_hip_hits_destroy);
    H->ctx = ctx;
    H->cap = opts.max_hits ? opts.max_hits : (1ull << 20);
    SPM_TRY(acquire_hits(ctx, H.get()));
    H->al_text = text;
    H->al_patterns = patterns;
    H->al_lo = opts.left_context ? 0 : begin;
    H->al_pos_offset = opts.pos_offset;
    H->al_stateful = state_in != nullptr;
    H->al_device_segs = d_seg_offsets != nullptr && seg_offsets == nullptr;
    if (seg_offsets)
        H->al_segs.assign(seg_offsets, seg_offsets + n_segments + 1);

    const bool has_state = state_in != nullptr, stateful = has_state || state_out != nullptr;
    const bool segmented = seg_offsets || d_seg_offsets;
    const uint64_t state_prefix = has_state && patterns->max_window > 0 ? patterns->max_window - 1 : 0;
    bool use_filter = false;
    SPM_TRY(choose_engine(ctx, patterns, opts, end - begin, stateful, segmented, state_prefix, use_filter));
    // the filter's part of a chunk: hits whose last symbol lies at or behind begin + window - 1, haystack = the chunk
    const bool chunk = use_filter && has_state;
    const scan_args A{ctx, text, chunk ? begin + state_prefix : begin, end, chunk || !opts.left_context ? begin : 0, patterns, opts,
                      H.get(), scan_tuning::from_env(), seg_offsets, n_segments, d_seg_offsets, d_seg_owned};
    // First symbol of a state-only pass that ends at `end`: from a cold start there the exit state is exact, because it
    // is the haystack's first symbol or lies 2 max|P| + 4 symbols before end (every DP cell D[i][j] <= i has an optimal
    // alignment spanning <= 2i symbols).  With state_in the pass continues from the state at begin instead.
    const uint64_t tail_len = 2ull * patterns->max_m + 4;
    const uint64_t tail_begin = std::max(has_state ? begin : A.ctx_begin, end > tail_len ? end - tail_len : 0);
    scan_call C{A, ctx, patterns, H.get(), begin, end, state_in, state_out, has_state, stateful, segmented, state_prefix, tail_begin,
                after_launch};
    C.S.segs = seg_offsets;

    SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[0], ctx->stream));
    H->timed = true;
    // (an empty range with left context and no state_in still owes the state after text[0, end): the brute path below)
    // A prefix hit ends within max_window symbols of the haystack start: a stateless prefix scan that begins later
    // has nothing to report and nothing to compute.
    const bool past_prefix_hits = patterns->algo == SPM_ALGO_MYERS_PREFIX && !stateful &&
                                  begin - A.ctx_begin >= patterns->max_window;
    if (patterns->n == 0 || past_prefix_hits || (end == begin && (has_state || !state_out || A.ctx_begin == begin))) {
        SPM_TRY(C.finish_trivial());
        *out = H.release();
        return SPM_OK;
    }
    if (use_filter) {
        H->stats.engine_used = SPM_ENGINE_FILTER;
        bool deferred = false;
        SPM_TRY(C.filter_attempts(use_filter, deferred));
        if (deferred) {
            *out = H.release();
            return SPM_OK;
        }
    }
    if (use_filter && stateful)
        SPM_TRY(C.stateful_remainder());
    if (!use_filter)
        SPM_TRY(C.brute_engine());
    if (spm_trace_on())
        C.trace(t_call);
    *out = H.release();
    return SPM_OK;
}


// A deferred scan's counters have arrived (or are waited for here).  The usual case: nothing overflowed, no span gave up --
// the hit list is final.  Otherwise the scan is repeated the ordinary way (with its retries and fallbacks) and its result
// takes this one's place.
int spm_complete_deferred(spm_hits *h)
{
    if (!h->pending)
        return SPM_OK;
    spm_ctx *ctx = h->ctx;
    h->pending = false;
    if (!h->c_on_the_way) {
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(h->h_c, h->d_count, kCntReadBack * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        SPM_HIP_CHECK(ctx, hipEventRecord(h->ev_done, ctx->stream));
        h->c_on_the_way = true;
    }
    SPM_HIP_CHECK(ctx, hipEventSynchronize(h->ev_done));
    const unsigned long long *c = h->h_c;
    take_stats(h, c);
    const bool clean = scan_clean(c, h->cand_cap);
    if (c[kCntVoid] != 0)
        ctx->band_dirty = true; // (a list or the table overflowed -- or the scan found the table poisoned: empty it next)
    // (more hits than the buffer takes is the caller's overflow, not a reason to scan again)
    if (clean || (c[kCntHits] > h->cap && c[kCntVoid] == 0)) {
        if (clean)
            raise_hints(*h->d_patterns, c);
        h->n = c[kCntHits];
        h->counted = true;
        return SPM_OK;
    }
    spm_scan_opts o = h->d_opts;
    o.flags &= ~SPM_SCAN_DEFER;
    spm_hits *again = nullptr;
    const int rc = scan_impl(ctx, h->d_text, h->d_begin, h->d_end, h->d_patterns, &o, nullptr, nullptr, nullptr, 0, &again);
    if (rc != SPM_OK)
        return rc;
    hits_adopt(*h, *again);
    spm_hip_hits_destroy(again);
    return SPM_OK;
}
