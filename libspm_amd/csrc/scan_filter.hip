// scan_filter.hip -- the seed-filter engine (filter.hpp): buffer sizing and the launches of one scan.  The kernels live in
// the units of filter_launch.hpp, one per stage.
// MI355X only; no CPU scan path exists in this library: if HIP fails the call fails.
#include "filter_launch.hpp"

// persistent band table of the context: empty between scans (the verification gives every slot back), so a scan pays
// for the bands it has, not for a memset of the table
int ensure_band_table(spm_ctx *ctx, uint64_t slots)
{
    if (ctx->band_slots >= slots && !ctx->band_dirty)
        return SPM_OK;
    if (ctx->band_slots < slots) {
        const auto t0 = clk::now();
        if (ctx->d_band_tab) {
            SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            hipFree(ctx->d_band_tab);
            ctx->d_band_tab = nullptr;
            ctx->band_slots = 0;
        }
        SPM_HIP_CHECK(ctx, hipMalloc(&ctx->d_band_tab, slots * sizeof(ulonglong2)));
        ctx->band_slots = slots;
        if (spm_trace_on())
            fprintf(stderr, "[spm_hip] band table grows to %.1f MiB: %.2f ms\n", slots * sizeof(ulonglong2) / 1048576.0, ms_since(t0));
    }
    SPM_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_band_tab, 0xFF, ctx->band_slots * sizeof(ulonglong2), ctx->stream)); // all free
    SPM_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_table_poison, 0, 4, ctx->stream)); // (and known to be)
    ctx->band_dirty = false;
    return SPM_OK;
}

namespace
{
struct filter_run // one run_filter: the request, its sizes, the scratch buffer laid out for them, and the launches in order
{
    const scan_args &A;
    const retry_state &retry;
    spm_ctx *ctx;
    const spm_patterns *ps;
    spm_hits *H;
    filter_sizes Z;
    survivor *surv = nullptr;
    unsigned long long *seen = nullptr;
    band_rec *bands = nullptr;
    uint64_t *ovf = nullptr;
    const uint64_t *d_seg = nullptr; // the segment table on the device
    uint64_t n_seg = 0;
    uint32_t seg_bits = 0;
    bool exact_hits = false, skip_seen = false;

    // scratch and band table for these sizes; which reporting path the set takes; the dedupe set cleared
    int lay_out()
    {
        SPM_TRY(ensure_scratch(ctx, Z.surv_bytes + Z.seen_bytes + Z.band_bytes + Z.ovf_bytes));
        // Exact sets whose needles are their own single seed (k = 0, no `N`, e.g. Shift-Or / Horspool sets): the whole-seed check
        // of the resolve kernel is the whole comparison, so it reports the hits itself -- no band table, no verification launch.
        // (Not for needles that are repeats: their merged index entries skip the per-offset check.)
        exact_hits = ps->max_k == 0 && !Z.overlap && ps->filter_max_range == 0 && ps->d_ranks;
        if (exact_hits && ps->exact_whole < 0) {
            bool whole = true;
            for (uint32_t p = 0; p < ps->n && whole; ++p)
                whole = ps->seed_n[p] == 1 && ps->seed_q[p] == (uint32_t)ps->m[p];
            ps->exact_whole = whole ? 1 : 0;
        }
        exact_hits = exact_hits && ps->exact_whole == 1;
        if (!exact_hits)
            SPM_TRY(ensure_band_table(ctx, Z.band_slots));
        surv = (survivor *)ctx->d_scratch;
        seen = (unsigned long long *)((uint8_t *)surv + Z.surv_bytes);
        bands = (band_rec *)((uint8_t *)seen + Z.seen_bytes);
        ovf = (uint64_t *)((uint8_t *)bands + Z.band_bytes);
        // Exact sets whose hits come from the resolve kernel report every occurrence once by construction (one sampled window,
        // one entry): no dedupe set, no 4 MiB memset in front of a 0.2 ms scan -- unless a span gives up (the brute-force
        // re-scan of that span would report its hits a second time): then the scan runs again with the set.
        skip_seen = exact_hits && !retry.need_seen;
        if (!skip_seen)
            SPM_HIP_CHECK(ctx, hipMemsetAsync(seen, 0xFF, Z.seen_bytes, ctx->stream));
        if (!exact_hits)
            ctx->band_dirty = true; // until the verification has consumed every band of this scan
        return SPM_OK;
    }

    // the streaming pass(es): one launch per pass of the seed index
    int launch_passes()
    {
        filter_params P{};
        P.text = A.text->d;
        P.text_alloc = A.text->owned ? A.text->alloc : A.text->n;
        // windows that can belong to an occurrence whose last symbol is owned
        const uint64_t reach = ps->max_window;
        P.lo = A.begin >= A.ctx_begin + reach ? A.begin - reach : A.ctx_begin;
        P.hi = A.end;
        P.surv = surv;
        P.counters = H->d_count;
        P.surv_cap = Z.surv_cap;
        P.ovf_spans = ovf;
        P.ovf_cap = kOvfCap;
        for (size_t fi = 0; fi < ps->fidx.size(); ++fi) {
            if (fi > 0) // each pass draws its spans from a fresh head
                SPM_HIP_CHECK(ctx, hipMemsetAsync(H->d_count + kCntSpanHead, 0, sizeof(unsigned long long), ctx->stream));
            SPM_TRY(launch_stream_pass(A, P, (uint32_t)fi)); // (the pass's tables, geometry and span plan: filter_stream.hip)
            SPM_HIP_CHECK(ctx, hipGetLastError());
            H->stats.main_launches++;
        }
        return SPM_OK;
    }

    // what resolve_params and verify_params share: text, ranges, segments, band table, hit buffer, dedupe set
    template <typename Params>
    void fill_shared(Params &X) const
    {
        X.text = A.text->d;
        X.text_alloc = A.text->owned ? A.text->alloc : A.text->n;
        X.scan_begin = A.begin;
        X.scan_end = A.end;
        X.pos_offset = A.opts.pos_offset;
        X.counters = H->d_count;
        X.bands = bands;
        X.band_cap = Z.band_cap;
        X.band_tab = ctx->d_band_tab;
        X.table_mask = (uint32_t)(Z.band_slots - 1);
        X.band_bits = 43 - seg_bits;
        X.Bw = Z.Bw;
        X.overlap = Z.overlap ? 1u : 0u;
        X.max_m = ps->max_m;
        X.m = ps->d_m;
        X.k = ps->d_k;
        X.report_begin = ps->is_myers() ? 0 : 1;
        X.seen_mask = (uint32_t)(Z.seen_slots - 1);
        X.hits = H->d_hits;
        X.hit_counter = H->d_count + kCntHits;
        X.overflow = H->d_count + kCntVoid;
        X.hit_cap = H->cap;
        X.seg_offsets = d_seg;
        X.n_segments = n_seg;
        X.seg_owned = A.d_seg_owned;
    }

    // ---- resolve: survivors -> needles -> whole-seed check -> diagonal bands (one launch for all passes) ----
    int launch_resolve()
    {
        // segmented scans: the table on the device (a host table is uploaded; the result owns the copy)
        if (A.d_seg_offsets) {
            d_seg = A.d_seg_offsets;
            n_seg = A.n_segments;
        } else if (A.seg_offsets) {
            uint64_t *d = nullptr;
            SPM_HIP_CHECK(ctx, hipMalloc(&d, (A.n_segments + 1) * sizeof(uint64_t)));
            hipFree(H->d_aux[1]);
            H->d_aux[1] = d;
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(d, A.seg_offsets, (A.n_segments + 1) * sizeof(uint64_t),
                                              hipMemcpyHostToDevice, ctx->stream));
            d_seg = d;
            n_seg = A.n_segments;
        }
        while (n_seg && (1ull << seg_bits) < n_seg + 1)
            ++seg_bits;
        resolve_params R{};
        fill_shared(R);
        R.surv = surv;
        R.surv_cap = Z.surv_cap;
        R.passes = ps->d_pass_tab;
        R.entries = ps->d_entries;
        R.key_len = ps->filter_key_len;
        R.needle_ranks = ps->d_ranks;
        R.needle_offsets = ps->d_offsets;
        R.seed_q = ps->d_seed_q;
        R.flank_check = (ps->sigma == 4 && !Z.overlap && R.needle_ranks) ? 1u : 0u;
        R.pieces_check = R.flank_check;
        R.hay_begin = A.ctx_begin;
        R.hay_end = A.end;
        R.needle_pk = ps->d_needle_pk;
        R.pk_offsets = ps->d_pk_offsets;
        R.exact_hits = exact_hits ? 1u : 0u;
        R.seen = skip_seen ? nullptr : seen;
        R.table_poison = ctx->d_table_poison;
        // grid: what earlier scans of this needle set produced (a full grid of idle workgroups costs ~30 us on a 2.6 ms scan);
        // a scan that produces more simply loops
        const uint64_t surv_expect = ps->cand_hint ? 2 * ps->cand_hint : Z.surv_cap;
        ::launch_resolve(R, surv_expect, (uint32_t)ctx->n_cu, ctx->stream);
        SPM_HIP_CHECK(ctx, hipGetLastError());
        return SPM_OK;
    }

    // ---- verification: one band = one verification.  `runs`: heads of runs of adjacent bands first (band_runs_kernel) ----
    int launch_bands(bool runs)
    {
        verify_params V{};
        fill_shared(V);
        V.ctx_begin = A.ctx_begin;
        V.surplus = ps->d_surplus;
        V.peq32 = ps->d_peq_verify ? ps->d_peq_verify : ps->d_peq;
        V.sigma = ps->sigma;
        V.nw_table = ps->NW;
        V.max_k = ps->max_k;
        V.max_span = Z.max_span;
        V.seen = seen;
        V.band_counter = kCntBandSlots;
        band_rec *kept = bands + Z.band_cap; // the second half of the band list: the bands a pre-pass keeps
        const uint32_t n_cu = (uint32_t)ctx->n_cu;
        if (runs) {
            launch_band_runs(V, bands, kept, H->d_count + kCntRunHeads, n_cu, ctx->stream);
            SPM_HIP_CHECK(ctx, hipGetLastError());
            V.runs = 1;
            V.bands = kept;
            V.band_counter = kCntRunHeads;
        }
        if (Z.overlap) {
            launch_band_select(V, kept, H->d_count + kCntBandsSelected, n_cu, ctx->stream);
            SPM_HIP_CHECK(ctx, hipGetLastError());
            V.bands = kept;
            V.band_counter = kCntBandsSelected;
            V.preselected = 1;
        }
        if (exact_hits) {
            // (the resolve kernel reported the hits)
        } else if (Z.use_wave) {
            launch_verify_wave(Z.nwn, V, ps->d_peq_bot, ps->max_m, n_cu, ctx->stream);
        } else {
            const uint32_t nwn = Z.nwn > 8 ? ps->NW : Z.nwn; // power of two beyond 8 words
            const uint64_t band_expect = ps->band_hint ? 2 * ps->band_hint : Z.band_cap;
            launch_verify(nwn, V, band_expect, n_cu, ctx->stream);
        }
        SPM_HIP_CHECK(ctx, hipGetLastError());
        if (runs) {
            launch_band_release(V, bands, n_cu, ctx->stream);
            SPM_HIP_CHECK(ctx, hipGetLastError());
        }
        return SPM_OK;
    }
};

} // namespace

int run_filter(const scan_args &A, const retry_state &R, filter_result &out)
{
    spm_ctx *ctx = A.ctx;
    spm_hits *H = A.hits;
    filter_run F{A, R, ctx, A.ps, H, size_filter(*A.ps, A.tune, A.end - A.begin, (uint64_t)ctx->n_cu, H->cap, R)};
    const filter_sizes &Z = F.Z;
    SPM_TRY(F.lay_out());
    // runs of adjacent bands (filter_verify.hpp, band_runs_kernel): when earlier scans of this set left a long band list -- a
    // repeat-rich text --, sets without surplus seeds, lane-per-band verification
    const bool runs = !Z.overlap && !F.exact_hits && !Z.use_wave && Z.Bw <= 32 && !R.need_seen && A.tune.verify_runs != 0 &&
                      A.ps->band_hint >= (uint64_t)std::max(0, A.tune.verify_runs_min_bands);
    // (heads of runs report most end positions without asking the dedupe set: if a span gives up, the brute-force re-scan
    // could report them again -- the scan then runs once more without runs, as for exact sets without the set)
    out = {F.seen, (uint32_t)(Z.seen_slots - 1), F.ovf, F.skip_seen || runs, Z.surv_cap, Z.band_cap};
    SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[1], ctx->stream));
    SPM_TRY(F.launch_passes());
    SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[2], ctx->stream));
    SPM_TRY(F.launch_resolve());
    SPM_TRY(F.launch_bands(runs));
    SPM_HIP_CHECK(ctx, hipEventRecord(H->ev[3], ctx->stream));
    return SPM_OK;
}
