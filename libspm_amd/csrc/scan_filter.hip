// scan_filter.hip -- the seed-filter engine (filter.hpp): buffer sizing and the launches of one scan.
// MI355X only; no CPU scan path exists in this library: if HIP fails the call fails.
#include "internal.hpp"
#include "filter.hpp"

namespace
{
// raise the kernel's dynamic LDS limit to what this launch asks for, then launch it
template <typename K, typename... Args>
void launch(K kernel, dim3 grid, uint32_t threads, size_t lds, hipStream_t s, Args... args)
{
    hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, args...);
}

using filter_kernel = void (*)(filter_params);
using packed_kernel = void (*)(filter_params, const uint4 *);

// The streaming kernel of each pass the index build (index_tables.hpp build_one_index, index_dense.hpp build_dense_index) can
// produce; nullptr for any other combination.
// Sparse passes on the 1-byte text, seed_filter_kernel<S, U, HV, SIG, KM>: U 1-KiB chunks per group (8 from stride 4 on,
// 2 at strides 1 and 2); KM = keys shorter than 16 symbols, which only strides 1 and 2 carry.
//   dna4, fingerprint table (HV 2): strides 4..16 (strides 1 and 2 use presence bits, unless anchored);
//   dna4, Bloom cascade (HV 1): every stride -- SPM_HIP_FILTER_HASH=1, or a fingerprint table that could not be built;
//   dna5 / dna15: fingerprint table only, every stride.
template <int S, int U, bool KM>
filter_kernel sparse_kernel(uint32_t hv, uint32_t sigma)
{
    if (hv == 2 && sigma == 5)
        return seed_filter_kernel<S, U, 2, 5, KM>;
    if (hv == 2 && sigma == 15)
        return seed_filter_kernel<S, U, 2, 15, KM>;
    if (hv == 1 && sigma == 4)
        return seed_filter_kernel<S, U, 1, 4, KM>;
    if constexpr (S >= 4)
        if (hv == 2 && sigma == 4)
            return seed_filter_kernel<S, U, 2, 4, KM>;
    return nullptr;
}

filter_kernel select_filter_kernel(const filter_index &F, uint32_t sigma, bool km)
{
    if (F.dense) { // the dense pass: anchors = a union of n_pat dimer patterns
        switch (F.n_pat) {
        case 0:
        case 1: return seed_filter_dense_kernel<4, 1>;
        case 2: return seed_filter_dense_kernel<4, 2>;
        case 3: return seed_filter_dense_kernel<4, 3>;
        default: return nullptr;
        }
    }
    if (F.hash_variant == 4) { // presence bits + L2 buckets as level 1 of a sparse dna4 pass
        if (F.stride == 1)
            return km ? seed_filter_dense_kernel<4, 1, 1, true> : seed_filter_dense_kernel<4, 1, 1, false>;
        if (F.stride == 2)
            return km ? seed_filter_dense_kernel<4, 1, 2, true> : seed_filter_dense_kernel<4, 1, 2, false>;
        return nullptr;
    }
    switch (F.stride) {
    case 16: return km ? nullptr : sparse_kernel<16, 8, false>(F.hash_variant, sigma);
    case 8: return km ? nullptr : sparse_kernel<8, 8, false>(F.hash_variant, sigma);
    case 4: return km ? nullptr : sparse_kernel<4, 8, false>(F.hash_variant, sigma);
    case 2: return km ? sparse_kernel<2, 2, true>(F.hash_variant, sigma) : sparse_kernel<2, 2, false>(F.hash_variant, sigma);
    case 1:
        // anchored pass: few windows per lane are looked up, so a lane can hold more text
        if (F.anchor_cm != 0 && F.hash_variant == 2 && sigma == 4 && !km)
            return seed_filter_kernel<1, 4, 2, 4, false, true>;
        return km ? sparse_kernel<1, 2, true>(F.hash_variant, sigma) : sparse_kernel<1, 2, false>(F.hash_variant, sigma);
    default: return nullptr;
    }
}

// sparse dna4 passes with the fingerprint table over the 2-bit shadow, seed_filter_packed_kernel<S, U2, 2, false>: strides
// 4..16 (stride 1 has 16 windows per word, and 4 words already fill the 32-bit survivor mask twice over; stride 2 uses
// presence bits)
packed_kernel select_packed_kernel(uint32_t stride, bool km)
{
    if (km)
        return nullptr;
    switch (stride) {
    case 16: return seed_filter_packed_kernel<16, 4, 2, false>;
    case 8: return seed_filter_packed_kernel<8, 4, 2, false>;
    case 4: return seed_filter_packed_kernel<4, 2, 2, false>;
    default: return nullptr;
    }
}

template <int NWN>
void launch_verify_nw(const verify_params &V, dim3 grid, hipStream_t s)
{
    // LDS holds (sigma+1)*NWN words per thread; keep the block within ~128 KiB
    uint32_t threads = 256;
    const size_t per_thread = (size_t)(V.sigma + 1) * NWN * 4 + 2 * 16; // match masks + the hits of one 16-symbol block
    while (threads > 64 && per_thread * threads > 128 * 1024)
        threads >>= 1;
    const size_t lds = per_thread * threads + (size_t)(threads / 64) * kHitStage * sizeof(spm_hit);
    launch(verify_kernel<NWN>, grid, threads, lds, s, V);
}

template <int G>
void launch_verify_wave_g(verify_params V, const uint32_t *peq_bot, uint32_t max_m, dim3 grid, hipStream_t s)
{
    // One wave per workgroup: a scan leaves a few thousand long bands, i.e. far fewer busy waves than the GPU has SIMDs,
    // and each is a serial chain ~1500 steps long.  With four-wave workgroups filled in order, the dispatcher packed the
    // busy waves four to a SIMD on a third of the CUs and left the rest idle.
    grid.x *= 4;
    const uint32_t n_slots = 2 * V.max_k + 1 + V.max_span;
    // text window of one candidate: cold start |P| + k symbols before the first end position, then the end positions
    V.wave_text = ((max_m + V.max_k + n_slots + 16 + 15) & ~15u) + 16;
    const size_t per_group = ((n_slots * 2 + 15) & ~15u) + V.wave_text;
    launch(verify_wave_kernel<G, 1>, grid, 64, (64 / G) * per_group, s, V, peq_bot);
}

// long needles: one 32-row block per lane, G = lanes per band >= blocks of the longest needle
void launch_verify_wave(uint32_t n_blocks, const verify_params &V, const uint32_t *peq_bot, uint32_t max_m, dim3 grid,
                        hipStream_t s)
{
    if (n_blocks <= 8)
        launch_verify_wave_g<8>(V, peq_bot, max_m, grid, s);
    else if (n_blocks <= 16)
        launch_verify_wave_g<16>(V, peq_bot, max_m, grid, s);
    else if (n_blocks <= 32)
        launch_verify_wave_g<32>(V, peq_bot, max_m, grid, s);
    else
        launch_verify_wave_g<64>(V, peq_bot, max_m, grid, s);
}

// nwn = 32-bit words that can hold needle rows = ceil(max |P| / 32), rounded up to an instantiated width
void launch_verify(uint32_t nwn, const verify_params &V, dim3 grid, hipStream_t s)
{
    switch (nwn) {
    case 1: launch_verify_nw<1>(V, grid, s); break;
    case 2: launch_verify_nw<2>(V, grid, s); break;
    case 3: launch_verify_nw<3>(V, grid, s); break;
    case 4: launch_verify_nw<4>(V, grid, s); break;
    case 5: launch_verify_nw<5>(V, grid, s); break;
    case 6: launch_verify_nw<6>(V, grid, s); break;
    case 7: launch_verify_nw<7>(V, grid, s); break;
    case 8: launch_verify_nw<8>(V, grid, s); break;
    case 16: launch_verify_nw<16>(V, grid, s); break;
    case 32: launch_verify_nw<32>(V, grid, s); break;
    default: launch_verify_nw<64>(V, grid, s); break;
    }
}

} // namespace

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
static_assert(sizeof(survivor) == kSurvivorBytes && sizeof(band_rec) == kBandRecBytes, "scan_plan.hpp sizes the lists");

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
            const filter_index &F = ps->fidx[fi];
            P.stride = F.stride;
            P.key_len = F.key_len;
            P.key_mask = F.key_len >= 16 ? 0xFFFFFFFFu : ((1u << (2 * F.key_len)) - 1);
            P.bitmap_words = F.hash_variant == 2 ? 1024 : F.bitmap_words;
            P.lds_words = F.lds_words;
            P.chd_slot_mask = F.chd_slot_mask;
            P.chd_bucket_shift = F.chd_bucket_shift;
            P.chd_disp_off = F.chd_disp_off;
            P.n_probes = F.n_probes;
            P.bitmap = F.d_bitmap;
            P.pass = (uint32_t)fi;
            P.anchor_c = F.anchor_c;
            P.anchor_cm = F.anchor_cm;
            P.n_pat = F.n_pat;
            for (uint32_t i = 0; i < kDensePatterns; ++i) {
                P.pat_c[i] = F.pat_c[i];
                P.pat_cm[i] = F.pat_cm[i];
            }
            P.bucket_shift = F.bucket_shift;
            P.buckets = reinterpret_cast<const uint4 *>(F.d_buckets);
            if (fi > 0) // each pass draws its spans from a fresh head
                SPM_HIP_CHECK(ctx, hipMemsetAsync(H->d_count + kCntSpanHead, 0, sizeof(unsigned long long), ctx->stream));
            const bool km = F.key_len < 16; // (masked keys)
            const bool bits = F.hash_variant == 4; // presence bits + L2 buckets as level 1 of a sparse pass: the dense kernel's machinery
            const bool use_packed = F.hash_variant == 2 && A.text->d_packed && ps->sigma == 4 && F.stride >= 2 &&
                                    !(A.opts.flags & SPM_SCAN_IGNORE_PACKED);
            // measured best: 8 waves per CU on the 1-byte text when HBM binds, 16 on the 2-bit shadow and at stride 1 with
            // 16-symbol keys (LDS-bound: C4 25.8 vs 29.1 ms; the other stride-1/2 variants need more than 128 VGPRs)
            // stride 2: two chunks per group (16 windows per lane) need < 128 VGPRs, so 16 waves per CU hide the LDS round trips
            // (C5: 0.53 -> 0.46 ms; four chunks per group hold 167 VGPRs at 8 waves)
            const bool wide_ok = use_packed || F.stride == 2 || (F.stride == 1 && !km && ps->sigma == 4);
            const uint32_t threads = (F.dense || bits || wide_ok) ? 1024 : 512;
            // + the workgroup's span-dequeue slot (4 words) + one survivor-chunk record per wave (+ dense: one queue per wave)
            const size_t lds = (size_t)F.lds_words * 4 + 16 + 16 * kCandRec * 4 + ((F.dense || bits) ? 16 * sizeof(dense_queue) : 0);
            const uint32_t wg_per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>((160 * 1024) / lds, 2048 / threads));
            const uint32_t grid = ctx->n_cu * wg_per_cu;
            const uint64_t n_waves = (uint64_t)grid * (threads / 64);
            const span_plan span = plan_span(stream_geometry_of(P.lo, P.hi, 1024).n_chunks, n_waves, 1024);
            P.span_chunks = span.span_chunks;
            P.span_unit = 1024;
            // candidates a span may produce before it gives up and is re-scanned by the brute-force kernel: one per 4 symbols
            // costs the verification about what the re-scan would
            const int sb = A.tune.span_budget;
            P.span_budget = sb > 0 ? (uint32_t)sb : (uint32_t)std::max<uint64_t>(256, (uint64_t)span.span_chunks * 1024 / 4);
            P.dynamic = span.dynamic;
            P.hash_variant = F.hash_variant;
            H->stats.span_symbols = P.span_chunks * P.span_unit;
            if (use_packed) {
                // p-chunks of 4096 symbols: recompute the span geometry in those units
                filter_params Q = P;
                const span_plan pspan = plan_span(stream_geometry_of(Q.lo, Q.hi, 4096).n_chunks, n_waves, 4096);
                Q.span_chunks = pspan.span_chunks;
                Q.span_unit = 4096;
                if (sb <= 0)
                    Q.span_budget = (uint32_t)std::max<uint64_t>(256, (uint64_t)pspan.span_chunks * 4096 / 4);
                Q.dynamic = pspan.dynamic;
                H->stats.span_symbols = Q.span_chunks * Q.span_unit;
                const packed_kernel k = select_packed_kernel(F.stride, km);
                if (!k) {
                    SPM_SET_ERR(ctx, "internal: no packed filter kernel for stride %u, key length %u", F.stride, F.key_len);
                    return SPM_E_UNSUPPORTED;
                }
                launch(k, dim3(grid), threads, lds, ctx->stream, Q, reinterpret_cast<const uint4 *>(A.text->d_packed));
            } else {
                const filter_kernel k = select_filter_kernel(F, ps->sigma, km);
                if (!k) {
                    SPM_SET_ERR(ctx, "internal: no filter kernel for stride %u, key length %u, sigma %u, hash variant %u, %u patterns",
                                F.stride, F.key_len, ps->sigma, F.hash_variant, F.n_pat);
                    return SPM_E_UNSUPPORTED;
                }
                launch(k, dim3(grid), threads, lds, ctx->stream, P);
            }
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
        // (5 workgroups per CU are resident at once -- LDS queues, 84 VGPRs --: a larger grid only adds a second, partly filled
        // round.  A lane takes ~4 survivors in turn: measured on C5, whose survivors are few and cheap, 0.137 -> 0.10 ms;
        // c3r 1.33 -> 1.25 ms with the cap alone.)
        const uint64_t rmax = (uint64_t)ctx->n_cu * 5;
        // (a short survivor list: one survivor per lane, its latency is the kernel's; a long one: four per lane)
        const uint64_t per_wg = (surv_expect + 255) / 256 <= rmax ? 256 : 1024;
        const uint32_t rgrid = (uint32_t)std::min<uint64_t>(rmax, std::max<uint64_t>(ctx->n_cu / 2, (surv_expect + per_wg - 1) / per_wg));
        hipLaunchKernelGGL(resolve_kernel, dim3(rgrid), dim3(256), 0, ctx->stream, R);
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
        if (runs) {
            hipLaunchKernelGGL(band_runs_kernel, dim3(ctx->n_cu * 8), dim3(256), 0, ctx->stream, V, bands, kept, H->d_count + kCntRunHeads);
            SPM_HIP_CHECK(ctx, hipGetLastError());
            V.runs = 1;
            V.bands = kept;
            V.band_counter = kCntRunHeads;
        }
        if (Z.overlap) {
            hipLaunchKernelGGL(band_select_kernel, dim3(ctx->n_cu * 2), dim3(256), 0, ctx->stream, V, kept, H->d_count + kCntBandsSelected);
            SPM_HIP_CHECK(ctx, hipGetLastError());
            V.bands = kept;
            V.band_counter = kCntBandsSelected;
            V.preselected = 1;
        }
        if (exact_hits) {
            // (the resolve kernel reported the hits)
        } else if (Z.use_wave) {
            // one verification is a ~1400-step serial chain: enough waves that every band gets its own right away
            launch_verify_wave(Z.nwn, V, ps->d_peq_bot, ps->max_m, dim3(ctx->n_cu * 16), ctx->stream);
        } else {
            const uint32_t nwn = Z.nwn > 8 ? ps->NW : Z.nwn; // power of two beyond 8 words
            const uint64_t band_expect = ps->band_hint ? 2 * ps->band_hint : Z.band_cap;
            const uint32_t vgrid = (uint32_t)std::min<uint64_t>((uint64_t)ctx->n_cu * 4, std::max<uint64_t>(ctx->n_cu / 2, (band_expect + 255) / 256));
            launch_verify(nwn, V, dim3(vgrid), ctx->stream);
        }
        SPM_HIP_CHECK(ctx, hipGetLastError());
        if (runs) {
            hipLaunchKernelGGL(band_release_kernel, dim3(ctx->n_cu * 8), dim3(256), 0, ctx->stream, V, bands, (uint32_t)kCntBandSlots);
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
    // runs of adjacent bands (filter.hpp, band_runs_kernel): when earlier scans of this set left a long band list -- a
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


void spm_warm_filter_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)resolve_kernel);
}
