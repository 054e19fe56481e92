// filter_stream.hip -- the streaming kernels of the seed filter's sparse passes (filter_stream.hpp): which kernel streams which
// pass, and the launch geometry of every streaming pass, the dense ones (filter_dense.hip) included.
#include "filter_launch.hpp"
#include "filter_stream.hpp"

namespace
{
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
    if (F.dense || F.hash_variant == 4)
        return select_dense_kernel(F, km);
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

} // namespace

int launch_stream_pass(const scan_args &A, filter_params P, uint32_t pass)
{
    spm_ctx *ctx = A.ctx;
    const spm_patterns *ps = A.ps;
    spm_hits *H = A.hits;
    const filter_index &F = ps->fidx[pass];
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
    P.pass = pass;
    P.anchor_c = F.anchor_c;
    P.anchor_cm = F.anchor_cm;
    P.n_pat = F.n_pat;
    for (uint32_t i = 0; i < kDensePatterns; ++i) {
        P.pat_c[i] = F.pat_c[i];
        P.pat_cm[i] = F.pat_cm[i];
    }
    P.bucket_shift = F.bucket_shift;
    P.buckets = reinterpret_cast<const uint4 *>(F.d_buckets);
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
    const size_t lds = (size_t)F.lds_words * 4 + 16 + 16 * kCandRec * 4 + ((F.dense || bits) ? 16 * kDenseQueueBytes : 0);
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
    return SPM_OK;
}

void warm_stream_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)seed_filter_kernel<16, 8, 2, 4, false>);
}
