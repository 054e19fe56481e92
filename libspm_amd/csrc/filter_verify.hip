// filter_verify.hip -- the verification stage of the seed filter (filter_verify.hpp): the band kernels, verify_kernel at every
// instantiated width and verify_wave_kernel at every group size, each with its launch.
#include "filter_launch.hpp"
#include "filter_verify.hpp"

namespace
{
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
} // namespace

void launch_band_runs(const verify_params &V, band_rec *bands, band_rec *heads, unsigned long long *head_count, uint32_t n_cu,
                      hipStream_t s)
{
    hipLaunchKernelGGL(band_runs_kernel, dim3(n_cu * 8), dim3(256), 0, s, V, bands, heads, head_count);
}

void launch_band_select(const verify_params &V, band_rec *out, unsigned long long *out_count, uint32_t n_cu, hipStream_t s)
{
    hipLaunchKernelGGL(band_select_kernel, dim3(n_cu * 2), dim3(256), 0, s, V, out, out_count);
}

void launch_band_release(const verify_params &V, const band_rec *bands, uint32_t n_cu, hipStream_t s)
{
    hipLaunchKernelGGL(band_release_kernel, dim3(n_cu * 8), dim3(256), 0, s, V, bands, (uint32_t)kCntBandSlots);
}

void launch_verify_wave(uint32_t n_blocks, const verify_params &V, const uint32_t *peq_bot, uint32_t max_m, uint32_t n_cu,
                        hipStream_t s)
{
    // one verification is a ~1400-step serial chain: enough waves that every band gets its own right away
    const dim3 grid(n_cu * 16);
    if (n_blocks <= 8)
        launch_verify_wave_g<8>(V, peq_bot, max_m, grid, s);
    else if (n_blocks <= 16)
        launch_verify_wave_g<16>(V, peq_bot, max_m, grid, s);
    else if (n_blocks <= 32)
        launch_verify_wave_g<32>(V, peq_bot, max_m, grid, s);
    else
        launch_verify_wave_g<64>(V, peq_bot, max_m, grid, s);
}

void launch_verify(uint32_t nwn, const verify_params &V, uint64_t band_expect, uint32_t n_cu, hipStream_t s)
{
    const dim3 grid((uint32_t)std::min<uint64_t>((uint64_t)n_cu * 4, std::max<uint64_t>(n_cu / 2, (band_expect + 255) / 256)));
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

void warm_verify_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)band_release_kernel);
}
