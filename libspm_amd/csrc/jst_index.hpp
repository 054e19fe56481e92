// jst_index.hpp -- building the pan-genome index (spm_hip_jst_index; scheme in jst.hpp).  gfx950.  Unit:
// jst.hip.  What a cell owns and what its context spells is jst_walk_core.hpp's; the kernels
// here only spread those functions over the cells.  The build, stage by stage:
//   starts   a_lo, the cells' length deltas, their column-wise prefix, hap_start            (synchronises: errors surface here)
//   group    the haplotypes of every (block, haplotype group) cell grouped by context signature (jst_dedupe_kernel)
//   layout   exclusive scans of contexts and bytes per cell; the one read-back of their totals (synchronises)
//   emit     the context tables and the context buffer, one representative per group spelled out (jst_emit_kernel)
//   finish   statistics and the trace line
// Temporaries live in a dev_scratch until the call returns; everything else belongs to the tree.
#pragma once

#include <hipcub/hipcub.hpp>

#include "internal.hpp"
#include "jst_handles.hpp"
#include "wave.hpp"

namespace spm_hip
{

__global__ void jst_alo_kernel(const uint64_t *pos, uint64_t n_alleles, uint64_t L, uint64_t n_blocks, uint64_t *a_lo)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= n_blocks)
        a_lo[j] = jst_alo_row(pos, n_alleles, L, n_blocks, j);
}

__global__ void jst_widen_kernel(const uint32_t *in, uint64_t n, uint64_t *out)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n)
        out[t] = in[t];
}

// delta[j][h] = sum over the alleles of block j that h carries of (alt_len - ref_len); row n_blocks = 0
__global__ void jst_delta_kernel(jst_dev J, int64_t *delta)
{
    const uint64_t j = blockIdx.x;
    for (uint32_t h = threadIdx.x; h < J.n_hap; h += blockDim.x)
        delta[j * J.n_hap + h] = jst_cell_delta(J, j, h);
}

// column-wise exclusive scan over blocks, chunks of `chunk` rows
__global__ void jst_chunk_sum_kernel(const int64_t *delta, uint64_t n_rows, uint32_t n_hap, uint32_t chunk, int64_t *csum)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_chunks = (n_rows + chunk - 1) / chunk;
    if (t >= n_chunks * n_hap)
        return;
    const uint64_t c = t / n_hap, h = t % n_hap;
    int64_t s = 0;
    for (uint64_t j = c * chunk; j < std::min<uint64_t>(n_rows, (c + 1) * chunk); ++j)
        s += delta[j * n_hap + h];
    csum[c * n_hap + h] = s;
}

__global__ void jst_chunk_scan_kernel(int64_t *csum, uint64_t n_chunks, uint32_t n_hap)
{
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n_hap)
        return;
    int64_t run = 0;
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const int64_t t = csum[c * n_hap + h];
        csum[c * n_hap + h] = run;
        run += t;
    }
}

// delta -> exclusive prefix (in place), rows 0..n_rows inclusive (row n_rows receives the total)
__global__ void jst_chunk_apply_kernel(int64_t *delta, uint64_t n_rows, uint32_t n_hap, uint32_t chunk, const int64_t *csum)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_chunks = (n_rows + chunk - 1) / chunk;
    if (t >= n_chunks * n_hap)
        return;
    const uint64_t c = t / n_hap, h = t % n_hap;
    int64_t run = csum[c * n_hap + h];
    const uint64_t j1 = std::min<uint64_t>(n_rows, (c + 1) * chunk);
    for (uint64_t j = c * chunk; j < j1; ++j) {
        const int64_t d = delta[j * n_hap + h];
        delta[j * n_hap + h] = run;
        run += d;
    }
    if (j1 == n_rows)
        delta[n_rows * n_hap + h] = run;
}

// shift (in place) -> hap_start
__global__ void jst_start_kernel(jst_dev J)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (J.n_blocks + 1) * J.n_hap)
        return;
    J.hap_start[t] = jst_hap_start(J, t / J.n_hap, (uint32_t)(t % J.n_hap), (int64_t)J.hap_start[t]);
}

struct jst_index_out
{
    uint16_t *local_id;           // [(je - jb) * n_hap]: group id | 0x8000 for the group's representative
    uint32_t *n_uniq;             // [je - jb]
    unsigned long long *bytes;    // [je - jb]
    unsigned long long *totals;   // [0] non-empty contexts, [1] owned symbols
};

// One workgroup per block: signatures in LDS, grouped through an LDS hash table with exact comparison.
__global__ __launch_bounds__(256) void jst_dedupe_kernel(jst_dev J, jst_index_out O)
{
    extern __shared__ uint32_t lds[];
    // this workgroup: block jr of the indexed range, haplotypes [h0, h0 + H)
    const uint64_t jr = blockIdx.x / J.n_groups;
    const uint32_t h0 = (uint32_t)(blockIdx.x % J.n_groups) * kJstGroup;
    const uint32_t H = min(kJstGroup, J.n_hap - h0);
    uint32_t n_slots = 64;
    while (n_slots < 2 * H)
        n_slots <<= 1;
    uint32_t *sig = lds;                       // [H][kJstSigWords]
    uint32_t *slots = sig + H * kJstSigWords;  // [n_slots] owner haplotype
    uint32_t *uid = slots + n_slots;           // [n_slots] group id of the slot
    uint32_t *slot_of = uid + n_slots;         // [H]
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_bytes, s_ctx, s_owned;
    const uint64_t j = J.jb + jr;
    if (threadIdx.x == 0) {
        s_n = 0;
        s_bytes = 0;
        s_ctx = 0;
        s_owned = 0;
    }
    for (uint32_t s = threadIdx.x; s < n_slots; s += blockDim.x)
        slots[s] = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < H; h += blockDim.x) {
        jst_walk W;
        jst_left_walk(J, j, h0 + h, W);
        for (uint32_t w = 0; w < kJstSigWords; ++w)
            sig[h * kJstSigWords + w] = W.sig[w];
        slot_of[h] = W.empty ? 0xFFFFFFFFu : 0;
        if (!W.empty) {
            atomicAdd(&s_ctx, 1ull);
            atomicAdd(&s_owned, (unsigned long long)(W.len - W.owned_from));
        }
    }
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < H; h += blockDim.x) {
        if (slot_of[h] == 0xFFFFFFFFu)
            continue;
        uint32_t x = 0x9E3779B9u;
        for (uint32_t w = 0; w < kJstSigWords; ++w) {
            x ^= sig[h * kJstSigWords + w] + 0x7F4A7C15u + (x << 6) + (x >> 2);
            x *= 0x85EBCA6Bu;
        }
        uint32_t s = (x ^ (x >> 15)) & (n_slots - 1);
        while (true) {
            uint32_t owner = atomicCAS(&slots[s], 0xFFFFFFFFu, h);
            if (owner == 0xFFFFFFFFu)
                owner = h;
            bool same = true;
            if (owner != h)
                for (uint32_t w = 0; w < kJstSigWords; ++w)
                    same = same && sig[owner * kJstSigWords + w] == sig[h * kJstSigWords + w];
            if (same) {
                slot_of[h] = s;
                break;
            }
            s = (s + 1) & (n_slots - 1);
        }
    }
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < H; h += blockDim.x) {
        const uint32_t s = slot_of[h];
        if (s != 0xFFFFFFFFu && slots[s] == h) {
            uid[s] = atomicAdd(&s_n, 1u);
            atomicAdd(&s_bytes, (unsigned long long)sig[h * kJstSigWords + 3]);
        }
    }
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < H; h += blockDim.x) {
        const uint32_t s = slot_of[h];
        uint16_t v = kJstNone;
        if (s != 0xFFFFFFFFu)
            v = (uint16_t)(uid[s] | (slots[s] == h ? 0x8000u : 0u));
        O.local_id[jr * J.n_hap + h0 + h] = v;
    }
    if (threadIdx.x == 0) {
        O.n_uniq[blockIdx.x] = s_n;
        O.bytes[blockIdx.x] = s_bytes;
        atomicAdd(&O.totals[0], s_ctx);
        atomicAdd(&O.totals[1], s_owned);
    }
}

// One workgroup per block: the representatives' contexts are laid out in group-id order and spelled out, one wave per
// context, lanes copying each reference / alt run side by side.  Writes T.ctx_off, T.ctx_block, T.ctx_owned.
__global__ __launch_bounds__(256) void jst_emit_kernel(jst_dev J, jst_ctx_tables T, const uint64_t *byte_base, uint8_t *buffer)
{
    extern __shared__ uint32_t lds[];
    const uint64_t cb = blockIdx.x; // (block, haplotype group) cell
    const uint64_t jr = cb / J.n_groups, j = J.jb + jr;
    const uint32_t h0 = (uint32_t)(cb % J.n_groups) * kJstGroup;
    const uint32_t H = min(kJstGroup, J.n_hap - h0);
    uint32_t *rep = lds;        // [n_uniq] representative haplotype of group id
    uint32_t *len = rep + kJstGroup;    // [n_uniq]
    uint32_t *off = len + kJstGroup;    // [n_uniq] byte offset inside the cell's stretch (fits: <= H * (L + window + alts))
    const uint32_t n_uniq = (uint32_t)(T.ctx_base[cb + 1] - T.ctx_base[cb]);
    if (n_uniq == 0)
        return;
    for (uint32_t h = threadIdx.x; h < H; h += blockDim.x) {
        const uint16_t v = T.local_id[jr * J.n_hap + h0 + h];
        if (v != kJstNone && (v & 0x8000u))
            rep[v & 0x7FFFu] = h0 + h;
    }
    __syncthreads();
    for (uint32_t u = threadIdx.x; u < n_uniq; u += blockDim.x) {
        jst_walk W;
        jst_left_walk(J, j, rep[u], W);
        len[u] = W.len;
        T.ctx_block[T.ctx_base[cb] + u] = (uint32_t)cb;
        T.ctx_owned[T.ctx_base[cb] + u] = W.owned_from;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t u = 0; u < n_uniq; ++u) {
            off[u] = run;
            run += len[u];
        }
    }
    __syncthreads();
    for (uint32_t u = threadIdx.x; u < n_uniq; u += blockDim.x)
        T.ctx_off[T.ctx_base[cb] + u] = byte_base[cb] + off[u];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (uint32_t u = wave; u < n_uniq; u += n_waves) {
        const uint32_t h = rep[u];
        jst_walk W; // wave-uniform: every lane walks the same haplotype
        jst_left_walk(J, j, h, W);
        uint8_t *out = buffer + byte_base[cb] + off[u];
        jst_run_cursor C(W, h);
        const uint8_t *src = nullptr;
        for (uint64_t n = 0; C.next(J, src, n); out += n)
            for (uint64_t x = lane; x < n; x += 64)
                out[x] = src[x];
    }
}

} // namespace spm_hip

// what the stages of one spm_hip_jst_index hand on
struct jst_index_build
{
    dev_scratch tmp; // temporaries of the build, released on every return path
    uint64_t nb = 0, nc = 0;  // indexed blocks; (block, haplotype group) cells
    uint32_t *d_nuniq = nullptr;
    unsigned long long *d_bytes = nullptr, *d_totals = nullptr;
    unsigned long long totals[2] = {0, 0}; // non-empty contexts, owned symbols
    uint64_t n_ctx = 0, ctx_bytes = 0;
};

static int jst_index_starts(spm_jst *J, jst_index_build &B)
{
    using namespace spm_hip;
    spm_ctx *ctx = J->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t H = J->H;
    const uint64_t n_blocks = J->n_blocks;
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_alo, (n_blocks + 2) * 8));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_hap_start, (n_blocks + 1) * (uint64_t)H * 8));
    hipLaunchKernelGGL(jst_alo_kernel, dim3((unsigned)((n_blocks + 1 + 255) / 256)), dim3(256), 0, st, J->d_pos,
                       (uint64_t)J->al.size(), J->L, n_blocks, J->d_alo);
    const jst_dev D = J->dev();
    int64_t *delta = reinterpret_cast<int64_t *>(J->d_hap_start);
    hipLaunchKernelGGL(jst_delta_kernel, dim3((unsigned)n_blocks), dim3(std::min<uint32_t>(256, (H + 63) & ~63u)), 0, st,
                       D, delta);
    const uint32_t chunk = 256;
    const uint64_t n_chunks = (n_blocks + chunk - 1) / chunk;
    int64_t *csum = nullptr;
    SPM_HIP_CHECK(ctx, B.tmp.alloc(&csum, n_chunks * H * 8));
    const unsigned g = (unsigned)((n_chunks * H + 255) / 256);
    hipLaunchKernelGGL(jst_chunk_sum_kernel, dim3(g), dim3(256), 0, st, delta, n_blocks, H, chunk, csum);
    hipLaunchKernelGGL(jst_chunk_scan_kernel, dim3((H + 63) / 64), dim3(64), 0, st, csum, n_chunks, H);
    hipLaunchKernelGGL(jst_chunk_apply_kernel, dim3(g), dim3(256), 0, st, delta, n_blocks, H, chunk, csum);
    hipLaunchKernelGGL(jst_start_kernel, dim3((unsigned)(((n_blocks + 1) * H + 255) / 256)), dim3(256), 0, st, D);
    SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    SPM_HIP_CHECK(ctx, hipGetLastError());
    return SPM_OK;
}

// group the haplotypes of every (block, haplotype group) cell by context signature
static int jst_index_group(spm_jst *J, jst_index_build &B)
{
    using namespace spm_hip;
    spm_ctx *ctx = J->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t H = J->H;
    const uint32_t Hg = std::min<uint32_t>(H, kJstGroup); // haplotypes a workgroup compares
    const jst_dev D = J->dev();
    const uint64_t nc = B.nb * D.n_groups;
    if (nc >= (1ull << 31)) {
        SPM_SET_ERR(ctx, "spm_hip_jst_index: too many (block, haplotype group) cells");
        return SPM_E_UNSUPPORTED;
    }
    B.nc = nc;
    uint32_t n_slots = 64;
    while (n_slots < 2 * Hg)
        n_slots <<= 1;
    const size_t lds_dedupe = ((size_t)Hg * kJstSigWords + 2 * n_slots + Hg) * 4;
    const uint64_t ncx = std::max<uint64_t>(nc, 1);
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_local_id, std::max<uint64_t>(B.nb, 1) * H * 2));
    SPM_HIP_CHECK(ctx, B.tmp.alloc(&B.d_nuniq, ncx * 4));
    SPM_HIP_CHECK(ctx, B.tmp.alloc(&B.d_bytes, ncx * 8));
    SPM_HIP_CHECK(ctx, B.tmp.alloc(&B.d_totals, 16));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(B.d_totals, 0, 16, st));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_ctx_base, (nc + 1) * 8));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_byte_base, (nc + 1) * 8));
    if (nc) {
        jst_index_out O{J->d_local_id, B.d_nuniq, B.d_bytes, B.d_totals};
        hipFuncSetAttribute((const void *)jst_dedupe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dedupe);
        hipLaunchKernelGGL(jst_dedupe_kernel, dim3((unsigned)nc), dim3(256), lds_dedupe, st, D, O);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    return SPM_OK;
}

// exclusive scans: contexts and bytes per cell; their totals and the statistics of the grouping in one read-back
static int jst_index_layout(spm_jst *J, jst_index_build &B)
{
    using namespace spm_hip;
    spm_ctx *ctx = J->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t nc = B.nc;
    if (nc == 0)
        return SPM_OK;
    uint64_t *d_n64 = nullptr;
    SPM_HIP_CHECK(ctx, B.tmp.alloc(&d_n64, (nc + 1) * 8));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(d_n64, 0, (nc + 1) * 8, st));
    hipLaunchKernelGGL(jst_widen_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, B.d_nuniq, nc, d_n64);
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_n64, J->d_ctx_base, (int)(nc + 1), st);
    SPM_HIP_CHECK(ctx, B.tmp.alloc(&tmp, std::max<size_t>(tmp_bytes, 16)));
    hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d_n64, J->d_ctx_base, (int)(nc + 1), st);
    uint64_t *d_b64 = nullptr;
    SPM_HIP_CHECK(ctx, B.tmp.alloc(&d_b64, (nc + 1) * 8));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(d_b64, 0, (nc + 1) * 8, st));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_b64, B.d_bytes, nc * 8, hipMemcpyDeviceToDevice, st));
    hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d_b64, J->d_byte_base, (int)(nc + 1), st);
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(&B.n_ctx, J->d_ctx_base + nc, 8, hipMemcpyDeviceToHost, st));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(&B.ctx_bytes, J->d_byte_base + nc, 8, hipMemcpyDeviceToHost, st));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(B.totals, B.d_totals, 16, hipMemcpyDeviceToHost, st));
    SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return SPM_OK;
}

// the context tables and the context buffer
static int jst_index_emit(spm_jst *J, const jst_index_build &B)
{
    using namespace spm_hip;
    spm_ctx *ctx = J->ctx;
    const uint64_t n_ctx = B.n_ctx;
    J->n_ctx = n_ctx;
    J->ctx_bytes = B.ctx_bytes;
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_ctx_off, (n_ctx + 1) * 8));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_ctx_block, std::max<uint64_t>(n_ctx, 1) * 4));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_ctx_owned, std::max<uint64_t>(n_ctx, 1) * 4));
    SPM_TRY(text_alloc(ctx, B.ctx_bytes, J->ref->sigma, &J->ctx_text));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(J->d_ctx_off + n_ctx, &B.ctx_bytes, 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_ctx) {
        const size_t lds_emit = (size_t)kJstGroup * 3 * 4;
        hipLaunchKernelGGL(jst_emit_kernel, dim3((unsigned)B.nc), dim3(256), lds_emit, ctx->stream, J->dev(), J->ctx_tables(),
                           J->d_byte_base, J->ctx_text->d);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    return SPM_OK;
}

static void jst_index_finish(spm_jst *J, const jst_index_build &B, float ms)
{
    J->stats = spm_jst_stats{};
    J->stats.haplotype_symbols = B.totals[1];
    J->stats.context_symbols = B.ctx_bytes;
    J->stats.contexts = B.totals[0];
    J->stats.unique_contexts = B.n_ctx;
    J->stats.n_blocks = B.nb;
    J->stats.block_len = (uint32_t)J->L;
    J->stats.window = J->window;
    J->stats.ms_index = ms;
    J->indexed = true;
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst_index: window %u, %llu blocks of %u: %llu contexts, %llu unique, %llu symbols laid out "
                        "for %llu haplotype symbols; %.3f ms\n", J->window, (unsigned long long)B.nb, (unsigned)J->L,
                B.totals[0], (unsigned long long)B.n_ctx, (unsigned long long)B.ctx_bytes, B.totals[1], ms);
}

extern "C" int spm_hip_jst_index(spm_jst *J, uint32_t window, uint32_t block_len, uint64_t block_begin,
                                 uint64_t block_end)
{
    using namespace spm_hip;
    if (!J || window == 0) {
        SPM_SET_ERR(J ? J->ctx : nullptr, "spm_hip_jst_index: invalid argument");
        return SPM_E_INVALID;
    }
    spm_ctx *ctx = J->ctx;
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    J->free_index();
    const uint64_t L = block_len ? block_len : std::max<uint64_t>(256, ((uint64_t)window + 255) & ~255ull);
    const uint64_t n_blocks = std::max<uint64_t>(1, (J->ref->n + L - 1) / L);
    const uint64_t jb = std::min(block_begin, n_blocks), je = block_end ? std::min(block_end, n_blocks) : n_blocks;
    if (jb > je || (uint64_t)window + L + J->max_rlen >= (1ull << 31)) {
        SPM_SET_ERR(ctx, "spm_hip_jst_index: bad block range or window");
        return SPM_E_INVALID;
    }
    J->window = window;
    J->L = L;
    J->n_blocks = n_blocks;
    J->jb = jb;
    J->je = je;
    jst_index_build B;
    B.nb = je - jb;
    hip_events<2> ev;
    SPM_HIP_CHECK(ctx, ev.create());
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], ctx->stream));
    SPM_TRY(jst_index_starts(J, B));
    SPM_TRY(jst_index_group(J, B));
    SPM_TRY(jst_index_layout(J, B));
    SPM_TRY(jst_index_emit(J, B));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], ctx->stream));
    SPM_HIP_CHECK(ctx, hipEventSynchronize(ev[1]));
    float ms = 0;
    hipEventElapsedTime(&ms, ev[0], ev[1]);
    jst_index_finish(J, B, ms);
    return SPM_OK;
}
