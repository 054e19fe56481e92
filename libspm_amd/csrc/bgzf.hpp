// bgzf.hpp -- BGZF framing of a device buffer (spm_hip_bgzf_frame; contract in spm_hip.h, scheme in DESIGN.md 4.12, geometry
// and CRC arithmetic in bgzf_core.hpp).  gfx950.  Unit: bgzf.hip.  The handle, spm_bgzf, is output_handles.hpp's.
//   bgzf_frame_kernel   one workgroup of 256 lanes per block, one pass: lane t takes bgzf_lane_range of the block's data, a
//                       contiguous chunk whose pieces are 16-byte aligned IN THE SOURCE (dwordx4 loads at any source
//                       alignment; the bytes in front of the first border go one by one, the fewer than 16 behind the last
//                       border to lane 0 at the end).  A piece is stored and folded into the lane's CRC remainder while it is
//                       in registers: the destination (+23, blocks of D + 31) is dword-aligned nowhere in particular, so a
//                       lane stores the dwords that lie inside its chunk, each funnel-shifted out of two source dwords, and
//                       the up to three bytes at either end one by one.  The remainders are table-free (32 shift-and-xor steps
//                       per dword: no LDS gather whose bank conflicts follow the data) and combine by a tree of multiplications
//                       with x^(8 chunk 2^k), which the host computes once per call.  Head, tail and the EOF block (the
//                       workgroup behind the last) are byte stores of bgzf_core.hpp's functions.  No store leaves the block's
//                       own [offset, offset + d + 31).  No atomics.  Its body is bgzf_frame_block over bgzf_block_crc<true>;
//                       bgzf_deflate.hpp uses both: a block that stays stored, and the CRC of one that does not (<false>).
#pragma once

#include <vector>

#include <hip/hip_runtime.h>

#include "bgzf_core.hpp"
#include "common.hpp"
#include "device_order.hpp"
#include "output_handles.hpp"

namespace spm_hip
{

struct bgzf_params
{
    const uint8_t *src = nullptr;
    uint8_t *dst = nullptr;
    uint64_t n = 0;        // source bytes
    uint64_t n_blocks = 0; // data blocks; workgroup n_blocks writes the EOF block
    uint32_t D = kBgzfBlockData;
    bgzf_lane_plan L{};
};

// The data of one block through the workgroup's registers: the CRC-32 of from[0, d), valid in lane 0, and, with kStore, the
// bytes at to[0, d).  wave_r: kBgzfLanes / kWave words of LDS.  All lanes call it; it holds one barrier.
template <bool kStore>
__device__ __forceinline__ uint32_t bgzf_block_crc(const uint8_t *from, uint32_t d, uint8_t *to, const bgzf_lane_plan &L, uint32_t *wave_r)
{
    const uint32_t t = threadIdx.x;
    const uint64_t a0 = reinterpret_cast<uint64_t>(from);
    const uint32_t body = bgzf_body(a0, d);
    uint32_t lo, hi;
    bgzf_lane_range(body, L.chunk, t, lo, hi);
    uint32_t r = 0;
    if (hi > lo) {
        uint32_t u = lo;
        if (lo == 0) { // the chunk that holds byte 0 starts the CRC, and starts where the source does
            r = 0xFFFFFFFFu;
            for (; u < hi && ((a0 + u) & 15); ++u) {
                const uint8_t c = from[u];
                if (kStore)
                    to[u] = c;
                r = crc_byte(r, c);
            }
        }
        if (u < hi) {
            // [u, hi) is whole 16-byte pieces of the source.  e: the bytes in front of the first dword border of the
            // destination; dword j of the destination is bytes e .. e + 3 of the source dwords j, j + 1.
            const uint32_t e = kStore ? (0u - (uint32_t)reinterpret_cast<uint64_t>(to + u)) & 3u : 0u;
            uint32_t *q = reinterpret_cast<uint32_t *>(to + u + e);
            uint4 v = *reinterpret_cast<const uint4 *>(from + u);
            if (kStore)
                for (uint32_t i = 0; i < e; ++i)
                    to[u + i] = (uint8_t)(v.x >> (8 * i));
            uint32_t prev = 0;
            bool first = true;
#pragma unroll 1
            while (true) {
                const uint32_t next_u = u + 16;
                const bool more = next_u < hi;
                uint4 nv = v;
                if (more)
                    nv = *reinterpret_cast<const uint4 *>(from + next_u); // (in flight while this piece is folded)
                if (kStore) {
                    if (!first)
                        *q++ = __builtin_amdgcn_alignbyte(v.x, prev, e);
                    q[0] = __builtin_amdgcn_alignbyte(v.y, v.x, e);
                    q[1] = __builtin_amdgcn_alignbyte(v.z, v.y, e);
                    q[2] = __builtin_amdgcn_alignbyte(v.w, v.z, e);
                    q += 3;
                }
                prev = v.w;
                first = false;
                r = crc_dword(crc_dword(crc_dword(crc_dword(r, v.x), v.y), v.z), v.w);
                if (!more)
                    break;
                v = nv;
                u = next_u;
            }
            // the last source dword has no successor in this chunk: its bytes e .. 3
            if (kStore) {
                if (e == 0)
                    *q = prev;
                else
                    for (uint32_t i = e; i < 4; ++i)
                        reinterpret_cast<uint8_t *>(q)[i - e] = (uint8_t)(prev >> (8 * i));
            }
        }
    }
    // R of the wave's 64 chunks in its lane 0, then of the four waves in lane 0 of the workgroup
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const uint32_t behind = __shfl_down(r, 1u << k);
        r = crc_mulmod(r, L.pw[k]) ^ behind;
    }
    if (t % kWave == 0)
        wave_r[t / kWave] = r;
    __syncthreads();
    uint32_t all = 0;
    if (t == 0) {
        all = wave_r[0];
        for (uint32_t w = 1; w < kBgzfLanes / kWave; ++w)
            all = crc_mulmod(all, L.pw[6]) ^ wave_r[w];
        if (!body)
            all = 0xFFFFFFFFu;
        for (uint32_t u = body; u < d; ++u) { // fewer than 16 bytes behind the last 16-byte border of the source
            const uint8_t c = from[u];
            if (kStore)
                to[u] = c;
            all = crc_byte(all, c);
        }
        all = ~all;
    }
    return all;
}

// one stored block at `block`: head, data, tail
__device__ __forceinline__ void bgzf_frame_block(const uint8_t *from, uint32_t d, uint8_t *block, const bgzf_lane_plan &L, uint32_t *wave_r)
{
    const uint32_t t = threadIdx.x;
    uint8_t *to = block + kBgzfHead;
    if (t < kBgzfHead)
        block[t] = bgzf_head_byte(d, t);
    const uint32_t crc = bgzf_block_crc<true>(from, d, to, L, wave_r);
    if (t == 0)
        for (uint32_t i = 0; i < kBgzfTail; ++i)
            to[d + i] = bgzf_tail_byte(d, crc, i);
}

__global__ __launch_bounds__(kBgzfLanes) void bgzf_frame_kernel(const bgzf_params P)
{
    __shared__ uint32_t wave_r[kBgzfLanes / kWave];
    const uint64_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    if (b >= P.n_blocks) { // (the whole workgroup: no barrier is left behind)
        if (t < kBgzfEof)
            P.dst[bgzf_framed_size(P.n, P.D, false) + t] = bgzf_eof_byte(t); // (behind the last block, which may be short)
        return;
    }
    const uint32_t d = bgzf_block_len(P.n, P.D, b);
    bgzf_frame_block(P.src + b * P.D, d, P.dst + bgzf_block_offset(P.D, b), P.L, wave_r);
}

// what spm_bgzf_opts may hold; why: the message of a refusal
inline int bgzf_check_opts(const spm_bgzf_opts &o, const char *&why)
{
    why = o.block_data > kBgzfBlockData ? "block_data above 65280"
          : (o.flags & ~SPM_BGZF_EOF)   ? "unknown flag bits"
          : o.reserved                  ? "reserved is not 0"
                                        : nullptr;
    return why ? SPM_E_INVALID : SPM_OK;
}

} // namespace spm_hip
