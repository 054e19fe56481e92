// bgzf_deflate.hpp -- BGZF blocks deflated on the device (spm_hip_bgzf_deflate; contract in spm_hip.h, scheme in DESIGN.md
// 4.12a, the token rule and the fixed-Huffman code in bgzf_deflate_core.hpp).  gfx950.  Unit: bgzf.hip, with bgzf.hpp.
//   bgzf_deflate_kernel   one workgroup of 256 lanes per block.  (1) Far candidates: ceil(d / 256) rounds over a table of 2^14
//                         words in LDS (64 KiB: two workgroups per CU); in a round lane t looks up position 256 r + t, and behind
//                         a barrier inserts it with an LDS atomicMax, so the table is "largest position per hash" whatever the
//                         order of the lanes.  The candidate of a position goes to a scratch of 2 bytes per input byte, written
//                         coalesced, read by the lane that owns the position's chunk.  (2) Parse: every lane walks its chunk
//                         with deflate_token_at, adds up deflate_token_bits and leaves each token in the scratch slots of the
//                         positions it covers (length at i, distance - 1 at i + 1: a match covers at least three).  (3) The
//                         workgroup's prefix sum of the bits gives every lane its first bit and the block its size: fixed
//                         Huffman if smaller than stored.  (4) A fixed block's bits are built in the LDS the table left: zeroed,
//                         each lane shifts its tokens' codes through a 64-bit register and stores whole words plainly, its first
//                         and its last word with an LDS atomicOr.  The words go to the block's staging row coalesced, the CRC of
//                         the data is folded from registers by bgzf_block_crc.  A stored block leaves only its size.
//   bgzf_place_kernel     one workgroup per block behind the 64-bit exclusive sum of the sizes: a fixed block's head with BSIZE,
//                         its payload out of the staging row (dwords funnel-shifted to the destination's alignment), CRC and
//                         ISIZE; a stored block by bgzf_frame_block, straight from the source; the workgroup behind the last
//                         writes the EOF block.  No store leaves the block's own bytes.
//                         bgzf_deflate_kernel<true> (SPM_BGZF_DYNAMIC) adds the block's own Huffman code: see at the kernel.
// Every loop is bounded by the chunk, 258, d / 256, an alphabet or the 15 levels of the code build; no lane waits for another outside a barrier.  No read passes src + n.
#pragma once

#include "bgzf.hpp"
#include "bgzf_deflate_core.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum : uint32_t { kDefCntStored = 0, kDefCntMatches, kDefCntLiterals, kDefCntDynamic, kDefCnts };

// words of a block's staging row: the longest coded payload (D + 4 bytes) and one word more for the funnel shift
inline uint32_t deflate_stage_words(uint32_t D) { return (D + kDefStored - 1 + 3) / 4 + 1; }

struct bgzf_deflate_params
{
    const uint8_t *src = nullptr;
    uint64_t n = 0;
    uint64_t n_blocks = 0;
    uint32_t D = kBgzfBlockData;
    uint32_t stage_words = 0;
    bgzf_lane_plan L{};
    uint16_t *slots = nullptr;           // [n] a position's far candidate, then its token
    uint32_t *stage = nullptr;           // [n_blocks][stage_words] the payload of a coded block
    uint32_t *size = nullptr;            // [n_blocks] the block's bytes in the file
    uint32_t *crc = nullptr;             // [n_blocks] of a coded block's data
    unsigned long long *offsets = nullptr; // [n_blocks + 1] file offsets behind the scan; [n_blocks] is where the EOF block goes
    unsigned long long *counts = nullptr;  // [kDefCnts]
    uint8_t *dst = nullptr;
};

struct huff_barrier
{
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};
static_assert(sizeof(huff_work) <= (4u << kDefHashBits), "the code build works in the LDS the hash table left");

// this lane's v summed over the lanes in front of it, and over the workgroup; wave_v is free again behind the call
__device__ __forceinline__ uint32_t deflate_block_prefix(uint32_t v, uint32_t *wave_v, uint32_t &total)
{
    const uint32_t t = threadIdx.x, incl = wave_prefix_incl(v);
    __syncthreads();
    if (t % kWave == kWave - 1)
        wave_v[t / kWave] = incl;
    __syncthreads();
    uint32_t before = incl - v;
    total = 0;
    for (uint32_t w = 0; w < kBgzfLanes / kWave; ++w) {
        before += w < t / kWave ? wave_v[w] : 0;
        total += wave_v[w];
    }
    return before;
}

// Dynamic: the block also sizes its tokens in a Huffman code of its own (SPM_BGZF_DYNAMIC; bgzf_huffman_core.hpp) and takes
// the smallest of the three forms.  Behind the candidate rounds the table's LDS holds the two histograms (LDS atomics: sums do
// not depend on the lanes' order) and the work space of huff_block_build, which the workgroup runs as one; the code itself
// (huff_code, 2 KiB) has LDS of its own, because the payload's words take the table's place.  A second walk of the lane's tokens
// gives its bits in that code, a second prefix its first bit; lane 0 writes the header in front of its tokens, the last lane
// the end-of-block code behind its own.  The false instantiation is the fixed coder as it was.
template <bool Dynamic> __global__ __launch_bounds__(kBgzfLanes) void bgzf_deflate_kernel(const bgzf_deflate_params P)
{
    __shared__ uint32_t table[1u << kDefHashBits]; // the hash table, then the payload's words
    __shared__ uint32_t wave_v[kBgzfLanes / kWave];
    const uint64_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const uint32_t d = bgzf_block_len(P.n, P.D, b);
    const uint8_t *from = P.src + b * P.D;
    uint16_t *slots = P.slots + b * P.D;
    for (uint32_t i = t; i < (1u << kDefHashBits); i += kBgzfLanes)
        table[i] = 0;
    __syncthreads();
    // ---- candidates ----
    const uint32_t rounds = (d + kDefSegment - 1) / kDefSegment;
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t pos = r * kDefSegment + t;
        const bool hashed = pos + 4 <= d;
        uint32_t h = 0;
        if (hashed) {
            h = deflate_hash4(deflate_load4(from + pos));
            slots[pos] = (uint16_t)table[h];
        } else if (pos < d) {
            slots[pos] = 0;
        }
        __syncthreads();
        if (hashed)
            atomicMax(&table[h], pos + 1);
        __syncthreads(); // (the last one also hands the slots to the lanes that parse them)
    }
    [[maybe_unused]] huff_work &W = *reinterpret_cast<huff_work *>(table);
    if constexpr (Dynamic) {
        for (uint32_t i = t; i < kHufSeq; i += kBgzfLanes)
            W.count[i] = i == kHufEob;
        __syncthreads();
    }
    // ---- parse ----
    const uint32_t c = deflate_chunk(d);
    const uint32_t lo = (uint64_t)t * c < d ? t * c : d, hi = lo + c < d ? lo + c : d;
    uint32_t bits = 0, n_matches = 0, n_literals = 0;
#pragma unroll 1
    for (uint32_t i = lo; i < hi;) {
        uint32_t len, v;
        deflate_token_at(from, i, hi, slots[i], len, v);
        bits += deflate_token_bits(len, v);
        if constexpr (Dynamic) {
            uint32_t ls, ds;
            huff_count_token(len, v, ls, ds);
            atomicAdd(&W.count[ls], 1u);
            if (ds < kHufDist)
                atomicAdd(&W.count[kHufLitLen + ds], 1u);
        }
        if (len > 1) {
            slots[i] = (uint16_t)len;
            slots[i + 1] = (uint16_t)(v - 1);
            ++n_matches;
        } else {
            slots[i] = 0;
            ++n_literals;
        }
        i += len;
    }
    // ---- the lanes' first bits, the block's size ----
    const uint32_t incl = wave_prefix_incl(bits);
    if (t % kWave == kWave - 1)
        wave_v[t / kWave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kBgzfLanes / kWave; ++w) {
        before += w < t / kWave ? wave_v[w] : 0;
        total += wave_v[w];
    }
    const uint32_t fixed = deflate_fixed_bytes(total);
    uint32_t dyn = d + kDefStored, dyn_before = 0;
    [[maybe_unused]] __shared__ huff_code K;
    if constexpr (Dynamic) {
        uint32_t floor_tokens = 0; // literals + 2 matches: what huff_may_win counts
        deflate_block_prefix(n_literals + 2 * n_matches, wave_v, floor_tokens);
        const uint32_t other = fixed < d + kDefStored ? fixed : d + kDefStored;
        if (huff_may_win(floor_tokens, 0, other)) { // (the whole workgroup)
            huff_block_build(W, K, t, kBgzfLanes, huff_barrier{});
            uint32_t dyn_bits = 0;
#pragma unroll 1
            for (uint32_t i = lo; i < hi;) {
                const uint32_t len = slots[i];
                dyn_bits += len ? huff_token_bits(K, len, slots[i + 1] + 1u) : huff_token_bits(K, 1, from[i]);
                i += len ? len : 1;
            }
            uint32_t dyn_total = 0;
            dyn_before = deflate_block_prefix(dyn_bits, wave_v, dyn_total);
            dyn = huff_dynamic_bytes(K, dyn_total);
        }
    }
    const uint32_t type = deflate_choose(fixed, dyn, d);
    if (type == 0) { // (the whole workgroup)
        if (t == 0) {
            P.size[b] = d + kBgzfFrame;
            atomicAdd(&P.counts[kDefCntStored], 1ull);
        }
        return;
    }
    const bool coded_dyn = Dynamic && type == 2;
    const uint32_t payload = coded_dyn ? dyn : fixed;
    // ---- the bits, in the LDS the table left ----
    const uint32_t words = (payload + 3) / 4;
    for (uint32_t i = t; i < words; i += kBgzfLanes)
        table[i] = 0;
    __syncthreads();
    {
        const uint32_t start = coded_dyn ? kHufHeaderBits + K.header_bits + dyn_before : kDefHeaderBits + before + incl - bits;
        uint32_t w = t ? start >> 5 : 0, fill = t ? start & 31 : kDefHeaderBits;
        uint64_t acc = t ? 0 : coded_dyn ? kHufHeader : kDefHeader;
        bool first = true;
        auto put = [&](uint64_t code, uint32_t n) { // n <= 32 bits behind the lane's last
            acc |= code << fill;
            fill += n;
            if (fill >= 32) {
                if (first)
                    atomicOr(&table[w], (uint32_t)acc);
                else
                    table[w] = (uint32_t)acc;
                first = false;
                ++w;
                acc >>= 32;
                fill -= 32;
            }
        };
        if constexpr (Dynamic)
            if (coded_dyn && t == 0)
                huff_put_header(K, put);
#pragma unroll 1
        for (uint32_t i = lo; i < hi;) {
            const uint32_t len = slots[i];
            if (coded_dyn) {
                deflate_code ka, kb;
                huff_token_code(K, len ? len : 1, len ? slots[i + 1] + 1u : from[i], ka, kb);
                put(ka.bits, ka.n);
                put(kb.bits, kb.n);
            } else {
                const deflate_code k = len ? deflate_token_code(len, slots[i + 1] + 1u) : deflate_token_code(1, from[i]);
                put(k.bits, k.n);
            }
            i += len ? len : 1;
        }
        if constexpr (Dynamic)
            if (coded_dyn && t == kBgzfLanes - 1)
                put(K.ll[kHufEob] & 0xffff, K.ll[kHufEob] >> 16);
        if (acc)
            atomicOr(&table[w], (uint32_t)acc);
    }
    __syncthreads();
    uint32_t *stage = P.stage + b * P.stage_words;
    for (uint32_t i = t; i < words; i += kBgzfLanes)
        stage[i] = table[i];
    const uint32_t crc = bgzf_block_crc<false>(from, d, nullptr, P.L, wave_v);
    if (t == 0) {
        P.size[b] = payload + kDefMember;
        P.crc[b] = crc;
        if (coded_dyn)
            atomicAdd(&P.counts[kDefCntDynamic], 1ull);
    }
    wave_count_add(&P.counts[kDefCntMatches], n_matches);
    wave_count_add(&P.counts[kDefCntLiterals], n_literals);
}

// what the scan adds up: the bytes in front of the blocks, then the blocks' sizes; out[i + 1] is then block i's file offset
struct deflate_size_op
{
    const uint32_t *size;
    uint64_t n_blocks, base;
    __host__ __device__ unsigned long long operator()(uint32_t i) const { return i == 0 ? base : i <= n_blocks ? size[i - 1] : 0; }
};

__global__ __launch_bounds__(kBgzfLanes) void bgzf_place_kernel(const bgzf_deflate_params P)
{
    __shared__ uint32_t wave_r[kBgzfLanes / kWave];
    const uint64_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    if (b >= P.n_blocks) { // (the whole workgroup: no barrier is left behind)
        if (t < kBgzfEof)
            P.dst[P.offsets[P.n_blocks] + t] = bgzf_eof_byte(t);
        return;
    }
    const uint32_t d = bgzf_block_len(P.n, P.D, b), size = P.size[b];
    uint8_t *block = P.dst + P.offsets[b];
    if (size == d + kBgzfFrame) { // (stored: a fixed block is smaller)
        bgzf_frame_block(P.src + b * P.D, d, block, P.L, wave_r);
        return;
    }
    const uint32_t m = size - kDefMember;
    const uint32_t *stage = P.stage + b * P.stage_words;
    const uint8_t *stage_bytes = reinterpret_cast<const uint8_t *>(stage);
    uint8_t *to = block + 18;
    if (t < 16)
        block[t] = bgzf_head_byte(d, t);
    else if (t < 18)
        block[t] = deflate_bsize_byte(size, t - 16);
    else if (t < 18 + kBgzfTail)
        to[m + t - 18] = bgzf_tail_byte(d, P.crc[b], t - 18);
    // e: the bytes in front of the first dword border of the destination; its dword j is bytes e .. e + 3 of words j, j + 1
    uint32_t e = (0u - (uint32_t)reinterpret_cast<uint64_t>(to)) & 3u;
    e = e < m ? e : m;
    if (t < e)
        to[t] = stage_bytes[t];
    const uint32_t n_dwords = (m - e) / 4;
    uint32_t *q = reinterpret_cast<uint32_t *>(to + e);
    for (uint32_t j = t; j < n_dwords; j += kBgzfLanes)
        q[j] = __builtin_amdgcn_alignbyte(stage[j + 1], stage[j], e);
    for (uint32_t i = e + 4 * n_dwords + t; i < m; i += kBgzfLanes)
        to[i] = stage_bytes[i];
}

} // namespace spm_hip
