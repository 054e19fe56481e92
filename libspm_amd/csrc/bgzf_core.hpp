// bgzf_core.hpp -- BGZF framing with stored deflate blocks, the part a host compiler takes too: the geometry of the container,
// the bytes around a block's data, CRC-32 as arithmetic over GF(2)[x] mod P, and the serial framer.  The kernel of bgzf.hpp and
// spm_hip_bgzf_frame_host call the same functions.  Contract in spm_hip.h, scheme in DESIGN.md 4.12.
//
// A block of d data bytes is d + 31 bytes: 18 header bytes (gzip member with the BC extra field, BSIZE = d + 30), 5 bytes of
// one stored deflate block (01, LEN = d, NLEN = ~d), the data, CRC32 and ISIZE = d.  Blocks 0 .. nb - 2 hold D bytes, the last
// the rest; no data, no block.  The byte at uncompressed offset u lies at (u / D) * (D + 31) + 23 + u % D.
//
// CRC-32 (reflected, P = 0xEDB88320): bit 31 of a register is x^0, bit 0 is x^31.  With R the pure remainder (initial value 0,
// no final xor):  R(A || B) = R(A) * x^(8|B|) mod P  xor  R(B);  leading zero bytes leave R alone;
// crc32(M) = R(M) xor (0xFFFFFFFF * x^(8|M|) mod P) xor 0xFFFFFFFF, which is R started from 0xFFFFFFFF, complemented.
#pragma once

#include <cstdint>

#include "hd.hpp"

namespace spm_hip
{

constexpr uint32_t kBgzfBlockData = 0xff00u; // htslib's block size: the most a block may hold
constexpr uint32_t kBgzfHead = 23, kBgzfTail = 8, kBgzfFrame = kBgzfHead + kBgzfTail, kBgzfEof = 28;
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint64_t kBgzfMaxBlocks = 0x7FFFFFFEull; // what the frame kernel's grid takes: one workgroup per block and one for EOF

// ---- geometry: n data bytes in blocks of D ----
SPM_HD inline uint32_t bgzf_block_data(uint32_t opt) { return opt ? opt : kBgzfBlockData; } // (the option: 0 is the default)
SPM_HD inline uint64_t bgzf_n_blocks(uint64_t n, uint32_t D) { return n / D + (n % D ? 1 : 0); }
SPM_HD inline uint32_t bgzf_block_len(uint64_t n, uint32_t D, uint64_t b) // data bytes of block b < bgzf_n_blocks
{
    const uint64_t left = n - b * D;
    return left < D ? (uint32_t)left : D;
}
SPM_HD inline uint64_t bgzf_block_offset(uint32_t D, uint64_t b) { return b * ((uint64_t)D + kBgzfFrame); } // of its first header byte
SPM_HD inline uint64_t bgzf_data_offset(uint32_t D, uint64_t u) { return bgzf_block_offset(D, u / D) + kBgzfHead + u % D; }
SPM_HD inline uint64_t bgzf_framed_size(uint64_t n, uint32_t D, bool eof)
{
    return n + bgzf_n_blocks(n, D) * kBgzfFrame + (eof ? kBgzfEof : 0);
}
// n so large that the framed size does not fit 64 bits
SPM_HD inline bool bgzf_size_overflows(uint64_t n, uint32_t D)
{
    return n > ~0ull - kBgzfEof || bgzf_n_blocks(n, D) > (~0ull - kBgzfEof - n) / kBgzfFrame;
}

// ---- the bytes around the data ----
SPM_HD inline uint8_t bgzf_head_byte(uint32_t d, uint32_t i) // i < 23
{
    const uint32_t bsize = d + 30, nlen = ~d;
    switch (i) {
    case 0: return 0x1f;
    case 1: return 0x8b;
    case 2: return 0x08; // CM: deflate
    case 3: return 0x04; // FLG: FEXTRA
    case 9: return 0xff; // OS: unknown  (4 .. 7 MTIME, 8 XFL: 0)
    case 10: return 0x06; // XLEN
    case 12: return 'B';
    case 13: return 'C';
    case 14: return 0x02; // SLEN
    case 16: return (uint8_t)bsize;
    case 17: return (uint8_t)(bsize >> 8);
    case 18: return 0x01; // BFINAL = 1, BTYPE = 00: stored
    case 19: return (uint8_t)d;
    case 20: return (uint8_t)(d >> 8);
    case 21: return (uint8_t)nlen;
    case 22: return (uint8_t)(nlen >> 8);
    default: return 0;
    }
}
SPM_HD inline uint8_t bgzf_tail_byte(uint32_t d, uint32_t crc, uint32_t i) // i < 8
{
    return (uint8_t)((i < 4 ? crc : d) >> (8 * (i & 3)));
}
// the end-of-file block: an empty member with an empty static-Huffman deflate block (03 00), CRC 0, ISIZE 0
SPM_HD inline uint8_t bgzf_eof_byte(uint32_t i) // i < 28
{
    return i < 16 ? bgzf_head_byte(0, i) : i == 16 ? 0x1b : i == 18 ? 0x03 : 0;
}

// ---- CRC-32 ----
SPM_HD inline uint32_t crc_step(uint32_t r) { return (r >> 1) ^ (kCrcPoly & (0u - (r & 1u))); } // r * x mod P
SPM_HD inline uint32_t crc_byte(uint32_t r, uint8_t b) // R(M || b) from R(M)
{
    r ^= b;
    for (int i = 0; i < 8; ++i)
        r = crc_step(r);
    return r;
}
SPM_HD inline uint32_t crc_dword(uint32_t r, uint32_t w) // four bytes at once, the first in the low byte of w
{
    r ^= w;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 32; ++i)
        r = crc_step(r);
    return r;
}
SPM_HD inline uint32_t crc_mulmod(uint32_t a, uint32_t b) // a * b mod P
{
    uint32_t p = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = crc_step(b);
    }
    return p;
}
SPM_HD inline uint32_t crc_xpow_bytes(uint64_t n) // x^(8n) mod P
{
    uint32_t p = 0x80000000u, sq = 0x00800000u; // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1)
            p = crc_mulmod(p, sq);
        sq = crc_mulmod(sq, sq);
    }
    return p;
}
SPM_HD inline uint32_t crc_shift_bytes(uint32_t r, uint64_t n) { return crc_mulmod(r, crc_xpow_bytes(n)); } // R(A) -> R(A || 0^n)
SPM_HD inline uint32_t crc_combine(uint32_t ra, uint32_t rb, uint64_t len_b) { return crc_shift_bytes(ra, len_b) ^ rb; }
SPM_HD inline uint32_t crc_pure(const uint8_t *p, uint64_t n, uint32_t r = 0)
{
    for (uint64_t i = 0; i < n; ++i)
        r = crc_byte(r, p[i]);
    return r;
}
SPM_HD inline uint32_t crc32_of_pure(uint32_t r, uint64_t len) { return r ^ crc_shift_bytes(0xFFFFFFFFu, len) ^ 0xFFFFFFFFu; }
SPM_HD inline uint32_t crc32_serial(const uint8_t *p, uint64_t n) { return ~crc_pure(p, n, 0xFFFFFFFFu); }

// ---- what the frame kernel's lanes agree on: every lane of a workgroup of kBgzfLanes takes `chunk` source bytes, a multiple of
// 16 that covers the longest block from any source alignment, so that lane t's R is shifted by the same x^(8 chunk) whatever
// the block holds (the lanes in front of a short block see zero bytes).  pw[k] = x^(8 chunk 2^k): the shifts of a tree over
// 64 lanes (k < 6) and of the four waves' results (k = 6). ----
constexpr uint32_t kBgzfLanes = 256;
struct bgzf_lane_plan
{
    uint32_t chunk;
    uint32_t pw[7];
};
SPM_HD inline bgzf_lane_plan bgzf_plan_lanes(uint32_t D)
{
    bgzf_lane_plan L;
    L.chunk = (((D + 15 + kBgzfLanes - 1) / kBgzfLanes) + 15) & ~15u;
    L.pw[0] = crc_xpow_bytes(L.chunk);
    for (int k = 1; k < 7; ++k)
        L.pw[k] = crc_mulmod(L.pw[k - 1], L.pw[k - 1]);
    return L;
}
// The source bytes [lo, hi) of lane t, as offsets into the block's data (hi <= lo: none).  The block's data lies at address
// a0 (any alignment) and has d bytes.  The lanes tile [0, body) with body = the bytes in front of the last 16-byte border of
// the source: every chunk ends on such a border, the chunk that holds byte 0 starts there, the others on a border.  The
// bytes [body, d), fewer than 16, are the block's tail and belong to no lane.
SPM_HD inline uint32_t bgzf_body(uint64_t a0, uint32_t d)
{
    const uint64_t t = (a0 + d) & ~15ull;
    return t > a0 ? (uint32_t)(t - a0) : 0u;
}
SPM_HD inline void bgzf_lane_range(uint32_t body, uint32_t chunk, uint32_t t, uint32_t &lo, uint32_t &hi)
{
    const int64_t l = (int64_t)body - (int64_t)(kBgzfLanes - t) * chunk, h = l + chunk;
    lo = l > 0 ? (uint32_t)l : 0u;
    hi = h > 0 ? (uint32_t)h : 0u;
}
// The host's rendering of what the kernel computes: the lanes' remainders over their ranges, the one that holds byte 0 started
// from 0xFFFFFFFF, folded by the tree, the tail appended.  The case program holds it against crc32_serial.
inline uint32_t bgzf_crc_by_lanes(const uint8_t *p, uint64_t a0, uint32_t d, const bgzf_lane_plan &L)
{
    const uint32_t body = bgzf_body(a0, d);
    uint32_t r[kBgzfLanes];
    for (uint32_t t = 0; t < kBgzfLanes; ++t) {
        uint32_t lo, hi;
        bgzf_lane_range(body, L.chunk, t, lo, hi);
        r[t] = hi > lo ? crc_pure(p + lo, hi - lo, lo == 0 ? 0xFFFFFFFFu : 0u) : 0u;
    }
    for (uint32_t k = 0, step = 1; step < 64; ++k, step <<= 1) // the tree of every wave
        for (uint32_t t = 0; t < kBgzfLanes; t += 2 * step)
            r[t] = crc_mulmod(r[t], L.pw[k]) ^ r[t + step];
    uint32_t all = r[0];
    for (uint32_t w = 1; w < kBgzfLanes / 64; ++w) // the waves' results, in order
        all = crc_mulmod(all, L.pw[6]) ^ r[64 * w];
    return ~crc_pure(p + body, d - body, body ? all : 0xFFFFFFFFu);
}

// ---- the serial framer: n bytes of src into dst, which has room for bgzf_framed_size bytes ----
inline void bgzf_frame_serial(const uint8_t *src, uint64_t n, uint32_t D, bool eof, uint8_t *dst)
{
    const uint64_t nb = bgzf_n_blocks(n, D);
    for (uint64_t b = 0; b < nb; ++b) {
        const uint32_t d = bgzf_block_len(n, D, b);
        const uint8_t *from = src + b * D;
        uint8_t *to = dst + bgzf_block_offset(D, b);
        for (uint32_t i = 0; i < kBgzfHead; ++i)
            to[i] = bgzf_head_byte(d, i);
        uint32_t r = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < d; ++i) {
            to[kBgzfHead + i] = from[i];
            r = crc_byte(r, from[i]);
        }
        for (uint32_t i = 0; i < kBgzfTail; ++i)
            to[kBgzfHead + d + i] = bgzf_tail_byte(d, ~r, i);
    }
    if (eof)
        for (uint32_t i = 0; i < kBgzfEof; ++i)
            dst[bgzf_framed_size(n, D, false) + i] = bgzf_eof_byte(i);
}

} // namespace spm_hip
