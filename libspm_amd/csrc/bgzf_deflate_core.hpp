// bgzf_deflate_core.hpp -- BGZF blocks with real deflate, the part a host compiler takes too: the rule that turns a block's data
// into tokens, the RFC 1951 fixed-Huffman code of a token, and the serial deflater.  The kernels of bgzf_deflate.hpp and
// spm_hip_bgzf_deflate_host call the same functions, so the bytes are a pure function of the data and the opts.  Contract in
// spm_hip.h, scheme in DESIGN.md 4.12a.  The container (header, BSIZE, CRC32, ISIZE, EOF block) is bgzf_core.hpp's.
//
// A block of d data bytes is ONE deflate block with BFINAL 1: fixed Huffman (BTYPE 01) if that is strictly smaller than the
// stored form (d + 5 bytes), else the stored block of bgzf_core.hpp.  With `dynamic` (SPM_BGZF_DYNAMIC) the same tokens are also
// sized in the block's own code (BTYPE 10, bgzf_huffman_core.hpp): stored if neither coded form is below d + 5, else the smaller
// of the two, fixed when they are equal.
//
// Chunks.  Lane t of kBgzfLanes owns the positions [t c, min((t + 1) c, d)), c = deflate_chunk(d) = max(64, ceil(d / 256)).  No
// token crosses a chunk border; a match's source lies anywhere earlier in the block and may overlap its target.
// Candidates, two per position i.  Near: i - 1.  Far: the largest j with hash4(j) == hash4(i) among the positions of EARLIER
// segments (kDefSegment consecutive positions; only positions with 4 bytes in the block are hashed).  "Largest per hash" is a
// maximum, so the table does not depend on the order in which a segment's positions are inserted.
// Parse.  Greedy, left to right.  At i both candidates are extended, no further than 258, the chunk's end, or (far) a distance
// of 32768; the longer wins, the near one on a tie; a match is emitted if its length is >= 4, or >= 3 at distance 1, else the
// literal.
// Bits.  3 header bits (1, then BTYPE 01 from its low bit), the lanes' tokens in lane order, the 7-bit end-of-block code, zero
// padding.  Huffman codes go in from their most significant bit, everything else from the least.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "bgzf_core.hpp"
#include "bgzf_huffman_core.hpp" // the RFC's length and distance symbols, deflate_code, the dynamic code

namespace spm_hip
{

// ---- every constant the output depends on ----
constexpr uint32_t kDefSegment = kBgzfLanes;  // positions per candidate round
constexpr uint32_t kDefHashBits = 14;         // the table: 2^14 entries of position + 1 (0: none)
constexpr uint32_t kDefChunkFloor = 64;       // the shortest chunk of a lane
constexpr uint32_t kDefMinMatch = 4;          // shortest match at any distance
constexpr uint32_t kDefMinRun = 3;            // shortest match at distance 1
constexpr uint32_t kDefMaxMatch = 258;
constexpr uint32_t kDefMaxDist = 32768;
constexpr uint32_t kDefStored = 5;            // a stored deflate block's bytes around its data
constexpr uint32_t kDefMember = 18 + kBgzfTail; // the gzip member around a deflate payload: header with BSIZE, CRC32, ISIZE

SPM_HD inline uint32_t deflate_chunk(uint32_t d)
{
    const uint32_t c = (d + kBgzfLanes - 1) / kBgzfLanes;
    return c < kDefChunkFloor ? kDefChunkFloor : c;
}
SPM_HD inline uint32_t deflate_load4(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
SPM_HD inline uint32_t deflate_hash4(uint32_t w) { return (w * 2654435761u) >> (32 - kDefHashBits); }

// the fixed code of a literal/length symbol 0 .. 287, as RFC 1951 prints it (first bit on the left), and its length
SPM_HD inline uint32_t deflate_litlen_code(uint32_t sym, uint32_t &n)
{
    if (sym < 144) {
        n = 8;
        return 0x30 + sym;
    }
    if (sym < 256) {
        n = 9;
        return 0x190 + (sym - 144);
    }
    if (sym < 280) {
        n = 7;
        return sym - 256;
    }
    n = 8;
    return 0xC0 + (sym - 280);
}

// ---- a token: len == 1 is the literal v (a byte), len >= 3 a match of that length at distance v.  Its size in bits, and its
// bits in stream order from bit 0 (at most 31).  The dynamic coder replaces this pair (huff_token_bits, huff_token_code) and
// nothing else. ----
SPM_HD inline uint32_t deflate_token_bits(uint32_t len, uint32_t v)
{
    if (len == 1)
        return v < 144 ? 8 : 9;
    uint32_t sym, e, x, dsym, de, dx;
    deflate_len_symbol(len, sym, e, x);
    deflate_dist_symbol(v, dsym, de, dx);
    return (sym < 280 ? 7 : 8) + e + 5 + de;
}
SPM_HD inline deflate_code deflate_token_code(uint32_t len, uint32_t v)
{
    deflate_code k;
    uint32_t n = 0;
    if (len == 1) {
        const uint32_t c = deflate_litlen_code(v, n);
        k.bits = deflate_reverse(c, n);
        k.n = n;
        return k;
    }
    uint32_t sym, e, x, dsym, de, dx;
    deflate_len_symbol(len, sym, e, x);
    deflate_dist_symbol(v, dsym, de, dx);
    const uint32_t c = deflate_litlen_code(sym, n);
    k.bits = deflate_reverse(c, n) | (uint64_t)x << n;
    n += e;
    k.bits |= (uint64_t)deflate_reverse(dsym, 5) << n | (uint64_t)dx << (n + 5);
    k.n = n + 5 + de;
    return k;
}
constexpr uint32_t kDefHeaderBits = 3, kDefHeader = 3 /* BFINAL 1, BTYPE 01 */, kDefEobBits = 7 /* symbol 256: seven zeros */;

// ---- the token at position i of a chunk that ends at `end` (<= d).  far1: the far candidate's position + 1 (0: none); it is
// below i.  No byte outside p[0, end) is read. ----
SPM_HD inline void deflate_token_at(const uint8_t *p, uint32_t i, uint32_t end, uint32_t far1, uint32_t &len, uint32_t &v)
{
    uint32_t cap = end - i;
    cap = cap > kDefMaxMatch ? kDefMaxMatch : cap;
    uint32_t ln = 0, lf = 0;
    if (i >= 1)
        while (ln < cap && p[i + ln] == p[i + ln - 1])
            ++ln;
    const uint32_t j = far1 - 1;
    if (far1 && i - j <= kDefMaxDist)
        while (lf < cap && p[i + lf] == p[j + lf])
            ++lf;
    len = lf > ln ? lf : ln;
    v = lf > ln ? i - j : 1;
    if (!(len >= kDefMinMatch || (len >= kDefMinRun && v == 1))) {
        len = 1;
        v = p[i];
    }
}

// the bytes of the fixed-Huffman payload whose tokens take token_bits bits, and whether the block takes it
SPM_HD inline uint32_t deflate_fixed_bytes(uint64_t token_bits) { return (uint32_t)((kDefHeaderBits + token_bits + kDefEobBits + 7) / 8); }
SPM_HD inline bool deflate_takes_fixed(uint32_t fixed_bytes, uint32_t d) { return fixed_bytes < d + kDefStored; }
// BSIZE of a block of `size` bytes in all
SPM_HD inline uint8_t deflate_bsize_byte(uint32_t size, uint32_t i) { return (uint8_t)((size - 1) >> (8 * i)); } // i < 2

// ---- the serial rendering ----
struct deflate_token
{
    uint32_t at, len, v;
};
struct deflate_counts
{
    uint64_t n_stored_blocks = 0, n_matches = 0, n_literals = 0; // tokens of the blocks that were not stored
    uint64_t n_dynamic_blocks = 0;
};

// far candidates of every position of a block: cand[i] = position + 1 or 0
inline void deflate_candidates_serial(const uint8_t *p, uint32_t d, std::vector<uint16_t> &cand)
{
    cand.assign(d, 0);
    if (d <= kDefSegment)
        return; // (one segment: no position has an earlier one)
    std::vector<uint32_t> table(1u << kDefHashBits, 0u);
    for (uint32_t s = 0; s < d; s += kDefSegment) {
        const uint32_t e = s + kDefSegment < d ? s + kDefSegment : d;
        for (uint32_t i = s; i < e && i + 4 <= d; ++i)
            cand[i] = (uint16_t)table[deflate_hash4(deflate_load4(p + i))];
        for (uint32_t i = s; i < e && i + 4 <= d; ++i) {
            uint32_t &slot = table[deflate_hash4(deflate_load4(p + i))];
            slot = slot > i + 1 ? slot : i + 1;
        }
    }
}
// the tokens of a block, lane by lane; returns their bits
inline uint64_t deflate_parse_serial(const uint8_t *p, uint32_t d, std::vector<deflate_token> &tokens)
{
    std::vector<uint16_t> cand;
    deflate_candidates_serial(p, d, cand);
    tokens.clear();
    const uint32_t c = deflate_chunk(d);
    uint64_t bits = 0;
    for (uint32_t t = 0; t < kBgzfLanes; ++t) {
        const uint32_t lo = (uint64_t)t * c < d ? t * c : d, hi = lo + c < d ? lo + c : d;
        for (uint32_t i = lo; i < hi;) {
            deflate_token k{i, 0, 0};
            deflate_token_at(p, i, hi, cand[i], k.len, k.v);
            bits += deflate_token_bits(k.len, k.v);
            tokens.push_back(k);
            i += k.len;
        }
    }
    return bits;
}
// The step-5 choice between the three forms: which deflate block type a block of d bytes takes, given its fixed payload's bytes
// and its dynamic payload's (any value >= d + 5 where there is none).
SPM_HD inline uint32_t deflate_choose(uint32_t fixed_bytes, uint32_t dynamic_bytes, uint32_t d)
{
    if (dynamic_bytes < d + kDefStored && dynamic_bytes < fixed_bytes)
        return 2;
    return deflate_takes_fixed(fixed_bytes, d) ? 1 : 0;
}

// The deflate payload of a block of d >= 1 bytes into out, which has room for d + 5: returns its length.
inline uint32_t deflate_block_serial(const uint8_t *p, uint32_t d, uint8_t *out, deflate_counts *counts = nullptr, bool dynamic = false)
{
    std::vector<deflate_token> tokens;
    const uint32_t fixed = deflate_fixed_bytes(deflate_parse_serial(p, d, tokens));
    uint64_t n_matches = 0;
    for (const deflate_token &k : tokens)
        n_matches += k.len > 1;
    uint32_t dyn = d + kDefStored;
    huff_code K;
    const uint32_t other = fixed < d + kDefStored ? fixed : d + kDefStored;
    if (dynamic && huff_may_win(tokens.size() - n_matches, n_matches, other)) {
        std::vector<huff_work> work(1);
        huff_work &W = work[0];
        W.count[kHufEob] = 1;
        for (const deflate_token &k : tokens) {
            uint32_t ls, ds;
            huff_count_token(k.len, k.v, ls, ds);
            ++W.count[ls];
            if (ds < kHufDist)
                ++W.count[kHufLitLen + ds];
        }
        huff_block_build(W, K, 0, 1, huff_serial{});
        uint64_t bits = 0;
        for (const deflate_token &k : tokens)
            bits += huff_token_bits(K, k.len, k.v);
        dyn = huff_dynamic_bytes(K, bits);
    }
    const uint32_t type = deflate_choose(fixed, dyn, d);
    if (type == 0) {
        for (uint32_t i = 0; i < kDefStored; ++i)
            out[i] = bgzf_head_byte(d, 18 + i);
        memcpy(out + kDefStored, p, d);
        if (counts)
            ++counts->n_stored_blocks;
        return d + kDefStored;
    }
    const uint32_t m = type == 2 ? dyn : fixed;
    memset(out, 0, m);
    uint64_t at = 0;
    auto put = [&](uint64_t bits, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i, ++at)
            out[at >> 3] |= (uint8_t)(((bits >> i) & 1) << (at & 7));
    };
    if (counts) {
        counts->n_matches += n_matches;
        counts->n_literals += tokens.size() - n_matches;
        counts->n_dynamic_blocks += type == 2;
    }
    if (type == 2) {
        put(kHufHeader, kHufHeaderBits);
        huff_put_header(K, put);
        for (const deflate_token &k : tokens) {
            deflate_code a, b;
            huff_token_code(K, k.len, k.v, a, b);
            put(a.bits, a.n);
            put(b.bits, b.n);
        }
        put(K.ll[kHufEob] & 0xffff, K.ll[kHufEob] >> 16);
        return m;
    }
    put(kDefHeader, kDefHeaderBits);
    for (const deflate_token &k : tokens) {
        const deflate_code code = deflate_token_code(k.len, k.v);
        put(code.bits, code.n);
    }
    put(0, kDefEobBits);
    return m;
}

// n bytes of src into dst, which has room for bgzf_framed_size bytes: returns the file's length.  offsets (or null) receives
// the file offset of every data block and, last, the end of the data blocks.
inline uint64_t bgzf_deflate_serial(const uint8_t *src, uint64_t n, uint32_t D, bool eof, uint8_t *dst, std::vector<uint64_t> *offsets = nullptr,
                                    deflate_counts *counts = nullptr, bool dynamic = false)
{
    const uint64_t nb = bgzf_n_blocks(n, D);
    uint64_t at = 0;
    if (offsets)
        offsets->clear();
    for (uint64_t b = 0; b < nb; ++b) {
        const uint32_t d = bgzf_block_len(n, D, b);
        const uint8_t *from = src + b * D;
        uint8_t *to = dst + at;
        if (offsets)
            offsets->push_back(at);
        const uint32_t m = deflate_block_serial(from, d, to + 18, counts, dynamic), size = m + kDefMember;
        for (uint32_t i = 0; i < 16; ++i)
            to[i] = bgzf_head_byte(d, i);
        to[16] = deflate_bsize_byte(size, 0);
        to[17] = deflate_bsize_byte(size, 1);
        const uint32_t crc = crc32_serial(from, d);
        for (uint32_t i = 0; i < kBgzfTail; ++i)
            to[18 + m + i] = bgzf_tail_byte(d, crc, i);
        at += size;
    }
    if (offsets)
        offsets->push_back(at);
    if (eof)
        for (uint32_t i = 0; i < kBgzfEof; ++i)
            dst[at++] = bgzf_eof_byte(i);
    return at;
}

} // namespace spm_hip
