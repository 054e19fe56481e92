// bgzf_huffman_core.hpp -- the dynamic Huffman code of a deflate block (RFC 1951 3.2.7), the part a host compiler takes too: the
// RFC's length and distance symbols as arithmetic, optimal length-limited code lengths, canonical codes, the run-length coded
// header, and a token's size and code from the two tables.  The kernel of bgzf_deflate.hpp and the serial deflater of
// bgzf_deflate_core.hpp call the same routines, so a block's bytes are a pure function of its tokens.  Contract in spm_hip.h
// (SPM_BGZF_DYNAMIC), scheme in DESIGN.md 4.12c.
//
// Every routine that a workgroup shares takes (t, T, sync): the caller is lane t of T and `sync` is their barrier.  A stage
// reads only what an earlier stage wrote, so one lane with T = 1 and a barrier that does nothing (the host) computes the same.
//
// Code lengths: package-merge without item sets.  The n symbols with a nonzero count are the leaves, sorted by (count, symbol).
// Level 1's list is the leaves; level l's is the leaves merged with the pairwise sums ("packages") of level l - 1's list, an odd
// last item dropped; on equal weight a leaf stands in front of a package, and equal leaves and equal packages keep their order.
// The optimal code takes the first 2n - 2 items of the last level, and of every level below it the items inside the packages
// taken above: again a prefix of the list, and the leaves inside a prefix are a prefix of the leaves.  So with a_l the leaves
// among the first m items of level l and m <- 2 (m - a_l), the length of the leaf of rank r is the number of levels with
// r < a_l.  That is the tie rule: among symbols of equal count the lower-numbered one gets the longer code, never the shorter.
#pragma once

#include <cstdint>

#include "bgzf_core.hpp"

namespace spm_hip
{

SPM_HD inline uint32_t deflate_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); } // v >= 1

// ---- the RFC 1951 tables as arithmetic: the symbol of a length or distance, its extra bits and their value ----
SPM_HD inline void deflate_len_symbol(uint32_t len, uint32_t &sym, uint32_t &ebits, uint32_t &eval) // 3 .. 258
{
    const uint32_t l = len - 3;
    sym = 285, ebits = 0, eval = 0;
    if (len == 258)
        return;
    if (l < 8) {
        sym = 257 + l;
        return;
    }
    ebits = deflate_log2(l) - 2;
    sym = 261 + 4 * ebits + ((l >> ebits) & 3);
    eval = l & ((1u << ebits) - 1);
}
SPM_HD inline void deflate_dist_symbol(uint32_t dist, uint32_t &sym, uint32_t &ebits, uint32_t &eval) // 1 .. 32768
{
    const uint32_t dd = dist - 1;
    sym = dd, ebits = 0, eval = 0;
    if (dd < 4)
        return;
    ebits = deflate_log2(dd) - 1;
    sym = 2 * ebits + 2 + ((dd >> ebits) & 1);
    eval = dd & ((1u << ebits) - 1);
}
SPM_HD inline uint32_t deflate_reverse(uint32_t code, uint32_t n) // the first bit of a Huffman code goes into the stream first
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i, code >>= 1)
        r = r << 1 | (code & 1);
    return r;
}
// bits in stream order from bit 0
struct deflate_code
{
    uint64_t bits;
    uint32_t n;
};

// ---- the alphabets and the work space of one block's code ----
constexpr uint32_t kHufLitLen = 286, kHufDist = 30, kHufCl = 19;
constexpr uint32_t kHufSeq = kHufLitLen + kHufDist; // the most code lengths a header transmits
constexpr uint32_t kHufLimit = 15, kHufClLimit = 7;
constexpr uint32_t kHufEob = 256;
constexpr uint32_t kHufHeaderBits = 3, kHufHeader = 5; // BFINAL 1, BTYPE 10 from its low bit

struct huff_work // dead once the code is built
{
    uint32_t count[kHufSeq + kHufCl];            // literal/length, distance, code-length symbols
    uint8_t len[kHufSeq + kHufCl + 1];           // their code lengths
    uint16_t sym_of_rank[kHufLitLen];
    uint32_t w[kHufLitLen];                      // the leaves' weights in rank order
    uint32_t list[2][2 * kHufLitLen];            // a level's weights and those of the level below
    uint16_t leafpos[kHufLimit][kHufLitLen];     // where in its level's list a leaf stands
    uint32_t a[kHufLimit + 1];
};
struct huff_code // what the bits are written from
{
    uint32_t ll[kHufLitLen]; // the code in stream order | its length << 16
    uint32_t dd[kHufDist];
    uint32_t cl[kHufCl];
    uint16_t seq[kHufSeq];   // the coded length sequence: code-length symbol | value of its extra bits << 8
    uint32_t n_seq, hlit, hdist, hclen, header_bits;
};
struct huff_serial
{
    SPM_HD void operator()() const {}
};

// step 1: an alphabet has at least two symbols with a nonzero count (zlib's device: every code sent is complete)
SPM_HD inline void huff_pad(uint32_t *count, uint32_t n_sym)
{
    uint32_t used = 0;
    for (uint32_t i = 0; i < n_sym; ++i)
        used += count[i] != 0;
    for (uint32_t i = 0; used < 2 && i < n_sym; ++i)
        if (!count[i]) {
            count[i] = 1;
            ++used;
        }
}

// a package's weight.  It saturates: the items an optimal code takes weigh its cost together, which is at most limit x the sum of
// the counts, so an item at 2^32 - 1 is never taken and its place among its like does not matter.
SPM_HD inline uint32_t huff_package(const uint32_t *below, uint32_t j)
{
    const uint64_t s = (uint64_t)below[2 * j] + below[2 * j + 1];
    return s > 0xffffffffull ? 0xffffffffu : (uint32_t)s;
}

// step 2: len[i] = the code length of symbol i, 0 where count[i] is 0.  At least two counts are nonzero, 2^limit >= their
// number, and limit x the sum of the counts is below 2^32 - 1.
template <class Sync>
SPM_HD inline void huff_lengths(const uint32_t *count, uint32_t n_sym, uint32_t limit, uint8_t *len, huff_work &W, uint32_t t, uint32_t T,
                                Sync sync)
{
    uint32_t n = 0;
    for (uint32_t j = 0; j < n_sym; ++j)
        n += count[j] != 0;
    for (uint32_t i = t; i < n_sym; i += T) { // the rank of a symbol by (count, symbol)
        len[i] = 0;
        const uint32_t c = count[i];
        if (!c)
            continue;
        uint32_t r = 0;
        for (uint32_t j = 0; j < n_sym; ++j) {
            const uint32_t cj = count[j];
            r += cj && (cj < c || (cj == c && j < i));
        }
        W.sym_of_rank[r] = (uint16_t)i;
        W.w[r] = c;
        W.list[0][r] = c;
        W.leafpos[0][r] = (uint16_t)r;
    }
    sync();
    uint32_t size = n;
    for (uint32_t l = 1; l < limit; ++l) { // level l + 1: every item finds its place by counting the other kind in front of it
        const uint32_t *below = W.list[(l - 1) & 1];
        uint32_t *list = W.list[l & 1];
        const uint32_t q = size / 2;
        for (uint32_t x = t; x < n + q; x += T) {
            uint32_t lo = 0;
            if (x < n) {
                const uint32_t wx = W.w[x];
                for (uint32_t hi = q; lo < hi;) { // packages lighter than the leaf
                    const uint32_t mid = (lo + hi) / 2;
                    if (huff_package(below, mid) < wx)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                list[x + lo] = wx;
                W.leafpos[l][x] = (uint16_t)(x + lo);
            } else {
                const uint32_t j = x - n, pk = huff_package(below, j);
                for (uint32_t hi = n; lo < hi;) { // leaves no heavier than the package
                    const uint32_t mid = (lo + hi) / 2;
                    if (W.w[mid] <= pk)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                list[j + lo] = pk;
            }
        }
        size = n + q;
        sync();
    }
    if (t == 0) {
        uint32_t m = 2 * n - 2;
        for (uint32_t l = limit; l-- > 0;) {
            uint32_t lo = 0;
            for (uint32_t hi = n; lo < hi;) { // leaves among the level's first m items
                const uint32_t mid = (lo + hi) / 2;
                if (W.leafpos[l][mid] < m)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            W.a[l] = lo;
            m = 2 * (m - lo);
        }
    }
    sync();
    for (uint32_t r = t; r < n; r += T) {
        uint32_t k = 0;
        for (uint32_t l = 0; l < limit; ++l)
            k += r < W.a[l];
        len[W.sym_of_rank[r]] = (uint8_t)k;
    }
    sync();
}

// the canonical code of RFC 1951 3.2.2: shorter codes first, then by symbol.  out[i] = code in stream order | length << 16
SPM_HD inline void huff_codes(const uint8_t *len, uint32_t n_sym, uint32_t *out, uint32_t t, uint32_t T)
{
    for (uint32_t i = t; i < n_sym; i += T) {
        const uint32_t L = len[i];
        uint32_t code = 0;
        for (uint32_t j = 0; L && j < n_sym; ++j) {
            const uint32_t lj = len[j];
            if (lj && lj < L)
                code += 1u << (L - lj);
            else if (lj == L && j < i)
                ++code;
        }
        out[i] = deflate_reverse(code, L) | L << 16;
    }
}

// the order in which a header sends the code-length code's lengths
SPM_HD inline uint32_t huff_cl_order(uint32_t i)
{
    constexpr uint8_t order[kHufCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}
SPM_HD inline uint32_t huff_cl_extra_bits(uint32_t sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// step 3, one lane: the n lengths at `at(i)` run-length coded greedily from the left into seq; returns how many symbols.
// A run of zeros of 3 or more: symbol 18 (11 .. 138) or 17 (3 .. 10), each as long as it can be.  A run of a nonzero length:
// once, then symbol 16 (3 .. 6) while 3 or more remain.  What is left goes as plain lengths.
template <class At> SPM_HD inline uint32_t huff_run_lengths(At at, uint32_t n, uint16_t *seq)
{
    uint32_t k = 0;
    for (uint32_t i = 0; i < n;) {
        const uint32_t v = at(i);
        uint32_t run = 1;
        while (i + run < n && at(i + run) == v)
            ++run;
        i += run;
        if (v) {
            seq[k++] = (uint16_t)v;
            --run;
        }
        const uint32_t least = 3, most = v ? 6 : 138;
        while (run >= least) {
            const uint32_t take = run < most ? run : most;
            if (v)
                seq[k++] = (uint16_t)(16 | (take - 3) << 8);
            else if (take >= 11)
                seq[k++] = (uint16_t)(18 | (take - 11) << 8);
            else
                seq[k++] = (uint16_t)(17 | (take - 3) << 8);
            run -= take;
        }
        for (; run; --run)
            seq[k++] = (uint16_t)v;
    }
    return k;
}

// The code of a block whose symbol counts stand in W.count[0, 286) (symbol 256 counted once) and W.count[286, 316).
template <class Sync> SPM_HD inline void huff_block_build(huff_work &W, huff_code &K, uint32_t t, uint32_t T, Sync sync)
{
    if (t == 0) {
        huff_pad(W.count, kHufLitLen);
        huff_pad(W.count + kHufLitLen, kHufDist);
    }
    sync();
    huff_lengths(W.count, kHufLitLen, kHufLimit, W.len, W, t, T, sync);
    huff_lengths(W.count + kHufLitLen, kHufDist, kHufLimit, W.len + kHufLitLen, W, t, T, sync);
    if (t == 0) { // the header's plan: at most 316 lengths, one lane
        uint32_t n_ll = kHufLitLen, n_dd = kHufDist;
        while (!W.len[n_ll - 1])
            --n_ll; // (symbol 256 has a code)
        while (!W.len[kHufLitLen + n_dd - 1])
            --n_dd;
        K.hlit = n_ll - 257;
        K.hdist = n_dd - 1;
        const uint8_t *len = W.len;
        K.n_seq = huff_run_lengths([=](uint32_t i) -> uint32_t { return i < n_ll ? len[i] : len[kHufLitLen + i - n_ll]; }, n_ll + n_dd, K.seq);
        for (uint32_t i = 0; i < kHufCl; ++i)
            W.count[kHufSeq + i] = 0;
        for (uint32_t i = 0; i < K.n_seq; ++i)
            ++W.count[kHufSeq + (K.seq[i] & 0xff)];
        huff_pad(W.count + kHufSeq, kHufCl);
    }
    sync();
    huff_lengths(W.count + kHufSeq, kHufCl, kHufClLimit, W.len + kHufSeq, W, t, T, sync);
    huff_codes(W.len, kHufLitLen, K.ll, t, T);
    huff_codes(W.len + kHufLitLen, kHufDist, K.dd, t, T);
    huff_codes(W.len + kHufSeq, kHufCl, K.cl, t, T);
    sync();
    if (t == 0) {
        uint32_t n_cl = kHufCl;
        while (n_cl > 4 && !(K.cl[huff_cl_order(n_cl - 1)] >> 16))
            --n_cl;
        K.hclen = n_cl - 4;
        uint32_t bits = 5 + 5 + 4 + 3 * n_cl;
        for (uint32_t i = 0; i < K.n_seq; ++i) {
            const uint32_t s = K.seq[i] & 0xff;
            bits += (K.cl[s] >> 16) + huff_cl_extra_bits(s);
        }
        K.header_bits = bits;
    }
    sync();
}

// step 4, the header behind the three block bits: put(bits, n) appends n <= 16 bits from bit 0
template <class Put> SPM_HD inline void huff_put_header(const huff_code &K, Put put)
{
    put(K.hlit, 5);
    put(K.hdist, 5);
    put(K.hclen, 4);
    for (uint32_t i = 0; i < K.hclen + 4; ++i)
        put(K.cl[huff_cl_order(i)] >> 16, 3);
    for (uint32_t i = 0; i < K.n_seq; ++i) {
        const uint32_t s = K.seq[i] & 0xff, c = K.cl[s], n = c >> 16, e = huff_cl_extra_bits(s);
        put((c & 0xffff) | (uint32_t)(K.seq[i] >> 8) << n, n + e);
    }
}

// ---- a token (len == 1: the literal v, else a match of len at distance v) in the block's code: its size, and its bits as
// the literal/length part (at most 20 bits) and the distance part (at most 28, none for a literal) ----
SPM_HD inline uint32_t huff_token_bits(const huff_code &K, uint32_t len, uint32_t v)
{
    if (len == 1)
        return K.ll[v] >> 16;
    uint32_t sym, e, x, dsym, de, dx;
    deflate_len_symbol(len, sym, e, x);
    deflate_dist_symbol(v, dsym, de, dx);
    return (K.ll[sym] >> 16) + e + (K.dd[dsym] >> 16) + de;
}
SPM_HD inline void huff_token_code(const huff_code &K, uint32_t len, uint32_t v, deflate_code &a, deflate_code &b)
{
    b.bits = 0, b.n = 0;
    if (len == 1) {
        a.bits = K.ll[v] & 0xffff, a.n = K.ll[v] >> 16;
        return;
    }
    uint32_t sym, e, x, dsym, de, dx;
    deflate_len_symbol(len, sym, e, x);
    deflate_dist_symbol(v, dsym, de, dx);
    const uint32_t c = K.ll[sym], dc = K.dd[dsym];
    a.n = c >> 16;
    a.bits = (c & 0xffff) | (uint64_t)x << a.n;
    a.n += e;
    b.n = dc >> 16;
    b.bits = (dc & 0xffff) | (uint64_t)dx << b.n;
    b.n += de;
}
SPM_HD inline void huff_count_token(uint32_t len, uint32_t v, uint32_t &ll_sym, uint32_t &dd_sym) // dd_sym: kHufDist for a literal
{
    ll_sym = v, dd_sym = kHufDist;
    if (len == 1)
        return;
    uint32_t e, x;
    deflate_len_symbol(len, ll_sym, e, x);
    deflate_dist_symbol(v, dd_sym, e, x);
}

// the dynamic payload's bytes from its tokens' bits
SPM_HD inline uint32_t huff_dynamic_bytes(const huff_code &K, uint64_t token_bits)
{
    return (uint32_t)((kHufHeaderBits + K.header_bits + token_bits + (K.ll[kHufEob] >> 16) + 7) / 8);
}
// No dynamic payload is shorter than this: the block bits, HLIT, HDIST, HCLEN, four code-length code lengths, and one bit for
// every literal/length, distance and end-of-block code.  A block whose floor is not below `other` (the smaller of its stored and
// fixed sizes) cannot come out dynamic, and skips the code build: the bytes are the same either way.
SPM_HD inline bool huff_may_win(uint64_t n_literals, uint64_t n_matches, uint32_t other)
{
    return (kHufHeaderBits + 14 + 12 + n_literals + 2 * n_matches + 1 + 7) / 8 < other;
}

} // namespace spm_hip
