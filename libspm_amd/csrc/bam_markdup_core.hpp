// bam_markdup_core.hpp -- duplicate marking of a BAM record stream, the part a host compiler takes too (spm_hip_bam_markdup,
// spm_hip_bam_markdup_records, spm_hip_bam_markdup_host; contract and rule in spm_hip.h, scheme in DESIGN.md 4.12d).  Everything
// the bytes depend on: what a line's record gives (md_rec_read), the 5' end of a placed read (md_cigar_item, md_end_of), the
// score of a run of quality bytes by bytes and by dwords, the word a read is summarised in (md_info), the sort keys of pairs
// and ends, and the serial builder.  The kernels of bam_markdup.hpp, spm_hip_bam_markdup_host and the case program all
// instantiate these functions.
#pragma once

#include <cstdint>
#include <unordered_map>
#include <vector>

#include "bam_index_core.hpp"
#include "hd.hpp"

namespace spm_hip
{

constexpr uint32_t kMdDefaultMinQual = 15, kMdMaxQual = 93; // a quality byte counts from min_qual up to the highest Phred a SAM line can print
constexpr uint32_t kMdMaxScore = (1u << 24) - 1;            // a record's score is clamped to this
constexpr uint32_t kMdNoLine = 0xFFFFFFFFu;                 // primary_of[read] of a read without a primary record
constexpr uint64_t kMdMaxRefLen = 1ull << 30;               // ref_len must lie below: a pair key holds two ends
constexpr uint32_t kMdFlagDup = 0x400, kMdFlagAt = 19;      // the bit, and the byte of the record that holds it (bit 2 of flag's high byte)

// ---- what the rule takes of one record ----
struct md_rec
{
    bam_rec R;
    uint32_t l_seq = 0;
    uint64_t qual_at = 0; // first quality byte, counted from the record's first byte
};
// -> false, and nothing is read beyond what was tested: bam_rec_read fails, or seq and qual leave the record
SPM_HD inline bool md_rec_read(const uint8_t *stream, uint64_t n_bytes, uint64_t offset, uint32_t len, md_rec &M)
{
    if (!bam_rec_read(stream, n_bytes, offset, len, M.R))
        return false;
    M.l_seq = bam_u32(stream + offset + 20);
    M.qual_at = (uint64_t)kBamFixed + M.R.l_read_name + 4ull * M.R.n_cigar_op + ((uint64_t)M.l_seq + 1) / 2;
    return M.qual_at + M.l_seq <= len;
}
SPM_HD inline bool md_is_primary(uint32_t flag) { return (flag & 0x900u) == 0; }

// ---- the 5' end ----
// one CIGAR word into the span (M D N = X) and the "clipped" mark (S H)
SPM_HD inline void md_cigar_item(uint32_t w, uint64_t &span, bool &clipped)
{
    const uint32_t op = w & 15u;
    span += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (w >> 4) : 0u;
    clipped = clipped || op == 4 || op == 5;
}
// rec: the record's first byte.  The serial form of what the wave does item by item.
SPM_HD inline void md_cigar_walk(const uint8_t *rec, const bam_rec &R, uint64_t &span, bool &clipped)
{
    const uint8_t *c = rec + kBamFixed + R.l_read_name;
    for (uint32_t i = 0; i < R.n_cigar_op; ++i)
        md_cigar_item(bam_u32(c + 4 * i), span, clipped);
}
// (u, s) of a placed record whose CIGAR spans `span`.  -> false: a refID other than 0, pos < 0, an end beyond ref_len, a clip.
// end = pos + max(span, 1) is bam_rec_end of a record without flag 0x4.
SPM_HD inline bool md_end_of(const bam_rec &R, uint64_t span, bool clipped, uint64_t ref_len, uint32_t &u, uint32_t &s)
{
    const uint64_t end = (uint64_t)(int64_t)R.pos + (span ? span : 1);
    if (R.ref_id != 0 || R.pos < 0 || end > ref_len || clipped)
        return false;
    s = (R.flag >> 4) & 1u;
    u = s ? (uint32_t)(end - 1) : (uint32_t)R.pos;
    return true;
}

// ---- the score ----
SPM_HD inline uint32_t md_min_qual(uint32_t asked) { return asked ? asked : kMdDefaultMinQual; }
SPM_HD inline uint32_t md_qual_value(uint32_t v, uint32_t min_qual) { return (v >= min_qual && v <= kMdMaxQual) ? v : 0u; }
SPM_HD inline uint32_t md_score_clamp(uint64_t sum) { return sum < kMdMaxScore ? (uint32_t)sum : kMdMaxScore; }
// the sum over n bytes at q, not clamped
SPM_HD inline uint64_t md_score_bytes(const uint8_t *q, uint64_t n, uint32_t min_qual)
{
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; ++i)
        sum += md_qual_value(q[i], min_qual);
    return sum;
}
// The share of one little-endian dword whose first byte is byte `at` of the stream: its bytes inside [q0, q1).
SPM_HD inline uint32_t md_score_dword(uint32_t w, uint64_t at, uint64_t q0, uint64_t q1, uint32_t min_qual)
{
    uint32_t sum = 0;
    for (uint32_t j = 0; j < 4; ++j) {
        const uint64_t p = at + j;
        sum += (p >= q0 && p < q1) ? md_qual_value((w >> (8 * j)) & 255u, min_qual) : 0u;
    }
    return sum;
}

// ---- a read in one word: bit 0 placed, bit 1 s, bit 2 flag 0x1 of its primary record, bits 8..31 score, bits 32..61 u.
// 0: not placed ----
SPM_HD inline uint64_t md_info_pack(uint32_t u, uint32_t s, bool paired, uint32_t score)
{
    return (uint64_t)u << 32 | (uint64_t)score << 8 | (paired ? 4u : 0u) | (s ? 2u : 0u) | 1u;
}
SPM_HD inline bool md_placed(uint64_t info) { return (info & 1u) != 0; }
SPM_HD inline uint32_t md_score(uint64_t info) { return (uint32_t)(info >> 8) & kMdMaxScore; }
SPM_HD inline uint64_t md_end_code(uint64_t info) { return (info >> 32) << 1 | ((info >> 1) & 1u); } // (u, s) as one number
// read r is a pair end: placed, flag 0x1, and read r ^ 1 likewise.  info: [n], by read
SPM_HD inline bool md_is_pair_end(const unsigned long long *info, uint64_t n, uint64_t r)
{
    const uint64_t mate = r ^ 1u;
    return (info[r] & 5u) == 5u && mate < n && (info[mate] & 5u) == 5u;
}

// ---- the items two sorts order.  Pairs: item p < (n + 1) / 2, reads 2p and 2p + 1.  Ends: item r < n.  An item that does
// not take part has the bit above its key set and sorts behind all that do. ----
SPM_HD inline uint64_t md_n_items(bool pairs, uint64_t n) { return pairs ? (n + 1) / 2 : n; }
SPM_HD inline uint32_t md_key_bits(bool pairs, uint32_t pos_bits) { return pairs ? 2 * (pos_bits + 1) + 1 : pos_bits + 3; }
SPM_HD inline uint64_t md_key_none(bool pairs, uint32_t pos_bits) { return 1ull << (md_key_bits(pairs, pos_bits) - 1); }
SPM_HD inline uint32_t md_score_bits(bool pairs) { return pairs ? 25 : 24; }
// pairs: (u_lo, s_lo, u_hi, s_hi); ends: (u, s, is_fragment), so that a run of one (u, s) has its pair ends in front
SPM_HD inline uint64_t md_item_key(bool pairs, const unsigned long long *info, uint64_t n, uint64_t item, uint32_t pos_bits)
{
    if (pairs) {
        if (2 * item + 1 >= n || !md_is_pair_end(info, n, 2 * item))
            return md_key_none(true, pos_bits);
        const uint64_t a = md_end_code(info[2 * item]), b = md_end_code(info[2 * item + 1]);
        return (a < b ? a : b) << (pos_bits + 1) | (a < b ? b : a);
    }
    if (!md_placed(info[item]))
        return md_key_none(false, pos_bits);
    return md_end_code(info[item]) << 1 | (md_is_pair_end(info, n, item) ? 0u : 1u);
}
// what the first of the two sorts orders by: the highest score first.  Of a pair, the sum of its mates' scores; of a pair end
// among the ends, nothing.
SPM_HD inline uint64_t md_item_inv_score(bool pairs, const unsigned long long *info, uint64_t n, uint64_t item)
{
    if (pairs)
        return 2 * item + 1 < n ? 2ull * kMdMaxScore - md_score(info[2 * item]) - md_score(info[2 * item + 1]) : 0;
    return kMdMaxScore - md_score(info[item]);
}
SPM_HD inline bool md_key_valid(bool pairs, uint64_t key, uint32_t pos_bits) { return (key & md_key_none(pairs, pos_bits)) == 0; }
// Behind both sorts the survivor heads every run.  A pair is a duplicate if its key is its left neighbour's; a fragment if
// its (u, s) is its left neighbour's, whatever that neighbour is.
SPM_HD inline bool md_item_is_dup(bool pairs, uint64_t key, uint64_t left, uint32_t pos_bits)
{
    if (!md_key_valid(pairs, key, pos_bits))
        return false;
    return pairs ? key == left : ((key & 1u) != 0 && key >> 1 == left >> 1);
}

struct md_counts
{
    uint64_t n_pairs = 0, n_fragments = 0, n_dup_pairs = 0, n_dup_fragments = 0, n_dup_records = 0, n_fragments_beside_pairs = 0;
};

// ---- the serial builder: maps, no sort.  dup: n_lines bytes.  -> false: the inputs disagree (dup is left as it was found) ----
inline bool markdup_serial(const uint8_t *stream, uint64_t n_bytes, const spm_sam_line *lines, uint64_t n_lines, uint64_t ref_len,
                           uint32_t min_qual, uint8_t *dup, md_counts &C)
{
    struct best
    {
        uint64_t score, item;
    };
    C = md_counts{};
    std::vector<uint32_t> primary_of(n_lines, kMdNoLine);
    std::vector<unsigned long long> info(n_lines, 0);
    for (uint64_t i = 0; i < n_lines; ++i) {
        md_rec M;
        const uint32_t r = lines[i].read;
        if (!md_rec_read(stream, n_bytes, lines[i].offset, lines[i].len, M) || r >= n_lines)
            return false;
        if (!md_is_primary(M.R.flag))
            continue;
        if (primary_of[r] != kMdNoLine)
            return false;
        primary_of[r] = (uint32_t)i;
        if (M.R.flag & 0x4u)
            continue;
        const uint8_t *rec = stream + lines[i].offset;
        uint64_t span = 0;
        bool clipped = false;
        uint32_t u = 0, s = 0;
        md_cigar_walk(rec, M.R, span, clipped);
        if (!md_end_of(M.R, span, clipped, ref_len, u, s))
            return false;
        info[r] = md_info_pack(u, s, (M.R.flag & 1u) != 0, md_score_clamp(md_score_bytes(rec + M.qual_at, M.l_seq, min_qual)));
    }
    std::vector<uint8_t> dup_read(n_lines, 0);
    // pairs: the best of every key, the ends of all of them
    std::unordered_map<uint64_t, best> pair_best, frag_best;
    std::unordered_map<uint64_t, bool> pair_ends;
    auto take = [](std::unordered_map<uint64_t, best> &m, uint64_t key, uint64_t score, uint64_t item) {
        auto it = m.find(key);
        if (it == m.end())
            m.emplace(key, best{score, item});
        else if (score > it->second.score) // (items arrive in ascending order: a tie stays with the lowest)
            it->second = best{score, item};
    };
    for (uint64_t p = 0; 2 * p + 1 < n_lines; ++p) {
        if (!md_is_pair_end(info.data(), n_lines, 2 * p))
            continue;
        ++C.n_pairs;
        const uint64_t a = md_end_code(info[2 * p]), b = md_end_code(info[2 * p + 1]);
        pair_ends[a] = pair_ends[b] = true;
        take(pair_best, (a < b ? a : b) << 32 | (a < b ? b : a), (uint64_t)md_score(info[2 * p]) + md_score(info[2 * p + 1]), p);
    }
    for (uint64_t p = 0; 2 * p + 1 < n_lines; ++p) {
        if (!md_is_pair_end(info.data(), n_lines, 2 * p))
            continue;
        const uint64_t a = md_end_code(info[2 * p]), b = md_end_code(info[2 * p + 1]);
        if (pair_best[(a < b ? a : b) << 32 | (a < b ? b : a)].item != p) {
            dup_read[2 * p] = dup_read[2 * p + 1] = 1;
            ++C.n_dup_pairs;
        }
    }
    // fragments
    for (uint64_t r = 0; r < n_lines; ++r) {
        if (!md_placed(info[r]) || md_is_pair_end(info.data(), n_lines, r))
            continue;
        ++C.n_fragments;
        if (pair_ends.count(md_end_code(info[r]))) {
            dup_read[r] = 1;
            ++C.n_fragments_beside_pairs;
        } else {
            take(frag_best, md_end_code(info[r]), md_score(info[r]), r);
        }
    }
    for (uint64_t r = 0; r < n_lines; ++r) {
        if (!md_placed(info[r]) || md_is_pair_end(info.data(), n_lines, r) || dup_read[r])
            continue;
        dup_read[r] = frag_best[md_end_code(info[r])].item != r;
    }
    for (uint64_t r = 0; r < n_lines; ++r)
        C.n_dup_fragments += md_placed(info[r]) && !md_is_pair_end(info.data(), n_lines, r) && dup_read[r];
    for (uint64_t i = 0; i < n_lines; ++i) {
        dup[i] = primary_of[lines[i].read] == i && dup_read[lines[i].read];
        C.n_dup_records += dup[i];
    }
    return true;
}

} // namespace spm_hip
