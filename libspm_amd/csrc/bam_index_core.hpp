// bam_index_core.hpp -- a coordinate-sorted BAM and its BAI index, the part a host compiler takes too (spm_hip_bam_sort,
// spm_hip_bam_index, spm_hip_bai_build; contract in spm_hip.h, scheme in DESIGN.md 4.12b).  Everything the bytes depend on:
// reading a record out of the stream at any byte alignment, a record's end, the sort key and the order test, the virtual
// offset of a stream offset, what the index takes of one record (bai_item), and the serial builder.  The kernels of
// bam_index.hpp, spm_hip_bai_build_host and the case program all instantiate these functions.
//
// The file (SAM specification 5.2, one reference):  "BAI\1" | n_ref = 1 | n_bin | per bin: bin u32, n_chunk i32, n_chunk x
// (begin u64, end u64) | n_intv i32 | n_intv x ioffset u64 | n_no_coor u64, all little-endian; every field lies on a 4-byte border.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "bgzf_core.hpp"
#include "hd.hpp"
#include "jst_bam_core.hpp"

namespace spm_hip
{

constexpr uint32_t kBaiPseudoBin = 37450, kBaiBins = 37449; // bins 0 .. 37448 hold records
constexpr uint32_t kBaiWindowShift = 14, kBaiMaxWindows = 1u << 15;
constexpr uint64_t kBaiMaxEnd = 1ull << 29; // the longest reference a BAI can address
constexpr uint32_t kBaiNoBin = 0xFFFFu;     // (of a record the index does not bin; sorts behind every bin)
constexpr uint64_t kBaiNoOffset = ~0ull;    // an empty window before the back-fill
constexpr uint32_t kBamKeyPosBits = 32;     // bam_key: reverse | (pos + 1) << 1 | rank of refID << 33

// ---- a record in the stream, at any byte alignment ----
SPM_HD inline uint32_t bam_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
SPM_HD inline uint32_t bam_u32(const uint8_t *p) { return bam_u16(p) | bam_u16(p + 2) << 16; }

struct bam_rec
{
    int32_t ref_id = -1, pos = -1;
    uint32_t bin = 4680, flag = 0, l_read_name = 0, n_cigar_op = 0;
};
// The fields of the record a line names.  -> false, and nothing is read beyond what was tested: the line leaves the stream,
// is shorter than the fixed part, its block_size is not len - 4, or name and CIGAR leave the record.
SPM_HD inline bool bam_rec_read(const uint8_t *stream, uint64_t n_bytes, uint64_t offset, uint32_t len, bam_rec &R)
{
    if (offset > n_bytes || len > n_bytes - offset || len < kBamFixed)
        return false;
    const uint8_t *p = stream + offset;
    if (bam_u32(p) != len - 4)
        return false;
    R.ref_id = (int32_t)bam_u32(p + 4);
    R.pos = (int32_t)bam_u32(p + 8);
    R.l_read_name = p[12];
    R.bin = bam_u16(p + 14);
    R.n_cigar_op = bam_u16(p + 16);
    R.flag = bam_u16(p + 18);
    return (uint64_t)kBamFixed + R.l_read_name + 4ull * R.n_cigar_op <= len;
}
// pos + max(span, 1), span the reference symbols of the CIGAR (M D N = X); pos + 1 for an unmapped record or one without CIGAR
SPM_HD inline uint64_t bam_rec_end(const uint8_t *rec, const bam_rec &R)
{
    uint64_t span = 0;
    if (!(R.flag & 0x4)) {
        const uint8_t *c = rec + kBamFixed + R.l_read_name;
        for (uint32_t i = 0; i < R.n_cigar_op; ++i) {
            const uint32_t w = bam_u32(c + 4 * i), op = w & 15u;
            span += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (w >> 4) : 0u;
        }
    }
    return (uint64_t)(int64_t)R.pos + (span ? span : 1);
}

// ---- the order: refID as unsigned (one reference: 0, then everything else, so -1 comes last), pos, forward before reverse ----
SPM_HD inline uint64_t bam_key(const bam_rec &R)
{
    return (uint64_t)(R.ref_id != 0) << (kBamKeyPosBits + 1) | (uint64_t)((uint32_t)R.pos + 1u) << 1 | ((R.flag >> 4) & 1u);
}
// What the radix sort takes: the key with its position part cut to the bits ref_len needs (pos + 1 <= ref_len).
SPM_HD inline uint32_t bam_pos_bits(uint64_t ref_len)
{
    uint32_t b = 1;
    while (b < kBamKeyPosBits && (ref_len >> b))
        ++b;
    return b;
}
SPM_HD inline uint32_t bam_sort_key_bits(uint32_t pos_bits) { return pos_bits + 2; }
SPM_HD inline bool bam_key_packs(uint64_t key, uint32_t pos_bits) { return ((key >> 1) & 0xFFFFFFFFull) >> pos_bits == 0; }
SPM_HD inline uint64_t bam_key_pack(uint64_t key, uint32_t pos_bits)
{
    return (key >> (kBamKeyPosBits + 1)) << (pos_bits + 1) | (key & ((2ull << pos_bits) - 1));
}

// ---- virtual offsets: the file offsets of the blocks, as a table of n_blocks + 1 or as the closed form of stored blocks ----
struct bai_blocks
{
    const unsigned long long *table = nullptr; // n_blocks + 1 offsets, or null: stored blocks behind `first`
    uint64_t first = 0;
    uint64_t n_stream = 0, n_blocks = 0;
    uint32_t D = kBgzfBlockData;
    SPM_HD uint64_t at(uint64_t b) const
    {
        if (table)
            return table[b];
        return first + (b < n_blocks ? bgzf_block_offset(D, b) : bgzf_framed_size(n_stream, D, false));
    }
};
SPM_HD inline uint64_t bai_voffset(const bai_blocks &B, uint64_t u) { return B.at(u / B.D) << 16 | u % B.D; } // u <= n_stream

// ---- what the index takes of one record ----
struct bai_item
{
    uint64_t key = 0, begin = 0, end = 0; // the order key; the virtual offsets of the record's first byte and of the byte behind it
    uint64_t ref_begin = 0, ref_end = 0;  // placed: pos, pos + max(span, 1)
    uint32_t bin = kBaiNoBin;             // placed: the record's bin field
    bool placed = false, unmapped = false;
};
// -> false: the record cannot be indexed (bam_rec_read fails; a refID other than 0 and -1; a placed record with pos < 0, an end
// beyond 2^29 or a bin field beyond 37448)
SPM_HD inline bool bai_item_of(const uint8_t *stream, uint64_t n_bytes, const bai_blocks &B, uint64_t offset, uint32_t len, bai_item &I)
{
    bam_rec R;
    if (!bam_rec_read(stream, n_bytes, offset, len, R) || R.ref_id < -1 || R.ref_id > 0)
        return false;
    I.key = bam_key(R);
    I.begin = bai_voffset(B, offset);
    I.end = bai_voffset(B, offset + len);
    I.placed = R.ref_id == 0;
    I.unmapped = (R.flag & 0x4) != 0;
    if (!I.placed)
        return true;
    I.bin = R.bin;
    I.ref_begin = (uint64_t)(int64_t)R.pos;
    I.ref_end = bam_rec_end(stream + offset, R);
    return R.pos >= 0 && I.ref_end <= kBaiMaxEnd && R.bin < kBaiBins;
}
// the lines tile the stream: line i starts where line i - 1 ended, the first at 0, the last ends the stream
SPM_HD inline bool bai_line_follows(const spm_sam_line *lines, uint64_t n_lines, uint64_t n_bytes, uint64_t i)
{
    const uint64_t want = i ? lines[i - 1].offset + lines[i - 1].len : 0;
    return lines[i].offset == want && (i + 1 < n_lines || lines[i].offset + lines[i].len == n_bytes);
}
SPM_HD inline uint32_t bai_n_intv(uint64_t max_end) { return max_end ? (uint32_t)((max_end - 1) >> kBaiWindowShift) + 1 : 0; }
SPM_HD inline uint64_t bai_size(uint64_t n_bins_file, uint64_t n_chunks, uint64_t n_intv, bool pseudo)
{
    return 12 + 8 * n_bins_file + 16 * (n_chunks + (pseudo ? 2 : 0)) + 4 + 8 * n_intv + 8;
}
SPM_HD inline void bai_put32(uint8_t *to, uint64_t at, uint32_t v) // at: a multiple of 4 (the file has no other)
{
    for (uint32_t i = 0; i < 4; ++i)
        to[at + i] = (uint8_t)(v >> (8 * i));
}
SPM_HD inline void bai_put64(uint8_t *to, uint64_t at, uint64_t v)
{
    bai_put32(to, at, (uint32_t)v);
    bai_put32(to, at + 4, (uint32_t)(v >> 32));
}

struct bai_counts
{
    uint64_t n_bins = 0;   // the file's n_bin: the pseudo-bin is counted
    uint64_t n_chunks = 0; // of the bins that hold records
    uint64_t n_intv = 0, n_mapped = 0, n_unmapped = 0, n_no_coor = 0;
};

// ---- the serial builder: one walk over the stream.  -> false: the inputs disagree (out is left empty) ----
inline bool bai_build_serial(const uint8_t *stream, uint64_t n_bytes, const spm_sam_line *lines, uint64_t n_lines, const bai_blocks &B,
                             std::vector<uint8_t> &out, bai_counts &C)
{
    struct chunk
    {
        uint32_t bin;
        uint64_t begin, end;
    };
    out.clear();
    C = bai_counts{};
    if (B.D == 0 || B.D > kBgzfBlockData || B.n_stream != n_bytes || B.n_blocks != bgzf_n_blocks(n_bytes, B.D) || (n_lines == 0) != (n_bytes == 0))
        return false;
    std::vector<chunk> chunks;
    std::vector<uint64_t> window;
    uint64_t prev_key = 0, max_end = 0, first_begin = 0, last_end = 0;
    bool open = false; // the last chunk takes the next record if it has the chunk's bin
    for (uint64_t i = 0; i < n_lines; ++i) {
        bai_item I;
        if (!bai_line_follows(lines, n_lines, n_bytes, i) || !bai_item_of(stream, n_bytes, B, lines[i].offset, lines[i].len, I) ||
            (i && I.key < prev_key))
            return false;
        prev_key = I.key;
        if (!I.placed) {
            ++C.n_no_coor;
            open = false;
            continue;
        }
        ++(I.unmapped ? C.n_unmapped : C.n_mapped);
        if (open && chunks.back().bin == I.bin)
            chunks.back().end = I.end;
        else
            chunks.push_back(chunk{I.bin, I.begin, I.end});
        open = true;
        if (max_end == 0)
            first_begin = I.begin;
        last_end = I.end;
        max_end = std::max(max_end, I.ref_end);
        const uint64_t w1 = (I.ref_end - 1) >> kBaiWindowShift;
        if (window.size() <= w1)
            window.resize(w1 + 1, kBaiNoOffset);
        for (uint64_t w = I.ref_begin >> kBaiWindowShift; w <= w1; ++w)
            window[w] = std::min(window[w], I.begin);
    }
    const bool pseudo = C.n_mapped + C.n_unmapped != 0;
    // an empty window takes the value of the next one to its right that is not (the last one never is empty)
    for (uint64_t w = window.size(); w-- > 1;)
        window[w - 1] = std::min(window[w - 1], window[w]);
    std::stable_sort(chunks.begin(), chunks.end(), [](const chunk &a, const chunk &b) { return a.bin < b.bin; });
    C.n_chunks = chunks.size();
    C.n_intv = bai_n_intv(max_end);
    for (size_t c = 0; c < chunks.size(); ++c)
        C.n_bins += c == 0 || chunks[c].bin != chunks[c - 1].bin;
    C.n_bins += pseudo ? 1 : 0;
    out.assign(bai_size(C.n_bins, C.n_chunks, C.n_intv, pseudo), 0);
    uint8_t *to = out.data();
    bai_put32(to, 0, 0x01494142u); // "BAI\1"
    bai_put32(to, 4, 1);
    bai_put32(to, 8, (uint32_t)C.n_bins);
    uint64_t at = 12;
    for (size_t c = 0; c < chunks.size(); ++c) {
        if (c == 0 || chunks[c].bin != chunks[c - 1].bin) {
            size_t e = c;
            while (e < chunks.size() && chunks[e].bin == chunks[c].bin)
                ++e;
            bai_put32(to, at, chunks[c].bin);
            bai_put32(to, at + 4, (uint32_t)(e - c));
            at += 8;
        }
        bai_put64(to, at, chunks[c].begin);
        bai_put64(to, at + 8, chunks[c].end);
        at += 16;
    }
    if (pseudo) {
        bai_put32(to, at, kBaiPseudoBin);
        bai_put32(to, at + 4, 2);
        bai_put64(to, at + 8, first_begin);
        bai_put64(to, at + 16, last_end);
        bai_put64(to, at + 24, C.n_mapped);
        bai_put64(to, at + 32, C.n_unmapped);
        at += 40;
    }
    bai_put32(to, at, (uint32_t)C.n_intv);
    for (uint64_t w = 0; w < C.n_intv; ++w)
        bai_put64(to, at + 4 + 8 * w, window[w]);
    bai_put64(to, at + 4 + 8 * C.n_intv, C.n_no_coor);
    return true;
}

} // namespace spm_hip
