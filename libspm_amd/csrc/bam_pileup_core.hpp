// bam_pileup_core.hpp -- the per-base pileup of a coordinate-sorted BAM record stream and its variant sites, the part a host
// compiler takes too (spm_hip_bam_pileup, spm_hip_bam_pileup_records, spm_hip_bam_pileup_host, spm_hip_pileup_sites,
// spm_hip_pileup_sites_host; contract and rule in spm_hip.h, scheme in DESIGN.md 4.12e).  Everything the counts depend on:
// what a line's record gives (pu_rec_read), which records take part and what is refused of them (pu_rec_test), the order test,
// a byte of the stream out of the dword that holds it, the plane of one column, the walk over a record's CIGAR clipped to a
// range of columns (pu_walk), the bounds of a tile's candidates, and the two serial builders.  The kernels of bam_pileup.hpp,
// the host calls and the case program all instantiate these functions.
//
// Overlapping mates of a pair are counted twice, once per record, as `samtools depth` counts them: mpileup-style overlap
// resolution is out of scope.
//
// Worked table (ref_len 1000, refID 0, min_baseq 0, every record forward; SEQ letters as SAM prints them, qualities ff unless given):
//     rec  POS(0-based)  CIGAR        SEQ          what it adds
//      0   10            4M           ACGT         A@10 C@11 G@12 T@13
//      1   10            2=1X1=       ACNT         A@10 C@11 N@12 T@13
//      2   11            2M2D2M       CGAA         C@11 G@12 DEL@13,14 A@15 A@16
//      3   12            2M3N2M       GTCC         G@12 T@13 (nothing at 14..16) C@17 C@18
//      4   12            2I3M         TTGTA        (the leading I is dropped) G@12 T@13 A@14
//      5   12            2S1I3M       AATGTA       (S, then I at r == pos: dropped) G@12 T@13 A@14
//      6   13            2M2I2M       TAGGAC       T@13 A@14 INS@14 A@15 C@16
//      7   13            3M2S         TAACC        T@13 A@14 A@15
//      8   14            2H3M1P2M3H   AACAC        A@14 A@15 C@16 A@17 C@18
//      9   15            3M  qual 0,20,ff   ACG    A@15 C@16 G@17; with min_baseq 1: LOWQ@15 C@16 G@17; with 93: LOWQ@15,16 G@17
//     10   15  flag 0x400 3M          AAA          nothing with the default exclude_flags; A@15,16,17 with exclude_flags 0x4
//     11   -1  refID -1 flag 0x4, no CIGAR         nothing: it does not take part
#pragma once

#include <cstdint>
#include <vector>

#include "bam_markdup_core.hpp" // md_rec_read, md_cigar_item
#include "hd.hpp"

namespace spm_hip
{

enum { kPuA, kPuC, kPuG, kPuT, kPuN, kPuDel, kPuIns, kPuLowq, kPuPlanes };
constexpr uint32_t kPuDefaultExclude = 0x704; // UNMAP | SECONDARY | QCFAIL | DUP
constexpr uint32_t kPuMaxBaseq = 93;
constexpr uint64_t kPuMaxRefLen = 1ull << 31; // a BAM pos is an int32; pos[] and end[] of the device are 32 bits
constexpr uint32_t kPuNoPos = 0xFFFFFFFFu;    // pos[] of a record without refID 0: behind every tile

struct pu_opts // what the rule takes of spm_pileup_opts: end resolved, 0x4 always excluded
{
    uint64_t begin = 0, end = 0;
    uint32_t exclude = kPuDefaultExclude, min_mapq = 0, min_baseq = 0;
};

// ---- what the rule takes of one record ----
struct pu_rec
{
    md_rec M;
    uint32_t mapq = 0;
    uint64_t cigar_at = 0, seq_at = 0; // first CIGAR byte and first SEQ byte, counted from the record's first byte
};
// -> false, and nothing is read beyond what was tested: md_rec_read fails
SPM_HD inline bool pu_rec_read(const uint8_t *stream, uint64_t n_bytes, uint64_t offset, uint32_t len, pu_rec &P)
{
    if (!md_rec_read(stream, n_bytes, offset, len, P.M))
        return false;
    P.mapq = stream[offset + 13];
    P.cigar_at = (uint64_t)kBamFixed + P.M.R.l_read_name;
    P.seq_at = P.cigar_at + 4ull * P.M.R.n_cigar_op;
    return true;
}
SPM_HD inline bool pu_takes_part(const pu_rec &P, const pu_opts &O)
{
    const uint32_t flag = P.M.R.flag;
    return !(flag & 0x4u) && !(flag & O.exclude) && P.mapq >= O.min_mapq && P.M.R.n_cigar_op > 0;
}
SPM_HD inline bool pu_op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
SPM_HD inline bool pu_op_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
SPM_HD inline bool pu_op_match(uint32_t op) { return op == 0 || op == 7 || op == 8; }

enum pu_status { kPuSkip, kPuTakes, kPuBad };
// The record a line names, read and tested.  kPuTakes: end = pos + max(span, 1), the BAI rule.  kPuBad: it cannot be read, or it
// takes part and has a refID other than 0, pos < 0, an end beyond ref_len, an op code above 8 or a query length that is not l_seq.
SPM_HD inline pu_status pu_rec_test(const uint8_t *stream, uint64_t n_bytes, uint64_t offset, uint32_t len, uint64_t ref_len, const pu_opts &O,
                                    pu_rec &P, uint64_t &end)
{
    end = 0;
    if (!pu_rec_read(stream, n_bytes, offset, len, P))
        return kPuBad;
    if (!pu_takes_part(P, O))
        return kPuSkip;
    const uint8_t *c = stream + offset + P.cigar_at;
    uint64_t span = 0, query = 0;
    bool bad_op = false;
    for (uint32_t i = 0; i < P.M.R.n_cigar_op; ++i) {
        const uint32_t w = bam_u32(c + 4 * i), op = w & 15u;
        span += pu_op_ref(op) ? (w >> 4) : 0u;
        query += pu_op_query(op) ? (w >> 4) : 0u;
        bad_op = bad_op || op > 8;
    }
    end = (uint64_t)(int64_t)P.M.R.pos + (span ? span : 1);
    if (P.M.R.ref_id != 0 || P.M.R.pos < 0 || end > ref_len || bad_op || query != P.M.l_seq)
        return kPuBad;
    return kPuTakes;
}
// Coordinate order, as far as the pileup needs it: among records of refID 0 pos does not descend, and no record of refID 0
// stands behind one of another refID.  prev: the record before cur.
SPM_HD inline bool pu_order_ok(const bam_rec &prev, const bam_rec &cur)
{
    return cur.ref_id != 0 || (prev.ref_id == 0 && prev.pos <= cur.pos);
}
// what the device keeps of a record's pos: monotone over a stream that passes pu_order_ok
SPM_HD inline uint32_t pu_pos_key(const bam_rec &R) { return R.ref_id != 0 ? kPuNoPos : R.pos < 0 ? 0u : (uint32_t)R.pos; }

// ---- a byte of the stream out of the dword that holds it.  load(a): the little-endian dword whose first byte is byte a of the
// stream, a such that (misalign + a) % 4 == 0 -- misalign the low bits of the stream's address; at >= 3 ----
template <class Load> SPM_HD inline uint32_t pu_byte_by_dword(Load load, uint32_t misalign, uint64_t at)
{
    const uint32_t sh = (uint32_t)((misalign + at) & 3u);
    return (load(at - sh) >> (8 * sh)) & 255u;
}
SPM_HD inline uint32_t pu_seq_code(uint32_t byte, uint64_t k) { return (k & 1u) ? (byte & 15u) : (byte >> 4); } // symbol k lies in byte k / 2
SPM_HD inline uint32_t pu_base_plane(uint32_t code) { return code == 1 ? kPuA : code == 2 ? kPuC : code == 4 ? kPuG : code == 8 ? kPuT : kPuN; }
// the plane one M = X column adds to; a quality of ff (absent) passes every threshold, as in htslib
SPM_HD inline uint32_t pu_column_plane(uint32_t code, uint32_t qual, uint32_t min_baseq)
{
    return (qual != 255u && qual < min_baseq) ? (uint32_t)kPuLowq : pu_base_plane(code);
}

// ---- the walk: every (plane, column) a record that takes part adds inside [lo, hi), in CIGAR order.  rec: its first byte ----
template <class Add> SPM_HD inline void pu_walk(const uint8_t *rec, const pu_rec &P, uint32_t min_baseq, uint64_t lo, uint64_t hi, Add add)
{
    const uint8_t *c = rec + P.cigar_at, *seq = rec + P.seq_at, *qual = rec + P.M.qual_at;
    const uint64_t pos = (uint64_t)(int64_t)P.M.R.pos;
    uint64_t r = pos, q = 0;
    for (uint32_t i = 0; i < P.M.R.n_cigar_op; ++i) {
        const uint32_t w = bam_u32(c + 4 * i), op = w & 15u;
        const uint64_t len = w >> 4;
        if (pu_op_match(op) || op == 2) {
            const uint64_t j0 = lo > r ? lo - r : 0, j1 = hi > r ? (hi - r < len ? hi - r : len) : 0;
            for (uint64_t j = j0; j < j1; ++j)
                add(op == 2 ? (uint32_t)kPuDel : pu_column_plane(pu_seq_code(seq[(q + j) / 2], q + j), qual[q + j], min_baseq), r + j);
        } else if (op == 1 && r > pos && r - 1 >= lo && r - 1 < hi) {
            add((uint32_t)kPuIns, r - 1);
        }
        r += pu_op_ref(op) ? len : 0;
        q += pu_op_query(op) ? len : 0;
    }
}

// ---- the candidates of a tile [t0, t1): from the first record whose running maximum of end lies above t0 up to the first
// whose pos is t1 or more.  pmax and pos are monotone ----
SPM_HD inline uint64_t pu_first_above(const uint32_t *pmax, uint64_t n, uint64_t t0)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pmax[mid] > t0)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}
SPM_HD inline uint64_t pu_first_at_or_behind(const uint32_t *pos, uint64_t n, uint64_t t1)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pos[mid] >= t1)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// ---- the serial builder: every record tested, then one loop over records and columns with plain increments into the
// caller's counters, no tiles.  counts: 8 * (end - begin), plane-major.
// -> false: the inputs disagree (counts is left as it was found) ----
inline bool pileup_serial(const uint8_t *stream, uint64_t n_bytes, const spm_sam_line *lines, uint64_t n_lines, uint64_t ref_len,
                          const pu_opts &O, uint32_t *counts)
{
    const uint64_t n = O.end - O.begin;
    std::vector<uint8_t> takes(n_lines, 0);
    bam_rec prev;
    for (uint64_t i = 0; i < n_lines; ++i) { // every record tested before the first counter is touched
        pu_rec P;
        uint64_t end = 0;
        const pu_status s = pu_rec_test(stream, n_bytes, lines[i].offset, lines[i].len, ref_len, O, P, end);
        if (s == kPuBad || (i && !pu_order_ok(prev, P.M.R)))
            return false;
        prev = P.M.R;
        takes[i] = s == kPuTakes;
    }
    for (uint64_t k = 0; k < kPuPlanes * n; ++k)
        counts[k] = 0;
    for (uint64_t i = 0; i < n_lines; ++i) {
        pu_rec P;
        if (!takes[i] || !pu_rec_read(stream, n_bytes, lines[i].offset, lines[i].len, P))
            continue;
        pu_walk(stream + lines[i].offset, P, O.min_baseq, O.begin, O.end, [&](uint32_t plane, uint64_t col) { ++counts[plane * n + (col - O.begin)]; });
    }
    return true;
}

// ---- variant sites ----
struct pu_site_opts
{
    uint32_t min_depth = 1, min_alt = 2, min_alt_permille = 200;
};
SPM_HD inline uint32_t pu_depth(const uint32_t *counts, uint64_t n, uint64_t k)
{
    return counts[kPuA * n + k] + counts[kPuC * n + k] + counts[kPuG * n + k] + counts[kPuT * n + k] + counts[kPuN * n + k] + counts[kPuDel * n + k];
}
// Column k of a pileup of n positions that begins at `begin`, against the reference rank there (above 3: plane N).
// -> it is a site, and S is filled.  counts[4] of a site are the base planes A C G T: N + DEL is depth less their sum, INS is
// alt - (depth - counts[ref]) for ref < 4.
SPM_HD inline bool pu_site_of(const uint32_t *counts, uint64_t n, uint64_t begin, uint64_t k, uint32_t ref_rank, const pu_site_opts &O,
                              spm_pileup_site &S)
{
    const uint32_t depth = pu_depth(counts, n, k), plane = ref_rank < 4 ? ref_rank : (uint32_t)kPuN;
    const uint32_t alt = depth - counts[plane * n + k] + counts[kPuIns * n + k];
    if (depth < O.min_depth || alt < O.min_alt || 1000ull * alt < (uint64_t)O.min_alt_permille * depth)
        return false;
    S.pos = (uint32_t)(begin + k);
    S.depth = depth;
    S.alt = alt;
    for (uint32_t b = 0; b < 4; ++b)
        S.counts[b] = counts[b * n + k];
    S.ref = (uint8_t)ref_rank;
    S.reserved[0] = S.reserved[1] = S.reserved[2] = 0;
    return true;
}
// the sites in position order; ref: the ranks of the whole reference (begin + n positions of it are read)
inline void pileup_sites_serial(const uint32_t *counts, uint64_t begin, uint64_t n, const uint8_t *ref, const pu_site_opts &O,
                                std::vector<spm_pileup_site> &out)
{
    out.clear();
    for (uint64_t k = 0; k < n; ++k) {
        spm_pileup_site S;
        if (pu_site_of(counts, n, begin, k, ref[begin + k], O, S))
            out.push_back(S);
    }
}

} // namespace spm_hip
