// pileup_vcf_core.hpp -- genotype calls for pileup sites and the VCF line of a variant site, the part a host compiler takes too
// (spm_hip_pileup_sites_vcf, spm_hip_pileup_sites_vcf_records, spm_hip_pileup_sites_calls_host, spm_hip_pileup_sites_vcf_host,
// spm_hip_vcf_header; contract and rule in spm_hip.h, scheme in DESIGN.md 4.12f).  Everything the bytes depend on: the options
// resolved (vc_opts_of), the cost of a genotype (vc_cost), the call of a site with its PLs (vc_call), the decimal writer
// (vc_put_u32), the line through a sink that counts or stores (vc_line_emit), the bound of a line's length, where a run of
// lines splits into head bytes, aligned dwords and tail bytes (vc_run_split), the header and the serial builders.  The kernels
// of pileup_vcf.hpp, the host calls and the case program all instantiate these functions.  Integer arithmetic throughout: the
// policy comes in as milli-Phred integers, no floating point runs on either side.
//
// Worked table (reference A, defaults, ploidy 2):
//     counts A,C,G,T   depth   tail of the line
//     10,10,0,0        20      A C 157 PASS DP=20 GT:AD:GQ:PL 0/1:10,10:99:157,0,190
//     0,0,3,0          3       A G 41 PASS DP=3 GT:AD:GQ:PL 1/1:0,3:6:41,6,0
//     0,8,0,8          16      A C,T 288 PASS DP=16 GT:AD:GQ:PL 1/2:0,8,8:99:288,144,123,144,0,123
//     19,1,0,0         20      no line: ref/ref wins (25607 against 90780 for A/C)
// The first row: AA = 10 * 44 + 10 * 24771 = 248150, AC = 20 * 3039 + 30000 = 90780, CC = 248150 + 33010 = 281160; the
// differences 157370 and 190380 give the PLs 157 and 190.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bam_pileup_core.hpp" // spm_pileup_site; jst_sam_name_ok and kSamMaxName through the cores behind it
#include "hd.hpp"

namespace spm_hip
{

// the defaults: milli-Phred costs of one read base at e = 0.01 and the priors at theta = 1e-3 (spm_hip.h has the formula in
// words; the case program recomputes the literals)
constexpr uint32_t kVcCostMatch = 44, kVcCostHet = 3039, kVcCostMiss = 24771;
constexpr uint32_t kVcPriorHet = 30000, kVcPriorHomAlt = 33010;
constexpr uint32_t kVcMinQual = 20;
constexpr uint32_t kVcMaxCost = 1000000;   // 4 * (2^32 - 1) * 10^6 + 2 * 10^6 stays far below 2^64
constexpr uint32_t kVcPlCap = 0x7FFFFFFFu; // a PL saturates here
constexpr uint32_t kVcMaxSample = 254;

struct vc_opts // spm_vcf_opts resolved
{
    uint32_t ploidy = 2;
    uint32_t cost_match = kVcCostMatch, cost_het = kVcCostHet, cost_miss = kVcCostMiss;
    uint32_t prior_het = kVcPriorHet, prior_hom_alt = kVcPriorHomAlt;
    uint32_t min_qual = kVcMinQual;
};
// -> what is wrong with the options, or null and O filled
inline const char *vc_opts_of(const spm_vcf_opts *opts, vc_opts &O)
{
    O = vc_opts{};
    if (!opts)
        return nullptr;
    if (opts->ploidy > 2)
        return "ploidy is not 1 or 2 (0: 2)";
    if (opts->flags)
        return "flags must be 0";
    if (opts->reserved0 || opts->reserved1)
        return "reserved fields must be 0";
    if (opts->cost_match > kVcMaxCost || opts->cost_het > kVcMaxCost || opts->cost_miss > kVcMaxCost || opts->prior_het > kVcMaxCost ||
        opts->prior_hom_alt > kVcMaxCost)
        return "a cost or prior above 1000000";
    O.ploidy = opts->ploidy ? opts->ploidy : 2;
    if (opts->cost_match || opts->cost_het || opts->cost_miss) {
        O.cost_match = opts->cost_match;
        O.cost_het = opts->cost_het;
        O.cost_miss = opts->cost_miss;
    }
    if (opts->prior_het || opts->prior_hom_alt) {
        O.prior_het = opts->prior_het;
        O.prior_hom_alt = opts->prior_hom_alt;
    }
    O.min_qual = opts->min_qual;
    return nullptr;
}

// ---- the cost of genotype (a, b), a <= b, ranks; ref the reference rank (below 4) ----
SPM_HD inline uint64_t vc_cost(const uint32_t counts[4], uint32_t a, uint32_t b, uint32_t ref, const vc_opts &O)
{
    uint64_t c = 0;
    for (uint32_t x = 0; x < 4; ++x) { // (four iterations: unrolled, counts[] by constant index)
        const uint32_t per = a == b ? (x == a ? O.cost_match : O.cost_miss) : ((x == a || x == b) ? O.cost_het : O.cost_miss);
        c += (uint64_t)counts[x] * per;
    }
    const bool ra = a == ref, rb = b == ref;
    if (O.ploidy == 1)
        return c + (ra ? 0u : O.prior_hom_alt);
    return c + (ra && rb ? 0u : (ra || rb) ? O.prior_het : a == b ? O.prior_hom_alt : 2u * O.prior_het);
}

// ---- the call of one site.  The loops below run over fixed bounds and every array index is a constant once they are unrolled,
// so on the device the ten costs, the kept alleles and the PLs stay in registers ----
#if defined(__HIP_DEVICE_COMPILE__)
#define SPM_VC_UNROLL _Pragma("unroll")
#else
#define SPM_VC_UNROLL
#endif
struct vc_eval
{
    uint32_t status = SPM_CALL_REF_N;
    uint32_t gt[2] = {0, 0};      // the best genotype, ranks, gt[0] <= gt[1]
    uint32_t gt_idx[2] = {0, 0};  // the same as indices into kept[]
    uint32_t n_kept = 0;          // 1 + n_alt
    uint32_t kept[3] = {0, 0, 0}; // REF, then the ALT ranks ascending
    uint32_t n_pl = 0;
    uint32_t pl[6] = {0, 0, 0, 0, 0, 0};
    uint32_t qual = 0, gq = 0;
};
SPM_HD inline uint32_t vc_pl_of(uint64_t cost, uint64_t best)
{
    const uint64_t v = (cost - best + 500) / 1000;
    return v > kVcPlCap ? kVcPlCap : (uint32_t)v;
}
// allele j of the order (the reference rank, then the other ranks ascending)
SPM_HD inline uint32_t vc_ordered(uint32_t ref, uint32_t j) { return j == 0 ? ref : (j - 1 < ref ? j - 1 : j); }
SPM_HD inline uint32_t vc_count_of(const spm_pileup_site &S, uint32_t x)
{
    return x == 0 ? S.counts[0] : x == 1 ? S.counts[1] : x == 2 ? S.counts[2] : S.counts[3];
}
SPM_HD inline void vc_call(const spm_pileup_site &S, const vc_opts &O, vc_eval &E)
{
    E = vc_eval{};
    const uint32_t ref = S.ref;
    if (ref > 3)
        return;
    // VCF genotype order over (ref, then the other ranks ascending): the first least cost wins
    uint64_t best = ~0ull;
    uint32_t bj = 0, bk = 0;
    SPM_VC_UNROLL
    for (uint32_t k = 0; k < 4; ++k) {
        SPM_VC_UNROLL
        for (uint32_t j = 0; j <= k; ++j) {
            if (O.ploidy == 1 && j != k)
                continue;
            const uint32_t x = vc_ordered(ref, j), y = vc_ordered(ref, k);
            const uint64_t c = vc_cost(S.counts, x < y ? x : y, x < y ? y : x, ref, O);
            if (c < best) {
                best = c;
                bj = j;
                bk = k;
            }
        }
    }
    // (bj <= bk, and the order ascends behind the reference: where both are ALTs, vc_ordered(ref, bj) is the lower rank)
    const uint32_t lo = vc_ordered(ref, bj), hi = vc_ordered(ref, bk);
    E.kept[0] = ref;
    if (bj > 0) {
        E.kept[1] = lo;
        E.kept[2] = bk != bj ? hi : 0u;
        E.n_kept = bk != bj ? 3 : 2;
        E.gt_idx[0] = 1;
        E.gt_idx[1] = bk != bj ? 2 : 1;
    } else {
        E.kept[1] = bk > 0 ? hi : 0u;
        E.n_kept = bk > 0 ? 2 : 1;
        E.gt_idx[1] = bk > 0 ? 1 : 0;
    }
    E.gt[0] = lo < hi ? lo : hi;
    E.gt[1] = lo < hi ? hi : lo;
    E.status = E.n_kept == 1 ? SPM_CALL_REF : SPM_CALL_VARIANT;
    E.n_pl = O.ploidy == 1 ? E.n_kept : E.n_kept * (E.n_kept + 1) / 2;
    uint32_t least = kVcPlCap, second = kVcPlCap; // the two smallest PLs
    SPM_VC_UNROLL
    for (uint32_t k = 0; k < 3; ++k) {
        SPM_VC_UNROLL
        for (uint32_t j = 0; j <= k; ++j) {
            if (k >= E.n_kept || (O.ploidy == 1 && j != k))
                continue;
            const uint32_t x = E.kept[j], y = E.kept[k];
            const uint32_t pl = vc_pl_of(vc_cost(S.counts, x < y ? x : y, x < y ? y : x, ref, O), best);
            if (O.ploidy == 1)
                E.pl[k] = pl;
            else
                E.pl[k * (k + 1) / 2 + j] = pl;
            if (pl < least) {
                second = least;
                least = pl;
            } else if (pl < second) {
                second = pl;
            }
        }
    }
    E.qual = E.pl[0];
    E.gq = E.n_pl < 2 ? 0u : second < 99u ? second : 99u;
}
// what a call record keeps of it; offset and len belong to the text
SPM_HD inline void vc_record(const spm_pileup_site &S, const vc_eval &E, uint32_t len, uint64_t offset, spm_variant_call &C)
{
    C.pos = S.pos;
    C.depth = S.depth;
    C.qual = E.status == SPM_CALL_REF_N ? 0u : E.qual;
    C.len = len;
    C.offset = offset;
    C.status = (uint8_t)E.status;
    C.gq = (uint8_t)E.gq;
    C.gt[0] = (uint8_t)E.gt[0];
    C.gt[1] = (uint8_t)E.gt[1];
    C.n_alt = (uint8_t)(E.n_kept ? E.n_kept - 1 : 0);
    C.alt[0] = (uint8_t)(E.n_kept > 1 ? E.kept[1] : 0);
    C.alt[1] = (uint8_t)(E.n_kept > 2 ? E.kept[2] : 0);
    C.reserved = 0;
}

// ---- the line.  A sink takes one byte at a time: it counts them (the call stage) or stores them (the write stage, the host) ----
struct vc_count_sink
{
    uint32_t n = 0;
    SPM_HD void byte(uint32_t) { ++n; }
};
struct vc_store_sink
{
    uint8_t *p;
    SPM_HD void byte(uint32_t c) { *p++ = (uint8_t)c; }
};
template <class Sink> SPM_HD inline void vc_put_u32(Sink &out, uint32_t v)
{
    uint32_t div = 1000000000u;
    while (div > v && div > 1)
        div /= 10;
    for (; div; div /= 10)
        out.byte('0' + (v / div) % 10);
}
template <class Sink> SPM_HD inline void vc_put(Sink &out, const char *s, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        out.byte((uint8_t)s[i]);
}
SPM_HD inline uint32_t vc_letter(uint32_t rank) { return rank == 0 ? 'A' : rank == 1 ? 'C' : rank == 2 ? 'G' : 'T'; }
// E.status is SPM_CALL_VARIANT
template <class Sink>
SPM_HD inline void vc_line_emit(Sink &out, const char *rname, uint32_t rname_len, const spm_pileup_site &S, const vc_eval &E, const vc_opts &O)
{
    vc_put(out, rname, rname_len);
    out.byte('\t');
    vc_put_u32(out, S.pos + 1); // (pos < ref_len <= 2^32 - 1 was tested: no wrap)
    out.byte('\t');
    out.byte('.');
    out.byte('\t');
    out.byte(vc_letter(E.kept[0]));
    out.byte('\t');
    out.byte(vc_letter(E.kept[1]));
    if (E.n_kept > 2) {
        out.byte(',');
        out.byte(vc_letter(E.kept[2]));
    }
    out.byte('\t');
    vc_put_u32(out, E.qual);
    if (E.qual >= O.min_qual)
        vc_put(out, "\tPASS\tDP=", 9);
    else
        vc_put(out, "\tLowQual\tDP=", 12);
    vc_put_u32(out, S.depth);
    vc_put(out, "\tGT:AD:GQ:PL\t", 13);
    out.byte('0' + E.gt_idx[0]);
    if (O.ploidy == 2) {
        out.byte('/');
        out.byte('0' + E.gt_idx[1]);
    }
    out.byte(':');
    SPM_VC_UNROLL
    for (uint32_t k = 0; k < 3; ++k)
        if (k < E.n_kept) {
            if (k)
                out.byte(',');
            vc_put_u32(out, vc_count_of(S, E.kept[k]));
        }
    out.byte(':');
    vc_put_u32(out, E.gq);
    out.byte(':');
    SPM_VC_UNROLL
    for (uint32_t k = 0; k < 6; ++k)
        if (k < E.n_pl) {
            if (k)
                out.byte(',');
            vc_put_u32(out, E.pl[k]);
        }
    out.byte('\n');
}
// The most one line takes, field by field: CHROM, POS, ".", REF, "C,T", QUAL, "LowQual", "DP=" and depth, the FORMAT keys, GT,
// three ADs, GQ, six PLs, the tabs, colons, commas and the newline between them.
constexpr uint32_t kVcMaxLineLessName = 10 + 1 + 1 + 3 + 10 + 7 + (3 + 10) + 11 + 3 + (3 * 10 + 2) + 2 + (6 * 10 + 5) + 9 /* tabs */ + 3 /* colons */ + 1;
constexpr uint32_t kVcMaxLine = kSamMaxName + kVcMaxLineLessName;
static_assert(kVcMaxLineLessName == 171 && kVcMaxLine == 425, "the widths above, added up");
// the length of a site's line: 0 where it has none
SPM_HD inline uint32_t vc_line_len(uint32_t rname_len, const spm_pileup_site &S, const vc_eval &E, const vc_opts &O)
{
    if (E.status != SPM_CALL_VARIANT)
        return 0;
    vc_count_sink n;
    vc_line_emit(n, (const char *)nullptr, 0, S, E, O);
    return n.n + rname_len;
}

// ---- a run of B bytes that lies at [shift, shift + B) of a buffer whose byte 0 stands on a 4-byte border of the destination
// (shift < 4): head bytes [shift, a), whole dwords [a, b), tail bytes [b, shift + B); a and b are multiples of 4 where the
// dword range is not empty ----
SPM_HD inline void vc_run_split(uint32_t shift, uint32_t B, uint32_t &a, uint32_t &b)
{
    const uint32_t e = shift + B, up = shift ? 4u : 0u;
    a = up < e ? up : e;
    b = (e & ~3u) > a ? (e & ~3u) : a;
}

// ---- the header ----
inline bool vc_sample_ok(const char *s, uint64_t len)
{
    if (len == 0 || len > kVcMaxSample)
        return false;
    for (uint64_t i = 0; i < len; ++i)
        if (s[i] < '!' || s[i] > '~')
            return false;
    return true;
}
inline std::string vc_header(const char *rname, const char *sample, uint64_t ref_len)
{
    return std::string("##fileformat=VCFv4.2\n##contig=<ID=") + rname + ",length=" + std::to_string(ref_len) +
           ">\n"
           "##FILTER=<ID=LowQual,Description=\"QUAL below the threshold\">\n"
           "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth: A + C + G + T + N + DEL\">\n"
           "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
           "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Base counts of the REF and ALT alleles\">\n"
           "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">\n"
           "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype costs\">\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
           sample + "\n";
}

// ---- the serial builders.  -> false: a pos that does not ascend strictly, or reaches ref_len (nothing is written) ----
inline bool vc_sites_in_order(const spm_pileup_site *sites, uint64_t n, uint64_t ref_len)
{
    for (uint64_t i = 0; i < n; ++i)
        if (sites[i].pos >= ref_len || (i && sites[i - 1].pos >= sites[i].pos))
            return false;
    return true;
}
// calls (may be null): one record per site, offset counted from `base`; text (may be null): the lines appended
inline void vc_serial(const spm_pileup_site *sites, uint64_t n, const char *rname, uint32_t rname_len, const vc_opts &O, uint64_t base,
                      bool with_lines, spm_variant_call *calls, std::string *text)
{
    uint8_t line[kVcMaxLine];
    uint64_t at = base;
    for (uint64_t i = 0; i < n; ++i) {
        vc_eval E;
        vc_call(sites[i], O, E);
        const uint32_t len = with_lines ? vc_line_len(rname_len, sites[i], E, O) : 0;
        if (calls)
            vc_record(sites[i], E, len, with_lines ? at : 0, calls[i]);
        if (len && text) {
            vc_store_sink out{line};
            vc_line_emit(out, rname, rname_len, sites[i], E, O);
            text->append(reinterpret_cast<const char *>(line), len);
        }
        at += len;
    }
}

} // namespace spm_hip
