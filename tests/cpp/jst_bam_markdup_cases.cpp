// jst_bam_markdup_cases.cpp -- duplicate marking through the C++ mirror, on the committed fixtures (tests/golden/jst):
// journaled_sequence_tree::map_bam with jst_bam_options::mark_duplicates by the device route (spm_hip_bam_markdup behind the BAM
// call and the sort, before deflate and index) returns the same file bytes, line records and index bytes as the host route
// (spm_hip_bam_markdup_host over the host's own records), and the flags of both equal the rule of spm_hip.h written again here as
// an all-pairs comparison over the records of the unmarked file.  The pairs are cut as jst_bam_cases.cpp cuts them, the second
// half of them repeating the first.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include <libspm/jst/journaled_sequence_tree.hpp>

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
        }                                                                                                              \
    } while (0)

static std::string const DATA = std::string(SPM_TEST_DATA) + "/";

static std::uint64_t mix64(std::uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<std::uint8_t> revcomp4(std::vector<std::uint8_t> const & r)
{
    std::vector<std::uint8_t> out;
    for (std::size_t i = r.size(); i-- > 0;)
        out.push_back(static_cast<std::uint8_t>(3 - r[i]));
    return out;
}

static constexpr std::size_t L = 60;
static constexpr std::uint32_t MIN_TLEN = 150, MAX_TLEN = 400, K = 8;

// pair i: a fragment of 200 .. 350 haplotype symbols; i % 4: 0 both mates exact, 1 the right mate diverged, 2 the left mate
// diverged, 3 the right mate is noise; every other pair has mate 1 on the reverse strand
static std::vector<std::vector<std::uint8_t>> cut_pairs(std::vector<spm::io::fasta_record> const & haps, std::size_t n_pairs)
{
    std::vector<std::vector<std::uint8_t>> out;
    std::uint64_t r = 0x5A3C0Eull;
    for (std::size_t i = 0; i < n_pairs; ++i) {
        r = mix64(r + i);
        std::vector<std::uint8_t> const & hap = haps[r % haps.size()].ranks;
        std::size_t const frag = 200 + (r >> 44) % 151, at = (r >> 20) % (hap.size() - 800);
        auto const cut = [&](std::size_t from) {
            return std::vector<std::uint8_t>(hap.begin() + static_cast<std::ptrdiff_t>(from), hap.begin() + static_cast<std::ptrdiff_t>(from + L));
        };
        std::vector<std::uint8_t> left = cut(at), right = cut(at + frag - L);
        auto const diverge = [](std::vector<std::uint8_t> & x) {
            for (std::size_t j = 5; j < L; j += 11)
                x[j] = static_cast<std::uint8_t>((x[j] + 1) & 3);
        };
        if (i % 4 == 1)
            diverge(right);
        if (i % 4 == 2)
            diverge(left);
        if (i % 4 == 3)
            for (std::size_t j = 0; j < L; ++j)
                right[j] = static_cast<std::uint8_t>(mix64(r + 77 * j) & 3);
        if (i % 2) {
            out.push_back(revcomp4(right));
            out.push_back(left);
        } else {
            out.push_back(left);
            out.push_back(revcomp4(right));
        }
    }
    return out;
}

static std::uint32_t le(std::string const & s, std::size_t at, int n)
{
    std::uint32_t v = 0;
    for (int i = 0; i < n; ++i)
        v |= static_cast<std::uint32_t>(static_cast<unsigned char>(s[at + static_cast<std::size_t>(i)])) << (8 * i);
    return v;
}

// what the rule takes of one record, read off its bytes
struct item
{
    std::uint32_t read = 0, flag = 0, score = 0;
    std::int64_t u = 0;
    bool primary = false, placed = false, reverse = false, paired = false;
};

static std::vector<item> items_of(spm::jst_bam const & b)
{
    std::vector<item> out;
    for (auto const & l : b.lines) {
        std::string const r = b.records.substr(l.offset, l.len);
        item it;
        it.read = l.read;
        it.flag = le(r, 18, 2);
        it.primary = (it.flag & 0x900u) == 0;
        it.placed = it.primary && (it.flag & 0x4u) == 0;
        it.reverse = (it.flag & 0x10u) != 0;
        it.paired = (it.flag & 0x1u) != 0;
        std::size_t const l_name = le(r, 12, 1), n_cigar = le(r, 16, 2), l_seq = le(r, 20, 4);
        std::int64_t span = 0;
        for (std::size_t c = 0; c < n_cigar; ++c) {
            std::uint32_t const w = le(r, 36 + l_name + 4 * c, 4), op = w & 15u;
            span += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? static_cast<std::int64_t>(w >> 4) : 0;
        }
        std::int64_t const pos = static_cast<std::int32_t>(le(r, 8, 4));
        it.u = it.reverse ? pos + std::max<std::int64_t>(span, 1) - 1 : pos;
        for (std::size_t q = 0; q < l_seq; ++q) {
            std::uint32_t const v = le(r, 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + q, 1);
            it.score += (v >= 15 && v <= 93) ? v : 0;
        }
        out.push_back(it);
    }
    return out;
}

// dup per line, by comparing every placed read with every other
static std::vector<bool> rule(std::vector<item> const & items, std::size_t n_reads, std::size_t & n_dup_pairs, std::size_t & n_beside)
{
    std::vector<item const *> of(n_reads, nullptr);
    for (item const & it : items)
        if (it.placed)
            of[it.read] = &it;
    auto const pair_end = [&](std::size_t r) { return of[r] && of[r]->paired && (r ^ 1) < n_reads && of[r ^ 1] && of[r ^ 1]->paired; };
    auto const end = [&](std::size_t r) { return std::make_pair(of[r]->u, of[r]->reverse); };
    auto const key = [&](std::size_t p) { // the two ends in order, by value
        auto const a = end(2 * p), b = end(2 * p + 1);
        return a < b ? std::make_pair(a, b) : std::make_pair(b, a);
    };
    std::vector<bool> dup_read(n_reads, false);
    n_dup_pairs = n_beside = 0;
    for (std::size_t r = 0; r < n_reads; ++r) {
        if (!of[r])
            continue;
        if (pair_end(r)) {
            std::size_t const p = r / 2;
            std::uint32_t const sp = of[2 * p]->score + of[2 * p + 1]->score;
            for (std::size_t q = 0; 2 * q + 1 < n_reads; ++q) {
                if (q == p || !pair_end(2 * q) || key(q) != key(p))
                    continue;
                std::uint32_t const sq = of[2 * q]->score + of[2 * q + 1]->score;
                if (sq > sp || (sq == sp && q < p))
                    dup_read[r] = true;
            }
            n_dup_pairs += (r & 1) && dup_read[r];
        } else {
            bool beside = false;
            for (std::size_t q = 0; q < n_reads; ++q) {
                if (q == r || !of[q] || end(q) != end(r))
                    continue;
                if (pair_end(q))
                    beside = true;
                else if (of[q]->score > of[r]->score || (of[q]->score == of[r]->score && q < r))
                    dup_read[r] = true;
            }
            dup_read[r] = dup_read[r] || beside;
            n_beside += beside;
        }
    }
    std::vector<bool> dup;
    for (item const & it : items)
        dup.push_back(it.placed && dup_read[it.read]);
    return dup;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps)
{
    std::size_t const n_pairs = 32, n_reads = 2 * n_pairs;
    unsigned const k = 2;
    auto reads = cut_pairs(haps, n_pairs);
    for (std::size_t p = n_pairs / 2; p < n_pairs; ++p) { // pair p repeats pair p - 16; every third of them with the mates swapped
        reads[2 * p] = reads[2 * (p - n_pairs / 2) + (p % 3 == 0 ? 1 : 0)];
        reads[2 * p + 1] = reads[2 * (p - n_pairs / 2) + (p % 3 == 0 ? 0 : 1)];
    }
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0};
    std::vector<std::uint16_t> ks(n_reads, static_cast<std::uint16_t>(k));
    std::vector<std::vector<std::uint8_t>> needles, qualities;
    for (std::size_t r = 0; r < n_reads; ++r) {
        auto const & rd = reads[r];
        cat.insert(cat.end(), rd.begin(), rd.end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
        needles.push_back(rd);
        needles.push_back(revcomp4(rd));
        std::vector<std::uint8_t> q(rd.size());
        for (std::size_t j = 0; j < q.size(); ++j)
            q[j] = static_cast<std::uint8_t>(mix64(1000 * r + j) % 94);
        qualities.push_back(q);
    }
    spm_ctx * ctx = spm::hip::default_context();
    spm_patterns * ps = nullptr;
    if (spm_hip_patterns_create_stranded(ctx, SPM_ALGO_MYERS, cat.data(), off.data(), static_cast<std::uint32_t>(n_reads), ks.data(), 4,
                                         &ps) != SPM_OK)
        spm::hip::fatal("spm_hip_patterns_create_stranded", ctx);
    spm::hip::patterns_ptr compiled{ps, spm::hip::patterns_deleter{}};
    std::size_t const window = L + k;
    spm::hip::hit_selection const sel{true, {}, 1u, true, true};
    auto const nr = static_cast<std::uint32_t>(n_reads);
    spm::jst_sam_pairing const single{}, rescued{true, MIN_TLEN, MAX_TLEN, true, K};
    for (int mode = 0; mode < 2; ++mode)
        for (bool sorted : {false, true}) {
            spm::jst_bam_options o;
            o.sam.rname = "sim_ref";
            o.sam.secondary = true;
            if (sorted)
                o.sam.qualities = qualities;
            o.ref_len = jst.reference().size();
            o.block_data = sorted ? 1000u : 0u;
            o.sort = o.index = o.deflate = sorted;
            spm::jst_sam_pairing const & pairing = mode == 0 ? single : rescued;
            spm::jst_bam const unmarked = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            o.mark_duplicates = true;
            spm::jst_bam const dev = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            spm::jst_bam const host = jst.map_bam_host(ps, window, needles, false, 2, nr, pairing, o, sel, 0, nullptr);
            EXPECT_TRUE(dev.file == host.file);
            EXPECT_TRUE(dev.records == host.records && dev.lines == host.lines);
            EXPECT_TRUE(dev.bai == host.bai && dev.bai.empty() == !sorted);
            EXPECT_TRUE(dev.block_offsets == host.block_offsets && dev.header_file_bytes == host.header_file_bytes);
            // the flags equal the rule; nothing else differs from the unmarked file's records
            std::size_t n_dup_pairs = 0, n_beside = 0, n_dup = 0;
            auto const items = items_of(unmarked);
            auto const want = rule(items, n_reads, n_dup_pairs, n_beside);
            EXPECT_TRUE(dev.lines.size() == unmarked.lines.size() && dev.records.size() == unmarked.records.size());
            bool flags_ok = dev.lines.size() == unmarked.lines.size(), rest_ok = dev.records.size() == unmarked.records.size();
            for (std::size_t i = 0; flags_ok && rest_ok && i < dev.lines.size(); ++i) {
                auto const & l = dev.lines[i];
                auto const & ul = unmarked.lines[i];
                std::uint32_t const expect = (items[i].flag & ~0x400u) | (want[i] ? 0x400u : 0u);
                flags_ok = le(dev.records, l.offset + 18, 2) == expect && l.flag == expect;
                std::string a = dev.records.substr(l.offset, l.len), b = unmarked.records.substr(ul.offset, ul.len);
                a[19] = b[19] = 0;
                rest_ok = a == b && l.offset == ul.offset && l.len == ul.len && l.read == ul.read && l.source == ul.source && l.mapq == ul.mapq &&
                          l.kind == ul.kind;
                n_dup += want[i];
            }
            EXPECT_TRUE(flags_ok);
            EXPECT_TRUE(rest_ok);
            EXPECT_TRUE(n_dup >= (mode == 0 ? 16u : 12u) && (mode == 0 ? n_dup_pairs == 0 : n_dup_pairs >= 4)); // the repeats are found
            EXPECT_TRUE(sorted == !dev.block_offsets.empty());
            std::printf("  mode %d, sorted %d: %zu records, %zu duplicates (%zu pairs, %zu fragments beside pairs), file %zu bytes\n", mode,
                        sorted ? 1 : 0, dev.lines.size(), n_dup, n_dup_pairs, n_beside, dev.file.size());
        }
}

int main()
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + "sim_ref_10Kb_SNP_INDELs.vcf");
    auto haps = spm::io::read_fasta(DATA + "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(ref.size() == 1 && haps.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    tree_cases(jst, haps);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
