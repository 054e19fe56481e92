// jst_bam_pileup_cases.cpp -- the pileup through the C++ mirror, on the committed fixtures (tests/golden/jst):
// journaled_sequence_tree::map_bam with jst_bam_options::pileup by the device route (spm_hip_bam_pileup behind the BAM call, the
// sort and the duplicate marks) returns the counts of the host route (spm_hip_bam_pileup_host over the host's own records), of
// the host call over the mirror's own file, and of the rule of spm_hip.h written again here as a plain walk over the record
// bytes.  The reads are cut as jst_bam_markdup_cases.cpp cuts them, the second half of them repeating the first, so that the
// marks change the counts.
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

// pair i: a fragment of 200 .. 350 haplotype symbols; i % 4 == 1: the right mate diverged; every other pair has mate 1 on the
// reverse strand
static std::vector<std::vector<std::uint8_t>> cut_pairs(std::vector<spm::io::fasta_record> const & haps, std::size_t n_pairs)
{
    std::vector<std::vector<std::uint8_t>> out;
    std::uint64_t r = 0x71E0Bull;
    for (std::size_t i = 0; i < n_pairs; ++i) {
        r = mix64(r + i);
        std::vector<std::uint8_t> const & hap = haps[r % haps.size()].ranks;
        std::size_t const frag = 200 + (r >> 44) % 151, at = (r >> 20) % (hap.size() - 800);
        auto const cut = [&](std::size_t from) {
            return std::vector<std::uint8_t>(hap.begin() + static_cast<std::ptrdiff_t>(from), hap.begin() + static_cast<std::ptrdiff_t>(from + L));
        };
        std::vector<std::uint8_t> left = cut(at), right = cut(at + frag - L);
        if (i % 4 == 1)
            for (std::size_t j = 5; j < L; j += 11)
                right[j] = static_cast<std::uint8_t>((right[j] + 1) & 3);
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

// the rule with the default options, record by record off the bytes; n_taking: the records that took part
static std::vector<std::uint32_t> rule(spm::jst_bam const & b, std::uint64_t ref_len, std::size_t & n_taking)
{
    std::vector<std::uint32_t> counts(8 * ref_len, 0);
    n_taking = 0;
    for (auto const & l : b.lines) {
        std::string const r = b.records.substr(l.offset, l.len);
        std::uint32_t const flag = le(r, 18, 2);
        std::size_t const l_name = le(r, 12, 1), n_cigar = le(r, 16, 2), l_seq = le(r, 20, 4);
        if ((flag & 0x704u) || n_cigar == 0)
            continue;
        ++n_taking;
        std::size_t const seq_at = 36 + l_name + 4 * n_cigar, qual_at = seq_at + (l_seq + 1) / 2;
        std::uint64_t const pos = le(r, 8, 4);
        std::uint64_t at = pos, q = 0;
        for (std::size_t c = 0; c < n_cigar; ++c) {
            std::uint32_t const w = le(r, 36 + l_name + 4 * c, 4), op = w & 15u, len = w >> 4;
            for (std::uint32_t j = 0; j < len; ++j) {
                if (op == 0 || op == 7 || op == 8) {
                    std::uint32_t const byte = le(r, seq_at + (q + j) / 2, 1), code = ((q + j) & 1) ? byte & 15u : byte >> 4;
                    std::uint32_t const plane = code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : 4;
                    (void)qual_at; // (min_baseq 0: no quality falls below it)
                    ++counts[plane * ref_len + at + j];
                } else if (op == 2) {
                    ++counts[5 * ref_len + at + j];
                }
            }
            if (op == 1 && at > pos)
                ++counts[6 * ref_len + at - 1];
            at += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? len : 0;
            q += (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? len : 0;
        }
    }
    return counts;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps)
{
    std::size_t const n_pairs = 32, n_reads = 2 * n_pairs;
    unsigned const k = 2;
    auto reads = cut_pairs(haps, n_pairs);
    for (std::size_t p = n_pairs / 2; p < n_pairs; ++p) { // pair p repeats pair p - 16
        reads[2 * p] = reads[2 * (p - n_pairs / 2)];
        reads[2 * p + 1] = reads[2 * (p - n_pairs / 2) + 1];
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
    std::uint64_t const ref_len = jst.reference().size();
    spm::jst_sam_pairing const single{}, rescued{true, MIN_TLEN, MAX_TLEN, true, K};
    for (int mode = 0; mode < 2; ++mode)
        for (bool marked : {false, true}) {
            spm::jst_bam_options o;
            o.sam.rname = "sim_ref";
            o.sam.secondary = true;
            o.sam.qualities = qualities;
            o.ref_len = ref_len;
            o.block_data = marked ? 1000u : 0u;
            o.sort = true;
            o.index = o.deflate = marked;
            o.mark_duplicates = marked;
            spm::jst_sam_pairing const & pairing = mode == 0 ? single : rescued;
            spm::jst_bam const plain = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            o.pileup = true;
            spm::jst_bam const dev = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            spm::jst_bam const host = jst.map_bam_host(ps, window, needles, false, 2, nr, pairing, o, sel, 0, nullptr);
            EXPECT_TRUE(plain.pileup.empty() && dev.pileup.size() == 8 * ref_len);
            EXPECT_TRUE(dev.pileup == host.pileup);
            EXPECT_TRUE(dev == host);
            EXPECT_TRUE(dev.file == plain.file && dev.records == plain.records && dev.lines == plain.lines && dev.bai == plain.bai);
            // the host call over the mirror's own file, and the rule
            std::vector<spm_sam_line> lines;
            for (auto const & l : dev.lines)
                lines.push_back(spm_sam_line{l.offset, l.len, l.read, l.source, l.flag, l.mapq, l.kind});
            std::vector<std::uint32_t> own(8 * ref_len, 7);
            EXPECT_TRUE(spm_hip_bam_pileup_host(dev.records.data(), dev.records.size(), lines.data(), lines.size(), ref_len, nullptr, own.data()) ==
                        SPM_OK);
            EXPECT_TRUE(own == dev.pileup);
            std::size_t n_taking = 0, n_dup = 0;
            EXPECT_TRUE(rule(dev, ref_len, n_taking) == dev.pileup);
            for (auto const & l : dev.lines)
                n_dup += (l.flag & 0x400u) != 0;
            std::uint64_t evidence = 0;
            for (std::uint32_t v : dev.pileup)
                evidence += v;
            EXPECT_TRUE(marked ? n_dup >= 12 : n_dup == 0);
            EXPECT_TRUE(n_taking >= 24 && evidence >= n_taking * (L - 2 * k));
            std::printf("  mode %d, marked %d: %zu records, %zu take part, %zu duplicates, evidence %llu\n", mode, marked ? 1 : 0, dev.lines.size(),
                        n_taking, n_dup, static_cast<unsigned long long>(evidence));
        }
    // a pileup needs the coordinate order: asked for without sort, the call ends the program, so that is not run here
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
