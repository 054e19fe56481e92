// jst_bam_sort_cases.cpp -- a coordinate-sorted BAM file and its BAI index through the C++ mirror, on the committed fixtures
// (tests/golden/jst): journaled_sequence_tree::map_bam with jst_bam_options::sort and ::index by the device route
// (spm_hip_bam_sort and spm_hip_bam_index behind the BAM call) returns the same file bytes, line records and index bytes as the
// host route (std::stable_sort over the converted records under the rule written again, spm_hip_bai_build_host), stored and
// deflated, at two block sizes.  The pairs are cut as jst_bam_cases.cpp cuts them.
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

static std::uint32_t le32(std::string const & s, std::size_t at)
{
    std::uint32_t v = 0;
    for (int i = 0; i < 4; ++i)
        v |= static_cast<std::uint32_t>(static_cast<unsigned char>(s[at + static_cast<std::size_t>(i)])) << (8 * i);
    return v;
}

// the records of a stream, each as its bytes
static std::vector<std::string> records_of(spm::jst_bam const & b)
{
    std::vector<std::string> out;
    for (auto const & l : b.lines)
        out.push_back(b.records.substr(l.offset, l.len));
    return out;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps)
{
    std::size_t const n_pairs = 32, n_reads = 2 * n_pairs;
    unsigned const k = 2;
    auto const reads = cut_pairs(haps, n_pairs);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0};
    std::vector<std::uint16_t> ks(n_reads, static_cast<std::uint16_t>(k));
    std::vector<std::vector<std::uint8_t>> needles;
    for (auto const & rd : reads) {
        cat.insert(cat.end(), rd.begin(), rd.end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
        needles.push_back(rd);
        needles.push_back(revcomp4(rd));
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
    for (std::uint32_t block_data : {0u, 1000u})
        for (int mode = 0; mode < 2; ++mode)
            for (bool deflate : {false, true}) {
                spm::jst_bam_options o;
                o.sam.rname = "sim_ref";
                o.sam.secondary = true;
                o.ref_len = jst.reference().size();
                o.block_data = block_data;
                o.deflate = deflate;
                spm::jst_sam_pairing const & pairing = mode == 0 ? single : rescued;
                spm::jst_bam const unsorted = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
                EXPECT_TRUE(unsorted.bai.empty());
                o.sort = true;
                spm::jst_bam const plain = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
                EXPECT_TRUE(plain.bai.empty());
                o.index = true;
                spm::jst_bam const dev = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
                spm::jst_bam const host = jst.map_bam_host(ps, window, needles, false, 2, nr, pairing, o, sel, 0, nullptr);
                EXPECT_TRUE(dev.file == host.file);
                EXPECT_TRUE(dev.records == host.records && dev.lines == host.lines);
                EXPECT_TRUE(dev.bai == host.bai);
                EXPECT_TRUE(dev.block_offsets == host.block_offsets && dev.header_file_bytes == host.header_file_bytes);
                EXPECT_TRUE(dev == jst.map_bam(ps, window, needles, false, 2, nr, pairing, o, sel, 0, nullptr));
                EXPECT_TRUE(dev.file == plain.file && dev.lines == plain.lines);
                // the same records as the file in read order, in another order: positions ascend, records without one come last
                auto a = records_of(unsorted), b = records_of(dev);
                EXPECT_TRUE(a != b && a.size() == b.size());
                bool ordered = true, seen_unplaced = false;
                std::int64_t last = -1;
                for (std::string const & r : b) {
                    bool const unplaced = le32(r, 4) != 0;
                    std::int64_t const pos = static_cast<std::int32_t>(le32(r, 8));
                    ordered = ordered && (unplaced ? true : !seen_unplaced && pos >= last);
                    seen_unplaced = seen_unplaced || unplaced;
                    last = unplaced ? last : pos;
                }
                EXPECT_TRUE(ordered);
                std::sort(a.begin(), a.end());
                std::sort(b.begin(), b.end());
                EXPECT_TRUE(a == b);
                EXPECT_TRUE(dev.bai.size() >= 24 + 40 && dev.bai.compare(0, 4, std::string("BAI\1", 4)) == 0 && le32(dev.bai, 4) == 1);
                EXPECT_TRUE(deflate == !dev.block_offsets.empty());
                std::printf("  block_data %u, mode %d, deflate %d: %zu records, %zu bytes, file %zu bytes, index %zu bytes in %u bins\n", block_data,
                            mode, deflate ? 1 : 0, dev.lines.size(), dev.records.size(), dev.file.size(), dev.bai.size(), le32(dev.bai, 8));
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
