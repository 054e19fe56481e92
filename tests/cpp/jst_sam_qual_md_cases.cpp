// jst_sam_qual_md_cases.cpp -- base qualities and the MD tag through the C++ mirror, on the committed fixtures (tests/golden/jst):
// journaled_sequence_tree::map_sam and map_bam with jst_sam_options::qualities and ::md by the device route
// (spm_hip_jst_ref_loci_sam_ex / spm_hip_jst_ref_loci_bam_ex behind the chain) return the same text, file bytes, record stream
// and line records as the host route (the plain formatter with its own MD writer; its lines converted to records from their text
// fields), single-end and paired with rescues, with each of the two fields and with both, stored and deflated.  The pairs are cut
// as jst_bam_cases.cpp cuts them.
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

static std::size_t count(std::string const & text, std::string const & what)
{
    std::size_t n = 0;
    for (std::size_t at = text.find(what); at != std::string::npos; at = text.find(what, at + 1))
        ++n;
    return n;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, std::size_t block)
{
    std::size_t const n_pairs = 32, n_reads = 2 * n_pairs;
    unsigned const k = 2;
    auto const reads = cut_pairs(haps, n_pairs);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0};
    std::vector<std::uint16_t> ks(n_reads, static_cast<std::uint16_t>(k));
    std::vector<std::vector<std::uint8_t>> needles, qualities;
    for (std::size_t r = 0; r < reads.size(); ++r) {
        cat.insert(cat.end(), reads[r].begin(), reads[r].end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
        needles.push_back(reads[r]);
        needles.push_back(revcomp4(reads[r]));
        std::vector<std::uint8_t> q;
        for (std::size_t j = 0; j < reads[r].size(); ++j) // 0 and 93 at the ends: the ends of the range
            q.push_back(j == 0 ? 0 : j + 1 == reads[r].size() ? 93 : static_cast<std::uint8_t>(mix64(977 * r + j) % 94));
        qualities.push_back(q);
    }
    spm_ctx * ctx = spm::hip::default_context();
    spm_patterns * ps = nullptr;
    if (spm_hip_patterns_create_stranded(ctx, SPM_ALGO_MYERS, cat.data(), off.data(), static_cast<std::uint32_t>(n_reads), ks.data(), 4,
                                         &ps) != SPM_OK)
        spm::hip::fatal("spm_hip_patterns_create_stranded", ctx);
    spm::hip::patterns_ptr compiled{ps, spm::hip::patterns_deleter{}};
    std::size_t const window = L + k;
    EXPECT_TRUE(jst.device_ready());
    spm::hip::hit_selection const sel{true, {}, 1u, true, true};
    auto const nr = static_cast<std::uint32_t>(n_reads);
    spm::jst_sam_pairing const single{}, rescued{true, MIN_TLEN, MAX_TLEN, true, K};
    for (int mode = 0; mode < 2; ++mode)
        for (int fields = 0; fields < 4; ++fields)
            for (int flags = 0; flags < 2; ++flags) {
                spm::jst_sam_pairing const & pairing = mode == 0 ? single : rescued;
                spm::jst_bam_options o;
                o.sam.rname = "sim_ref";
                o.sam.cigar_m = flags != 0;
                o.sam.secondary = true;
                if (fields & 1)
                    o.sam.qualities = qualities;
                o.sam.md = (fields & 2) != 0;
                o.ref_len = jst.reference().size();
                o.block_data = flags ? 1000 : 0;
                spm::jst_sam const dev = jst.map_sam_device(ps, window, 2, nr, pairing, o.sam, sel, block, nullptr);
                spm::jst_sam const host = jst.map_sam_host(ps, window, needles, false, 2, nr, pairing, o.sam, sel, block, nullptr);
                EXPECT_TRUE(dev.text == host.text);
                EXPECT_TRUE(dev.lines == host.lines);
                if (dev.text != host.text)
                    for (std::size_t i = 0; i < dev.lines.size() && i < host.lines.size(); ++i) {
                        std::string const a = dev.text.substr(dev.lines[i].offset, dev.lines[i].len);
                        std::string const b = host.text.substr(host.lines[i].offset, host.lines[i].len);
                        if (a != b) {
                            std::printf("  line %zu differs:\n  device %s  host   %s", i, a.c_str(), b.c_str());
                            break;
                        }
                    }
                std::size_t mapped = 0;
                for (spm::jst_sam_line const & x : dev.lines)
                    mapped += x.kind != SPM_SAM_UNMAPPED;
                EXPECT_TRUE(count(dev.text, "\tMD:Z:") == (o.sam.md ? mapped : 0u) && mapped >= n_reads / 2);
                if (fields == 0) { // neither field: the old call's bytes
                    spm::jst_sam_options plain = o.sam;
                    EXPECT_TRUE(dev == jst.map_sam(ps, window, needles, false, 2, nr, pairing, plain, sel, block, nullptr));
                    EXPECT_TRUE(count(dev.text, "\t*\tNM:i:") + count(dev.text, "\t*\n") == dev.lines.size());
                }
                for (int deflate = 0; deflate < 2; ++deflate) {
                    o.deflate = deflate != 0;
                    spm::jst_bam const bdev = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, block, nullptr);
                    spm::jst_bam const bhost = jst.map_bam_host(ps, window, needles, false, 2, nr, pairing, o, sel, block, nullptr);
                    EXPECT_TRUE(bdev.file == bhost.file);
                    EXPECT_TRUE(bdev.records == bhost.records);
                    EXPECT_TRUE(bdev.lines == bhost.lines);
                    EXPECT_TRUE(bdev.block_offsets == bhost.block_offsets && bdev.header_file_bytes == bhost.header_file_bytes);
                    EXPECT_TRUE(bdev.lines.size() == dev.lines.size());
                    EXPECT_TRUE(!o.sam.md || count(bdev.records, std::string("MDZ")) >= mapped);
                }
                if (flags == 0)
                    std::printf("  block %zu, mode %d, fields %d: %zu lines, %zu bytes of text\n", block, mode, fields, dev.lines.size(),
                                dev.text.size());
            }
}

int main()
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + "sim_ref_10Kb_SNP_INDELs.vcf");
    auto haps = spm::io::read_fasta(DATA + "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(ref.size() == 1 && haps.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    tree_cases(jst, haps, 0);
    tree_cases(jst, haps, 64);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
