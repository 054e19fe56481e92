// jst_bam_vcf_cases.cpp -- variant calls through the C++ mirror, on the committed fixtures (tests/golden/jst):
// journaled_sequence_tree::map_bam with jst_bam_options::call_variants by the device route (spm_hip_pileup_sites and
// spm_hip_pileup_sites_vcf behind the BAM call, the sort, the duplicate marks and the pileup) returns the text and the call
// records of the host route (the host twins over the host's own counts) and of the host twins called here over the mirror's own
// pileup; every call record names its line.  The reads are cut as jst_bam_pileup_cases.cpp cuts them.  With the argument
// "fatal" the program asks the host route's converter, which needs no device, for call_variants without pileup: that ends it.
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
            o.mark_duplicates = marked;
            o.pileup = true;
            spm::jst_sam_pairing const & pairing = mode == 0 ? single : rescued;
            spm::jst_bam const plain = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            o.call_variants = true;
            o.sample = marked ? "s" : "sample_1";
            spm::jst_bam const dev = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            spm::jst_bam const host = jst.map_bam_host(ps, window, needles, false, 2, nr, pairing, o, sel, 0, nullptr);
            EXPECT_TRUE(plain.vcf.empty() && plain.calls.empty());
            EXPECT_TRUE(dev.vcf == host.vcf);
            EXPECT_TRUE(dev.calls == host.calls);
            EXPECT_TRUE(dev == host);
            EXPECT_TRUE(dev.file == plain.file && dev.records == plain.records && dev.lines == plain.lines && dev.pileup == plain.pileup);
            // the host twins over the mirror's own pileup
            std::vector<spm_pileup_site> sites(ref_len);
            std::uint64_t n_sites = 0, n_text = 0, n_head = 0;
            EXPECT_TRUE(spm_hip_pileup_sites_host(dev.pileup.data(), 0, ref_len, jst.reference().data(), ref_len, nullptr, sites.data(), sites.size(),
                                                  &n_sites) == SPM_OK);
            std::string own(dev.vcf.size() + 1, '\7');
            EXPECT_TRUE(spm_hip_pileup_sites_vcf_host(sites.data(), n_sites, o.sam.rname.c_str(), o.sample.c_str(), ref_len, nullptr, own.data(),
                                                      own.size(), &n_text) == SPM_OK);
            EXPECT_TRUE(n_text == dev.vcf.size() && own.compare(0, n_text, dev.vcf) == 0);
            EXPECT_TRUE(spm_hip_vcf_header(o.sam.rname.c_str(), o.sample.c_str(), ref_len, nullptr, 0, &n_head) == SPM_E_OVERFLOW);
            // every call record names its line: the lines in site order, back to back behind the header
            std::uint64_t at = n_head;
            std::size_t n_lines = 0;
            bool named = dev.calls.size() == n_sites;
            for (std::size_t i = 0; i < dev.calls.size() && named; ++i) {
                spm::jst_variant_call const & c = dev.calls[i];
                named = c.pos == sites[i].pos && c.depth == sites[i].depth && c.offset == at && (c.len != 0) == (c.status == SPM_CALL_VARIANT);
                if (named && c.len) {
                    std::string const line = dev.vcf.substr(c.offset, c.len);
                    named = line.rfind("sim_ref\t" + std::to_string(c.pos + 1) + "\t.\t", 0) == 0 && line.back() == '\n' &&
                            std::count(line.begin(), line.end(), '\n') == 1;
                    ++n_lines;
                }
                at += c.len;
            }
            EXPECT_TRUE(named && at == dev.vcf.size());
            EXPECT_TRUE(marked || (n_sites >= 1 && n_lines >= 1)); // the repeated pairs show every departure twice where they are not marked
            std::printf("  mode %d, marked %d: %zu records, %llu sites, %zu lines, %zu bytes\n", mode, marked ? 1 : 0, dev.lines.size(),
                        static_cast<unsigned long long>(n_sites), n_lines, dev.vcf.size());
        }
}

int main(int argc, char ** argv)
{
    if (argc > 1 && std::string(argv[1]) == "fatal") { // host only: no context is made, no device is opened
        spm::jst_bam_options o;
        o.sam.rname = "sim_ref";
        o.ref_len = 100;
        o.sort = true;
        o.call_variants = true;
        (void)spm::journaled_sequence_tree::bam_of_sam(spm::jst_sam{}, o);
        std::printf("call_variants without pileup was taken\n");
        return 0;
    }
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + "sim_ref_10Kb_SNP_INDELs.vcf");
    auto haps = spm::io::read_fasta(DATA + "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(ref.size() == 1 && haps.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    tree_cases(jst, haps);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
