// strands_mirror_cases.cpp -- reads on both strands through the C++ mirror, on the committed fixtures (tests/golden/jst):
//   * journaled_sequence_tree::locate_reads: the device route (the normalised-loci chain plus spm_hip_jst_ref_loci_reads) and
//     the host route (host loci plus a plain loop) return the same loci and the same read records, under
//     hit_selection::strands with and without across; journaled_sequence_tree::search with that selection likewise;
//   * batch_matcher{both_strands, reads, k} fires the callbacks of a batch_matcher over the explicit 2n needles;
//   * hip::reverse_complement on the three alphabets.
#include <cstdio>
#include <string>
#include <tuple>

#include <libspm/jst/journaled_sequence_tree.hpp>
#include <libspm/matcher/hip_batch.hpp>

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

// the complement by letter, written out again
static std::vector<std::uint8_t> revcomp4(std::vector<std::uint8_t> const & r)
{
    std::string const letters = "ACGT", complement = "TGCA";
    std::vector<std::uint8_t> out;
    for (std::size_t i = r.size(); i-- > 0;)
        out.push_back(static_cast<std::uint8_t>(letters.find(complement[r[i]])));
    return out;
}

// `count` reads of length L cut from the fixture haplotypes, one in three with a substitution; every odd one reverse-complemented
static std::vector<std::vector<std::uint8_t>> cut_reads(std::vector<spm::io::fasta_record> const & haps, std::size_t L, std::size_t count)
{
    std::vector<std::vector<std::uint8_t>> out;
    std::uint64_t r = 0x57A4D5ull;
    for (std::size_t i = 0; i < count; ++i) {
        r = mix64(r + i);
        std::vector<std::uint8_t> const & hap = haps[r % haps.size()].ranks;
        std::size_t const at = (r >> 20) % (hap.size() - L - 8);
        std::vector<std::uint8_t> nd(hap.begin() + static_cast<std::ptrdiff_t>(at), hap.begin() + static_cast<std::ptrdiff_t>(at + L));
        if (i % 3 == 2)
            nd[5 + (r >> 40) % (L - 10)] ^= 1;
        out.push_back(i % 2 ? revcomp4(nd) : nd);
    }
    return out;
}

static void reverse_complement_cases()
{
    using namespace spm::literals;
    EXPECT_TRUE(spm::hip::reverse_complement("AACGT"_dna4) == "ACGTT"_dna4);
    EXPECT_TRUE(spm::hip::reverse_complement("ANCGT"_dna5) == "ACGNT"_dna5);
    EXPECT_TRUE(spm::hip::reverse_complement("ABCDGHKMNRSTVWY"_dna15) == "RWBASYNKMDCHGVT"_dna15);
    EXPECT_TRUE(spm::hip::reverse_complement(spm::hip::reverse_complement("GATTACA"_dna4)) == "GATTACA"_dna4);
    EXPECT_TRUE(spm::hip::read_of(7) == 3 && spm::hip::strand_of(7) == 1 && spm::hip::read_of(6) == 3 && spm::hip::strand_of(6) == 0);
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, std::size_t block)
{
    std::size_t const L = 60, n_reads = 32;
    unsigned const k = 2;
    auto const reads = cut_reads(haps, L, n_reads);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0};
    std::vector<std::uint16_t> ks(n_reads, static_cast<std::uint16_t>(k));
    std::vector<std::vector<std::uint8_t>> needles; // the 2n needles, for the host route
    std::vector<std::uint32_t> needle_len;
    for (auto const & rd : reads) {
        cat.insert(cat.end(), rd.begin(), rd.end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
        needles.push_back(rd);
        needles.push_back(revcomp4(rd));
        needle_len.insert(needle_len.end(), 2, static_cast<std::uint32_t>(L));
    }
    spm_ctx * ctx = spm::hip::default_context();
    spm_patterns * ps = nullptr;
    if (spm_hip_patterns_create_stranded(ctx, SPM_ALGO_MYERS, cat.data(), off.data(), static_cast<std::uint32_t>(n_reads), ks.data(), 4,
                                         &ps) != SPM_OK)
        spm::hip::fatal("spm_hip_patterns_create_stranded", ctx);
    spm::hip::patterns_ptr compiled{ps, spm::hip::patterns_deleter{}};
    EXPECT_TRUE(spm_hip_patterns_strands(ps) == 2 && spm_hip_patterns_count(ps) == 2 * n_reads);
    for (std::uint32_t p = 0; p < 2 * n_reads; ++p) {
        std::vector<std::uint8_t> got(L);
        std::uint32_t len = 0;
        EXPECT_TRUE(spm_hip_patterns_needle(ps, p, got.data(), static_cast<std::uint32_t>(L), &len) == SPM_OK && len == L && got == needles[p]);
    }
    std::size_t const window = L + k;
    EXPECT_TRUE(jst.device_ready());

    using sel_t = spm::hip::hit_selection;
    sel_t const modes[] = {sel_t{true, {}, 0u, true, true}, sel_t{true, {}, 0u, false, true}, sel_t{true, {}, 1u, true, true}};
    sel_t const unstranded{true, {}, 0u, true, false};
    for (sel_t const & sel : modes) {
        auto const dev_hits = jst.search_device(ps, window, sel, block, nullptr);
        auto const host_hits = spm::journaled_sequence_tree::select_host(jst.search_host(ps, window, needle_len, false, block, nullptr),
                                                                        ps, needle_len, false, sel);
        EXPECT_TRUE(!dev_hits.empty() && dev_hits == host_hits);
        auto const dev = jst.locate_reads(ps, window, needles, false, 2, static_cast<std::uint32_t>(n_reads), sel, block, nullptr);
        auto const host = jst.locate_reads_host(ps, window, needles, false, 2, static_cast<std::uint32_t>(n_reads), sel, block, nullptr);
        EXPECT_TRUE(!dev.loci.empty() && dev.reads.size() == n_reads);
        EXPECT_TRUE(dev.loci == host.loci);
        EXPECT_TRUE(dev.reads == host.reads);
        EXPECT_TRUE(dev.reads == spm::journaled_sequence_tree::reads_host(dev.loci, 2, static_cast<std::uint32_t>(n_reads)));
        std::size_t mapped = 0, reverse_primary = 0, forward_primary = 0, n_loci = 0;
        for (std::size_t r = 0; r < dev.reads.size(); ++r) {
            spm::jst_read const & R = dev.reads[r];
            n_loci += R.n_loci;
            if (R.n_loci == 0)
                continue;
            ++mapped;
            EXPECT_TRUE(R.primary >= R.first_locus && R.primary < R.first_locus + R.n_loci && R.n_best >= 1);
            EXPECT_TRUE(spm::hip::read_of(dev.loci[R.primary].needle) == r && dev.loci[R.primary].haplotype_errors == R.best);
            (spm::hip::strand_of(dev.loci[R.primary].needle) ? reverse_primary : forward_primary) += 1;
        }
        EXPECT_TRUE(n_loci == dev.loci.size() && mapped >= n_reads - 2);
        EXPECT_TRUE(reverse_primary >= n_reads / 2 - 2 && forward_primary >= n_reads / 2 - 2); // the odd reads map in reverse
        std::printf("  block %zu, strata %u%s: %zu hits, %zu loci, %zu of %zu reads mapped, %zu primaries in reverse\n", block,
                    *sel.strata, sel.across ? " across" : "", dev_hits.size(), dev.loci.size(), mapped, n_reads, reverse_primary);
    }
    // the plain summary of the same needles as 2n reads on one strand
    auto const plain = jst.locate_reads(ps, window, needles, false, 1, static_cast<std::uint32_t>(2 * n_reads), unstranded, block, nullptr);
    auto const plain_host = jst.locate_reads_host(ps, window, needles, false, 1, static_cast<std::uint32_t>(2 * n_reads), unstranded, block, nullptr);
    EXPECT_TRUE(plain.reads.size() == 2 * n_reads && plain.loci == plain_host.loci && plain.reads == plain_host.reads);
}

static void batch_cases(std::vector<spm::io::fasta_record> const & haps)
{
    std::size_t const n_reads = 24;
    auto const reads = cut_reads(haps, 40, n_reads);
    auto const as_dna4 = [](std::vector<std::uint8_t> const & r) {
        std::vector<spm::dna4> v;
        for (std::uint8_t x : r)
            v.emplace_back(x);
        return v;
    };
    std::vector<std::vector<spm::dna4>> rd, both;
    std::vector<std::uint16_t> ks, ks2;
    for (std::size_t i = 0; i < n_reads; ++i) {
        rd.push_back(as_dna4(reads[i]));
        both.push_back(rd.back());
        both.push_back(spm::hip::reverse_complement(rd.back()));
        EXPECT_TRUE(both.back() == as_dna4(revcomp4(reads[i])));
        ks.push_back(static_cast<std::uint16_t>(i % 3));
        ks2.insert(ks2.end(), 2, ks.back());
    }
    spm::batch_myers_matcher stranded{spm::hip::both_strands, rd, ks};
    spm::batch_myers_matcher explicit_set{both, ks2};
    EXPECT_TRUE(stranded.size() == 2 * n_reads && explicit_set.size() == 2 * n_reads);
    EXPECT_TRUE(spm::window_size(stranded) == spm::window_size(explicit_set));
    std::vector<spm::dna4> const haystack = as_dna4(haps[3].ranks);
    using row = std::tuple<std::size_t, std::size_t, std::size_t, int>;
    std::vector<row> a, b, c;
    stranded(haystack, [&](std::size_t p, spm::finder const & f) { a.emplace_back(p, f.begin_position(), f.end_position(), f.errors()); });
    explicit_set(haystack, [&](std::size_t p, spm::finder const & f) { b.emplace_back(p, f.begin_position(), f.end_position(), f.errors()); });
    EXPECT_TRUE(!a.empty() && a == b);
    std::size_t reverse = 0;
    for (row const & x : a)
        reverse += spm::hip::strand_of(std::get<0>(x));
    EXPECT_TRUE(reverse > 0 && reverse < a.size());
    // the best stratum per read: a subset, and no read keeps a hit worse than its best on either strand
    spm::hip::hit_selection const sel{true, {}, 0u, false, true};
    stranded(haystack, [&](std::size_t p, spm::finder const & f) { c.emplace_back(p, f.begin_position(), f.end_position(), f.errors()); }, sel);
    EXPECT_TRUE(!c.empty() && c.size() < a.size());
    std::vector<int> best(n_reads, 1 << 30);
    for (row const & x : a)
        best[spm::hip::read_of(std::get<0>(x))] = std::min(best[spm::hip::read_of(std::get<0>(x))], std::get<3>(x));
    bool ok = true;
    for (row const & x : c)
        ok = ok && std::get<3>(x) == best[spm::hip::read_of(std::get<0>(x))];
    EXPECT_TRUE(ok);
    std::printf("  batch: %zu callbacks on both strands (%zu in reverse), %zu in the best stratum per read\n", a.size(), reverse, c.size());
}

int main()
{
    reverse_complement_cases();
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + "sim_ref_10Kb_SNP_INDELs.vcf");
    auto haps = spm::io::read_fasta(DATA + "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(ref.size() == 1 && haps.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    tree_cases(jst, haps, 0);
    tree_cases(jst, haps, 64);
    batch_cases(haps);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
