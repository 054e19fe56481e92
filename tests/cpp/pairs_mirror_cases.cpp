// pairs_mirror_cases.cpp -- paired-end reads through the C++ mirror, on the committed fixtures (tests/golden/jst):
// journaled_sequence_tree::locate_pairs on the device route (the chain of locate_reads plus spm_hip_jst_ref_loci_pairs) and on
// the host route (host loci, host summary, a plain loop over all combinations) return the same loci, the same read records
// and the same pair records.  The pairs are cut from the materialised haplotypes: fragments inside and outside the allowed
// length, mate 1 on either strand, same-strand mates, a mate that maps nowhere.
#include <cstdio>
#include <string>

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
        out.push_back(static_cast<std::uint8_t>(3 - r[i])); // ACGT: the complement of rank x is 3 - x
    return out;
}

static constexpr std::size_t L = 60;
static constexpr std::uint32_t MIN_TLEN = 150, MAX_TLEN = 400;

// pair i: a fragment of a haplotype; its kind by i % 8
//   0, 1, 2: mate 1 forward, fragment 200 .. 350      3, 4: mate 1 reverse      5: fragment 700 (too long)
//   6: both mates forward      7: mate 2 is noise
static std::vector<std::vector<std::uint8_t>> cut_pairs(std::vector<spm::io::fasta_record> const & haps, std::size_t n_pairs)
{
    std::vector<std::vector<std::uint8_t>> out;
    std::uint64_t r = 0x9A125ull;
    for (std::size_t i = 0; i < n_pairs; ++i) {
        r = mix64(r + i);
        std::vector<std::uint8_t> const & hap = haps[r % haps.size()].ranks;
        std::size_t const kind = i % 8, frag = kind == 5 ? 700 : 200 + (r >> 44) % 151;
        std::size_t const at = (r >> 20) % (hap.size() - 800);
        auto const cut = [&](std::size_t from) {
            return std::vector<std::uint8_t>(hap.begin() + static_cast<std::ptrdiff_t>(from), hap.begin() + static_cast<std::ptrdiff_t>(from + L));
        };
        std::vector<std::uint8_t> left = cut(at), right = cut(at + frag - L);
        if (i % 3 == 1)
            left[7 + (r >> 50) % (L - 14)] ^= 1; // a substitution
        if (kind == 7)
            for (std::size_t j = 0; j < L; ++j)
                right[j] = static_cast<std::uint8_t>(mix64(r + 77 * j) & 3);
        if (kind == 6) {
            out.push_back(left);
            out.push_back(right);
        } else if (kind == 3 || kind == 4) {
            out.push_back(revcomp4(right));
            out.push_back(left);
        } else {
            out.push_back(left);
            out.push_back(revcomp4(right));
        }
    }
    return out;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, std::size_t block)
{
    std::size_t const n_pairs = 32, n_reads = 2 * n_pairs;
    unsigned const k = 2;
    auto const reads = cut_pairs(haps, n_pairs);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0};
    std::vector<std::uint16_t> ks(n_reads, static_cast<std::uint16_t>(k));
    std::vector<std::vector<std::uint8_t>> needles; // the 2n needles, for the host route
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
    EXPECT_TRUE(jst.device_ready());

    using sel_t = spm::hip::hit_selection;
    sel_t const modes[] = {sel_t{true, {}, 1u, true, true}, sel_t{true, {}, 0u, true, true}, sel_t{true, {}, 1u, false, true}};
    for (sel_t const & sel : modes) {
        auto const dev = jst.locate_pairs(ps, window, needles, false, static_cast<std::uint32_t>(n_reads), MIN_TLEN, MAX_TLEN, sel, block, nullptr);
        auto const host = jst.locate_pairs_host(ps, window, needles, false, static_cast<std::uint32_t>(n_reads), MIN_TLEN, MAX_TLEN, sel, block, nullptr);
        EXPECT_TRUE(!dev.mapped.loci.empty() && dev.mapped.reads.size() == n_reads && dev.pairs.size() == n_pairs);
        EXPECT_TRUE(dev.mapped.loci == host.mapped.loci);
        EXPECT_TRUE(dev.mapped.reads == host.mapped.reads);
        EXPECT_TRUE(dev.pairs == host.pairs);
        EXPECT_TRUE(dev == host);
        EXPECT_TRUE(dev.pairs == spm::journaled_sequence_tree::pairs_host(dev.mapped, MIN_TLEN, MAX_TLEN));
        std::size_t proper = 0, mate1_reverse = 0, discordant = 0, one_mate = 0, multi = 0;
        for (std::size_t p = 0; p < n_pairs; ++p) {
            spm::jst_pair const & P = dev.pairs[p];
            EXPECT_TRUE(P == host.pairs[p]);
            bool const is_proper = (P.flag1 & 2) != 0;
            EXPECT_TRUE(is_proper == (P.best >= 0) && is_proper == (P.tlen != 0) && is_proper == (P.n_best >= 1) && (P.flag2 & 2) == (P.flag1 & 2));
            EXPECT_TRUE((P.flag1 & 0xC1) == 0x41 && (P.flag2 & 0xC1) == 0x81);
            if (is_proper) {
                auto const &A = dev.mapped.loci[P.locus1], &B = dev.mapped.loci[P.locus2];
                EXPECT_TRUE(spm::hip::read_of(A.needle) == 2 * p && spm::hip::read_of(B.needle) == 2 * p + 1);
                EXPECT_TRUE(spm::hip::strand_of(A.needle) != spm::hip::strand_of(B.needle));
                auto const & fwd = spm::hip::strand_of(A.needle) ? B : A;
                auto const & rev = spm::hip::strand_of(A.needle) ? A : B;
                long const t = static_cast<long>(rev.aln.end_position()) - static_cast<long>(fwd.aln.begin_position());
                EXPECT_TRUE(t >= MIN_TLEN && t <= MAX_TLEN && P.tlen == (spm::hip::strand_of(A.needle) ? -t : t));
                EXPECT_TRUE(P.best == A.haplotype_errors + B.haplotype_errors && P.n_pairs >= P.n_best + P.n_next);
                ++proper;
                mate1_reverse += P.tlen < 0;
                multi += P.n_pairs > 1;
            } else {
                EXPECT_TRUE(P.locus1 == dev.mapped.reads[2 * p].primary && P.locus2 == dev.mapped.reads[2 * p + 1].primary && P.n_pairs == 0);
                bool const un1 = (P.flag1 & 4) != 0, un2 = (P.flag1 & 8) != 0;
                discordant += !un1 && !un2;
                one_mate += un1 != un2;
            }
            if (p % 8 <= 4) // a fragment of 200 .. 350 haplotype symbols: proper on the reference too (the indels are short)
                EXPECT_TRUE(is_proper && (P.tlen < 0) == (p % 8 >= 3));
            else
                EXPECT_TRUE(!is_proper);
        }
        EXPECT_TRUE(proper >= 20 && mate1_reverse >= 8 && discordant >= 8 && one_mate >= 4);
        std::printf("  block %zu, strata %u%s: %zu loci, %zu of %zu pairs proper (%zu with mate 1 in reverse, %zu with several "
                    "combinations), %zu discordant, %zu with one mate\n", block, *sel.strata, sel.across ? " across" : "",
                    dev.mapped.loci.size(), proper, n_pairs, mate1_reverse, multi, discordant, one_mate);
    }
    // a window that nothing fits: the primaries
    sel_t const sel{true, {}, 0u, true, true};
    auto const none = jst.locate_pairs(ps, window, needles, false, static_cast<std::uint32_t>(n_reads), 1, 50, sel, block, nullptr);
    auto const none_host = jst.locate_pairs_host(ps, window, needles, false, static_cast<std::uint32_t>(n_reads), 1, 50, sel, block, nullptr);
    EXPECT_TRUE(none == none_host);
    for (std::size_t p = 0; p < n_pairs; ++p)
        EXPECT_TRUE((none.pairs[p].flag1 & 2) == 0 && none.pairs[p].tlen == 0 && none.pairs[p].locus1 == none.mapped.reads[2 * p].primary);
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
