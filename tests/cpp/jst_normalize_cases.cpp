// jst_normalize_cases.cpp -- journaled_sequence_tree::locate_reference_normalized and locate_reference_loci_normalized on the
// committed fixtures (tests/golden/jst): the alignments of a pan-genome search in reference coordinates with every indel at its
// leftmost equivalent place, and their loci.  Two routes must return the same vector:
//   (1) the device route (locate on the device, spm_hip_jst_alns_project, spm_hip_jst_ref_alns_normalize, and for the loci
//       spm_hip_jst_ref_alns_collapse),
//   (2) the host route (locate_reference_host through normalize_host, the rule in column form, folded by collapse_host),
// with and without a hit_selection.  Every alignment is replayed against the fixture reference and keeps range, errors and
// haplotype of the alignment locate_reference returns in its place.
#include <cstdio>
#include <set>
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

// `count` needles of length L cut from the fixture haplotypes; with `edits` two of three carry a deletion or a substitution
static std::vector<std::vector<std::uint8_t>> cut_needles(std::vector<spm::io::fasta_record> const & haps, std::size_t L,
                                                          bool edits, std::size_t count)
{
    std::vector<std::vector<std::uint8_t>> out;
    std::uint64_t r = 0x5EED0C35ull;
    for (std::size_t i = 0; i < count; ++i) {
        r = mix64(r + i);
        std::vector<std::uint8_t> const & hap = haps[r % haps.size()].ranks;
        std::size_t const at = (r >> 20) % (hap.size() - L - 8);
        std::vector<std::uint8_t> nd(hap.begin() + static_cast<std::ptrdiff_t>(at), hap.begin() + static_cast<std::ptrdiff_t>(at + L + 1));
        if (edits && i % 3 == 1)
            nd.erase(nd.begin() + static_cast<std::ptrdiff_t>(5 + (r >> 40) % (L - 10)));
        if (edits && i % 3 == 2)
            nd[5 + (r >> 40) % (L - 10)] ^= 1;
        nd.resize(L);
        out.push_back(std::move(nd));
    }
    return out;
}

static bool replays(std::vector<std::uint8_t> const & ref, std::vector<std::uint8_t> const & P, spm::alignment const & a)
{
    std::size_t i = 0, j = a.begin_position();
    long cost = 0;
    std::uint32_t prev = 0;
    for (std::uint32_t const w : a.cigar()) {
        std::uint32_t const op = w & 15u, n = w >> 4;
        if (n == 0 || op == prev)
            return false;
        prev = op;
        for (std::uint32_t c = 0; c < n; ++c) {
            if (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X) {
                if (i >= P.size() || j >= a.end_position() || (P[i] == ref[j]) != (op == SPM_CIGAR_EQ))
                    return false;
                ++i, ++j;
            } else if (op == SPM_CIGAR_INS)
                ++i;
            else if (op == SPM_CIGAR_DEL)
                ++j;
            else
                return false;
            cost += op != SPM_CIGAR_EQ;
        }
    }
    return i == P.size() && j == a.end_position() && cost == a.errors();
}

// what normalisation may not touch: record i of the normalised vector is record i of the plain one but for its CIGAR
static bool same_but_cigar(std::vector<spm::jst_ref_alignment> const & a, std::vector<spm::jst_ref_alignment> const & b)
{
    if (a.size() != b.size())
        return false;
    for (std::size_t i = 0; i < a.size(); ++i)
        if (a[i].haplotype != b[i].haplotype || a[i].needle != b[i].needle || a[i].haplotype_errors != b[i].haplotype_errors ||
            a[i].aln.begin_position() != b[i].aln.begin_position() || a[i].aln.end_position() != b[i].aln.end_position() ||
            a[i].aln.errors() != b[i].aln.errors())
            return false;
    return true;
}

struct shown
{
    std::size_t changed = 0, merged = 0;
};

static shown normalize_case(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, int algo,
                            std::size_t L, unsigned k, bool reports_begin, std::size_t block)
{
    std::size_t const count = 64;
    auto const needles = cut_needles(haps, L, k > 0, count);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0};
    std::vector<std::uint16_t> ks(count, static_cast<std::uint16_t>(k));
    for (std::size_t p = 0; p < count; ++p) {
        cat.insert(cat.end(), needles[p].begin(), needles[p].end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
    }
    spm_ctx * ctx = spm::hip::default_context();
    spm_patterns * ps = nullptr;
    if (spm_hip_patterns_create(ctx, algo, cat.data(), off.data(), static_cast<std::uint32_t>(count), ks.data(), 4, &ps) != SPM_OK)
        spm::hip::fatal("spm_hip_patterns_create", ctx);
    spm::hip::patterns_ptr compiled{ps, spm::hip::patterns_deleter{}};
    std::size_t const window = L + k;
    EXPECT_TRUE(jst.device_ready());

    shown S;
    auto const plain = jst.locate_reference(ps, window, needles, reports_begin, block, nullptr);
    auto const dev = jst.locate_reference_normalized(ps, window, needles, reports_begin, block, nullptr);
    auto const host = jst.locate_reference_normalized_host(ps, window, needles, reports_begin, block, nullptr);
    EXPECT_TRUE(!dev.empty() && dev == host);
    EXPECT_TRUE(same_but_cigar(dev, plain));
    bool ok = true;
    for (std::size_t i = 0; i < dev.size(); ++i) {
        ok = ok && replays(jst.reference(), needles[dev[i].needle], dev[i].aln);
        S.changed += i < plain.size() && !(dev[i].aln == plain[i].aln);
    }
    EXPECT_TRUE(ok);
    // normalising the normalised alignments changes nothing
    EXPECT_TRUE(spm::journaled_sequence_tree::normalize_host(dev, needles, jst.reference()) == dev);

    auto const loci_plain = jst.locate_reference_loci(ps, window, needles, reports_begin, block, nullptr);
    auto const loci_dev = jst.locate_reference_loci_normalized(ps, window, needles, reports_begin, block, nullptr);
    auto const loci_host = jst.locate_reference_loci_normalized_host(ps, window, needles, reports_begin, block, nullptr);
    EXPECT_TRUE(!loci_dev.empty() && loci_dev == loci_host);
    EXPECT_TRUE(loci_dev == spm::journaled_sequence_tree::collapse_host(dev));
    EXPECT_TRUE(loci_dev.size() <= loci_plain.size());
    S.merged = loci_plain.size() - std::min(loci_plain.size(), loci_dev.size());

    using sel_t = spm::hip::hit_selection;
    sel_t const modes[] = {sel_t{}, sel_t{true, {}, 0u}, sel_t{true, {}, 0u, true}};
    for (sel_t const & sel : modes) {
        auto const sel_plain = jst.locate_reference(ps, window, needles, reports_begin, sel, block, nullptr);
        auto const sel_dev = jst.locate_reference_normalized(ps, window, needles, reports_begin, sel, block, nullptr);
        auto const sel_host = jst.locate_reference_normalized_host(ps, window, needles, reports_begin, sel, block, nullptr);
        EXPECT_TRUE(!sel_dev.empty() && sel_dev == sel_host);
        EXPECT_TRUE(same_but_cigar(sel_dev, sel_plain));
        bool sel_ok = true;
        for (auto const & x : sel_dev)
            sel_ok = sel_ok && replays(jst.reference(), needles[x.needle], x.aln);
        EXPECT_TRUE(sel_ok);
        auto const sel_loci = jst.locate_reference_loci_normalized(ps, window, needles, reports_begin, sel, block, nullptr);
        auto const sel_loci_host = jst.locate_reference_loci_normalized_host(ps, window, needles, reports_begin, sel, block, nullptr);
        EXPECT_TRUE(!sel_loci.empty() && sel_loci == sel_loci_host);
        EXPECT_TRUE(sel_loci == spm::journaled_sequence_tree::collapse_host(sel_dev));
    }
    std::printf("  algo %d |P|=%zu k=%u block %zu: %zu alignments, %zu transcripts changed; %zu loci -> %zu, %zu merged\n", algo, L,
                k, block, dev.size(), S.changed, loci_plain.size(), loci_dev.size(), S.merged);
    return S;
}

static shown fixture_cases(char const * vcf, char const * haplotypes, bool all)
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + vcf);
    auto expected = spm::io::read_fasta(DATA + haplotypes);
    EXPECT_TRUE(ref.size() == 1 && expected.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    std::printf("%s\n", vcf);
    shown S = normalize_case(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 0);
    if (all) {
        shown const b = normalize_case(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 64); // blocks shorter than |P|
        shown const c = normalize_case(jst, expected, SPM_ALGO_SHIFTOR, 32, 0, true, 0);
        S.changed += b.changed + c.changed;
        S.merged += b.merged + c.merged;
    }
    std::printf("  fixture: %zu transcripts changed, %zu loci merged\n", S.changed, S.merged);
    return S;
}

int main()
{
    shown const a = fixture_cases("sim_ref_10Kb_SNPs.vcf", "sim_ref_10Kb_SNPs_haplotypes.fasta.gz", false);
    shown const b = fixture_cases("sim_ref_10Kb_SNP_INDELs.vcf", "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz", true);
    EXPECT_TRUE(a.changed + b.changed > 0);
    EXPECT_TRUE(a.merged + b.merged > 0);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
