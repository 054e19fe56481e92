// jst_collapse_cases.cpp -- journaled_sequence_tree::locate_reference_loci on the committed fixtures (tests/golden/jst): the
// alignments of a pan-genome search in reference coordinates, one record per distinct alignment.  Two routes must return the
// same vector:
//   (1) the device route (locate on the device, spm_hip_jst_alns_project, spm_hip_jst_ref_alns_collapse),
//   (2) the host route (locate_reference_host, sorted and folded on the host),
// with and without a hit_selection.  Every locus is replayed against the fixture reference, holds what locate_reference
// returns for its members, and the loci are strictly ascending.
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

// loci against the alignments they were folded from: every alignment lies in exactly one locus, with its haplotype a member
static bool covers(std::vector<spm::jst_ref_locus> const & loci, std::vector<spm::jst_ref_alignment> const & alns)
{
    std::size_t records = 0;
    for (std::size_t i = 0; i < loci.size(); ++i) {
        spm::jst_ref_locus const & l = loci[i];
        records += l.records;
        if (l.members.empty() || l.records < l.members.size())
            return false;
        std::int32_t best = l.members.front().second;
        for (std::size_t m = 0; m < l.members.size(); ++m) {
            best = std::min(best, l.members[m].second);
            if (m && l.members[m - 1].first >= l.members[m].first)
                return false;
        }
        if (best != l.haplotype_errors)
            return false;
        if (i) { // strictly ascending in (needle, begin, end, errors, CIGAR length, CIGAR words)
            spm::jst_ref_locus const & p = loci[i - 1];
            auto const kp = std::tuple{p.needle, p.aln.begin_position(), p.aln.end_position(), p.aln.errors(), p.aln.cigar().size()};
            auto const kl = std::tuple{l.needle, l.aln.begin_position(), l.aln.end_position(), l.aln.errors(), l.aln.cigar().size()};
            if (!(kp < kl || (kp == kl && p.aln.cigar() < l.aln.cigar())))
                return false;
        }
    }
    if (records != alns.size())
        return false;
    for (spm::jst_ref_alignment const & x : alns) {
        bool found = false;
        for (spm::jst_ref_locus const & l : loci)
            if (l.needle == x.needle && l.aln == x.aln) {
                for (auto const & m : l.members)
                    found = found || (m.first == x.haplotype && m.second <= x.haplotype_errors);
                break;
            }
        if (!found)
            return false;
    }
    return true;
}

// returns the number of loci that merge alignments of several haplotypes
static std::size_t collapse_case(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, int algo,
                                 std::size_t L, unsigned k, bool reports_begin, std::size_t block)
{
    std::size_t const count = 48;
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

    auto const alns = jst.locate_reference(ps, window, needles, reports_begin, block, nullptr);
    auto const dev = jst.locate_reference_loci(ps, window, needles, reports_begin, block, nullptr);
    auto const host = jst.locate_reference_loci_host(ps, window, needles, reports_begin, block, nullptr);
    EXPECT_TRUE(jst.device_ready());
    EXPECT_TRUE(!dev.empty() && dev.size() < alns.size());
    EXPECT_TRUE(dev == host);
    EXPECT_TRUE(covers(dev, alns));
    bool ok = true;
    std::size_t merged = 0;
    for (auto const & l : dev) {
        ok = ok && replays(jst.reference(), needles[l.needle], l.aln);
        merged += l.members.size() > 1;
    }
    EXPECT_TRUE(ok);

    using sel_t = spm::hip::hit_selection;
    sel_t const modes[] = {sel_t{}, sel_t{true, {}, 0u}, sel_t{true, {}, 0u, true}};
    for (sel_t const & sel : modes) {
        auto const sel_alns = jst.locate_reference(ps, window, needles, reports_begin, sel, block, nullptr);
        auto const sel_dev = jst.locate_reference_loci(ps, window, needles, reports_begin, sel, block, nullptr);
        auto const sel_host = jst.locate_reference_loci_host(ps, window, needles, reports_begin, sel, block, nullptr);
        EXPECT_TRUE(sel_dev == sel_host);
        EXPECT_TRUE(!sel_dev.empty() && sel_dev.size() <= dev.size());
        EXPECT_TRUE(covers(sel_dev, sel_alns));
        // every selected locus is a locus of the full result with a subset of its members
        bool sub = true;
        for (auto const & x : sel_dev) {
            bool found = false;
            for (auto const & l : dev)
                if (l.needle == x.needle && l.aln == x.aln) {
                    found = std::includes(l.members.begin(), l.members.end(), x.members.begin(), x.members.end());
                    break;
                }
            sub = sub && found && replays(jst.reference(), needles[x.needle], x.aln);
        }
        EXPECT_TRUE(sub);
    }
    std::printf("  algo %d |P|=%zu k=%u block %zu: %zu alignments -> %zu loci, %zu of them on several haplotypes\n", algo, L, k,
                block, alns.size(), dev.size(), merged);
    return merged;
}

static std::size_t fixture_cases(char const * vcf, char const * haplotypes)
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + vcf);
    auto expected = spm::io::read_fasta(DATA + haplotypes);
    EXPECT_TRUE(ref.size() == 1 && expected.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    std::printf("%s\n", vcf);
    std::size_t merged = 0;
    merged += collapse_case(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 0);
    merged += collapse_case(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 64); // blocks shorter than |P|
    merged += collapse_case(jst, expected, SPM_ALGO_SHIFTOR, 32, 0, true, 0);
    return merged;
}

int main()
{
    std::size_t const a = fixture_cases("sim_ref_10Kb_SNPs.vcf", "sim_ref_10Kb_SNPs_haplotypes.fasta.gz");
    std::size_t const b = fixture_cases("sim_ref_10Kb_SNP_INDELs.vcf", "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(a > 0 && b > 0);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
