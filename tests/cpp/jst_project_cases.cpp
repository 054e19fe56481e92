// jst_project_cases.cpp -- journaled_sequence_tree::locate_reference on the committed fixtures (tests/golden/jst): the
// alignments of a pan-genome search in the coordinates of the reference.  Two routes must return the same vector:
//   (1) the device route (locate_device followed by spm_hip_jst_alns_project: one projection per shared transcript),
//   (2) the host route (locate_host, projected on the host through the event table of every haplotype),
// with and without a hit_selection.  Every alignment is replayed against the fixture reference: it consumes exactly the needle
// and ref[begin, end), = / X agree with the symbols, runs are merged, cost = errors.
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

// returns the number of alignments whose projected transcript differs from the haplotype one
static std::size_t project_case(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, int algo,
                                std::size_t L, unsigned k, bool reports_begin, std::size_t block)
{
    std::size_t const count = 48;
    auto const needles = cut_needles(haps, L, k > 0, count);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0}, lens;
    std::vector<std::uint16_t> ks(count, static_cast<std::uint16_t>(k));
    for (std::size_t p = 0; p < count; ++p) {
        cat.insert(cat.end(), needles[p].begin(), needles[p].end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
        lens.push_back(static_cast<std::uint32_t>(needles[p].size()));
    }
    spm_ctx * ctx = spm::hip::default_context();
    spm_patterns * ps = nullptr;
    if (spm_hip_patterns_create(ctx, algo, cat.data(), off.data(), static_cast<std::uint32_t>(count), ks.data(), 4, &ps) != SPM_OK)
        spm::hip::fatal("spm_hip_patterns_create", ctx);
    spm::hip::patterns_ptr compiled{ps, spm::hip::patterns_deleter{}};
    std::size_t const window = L + k;
    std::size_t changed = 0;

    auto const located = jst.locate(ps, window, lens, reports_begin, block, nullptr);
    auto const dev = jst.locate_reference(ps, window, needles, reports_begin, block, nullptr);
    auto const host = jst.locate_reference_host(ps, window, needles, reports_begin, block, nullptr);
    EXPECT_TRUE(jst.device_ready());
    EXPECT_TRUE(dev.size() >= count && dev.size() == located.size());
    EXPECT_TRUE(dev == host);
    bool ok = dev.size() == located.size();
    for (std::size_t i = 0; ok && i < dev.size(); ++i) {
        ok = dev[i].haplotype == located[i].haplotype && dev[i].needle == located[i].needle &&
             dev[i].haplotype_errors == located[i].aln.errors() && replays(jst.reference(), needles[dev[i].needle], dev[i].aln);
        changed += dev[i].aln.cigar() != located[i].aln.cigar();
    }
    EXPECT_TRUE(ok);

    using sel_t = spm::hip::hit_selection;
    sel_t const modes[] = {sel_t{}, sel_t{true, {}, 0u}, sel_t{true, {}, 0u, true}};
    for (sel_t const & sel : modes) {
        auto const sel_loc = jst.locate(ps, window, lens, reports_begin, sel, block, nullptr);
        auto const sel_dev = jst.locate_reference(ps, window, needles, reports_begin, sel, block, nullptr);
        auto const sel_host = jst.locate_reference_host(ps, window, needles, reports_begin, sel, block, nullptr);
        EXPECT_TRUE(sel_dev == sel_host);
        EXPECT_TRUE(!sel_dev.empty() && sel_dev.size() <= dev.size() && sel_dev.size() == sel_loc.size());
        // every selected projection is the projection of that record in the full result
        bool sub = true;
        std::size_t at = 0;
        if (!sel.across)
            for (auto const & x : sel_dev) {
                while (at < dev.size() && !(dev[at] == x))
                    ++at;
                sub = sub && at < dev.size();
            }
        for (auto const & x : sel_dev)
            sub = sub && replays(jst.reference(), needles[x.needle], x.aln);
        EXPECT_TRUE(sub);
    }
    std::printf("  algo %d |P|=%zu k=%u block %zu: %zu alignments, %zu projected transcripts differ from the haplotype's\n", algo, L,
                k, block, dev.size(), changed);
    return changed;
}

static std::size_t fixture_cases(char const * vcf, char const * haplotypes)
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + vcf);
    auto expected = spm::io::read_fasta(DATA + haplotypes);
    EXPECT_TRUE(ref.size() == 1 && expected.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    std::printf("%s\n", vcf);
    std::size_t changed = 0;
    changed += project_case(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 0);
    changed += project_case(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 64); // blocks shorter than |P|
    changed += project_case(jst, expected, SPM_ALGO_SHIFTOR, 32, 0, true, 0);
    return changed;
}

int main()
{
    std::size_t const a = fixture_cases("sim_ref_10Kb_SNPs.vcf", "sim_ref_10Kb_SNPs_haplotypes.fasta.gz");
    std::size_t const b = fixture_cases("sim_ref_10Kb_SNP_INDELs.vcf", "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(a > 0 && b > 0);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
