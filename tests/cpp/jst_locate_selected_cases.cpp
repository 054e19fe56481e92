// jst_locate_selected_cases.cpp -- journaled_sequence_tree::locate(..., hip::hit_selection) on the committed fixtures
// (tests/golden/jst): begin, end, errors and CIGAR transcript of the SELECTED hits of a pan-genome search.  Three routes must
// return the same vector:
//   (1) the device route (spm_hip_jst_search + spm_hip_jst_hits_select + spm_hip_jst_selection_align: the kept records are
//       located in the tree's index, their distinct segment hits aligned once),
//   (2) the host route (locate_host filtered to what select_host keeps),
//   (3) batch_matcher::locate(haystack, callback, selection) on every haplotype of the fixture FASTA, spelled out -- the
//       route without the tree (not for `across`, which no single haplotype can answer: there (1) == (2), and the result is
//       the per-haplotype result filtered by the needle's minimum over all haplotypes).
#include <cstdio>
#include <map>
#include <string>

#include <libspm/jst/journaled_sequence_tree.hpp>
#include <libspm/matcher/hip_batch.hpp>
#include <libspm/seqan/alphabet.hpp>

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

// `count` needles of length L cut from the fixture haplotypes; with `edits` two of three carry a deletion or a substitution,
// so that begins move away from end - |P| and every occurrence comes back as a cluster of ends
static std::vector<std::vector<std::uint8_t>> cut_needles(std::vector<spm::io::fasta_record> const & haps, std::size_t L,
                                                          bool edits, std::size_t count)
{
    std::vector<std::vector<std::uint8_t>> out;
    std::uint64_t r = 0x5EED0C33ull;
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

template <typename batch_t>
static void locate_case(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, int algo,
                        std::size_t L, unsigned k, bool reports_begin, std::size_t block)
{
    std::size_t const count = 48;
    auto const needles = cut_needles(haps, L, k > 0, count);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0}, lens;
    std::vector<std::uint16_t> ks(count, static_cast<std::uint16_t>(k));
    std::vector<std::vector<spm::dna4>> typed(count);
    for (std::size_t p = 0; p < count; ++p) {
        cat.insert(cat.end(), needles[p].begin(), needles[p].end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
        lens.push_back(static_cast<std::uint32_t>(needles[p].size()));
        typed[p].resize(needles[p].size());
        for (std::size_t i = 0; i < needles[p].size(); ++i)
            typed[p][i].assign_rank(needles[p][i]);
    }
    spm_ctx * ctx = spm::hip::default_context();
    spm_patterns * ps = nullptr;
    if (spm_hip_patterns_create(ctx, algo, cat.data(), off.data(), static_cast<std::uint32_t>(count), ks.data(), 4, &ps) != SPM_OK)
        spm::hip::fatal("spm_hip_patterns_create", ctx);
    spm::hip::patterns_ptr compiled{ps, spm::hip::patterns_deleter{}};
    std::size_t const window = L + k;
    batch_t batch{typed, k};

    auto const all = jst.locate(ps, window, lens, reports_begin, block, nullptr);
    EXPECT_TRUE(jst.device_ready());
    EXPECT_TRUE(all.size() >= count);

    using sel_t = spm::hip::hit_selection;
    sel_t const modes[] = {sel_t{}, sel_t{true, {}, 0u}, sel_t{false, {}, {}}, sel_t{true, 2u, {}}};
    for (sel_t const & sel : modes) {
        auto const dev = jst.locate(ps, window, lens, reports_begin, sel, block, nullptr);
        auto const host = jst.locate_selected_host(ps, window, lens, reports_begin, sel, block, nullptr);
        std::vector<spm::jst_alignment> want;
        for (std::size_t h = 0; h < haps.size(); ++h) {
            std::vector<spm::dna4> text(haps[h].ranks.size());
            for (std::size_t i = 0; i < text.size(); ++i)
                text[i].assign_rank(haps[h].ranks[i]);
            batch.locate(text, [&](std::size_t needle, auto const &, spm::alignment const & a) {
                want.push_back({static_cast<std::uint32_t>(h), static_cast<std::uint32_t>(needle), a});
            }, sel);
        }
        spm::journaled_sequence_tree::sort_alignments(want, reports_begin);
        // ... and the hits of search(..., selection) are the same records without begin and transcript
        auto const hits = jst.search(ps, window, lens, reports_begin, sel, block, nullptr);
        bool same_hits = hits.size() == dev.size();
        for (std::size_t i = 0; same_hits && i < hits.size(); ++i)
            same_hits = hits[i].haplotype == dev[i].haplotype && hits[i].needle == dev[i].needle &&
                        hits[i].errors == dev[i].aln.errors() &&
                        hits[i].position == (reports_begin ? dev[i].aln.begin_position() : dev[i].aln.end_position());
        std::size_t moved = 0;
        for (auto const & x : dev)
            moved += x.aln.begin_position() + L != x.aln.end_position();
        std::printf("  algo %d |P|=%zu k=%u block %zu loci %d window %ld strata %ld: %zu of %zu alignments, %zu moved begins\n",
                    algo, L, k, block, int(sel.loci), sel.window ? long(*sel.window) : -1L, sel.strata ? long(*sel.strata) : -1L,
                    dev.size(), all.size(), moved);
        EXPECT_TRUE(dev == want);
        EXPECT_TRUE(host == want);
        EXPECT_TRUE(same_hits);
        bool const keeps_all = (!sel.loci && !sel.strata) || (k == 0 && !(sel.loci && sel.window));
        if (keeps_all)
            EXPECT_TRUE(dev == all);
        else
            EXPECT_TRUE((k > 0 ? dev.size() < all.size() : dev.size() <= all.size()) && dev.size() >= count);
        if (k > 0)
            EXPECT_TRUE(moved > 0);
    }
    for (std::uint32_t strata : {0u, 1u}) {
        sel_t const sel{true, {}, strata, true};
        auto const dev = jst.locate(ps, window, lens, reports_begin, sel, block, nullptr);
        auto const host = jst.locate_selected_host(ps, window, lens, reports_begin, sel, block, nullptr);
        EXPECT_TRUE(dev == host);
        std::map<std::uint32_t, std::int64_t> best;
        for (auto const & x : all)
            best[x.needle] = best.count(x.needle) ? std::min<std::int64_t>(best[x.needle], x.aln.errors()) : x.aln.errors();
        auto loci = jst.locate(ps, window, lens, reports_begin, sel_t{}, block, nullptr);
        std::erase_if(loci, [&](spm::jst_alignment const & x) {
            return static_cast<std::int64_t>(x.aln.errors()) > best[x.needle] + static_cast<std::int64_t>(strata);
        });
        EXPECT_TRUE(dev == loci);
        EXPECT_TRUE(dev.size() >= best.size());
        std::printf("  across strata %u: %zu alignments\n", strata, dev.size());
    }
}

static void fixture_cases(char const * vcf, char const * haplotypes)
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + vcf);
    auto expected = spm::io::read_fasta(DATA + haplotypes);
    EXPECT_TRUE(ref.size() == 1 && expected.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    std::printf("%s\n", vcf);
    locate_case<spm::batch_myers_matcher>(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 0);
    locate_case<spm::batch_myers_matcher>(jst, expected, SPM_ALGO_MYERS, 100, 3, false, 64); // blocks shorter than |P|
    locate_case<spm::batch_shiftor_matcher>(jst, expected, SPM_ALGO_SHIFTOR, 32, 0, true, 0);
}

int main()
{
    fixture_cases("sim_ref_10Kb_SNPs.vcf", "sim_ref_10Kb_SNPs_haplotypes.fasta.gz");
    fixture_cases("sim_ref_10Kb_SNP_INDELs.vcf", "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
