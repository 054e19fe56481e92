// rescue_mirror_cases.cpp -- mate rescue through the C++ mirror, on the committed fixtures (tests/golden/jst):
// journaled_sequence_tree::locate_pairs_rescued returns what locate_pairs returns plus the rescue records, and every record
// agrees with the rule written out again here: the jobs of the pair records, the window, a plain dynamic-programming search
// over it for the minimum of (distance, end), the classification of the alignment the device returned, whose transcript is
// replayed against needle and reference.  The pairs are cut from the materialised haplotypes; one mate in two gets 5
// substitutions, too many for the search at k = 2.
#include <algorithm>
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
    std::uint64_t r = 0x5E5C0Eull;
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

// the minimum of (d, e) over the ends [e0, e1] of the needle in ref[lo ..), d <= k; false: none
static bool plain_search(std::vector<std::uint8_t> const & ref, std::vector<std::uint8_t> const & q, std::size_t lo, std::size_t e0,
                         std::size_t e1, std::uint32_t k, std::uint32_t & d, std::size_t & e)
{
    std::vector<std::uint32_t> col(q.size() + 1), nxt(q.size() + 1);
    for (std::size_t i = 0; i <= q.size(); ++i)
        col[i] = static_cast<std::uint32_t>(i);
    bool found = false;
    for (std::size_t t = lo; t < e1; ++t) {
        nxt[0] = 0;
        for (std::size_t i = 1; i <= q.size(); ++i)
            nxt[i] = std::min({col[i - 1] + (q[i - 1] == ref[t] ? 0u : 1u), col[i] + 1, nxt[i - 1] + 1});
        col.swap(nxt);
        if (t + 1 >= e0 && col[q.size()] <= k && (!found || col[q.size()] < d)) {
            found = true;
            d = col[q.size()];
            e = t + 1;
        }
    }
    return found;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, std::size_t block)
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
    EXPECT_TRUE(jst.device_ready());
    spm::hip::hit_selection const sel{true, {}, 1u, true, true};
    auto const nr = static_cast<std::uint32_t>(n_reads);
    auto const got = jst.locate_pairs_rescued(ps, window, nr, MIN_TLEN, MAX_TLEN, K, sel, block, nullptr);
    auto const again = jst.locate_pairs_rescued(ps, window, nr, MIN_TLEN, MAX_TLEN, K, sel, block, nullptr);
    EXPECT_TRUE(got == again);
    EXPECT_TRUE(got.located == jst.locate_pairs(ps, window, needles, false, nr, MIN_TLEN, MAX_TLEN, sel, block, nullptr));
    auto const & loci = got.located.mapped.loci;
    auto const & ref = jst.reference();
    std::size_t const N = ref.size();
    // the jobs of the pair records, in order
    std::size_t j = 0, rescued = 0, none = 0, not_concordant = 0;
    for (std::size_t p = 0; p < n_pairs; ++p) {
        spm::jst_pair const & P = got.located.pairs[p];
        if (P.flag1 & 2)
            continue;
        for (int x = 1; x >= 0; --x) {
            std::uint32_t const a = x ? P.locus2 : P.locus1;
            if (a == 0xFFFFFFFFu)
                continue;
            EXPECT_TRUE(j < got.rescues.size());
            if (j >= got.rescues.size())
                return;
            spm::jst_rescue const & R = got.rescues[j++];
            auto const & A = loci[a];
            bool const a_rev = (A.needle & 1u) != 0;
            std::size_t const ab = A.aln.begin_position(), ae = A.aln.end_position();
            std::uint32_t const q = static_cast<std::uint32_t>(4 * p + 2 * (1 - x) + (a_rev ? 0 : 1));
            EXPECT_TRUE(R.pair == p && R.anchor == a && R.needle == q);
            std::size_t const lo = a_rev ? (ae > MAX_TLEN ? ae - MAX_TLEN : 0) : ab;
            std::size_t const e1 = a_rev ? ae : std::min<std::size_t>(lo + MAX_TLEN, N);
            std::size_t const e0 = a_rev ? lo + 1 : std::max<std::size_t>(lo + MIN_TLEN, ae);
            std::uint32_t d = 0;
            std::size_t e = 0;
            bool const found = e0 <= e1 && plain_search(ref, needles[q], lo, e0, e1, K, d, e);
            EXPECT_TRUE(found == (R.status != SPM_RESCUE_NONE));
            std::uint16_t const mate_bit = x == 0 ? 0x80 : 0x40;
            if (!found) {
                EXPECT_TRUE(R.aln.errors() == -1 && R.tlen == 0 && R.aln.cigar().empty() && R.flag == (0x1 | 0x4 | (a_rev ? 0x20 : 0) | mate_bit));
                ++none;
                continue;
            }
            EXPECT_TRUE(R.aln.end_position() == e && R.aln.errors() == static_cast<std::int32_t>(d) && R.aln.begin_position() >= lo);
            // the transcript consumes the needle and ref[begin, end) with exactly d edits
            std::size_t i = 0, t = R.aln.begin_position(), cost = 0;
            bool true_ops = true;
            for (std::uint32_t const w : R.aln.cigar())
                for (std::uint32_t c = 0; c < w >> 4; ++c) {
                    std::uint32_t const op = w & 15u;
                    if (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X) {
                        true_ops = true_ops && i < needles[q].size() && t < N && (needles[q][i] == ref[t]) == (op == SPM_CIGAR_EQ);
                        ++i;
                        ++t;
                    } else if (op == SPM_CIGAR_INS) {
                        ++i;
                    } else {
                        ++t;
                    }
                    cost += op != SPM_CIGAR_EQ;
                }
            EXPECT_TRUE(true_ops && i == needles[q].size() && t == e && cost == d);
            std::size_t const b = R.aln.begin_position();
            std::size_t const fb = a_rev ? b : ab, fe = a_rev ? e : ae, vb = a_rev ? ab : b, ve = a_rev ? ae : e;
            bool const ok = fb <= vb && fe <= ve && ve - fb >= MIN_TLEN && ve - fb <= MAX_TLEN;
            EXPECT_TRUE(R.status == (ok ? SPM_RESCUE_RESCUED : SPM_RESCUE_NOT_CONCORDANT));
            bool const mate1_forward = a_rev ? x == 1 : x == 0;
            auto const tl = static_cast<std::int32_t>(ve - fb);
            EXPECT_TRUE(R.tlen == (ok ? (mate1_forward ? tl : -tl) : 0));
            EXPECT_TRUE(R.flag == (0x1 | (ok ? 0x2 : 0) | (a_rev ? 0x20 : 0x10) | mate_bit));
            rescued += ok;
            not_concordant += !ok;
        }
    }
    EXPECT_TRUE(j == got.rescues.size());
    EXPECT_TRUE(rescued >= 10 && none >= 6);
    std::printf("  block %zu: %zu loci, %zu jobs: %zu rescued, %zu none, %zu not concordant\n", block, loci.size(), j, rescued, none,
                not_concordant);
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
