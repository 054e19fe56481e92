// select_cases.cpp -- the hit_selection overloads of the C++ mirror (batch_matcher and the single-needle Myers matcher):
// operator()(haystack, callback, selection) and locate(haystack, callback, selection).  The input is generated from
// splitmix64 (tests/test_select_cpp.py regenerates it and compares every printed callback with Hits.select() in Python);
// the program itself checks what needs no second opinion: callback order (per needle, ascending), that the selected
// callbacks are a subset of the unselected ones, that no two selected hits of a needle lie within its window, and that
// the resident-haystack overloads agree with the host-range ones.
//   select_cases            run and print:  op|loc|single <needle> <begin> <end> <errors> [cigar]
#include <cstdio>
#include <string>
#include <tuple>
#include <vector>

#include <libspm/matcher/hip_batch.hpp>
#include <libspm/matcher/myers_matcher.hpp>
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

static std::uint64_t mix64(std::uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr std::size_t N = 1u << 16, NEEDLES = 24, L = 60;
constexpr std::uint64_t SEED = 0x5E1EC7ull;

using hit = std::tuple<std::size_t, std::size_t, std::size_t, int>; // needle, begin, end, errors

static bool ordered(std::vector<hit> const & v) // per needle, ascending end
{
    for (std::size_t i = 1; i < v.size(); ++i)
        if (std::get<0>(v[i]) < std::get<0>(v[i - 1]) ||
            (std::get<0>(v[i]) == std::get<0>(v[i - 1]) && std::get<2>(v[i]) <= std::get<2>(v[i - 1])))
            return false;
    return true;
}

static bool subset(std::vector<hit> const & part, std::vector<hit> const & all)
{
    std::size_t j = 0;
    for (hit const & h : part) {
        while (j < all.size() && all[j] != h)
            ++j;
        if (j == all.size())
            return false;
    }
    return true;
}

int main()
{
    // text[i] = splitmix64(SEED + i) & 3; needle p = text[at, at + L) with at = splitmix64(SEED ^ (p + 1) << 32) % (N - L),
    // odd needles with one substitution in the middle; k = p % 4
    std::vector<spm::dna4> text(N);
    for (std::size_t i = 0; i < N; ++i)
        text[i].assign_rank(static_cast<std::uint8_t>(mix64(SEED + i) & 3));
    std::vector<std::vector<spm::dna4>> needles(NEEDLES);
    std::vector<std::uint16_t> ks(NEEDLES);
    for (std::size_t p = 0; p < NEEDLES; ++p) {
        std::size_t const at = mix64(SEED ^ ((p + 1) << 32)) % (N - L);
        needles[p].assign(text.begin() + static_cast<std::ptrdiff_t>(at), text.begin() + static_cast<std::ptrdiff_t>(at + L));
        if (p % 2)
            needles[p][L / 2].assign_rank(static_cast<std::uint8_t>((mix64(SEED + at + L / 2) + 1) & 3));
        ks[p] = static_cast<std::uint16_t>(p % 4);
    }
    spm::batch_myers_matcher batch{needles, ks};
    spm::hip::resident_haystack resident{text};

    for (int mode = 0; mode < 3; ++mode) {
        // 0: loci at the needles' own k; 1: loci + the best stratum; 2: an explicit window of 1 and two strata
        spm::hip::hit_selection sel{};
        if (mode == 1)
            sel.strata = 0;
        if (mode == 2) {
            sel.window = 1;
            sel.strata = 1;
        }
        std::vector<hit> all, kept, kept_resident, located, located_resident;
        batch(text, [&](std::size_t p, spm::finder const & f) { all.emplace_back(p, f.begin_position(), f.end_position(), f.errors()); });
        batch(text, [&](std::size_t p, spm::finder const & f) { kept.emplace_back(p, f.begin_position(), f.end_position(), f.errors()); }, sel);
        batch(resident, [&](std::size_t p, spm::finder const & f) { kept_resident.emplace_back(p, f.begin_position(), f.end_position(), f.errors()); }, sel);
        EXPECT_TRUE(!all.empty() && !kept.empty() && kept.size() < all.size());
        EXPECT_TRUE(ordered(all) && ordered(kept) && subset(kept, all) && kept == kept_resident);
        for (std::size_t i = 1; i < kept.size(); ++i)
            if (std::get<0>(kept[i]) == std::get<0>(kept[i - 1]))
                EXPECT_TRUE(std::get<2>(kept[i]) - std::get<2>(kept[i - 1]) > (mode == 2 ? 1u : ks[std::get<0>(kept[i])]));
        for (hit const & h : kept)
            std::printf("op%d %zu %zu %zu %d\n", mode, std::get<0>(h), std::get<1>(h), std::get<2>(h), std::get<3>(h));

        std::vector<std::string> cigars;
        batch.locate(text, [&](std::size_t p, spm::finder const & f, spm::alignment const & a) {
            located.emplace_back(p, f.begin_position(), f.end_position(), f.errors());
            EXPECT_TRUE(a.begin_position() == f.begin_position() && a.end_position() == f.end_position() && a.errors() == f.errors());
            cigars.push_back(a.cigar_string());
        }, sel);
        batch.locate(resident, [&](std::size_t p, spm::finder const & f, spm::alignment const &) {
            located_resident.emplace_back(p, f.begin_position(), f.end_position(), f.errors());
        }, sel);
        EXPECT_TRUE(located.size() == kept.size() && located == located_resident && ordered(located));
        for (std::size_t i = 0; i < located.size() && i < kept.size(); ++i) // the same hits, now with their true begins
            EXPECT_TRUE(std::get<0>(located[i]) == std::get<0>(kept[i]) && std::get<2>(located[i]) == std::get<2>(kept[i]) &&
                        std::get<3>(located[i]) == std::get<3>(kept[i]));
        for (std::size_t i = 0; i < located.size(); ++i)
            std::printf("loc%d %zu %zu %zu %d %s\n", mode, std::get<0>(located[i]), std::get<1>(located[i]), std::get<2>(located[i]),
                        std::get<3>(located[i]), cigars[i].c_str());
    }

    // the single-needle Myers matcher: needle 3 (k = 3)
    spm::myers_matcher single{needles[3], 3};
    std::vector<hit> all, kept, kept_resident, located;
    single(text, [&](spm::finder const & f) { all.emplace_back(3, f.begin_position(), f.end_position(), f.errors()); });
    single(text, [&](spm::finder const & f) { kept.emplace_back(3, f.begin_position(), f.end_position(), f.errors()); },
           spm::hip::hit_selection{});
    single(resident, [&](spm::finder const & f) { kept_resident.emplace_back(3, f.begin_position(), f.end_position(), f.errors()); },
           spm::hip::hit_selection{});
    single.locate(text, [&](spm::finder const & f, spm::alignment const &) {
        located.emplace_back(3, f.begin_position(), f.end_position(), f.errors());
    }, spm::hip::hit_selection{});
    EXPECT_TRUE(!kept.empty() && kept.size() < all.size() && ordered(kept) && subset(kept, all) && kept == kept_resident);
    EXPECT_TRUE(located.size() == kept.size());
    for (hit const & h : kept)
        std::printf("single 3 %zu %zu %d\n", std::get<1>(h), std::get<2>(h), std::get<3>(h));

    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
