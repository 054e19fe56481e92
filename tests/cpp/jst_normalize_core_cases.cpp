// jst_normalize_core_cases.cpp -- the left-normalisation rule (libspm_amd/csrc/jst_normalize_core.hpp) on the host: the same
// template the normalise kernel instantiates, here with a vector as its word store.  A program of its own (plain g++, and
// g++ -fsanitize=address,undefined): needle, reference, words and store are heap blocks of exactly their size, so a read or
// write past one of them is what the sanitizer build is for.
//   * the worked cases of the header;
//   * thousands of random true alignments over alphabets of 1-4 symbols against a restatement of the rule in COLUMN form
//     (one op per column, one step at a time), with the invariants of the contract and idempotence;
//   * malformed input -- words that over- or under-consume, a range past the reference, words of no columns, an unknown op, a
//     store too small -- which must be refused, not read through.
#include <cstdio>
#include <cstdint>
#include <random>
#include <string>
#include <vector>

#include "jst_normalize_core.hpp"

using namespace spm_hip;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
        }                                                                                                              \
    } while (0)

static constexpr uint32_t EQ = 7, X = 8, I = 1, D = 2;

struct vec_store
{
    std::vector<uint32_t> w;
    explicit vec_store(size_t cap) : w(cap) {}
    uint64_t cap() const { return w.size(); }
    uint32_t get(uint64_t k) const { return w.at(k); }
    void put(uint64_t k, uint32_t v) { w.at(k) = v; }
};

using bytes = std::vector<uint8_t>;
using words_t = std::vector<uint32_t>;

static bytes ranks(std::string const & s)
{
    bytes r;
    for (char c : s)
        r.push_back(static_cast<uint8_t>(std::string("ACGT").find(c)));
    return r;
}

static words_t parse(std::string const & s)
{
    words_t w;
    uint32_t n = 0;
    for (char c : s) {
        if (c >= '0' && c <= '9') {
            n = n * 10 + static_cast<uint32_t>(c - '0');
            continue;
        }
        w.push_back(n << 4 | (c == '=' ? EQ : c == 'X' ? X : c == 'I' ? I : D));
        n = 0;
    }
    return w;
}

static std::string show(words_t const & w)
{
    std::string s;
    for (uint32_t x : w)
        s += std::to_string(x >> 4) + "-ID----=X"[x & 15];
    return s;
}

static std::vector<uint32_t> columns(words_t const & w)
{
    std::vector<uint32_t> c;
    for (uint32_t x : w)
        c.insert(c.end(), x >> 4, x & 15);
    return c;
}

static words_t merge(std::vector<uint32_t> const & col)
{
    words_t w;
    for (size_t a = 0; a < col.size();) {
        size_t b = a;
        while (b < col.size() && col[b] == col[a])
            ++b;
        w.push_back(static_cast<uint32_t>(b - a) << 4 | col[a]);
        a = b;
    }
    return w;
}

struct tally
{
    uint64_t steps = 0, joined = 0, pinned = 0;
};

// the rule of the header, column by column
static words_t restated(bytes const & P, bytes const & ref, uint64_t ref_begin, words_t const & w, tally & T)
{
    std::vector<uint32_t> col = columns(w);
    size_t const n = col.size();
    size_t at = 0;
    while (at < n) {
        uint32_t const op = col[at];
        if (op != I && op != D) {
            ++at;
            continue;
        }
        size_t c = at, L = 0;
        while (c + L < n && col[c + L] == op)
            ++L;
        while (true) {
            size_t i = 0, r = ref_begin;
            for (size_t k = 0; k < c; ++k) {
                i += col[k] != D;
                r += col[k] != I;
            }
            bool const same = c >= 1 && col[c - 1] == EQ && (op == I ? P.at(i - 1) == P.at(i + L - 1) : ref.at(r - 1) == ref.at(r + L - 1));
            if (!(c >= 2 && same)) {
                T.pinned += c == 1 && same;
                break;
            }
            col[c - 1] = op;
            col[c - 1 + L] = EQ;
            --c;
            ++T.steps;
            if (c >= 1 && col[c - 1] == op) {
                ++T.joined;
                while (c >= 1 && col[c - 1] == op) {
                    --c;
                    ++L;
                }
            }
        }
        at = c + L;
    }
    return merge(col);
}

struct outcome
{
    bool ok = false;
    words_t w;
    jst_norm_result R;
};

static outcome run(bytes const & P, bytes const & ref, uint64_t rb, uint64_t re, words_t const & w, size_t cap)
{
    // (copies of exactly the sizes the call is told: the sanitizers see every byte past them)
    bytes const p(P.begin(), P.end()), r(ref.begin(), ref.end());
    words_t const in(w.begin(), w.end());
    vec_store S(cap);
    outcome o;
    o.ok = jst_normalize_walk(in.data(), static_cast<uint32_t>(in.size()), p.data(), static_cast<uint32_t>(p.size()), r.data(),
                              r.size(), rb, re, S, o.R);
    if (o.ok)
        o.w.assign(S.w.begin(), S.w.begin() + static_cast<std::ptrdiff_t>(o.R.n_words));
    return o;
}

// true: every = / X column says the truth and the words consume exactly P and ref[rb, re)
static bool true_alignment(bytes const & P, bytes const & ref, uint64_t rb, uint64_t re, words_t const & w)
{
    size_t i = 0, r = rb;
    for (uint32_t o : columns(w)) {
        if (o == EQ || o == X) {
            if (i >= P.size() || r >= re || (P[i] == ref[r]) != (o == EQ))
                return false;
        }
        i += o != D;
        r += o != I;
    }
    for (size_t k = 0; k + 1 < w.size(); ++k)
        if ((w[k] & 15) == (w[k + 1] & 15))
            return false;
    return i == P.size() && r == re;
}

static void worked_cases()
{
    struct row
    {
        std::string ref, P;
        uint64_t rb;
        std::vector<std::string> in;
        std::string out;
    };
    std::string const rep = "ACTACTACTACTACT";
    std::vector<row> const rows = {
        {"GATTCGCAAAAGTCCATG", "TTCGCAAAGTCCA", 2, {"8=1D5=", "6=1D7=", "5=1D8="}, "5=1D8="},
        {"GGAC" + rep + "GGTC", "AC" + rep.substr(3) + "GG", 2, {"2=3D14=", "5=3D11=", "8=3D8=", "11=3D5=", "14=3D2="}, "2=3D14="},
        {"GATCCGT", "ATCCCG", 1, {"4=1I1=", "3=1I2="}, "2=1I3="},
        {"GACGTCGTA", "ACGTCGTCGTA", 1, {"7=3I1="}, "1=3I7="},
        {"CAAAAG", "AAAG", 1, {"3=1D1="}, "1=1D3="},
        {"CAAAAAAG", "AAAAG", 1, {"2=1D1=1D2=", "1=1D2=1D2=", "4=2D1="}, "1=2D4="},
        {"GACGTTA", "ACGATTA", 1, {"3=1X1I2="}, "3=1X1I2="},
    };
    for (row const & c : rows)
        for (std::string const & s : c.in) {
            bytes const ref = ranks(c.ref), P = ranks(c.P);
            words_t const w = parse(s);
            uint64_t re = c.rb;
            for (uint32_t o : columns(w))
                re += o != I;
            EXPECT_TRUE(true_alignment(P, ref, c.rb, re, w));
            outcome const o = run(P, ref, c.rb, re, w, 2 * w.size());
            EXPECT_TRUE(o.ok);
            EXPECT_TRUE(show(o.w) == c.out);
            if (show(o.w) != c.out)
                std::printf("  %s: %s -> %s, expected %s\n", c.ref.c_str(), s.c_str(), show(o.w).c_str(), c.out.c_str());
            tally T;
            EXPECT_TRUE(show(restated(P, ref, c.rb, w, T)) == c.out);
        }
    // a transcript wholly inside an insertion; the counters of two of the cases
    outcome o = run(ranks("ACGT"), ranks("ACGT"), 2, 2, parse("4I"), 2);
    EXPECT_TRUE(o.ok && show(o.w) == "4I" && o.R.n_steps == 0);
    o = run(ranks("AAAG"), ranks("CAAAAG"), 1, 6, parse("3=1D1="), 6);
    EXPECT_TRUE(o.ok && o.R.n_pinned == 1 && o.R.n_steps == 2 && o.R.n_joined == 0);
    o = run(ranks("AAAAG"), ranks("CAAAAAAG"), 1, 8, parse("2=1D1=1D2="), 10);
    EXPECT_TRUE(o.ok && o.R.n_joined == 1 && o.R.n_pinned == 2); // (the first run stops pinned, and so does the joined one)
    // adjacent words of one op are one run
    o = run(ranks("TTCGCAAAGTCCA"), ranks("GATTCGCAAAAGTCCATG"), 2, 16, {3u << 4 | EQ, 5u << 4 | EQ, 1u << 4 | D, 5u << 4 | EQ}, 8);
    EXPECT_TRUE(o.ok && show(o.w) == "5=1D8=");
    o = run(ranks("AAAAG"), ranks("CAAAAAAG"), 1, 8, {4u << 4 | EQ, 1u << 4 | D, 1u << 4 | D, 1u << 4 | EQ}, 8);
    EXPECT_TRUE(o.ok && show(o.w) == "1=2D4=");
}

struct counts
{
    uint64_t stepped = 0, grew = 0, shrank = 0, joined = 0, pinned = 0;
};

static void random_cases(counts & C)
{
    std::mt19937_64 rng(20261);
    auto below = [&](uint64_t n) { return static_cast<uint64_t>(rng() % n); };
    for (int it = 0; it < 12000; ++it) {
        uint32_t const sigma = 1 + static_cast<uint32_t>(it % 4);
        uint64_t const rb = below(4);
        bytes ref, P;
        std::vector<uint32_t> col;
        for (uint64_t k = 0; k < rb; ++k)
            ref.push_back(static_cast<uint8_t>(below(sigma)));
        uint64_t const n_cols = 1 + below(48);
        for (uint64_t k = 0; k < n_cols; ++k) {
            uint64_t const u = below(100);
            uint8_t const s = static_cast<uint8_t>(below(sigma));
            if (u >= 25) {
                ref.push_back(s), P.push_back(s), col.push_back(EQ);
            } else if (u < 8 && sigma > 1) {
                ref.push_back(s), P.push_back(static_cast<uint8_t>((s + 1 + below(sigma - 1)) % sigma)), col.push_back(X);
            } else if (u < 16) {
                P.push_back(s), col.push_back(I);
            } else {
                ref.push_back(s), col.push_back(D);
            }
        }
        if (P.empty())
            P.push_back(0), col.push_back(I);
        uint64_t const re = ref.size();
        for (uint64_t k = below(3); k > 0; --k)
            ref.push_back(static_cast<uint8_t>(below(sigma)));
        words_t const w = merge(col);
        EXPECT_TRUE(true_alignment(P, ref, rb, re, w));
        tally T;
        words_t const want = restated(P, ref, rb, w, T);
        outcome const o = run(P, ref, rb, re, w, 2 * w.size());
        EXPECT_TRUE(o.ok);
        EXPECT_TRUE(o.w == want);
        if (o.w != want)
            std::printf("  %s -> %s, expected %s\n", show(w).c_str(), show(o.w).c_str(), show(want).c_str());
        EXPECT_TRUE(o.R.n_steps == T.steps && o.R.n_joined == T.joined && o.R.n_pinned == T.pinned);
        EXPECT_TRUE(true_alignment(P, ref, rb, re, o.w));
        EXPECT_TRUE(o.w.size() <= 2 * w.size());
        std::vector<uint32_t> const a = columns(w), b = columns(o.w);
        for (uint32_t op : {EQ, X, I, D}) {
            size_t na = 0, nb = 0;
            for (uint32_t x : a)
                na += x == op;
            for (uint32_t x : b)
                nb += x == op;
            EXPECT_TRUE(na == nb);
        }
        outcome const again = run(P, ref, rb, re, o.w, 2 * o.w.size());
        EXPECT_TRUE(again.ok && again.w == o.w && again.R.n_steps == 0 && again.R.n_joined == 0);
        // a store smaller than the result is refused, not overrun
        EXPECT_TRUE(!run(P, ref, rb, re, w, o.w.size() - 1).ok);
        C.stepped += T.steps > 0;
        C.grew += o.w.size() > w.size();
        C.shrank += o.w.size() < w.size();
        C.joined += T.joined > 0;
        C.pinned += T.pinned > 0;
    }
}

static void malformed_cases()
{
    bytes const ref = ranks("GATTCGCAAAAGTCCATG"), P = ranks("TTCGCAAAGTCCA");
    auto refused = [&](words_t const & w, uint64_t rb, uint64_t re, size_t cap) { return !run(P, ref, rb, re, w, cap).ok; };
    EXPECT_TRUE(!refused(parse("8=1D5="), 2, 16, 6));
    EXPECT_TRUE(refused(parse("8=1D6="), 2, 16, 6));        // consumes more than the needle
    EXPECT_TRUE(refused(parse("8=1D60="), 2, 16, 6));
    EXPECT_TRUE(refused(parse("8=1D4="), 2, 16, 6));        // ... less
    EXPECT_TRUE(refused(parse("8=1D4=1I"), 2, 16, 8));      // the needle, but less than the range
    EXPECT_TRUE(refused(parse("8=2D5="), 2, 16, 6));        // more than the range
    EXPECT_TRUE(refused(parse("8=900D5="), 2, 16, 6));
    EXPECT_TRUE(refused(parse("8=1D5=9D"), 2, 16, 8));
    EXPECT_TRUE(refused(parse("8=9I5="), 2, 16, 6));        // an I run longer than what is left of the needle
    EXPECT_TRUE(refused(parse("14I"), 2, 2, 2));
    EXPECT_TRUE(!refused(parse("13I"), 2, 2, 2));
    EXPECT_TRUE(refused(parse("8=1D5="), 2, 19, 6));        // a range past the reference
    EXPECT_TRUE(refused(parse("8=1D5="), 17, 16, 6));       // begin behind end
    EXPECT_TRUE(refused(parse("8=1D5="), 6, 20, 6));
    EXPECT_TRUE(refused(parse("8=0D1D5="), 2, 16, 8));      // words of no columns
    EXPECT_TRUE(refused(parse("0=8=1D5="), 2, 16, 8));
    EXPECT_TRUE(refused(parse("8=1D0D5="), 2, 16, 8));
    EXPECT_TRUE(refused({8u << 4 | EQ, 1u << 4 | 3u, 5u << 4 | EQ}, 2, 16, 6)); // an unknown op
    EXPECT_TRUE(refused({8u << 4 | EQ, 1u << 4 | 0u, 5u << 4 | EQ}, 2, 16, 6));
    EXPECT_TRUE(refused(parse("8=1D5="), 2, 16, 2));        // a store too small
    EXPECT_TRUE(refused(parse("8=1D5="), 2, 16, 0));
    EXPECT_TRUE(refused(words_t{}, 2, 16, 0));              // no words at all
    // a run of the longest word: lengths are added in 64 bits and refused by what they consume
    EXPECT_TRUE(refused({8u << 4 | EQ, 0x0FFFFFFFu << 4 | D, 0x0FFFFFFFu << 4 | D, 5u << 4 | EQ}, 2, 16, 8));
    EXPECT_TRUE(refused({0x0FFFFFFFu << 4 | I, 0x0FFFFFFFu << 4 | I}, 2, 2, 4));
}

int main()
{
    worked_cases();
    counts C;
    random_cases(C);
    malformed_cases();
    std::printf("stepped %llu, grew %llu, shrank %llu, joined %llu, pinned %llu\n", static_cast<unsigned long long>(C.stepped),
                static_cast<unsigned long long>(C.grew), static_cast<unsigned long long>(C.shrank),
                static_cast<unsigned long long>(C.joined), static_cast<unsigned long long>(C.pinned));
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
