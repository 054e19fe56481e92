// The composition of a haplotype transcript with the journal of its haplotype (libspm_amd/csrc/jst_project_core.hpp): the
// header alone, plain checks, no device.  Random small journals and transcripts against a brute-force composition over an
// explicit column list written here; the counting sink and the writing sink must agree; a cursor started from the state the
// kernels derive from the index (block start, first allele of the block, first reference position still read) must stand
// where the cursor from the haplotype's first symbol stands.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../libspm_amd/csrc/jst_project_core.hpp"

using namespace spm_hip;

static long n_checks = 0, n_failures = 0;
#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        ++n_checks;                                                                                                    \
        if (!(c)) {                                                                                                    \
            ++n_failures;                                                                                              \
            if (n_failures < 20)                                                                                       \
                std::printf("FAILED %s:%d: %s (case %ld)\n", __FILE__, __LINE__, #c, case_no);                         \
        }                                                                                                              \
    } while (0)
static long case_no = 0;

struct allele
{
    uint64_t pos;
    uint32_t rlen;
    std::vector<uint8_t> alt;
};

struct column // of the alignment haplotype ~ reference
{
    long x;      // haplotype index or -1
    long rho;    // reference position or -1
    long anchor; // of an inserted symbol
    long org;    // the reference position a haplotype symbol stems from (an alt symbol: its allele's): block ownership
};

struct tree
{
    std::vector<uint8_t> ref;
    std::vector<allele> al;
    std::vector<uint64_t> pos, cov;
    std::vector<uint32_t> rlen, alen;
    uint32_t n_hap = 3;
    jst_journal_view view() const
    {
        jst_journal_view V;
        V.pos = pos.data();
        V.rlen = rlen.data();
        V.alen = alen.data();
        V.cov = cov.data();
        V.n_alleles = al.size();
        V.cw = 1;
        V.n_hap = n_hap;
        V.n_ref = ref.size();
        return V;
    }
};

// Alleles that never overlap, so any coverage is valid: back-to-back alleles, an insertion directly behind a deletion,
// alleles at reference position 0 and alleles that end at (or are inserted at) the end of the reference.
static tree random_tree(std::mt19937_64 &rng)
{
    tree T;
    const uint64_t n_ref = 20 + rng() % 50;
    for (uint64_t i = 0; i < n_ref; ++i)
        T.ref.push_back((uint8_t)(rng() % 4));
    uint64_t p = rng() % 3 == 0 ? 0 : rng() % 6;
    while (p <= n_ref) {
        allele a;
        a.pos = p;
        const unsigned kind = (unsigned)(rng() % 6);
        a.rlen = kind == 1 ? 0 : (uint32_t)(1 + rng() % (kind == 0 ? 1 : 5));
        const unsigned alen = kind == 0 ? 1 : kind == 2 ? 0 : (unsigned)(rng() % 7) + (kind == 1 ? 1 : 0);
        if (a.pos + a.rlen > n_ref)
            a.rlen = (uint32_t)(n_ref - a.pos);
        for (unsigned i = 0; i < alen; ++i)
            a.alt.push_back((uint8_t)(rng() % 4));
        if (a.rlen || !a.alt.empty())
            T.al.push_back(a);
        const unsigned gap = (unsigned)(rng() % 4); // 0, 0: back to back (an insertion directly behind a deletion among them)
        p = a.pos + a.rlen + (gap < 2 ? 0 : rng() % 9);
        if (a.rlen == 0 && gap < 2)
            p += 1; // (two insertions at one position on one haplotype would still be valid, but say nothing new)
        if (rng() % 5 == 0 && p < n_ref)
            p = std::max<uint64_t>(p, n_ref - rng() % 3); // alleles at the end of the reference
    }
    for (const allele &a : T.al) {
        T.pos.push_back(a.pos);
        T.rlen.push_back(a.rlen);
        T.alen.push_back((uint32_t)a.alt.size());
        T.cov.push_back(rng() % 8);
    }
    if (T.al.empty()) { // (the tables are never null)
        T.pos.push_back(0);
        T.rlen.push_back(0);
        T.alen.push_back(0);
        T.cov.push_back(0);
    }
    return T;
}

// the journal of haplotype h spelled out: its symbols and the column list; the deleted columns of an allele stand directly
// before the next paired column (the contract's order)
static void spell(const tree &T, uint32_t h, std::vector<uint8_t> &hap, std::vector<column> &cols)
{
    std::vector<long> pend;
    uint64_t r = 0;
    auto paired = [&](uint64_t rho, uint8_t sym, long org = -1) {
        for (long d : pend)
            cols.push_back({-1, d, -1, -1});
        pend.clear();
        cols.push_back({(long)hap.size(), (long)rho, (long)rho, org < 0 ? (long)rho : org});
        hap.push_back(sym);
    };
    for (size_t i = 0; i < T.al.size(); ++i) {
        if (!((T.cov[i] >> h) & 1))
            continue;
        const allele &a = T.al[i];
        for (; r < a.pos; ++r)
            paired(r, T.ref[r]);
        const uint32_t al = (uint32_t)a.alt.size(), mn = std::min(a.rlen, al);
        for (uint32_t k = 0; k < mn; ++k)
            paired(a.pos + k, a.alt[k], (long)a.pos);
        for (uint32_t k = mn; k < al; ++k) {
            cols.push_back({(long)hap.size(), -1, (long)(a.pos + mn), (long)a.pos});
            hap.push_back(a.alt[k]);
        }
        for (uint32_t k = al; k < a.rlen; ++k)
            pend.push_back((long)(a.pos + k));
        r = a.pos + a.rlen;
    }
    for (; r < T.ref.size(); ++r)
        paired(r, T.ref[r]);
}

static void push_op(std::vector<uint32_t> &words, uint32_t op)
{
    if (!words.empty() && (words.back() & 15u) == op)
        words.back() += 16;
    else
        words.push_back(16u | op);
}

struct expect
{
    std::vector<uint32_t> words;
    uint64_t ref_begin = 0, ref_end = 0, score = 0;
    bool inside = false;
};

static expect brute(const tree &T, const std::vector<column> &cols, const std::vector<long> &col_of, uint64_t begin,
                    const std::vector<uint32_t> &words, const std::vector<uint8_t> &P, size_t hap_len)
{
    expect E;
    long last = -1, first_rho = -1, last_rho = -1;
    uint64_t x = begin;
    size_t i = 0;
    auto out = [&](uint32_t op) {
        push_op(E.words, op);
        E.score += op != kProjEq;
    };
    for (uint32_t w : words)
        for (uint32_t c = 0; c < (w >> 4); ++c) {
            const uint32_t op = w & 15u;
            if (op == kProjIns) {
                out(kProjIns);
                ++i;
                continue;
            }
            const long col = col_of[x++];
            if (cols[(size_t)col].rho >= 0) {
                if (last >= 0)
                    for (long k = last + 1; k < col; ++k)
                        if (cols[(size_t)k].x < 0)
                            out(kProjDel);
                last = col;
                last_rho = cols[(size_t)col].rho;
                if (first_rho < 0)
                    first_rho = last_rho;
                if (op == kProjDel)
                    out(kProjDel);
                else
                    out(P[i++] == T.ref[(size_t)last_rho] ? kProjEq : kProjX);
            } else if (op != kProjDel) {
                out(kProjIns);
                ++i;
            }
        }
    E.inside = last < 0;
    if (E.inside)
        E.ref_begin = E.ref_end = begin < hap_len ? (uint64_t)cols[(size_t)col_of[begin]].anchor : T.ref.size();
    else {
        E.ref_begin = (uint64_t)first_rho;
        E.ref_end = (uint64_t)last_rho + 1;
    }
    return E;
}

// the projected transcript consumes exactly P and ref[ref_begin, ref_end), = / X agree with the symbols, cost = score
static bool replays(const tree &T, const std::vector<uint8_t> &P, const std::vector<uint32_t> &words, uint64_t b, uint64_t e,
                    uint64_t score)
{
    size_t i = 0;
    uint64_t j = b, cost = 0;
    uint32_t prev = 0;
    for (uint32_t w : words) {
        const uint32_t op = w & 15u, n = w >> 4;
        if (n == 0 || op == prev)
            return false;
        prev = op;
        for (uint32_t c = 0; c < n; ++c) {
            if (op == kProjEq || op == kProjX) {
                if (i >= P.size() || j >= e || (P[i] == T.ref[j]) != (op == kProjEq))
                    return false;
                ++i, ++j;
            } else if (op == kProjIns)
                ++i;
            else
                ++j;
            cost += op != kProjEq;
        }
    }
    return i == P.size() && j == e && cost == score;
}

int main()
{
    std::mt19937_64 rng(0x5EED0005);
    long n_inside = 0, n_gap = 0, n_changed = 0, n_ins_behind_del = 0, n_at_ends = 0;
    for (case_no = 0; case_no < 3000; ++case_no) {
        const tree T = random_tree(rng);
        const uint32_t h = (uint32_t)(rng() % T.n_hap);
        std::vector<uint8_t> hap;
        std::vector<column> cols;
        spell(T, h, hap, cols);
        std::vector<long> col_of;
        for (size_t c = 0; c < cols.size(); ++c)
            if (cols[c].x >= 0)
                col_of.push_back((long)c);
        for (size_t i = 0; i + 1 < T.al.size(); ++i)
            n_ins_behind_del += ((T.cov[i] & T.cov[i + 1]) >> h & 1) && T.al[i].alt.empty() && T.al[i + 1].rlen == 0 &&
                                T.al[i + 1].pos == T.al[i].pos + T.al[i].rlen;
        for (size_t i = 0; i < T.al.size(); ++i)
            n_at_ends += ((T.cov[i] >> h) & 1) && (T.al[i].pos == 0 || T.al[i].pos + T.al[i].rlen == T.ref.size());
        if (hap.empty())
            continue;
        // a random transcript from a random begin: ops as long as there are haplotype symbols
        const uint64_t begin = rng() % hap.size();
        std::vector<uint32_t> words;
        std::vector<uint8_t> P;
        uint64_t x = begin;
        const unsigned want = 1 + (unsigned)(rng() % 24);
        for (unsigned c = 0; c < want; ++c) {
            const unsigned kind = (unsigned)(rng() % 10);
            if (kind == 0) {
                push_op(words, kProjIns);
                P.push_back((uint8_t)(rng() % 4));
            } else if (x >= hap.size()) {
                break;
            } else if (kind == 1) {
                push_op(words, kProjDel);
                ++x;
            } else if (kind == 2) {
                push_op(words, kProjX);
                P.push_back((uint8_t)((hap[x++] + 1 + rng() % 3) & 3));
            } else {
                push_op(words, kProjEq);
                P.push_back(hap[x++]);
            }
        }
        if (P.empty()) {
            push_op(words, kProjIns);
            P.push_back(0);
        }
        const expect E = brute(T, cols, col_of, begin, words, P, hap.size());
        CHECK(replays(T, P, E.words, E.ref_begin, E.ref_end, E.score)); // (the brute force itself)
        n_inside += E.inside;
        n_changed += E.words != words;
        for (uint32_t w : E.words)
            n_gap += (w & 15u) == kProjDel;
        // the cursor: reached by skip() and, a second time, by single steps; the counting sink, then the writing sink
        const jst_journal_view V = T.view();
        for (int mode = 0; mode < 2; ++mode) {
            jst_journal_cursor C;
            C.start(V, h, 0, 0);
            bool ok = true;
            if (mode == 0)
                ok = C.skip(begin);
            else
                for (uint64_t s = 0; s < begin; ++s)
                    C.next();
            CHECK(ok && !C.at_end());
            CHECK(C.paired() == (cols[(size_t)col_of[begin]].rho >= 0));
            CHECK(C.rho() == (uint64_t)cols[(size_t)col_of[begin]].anchor);
            jst_journal_cursor C2 = C;
            jst_proj_count_sink S;
            jst_proj_result R;
            CHECK(jst_project_compose(C, words.data(), (uint32_t)words.size(), P.data(), (uint32_t)P.size(), T.ref.data(),
                                      T.ref.size(), S, R));
            CHECK(R.n_words == E.words.size() && R.ref_begin == E.ref_begin && R.ref_end == E.ref_end);
            CHECK(R.ref_score == E.score && (R.inside != 0) == E.inside);
            std::vector<uint32_t> got(E.words.size() + 2, 0xDEADBEEFu);
            jst_proj_write_sink W;
            W.out = got.data();
            W.cap = E.words.size();
            jst_proj_result R2;
            CHECK(jst_project_compose(C2, words.data(), (uint32_t)words.size(), P.data(), (uint32_t)P.size(), T.ref.data(),
                                      T.ref.size(), W, R2));
            CHECK(R2.n_words == R.n_words && R2.ref_begin == R.ref_begin && R2.ref_end == R.ref_end &&
                  R2.ref_score == R.ref_score && R2.inside == R.inside);
            CHECK(std::equal(E.words.begin(), E.words.end(), got.begin()));
            CHECK(got[E.words.size()] == 0xDEADBEEFu); // nothing beyond the slot
        }
        // The start the kernels use.  The index cuts the reference into blocks of L positions; hap_start[j] is the number of
        // haplotype symbols that stem from reference positions below jL, a_lo[j] the first allele at or behind jL, and the
        // first reference position the haplotype still reads at or behind jL follows from the nearest carried allele before
        // a_lo[j] (a carried deletion may span the border).  A cursor started there and moved begin - hap_start[j] symbols on
        // stands where the cursor from the haplotype's first symbol stands.
        {
            const uint64_t L = 1 + rng() % 24, n_ref = T.ref.size();
            const uint64_t n_blocks = std::max<uint64_t>(1, (n_ref + L - 1) / L);
            uint32_t max_rlen = 0;
            for (const allele &a : T.al)
                max_rlen = std::max(max_rlen, a.rlen);
            uint64_t j = 0, start = 0;
            for (uint64_t b = 0; b <= n_blocks; ++b) { // the largest block whose start is at or before begin
                uint64_t owned_before = 0;
                for (const column &c : cols)
                    owned_before += c.x >= 0 && (uint64_t)c.org < b * L;
                if (owned_before <= begin) {
                    j = b;
                    start = owned_before;
                }
            }
            uint64_t a_lo = 0;
            while (a_lo < T.al.size() && T.al[a_lo].pos < j * L)
                ++a_lo;
            uint64_t first_ref = j >= n_blocks ? n_ref : j * L;
            if (j < n_blocks)
                for (long i = (long)a_lo - 1; i >= 0 && T.al[(size_t)i].pos + max_rlen > j * L; --i)
                    if ((T.cov[(size_t)i] >> h) & 1) {
                        first_ref = std::max<uint64_t>(j * L, T.al[(size_t)i].pos + T.al[(size_t)i].rlen);
                        break;
                    }
            jst_journal_cursor A, B;
            A.start(V, h, 0, 0);
            B.start(V, h, first_ref, a_lo);
            CHECK(A.skip(begin) && B.skip(begin - start));
            bool same = true;
            for (int s = 0; s < 40 && !A.at_end(); ++s) {
                same = same && !B.at_end() && A.paired() == B.paired() && A.rho() == B.rho();
                A.next();
                B.next();
            }
            CHECK(same && A.at_end() == B.at_end());
        }
        // the whole haplotype through the cursor: its end, and every symbol's pairing
        if (case_no % 8 == 0) {
            jst_journal_cursor C;
            C.start(V, h, 0, 0);
            bool same = true;
            for (size_t s = 0; s < hap.size(); ++s) {
                const column &c = cols[(size_t)col_of[s]];
                same = same && !C.at_end() && C.paired() == (c.rho >= 0) && C.rho() == (uint64_t)c.anchor;
                C.next();
            }
            CHECK(same && C.at_end() && C.rho() == T.ref.size() && !C.skip(1));
        }
        // a transcript that does not fit is refused, not followed
        if (case_no % 16 == 0) {
            jst_journal_cursor C;
            C.start(V, h, 0, 0);
            C.skip(begin);
            std::vector<uint32_t> bad = words;
            bad.push_back((uint32_t)(hap.size() + 1) << 4 | kProjEq);
            jst_proj_count_sink S;
            jst_proj_result R;
            CHECK(!jst_project_compose(C, bad.data(), (uint32_t)bad.size(), P.data(), (uint32_t)P.size(), T.ref.data(),
                                       T.ref.size(), S, R));
        }
    }
    // a run longer than a word holds is split
    {
        jst_proj_count_sink S;
        S.put(kProjDel, kProjMaxRun + 5);
        S.flush();
        CHECK(S.n_words == 2);
    }
    CHECK(n_inside > 0 && n_gap > 0 && n_changed > 0 && n_ins_behind_del > 0 && n_at_ends > 0);
    std::printf("inside an insertion %ld, D words %ld, changed %ld, insertion behind deletion %ld, alleles at the ends %ld\n",
                n_inside, n_gap, n_changed, n_ins_behind_del, n_at_ends);
    std::printf("%ld checks, %ld failures\n", n_checks, n_failures);
    return n_failures ? 1 : 0;
}
