// jst_sam_core_cases.cpp -- the rule of spm_hip_jst_ref_loci_sam on the host (libspm_amd/csrc/jst_sam_core.hpp): digit counts
// and digits, for every kind of field length == bytes written, CIGAR text with and without M, the MAPQ tables at every
// index and at clamped counts, the reported lines of every pair class crossed with every rescue status, the flag fix-up of
// the anchor, every agreement predicate with one field wrong at a time, and the worked lines of spm_hip.h.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/jst_sam_core.hpp"

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
#define EXPECT_STR(got, want)                                                                                          \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        const std::string g_ = (got), w_ = (want);                                                                     \
        if (g_ != w_) {                                                                                                \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d:\n  got  %s\n  want %s\n", __FILE__, __LINE__, g_.c_str(), w_.c_str());          \
        }                                                                                                              \
    } while (0)

static const uint32_t X = kSamNone;

// ---- numbers ----
static void number_cases()
{
    std::vector<uint64_t> vs = {0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 4294967295ull, 4294967296ull,
                                9999999999999999999ull, 10000000000000000000ull, 18446744073709551615ull};
    for (uint64_t p = 10; p < 1000000000000000000ull; p *= 10) {
        vs.push_back(p - 1);
        vs.push_back(p);
        vs.push_back(p + 1);
    }
    for (uint64_t v : vs) {
        const std::string want = std::to_string(v);
        const uint32_t len = jst_sam_dec_len(v);
        EXPECT_TRUE(len == want.size());
        std::string got;
        for (uint32_t i = 0; i < len; ++i)
            got += jst_sam_dec_char(v, len, i);
        EXPECT_STR(got, want);
    }
    for (int32_t v : {0, 1, -1, 9, -9, 10, -10, 99, -99, 100, -100, 200, -200, 2147483647, -2147483647, INT32_MIN}) {
        const std::string want = std::to_string(v);
        const uint32_t len = jst_sam_int_len(v);
        EXPECT_TRUE(len == want.size());
        std::string got;
        for (uint32_t i = 0; i < len; ++i)
            got += jst_sam_int_char(v, len, i);
        EXPECT_STR(got, want);
    }
}

// ---- every sink operation: what the measuring sink adds is what the serial sink writes ----
template <class Op> static std::string through(Op &&op)
{
    jst_sam_measure M;
    op(M);
    std::string s(M.n + 4, '#');
    jst_sam_serial W{s.data(), M.n, 0};
    op(W);
    EXPECT_TRUE(W.n == M.n);
    EXPECT_TRUE(s.compare(M.n, 4, "####") == 0); // nothing beyond what was measured
    // a sink with too little room counts on and writes nothing beyond its cap
    std::string t(M.n + 1, '#');
    jst_sam_serial C{t.data(), M.n / 2, 0};
    op(C);
    EXPECT_TRUE(C.n == M.n && t.compare(M.n / 2, std::string::npos, std::string(M.n + 1 - M.n / 2, '#')) == 0);
    EXPECT_TRUE(t.compare(0, M.n / 2, s, 0, M.n / 2) == 0);
    s.resize(M.n);
    return s;
}

static uint32_t word(uint32_t len, uint32_t op) { return len << 4 | op; }
static const uint32_t EQ = SPM_CIGAR_EQ, MM = SPM_CIGAR_X, IN = SPM_CIGAR_INS, DE = SPM_CIGAR_DEL;

static std::string cigar_text(const std::vector<uint32_t> &w, bool merge)
{
    return through([&](auto &k) { k.cigar(w.data(), (uint32_t)w.size(), merge); });
}

static void field_cases()
{
    EXPECT_STR(through([](auto &k) { k.text(SPM_SAM_LIT("\t*\t*")); }), "\t*\t*");
    EXPECT_STR(through([](auto &k) { k.text(SPM_SAM_LIT("")); }), "");
    EXPECT_STR(through([](auto &k) { k.text(SPM_SAM_LIT("\tXR:i:1")); }), "\tXR:i:1");
    EXPECT_STR(through([](auto &k) { k.num(0, 0, 0, false); }), "0");
    EXPECT_STR(through([](auto &k) { k.num(SPM_SAM_LIT("\t"), 4294967295ull, false); }), "\t4294967295");
    EXPECT_STR(through([](auto &k) { k.num(SPM_SAM_LIT("\tNM:i:"), 18446744073709551615ull, false); }), "\tNM:i:18446744073709551615");
    EXPECT_STR(through([](auto &k) { k.num(SPM_SAM_LIT("\t"), jst_sam_int_abs(-200), true); }), "\t-200");
    EXPECT_STR(through([](auto &k) { k.num(SPM_SAM_LIT("\t=\t"), jst_sam_int_abs(INT32_MIN), true); }), "\t=\t-2147483648");
    const char name[] = "read/1@x";
    EXPECT_STR(through([&](auto &k) { k.bytes(name, 8); }), "read/1@x");
    EXPECT_STR(through([&](auto &k) { k.bytes(name, 0); }), "");
    const uint8_t ranks[] = {0, 1, 2, 3, 4, 200, 3, 2};
    EXPECT_STR(through([&](auto &k) { k.seq(ranks, 8, "ACGT", 4); }), "ACGTNNTG");
    EXPECT_STR(through([&](auto &k) { k.seq(ranks, 8, "ACGTN", 5); }), "ACGTNNTG");
    EXPECT_STR(through([&](auto &k) { k.seq(ranks, 0, "ACGT", 4); }), "");
    // CIGAR
    EXPECT_STR(cigar_text({word(30, EQ)}, false), "30=");
    EXPECT_STR(cigar_text({word(30, EQ)}, true), "30M");
    EXPECT_STR(cigar_text({word(30, IN)}, true), "30I");
    EXPECT_STR(cigar_text({word(20, EQ), word(1, MM), word(11, EQ)}, false), "20=1X11=");
    EXPECT_STR(cigar_text({word(20, EQ), word(1, MM), word(11, EQ)}, true), "32M");
    EXPECT_STR(cigar_text({word(5, EQ), word(2, IN), word(7, EQ), word(1, MM)}, false), "5=2I7=1X");
    EXPECT_STR(cigar_text({word(5, EQ), word(2, IN), word(7, EQ), word(1, MM)}, true), "5M2I8M");
    EXPECT_STR(cigar_text({word(3, DE), word(9, MM), word(1, DE)}, true), "3D9M1D");
    EXPECT_STR(cigar_text({word(0xFFFFFFF, EQ), word(0xFFFFFFF, MM)}, true), "536870910M");
    EXPECT_STR(cigar_text({word(0xFFFFFFF, EQ), word(0xFFFFFFF, MM)}, false), "268435455=268435455X");
    for (uint32_t n : {63u, 64u, 65u, 128u, 129u}) { // alternating 1= 1X ... : n words, one M; with an I in the middle, three items
        std::vector<uint32_t> w;
        std::string plain;
        for (uint32_t i = 0; i < n; ++i) {
            w.push_back(word(i % 9 + 1, i % 2 ? MM : EQ));
            plain += std::to_string(i % 9 + 1) + (i % 2 ? "X" : "=");
        }
        uint64_t q, r, total = 0;
        for (uint32_t x : w)
            total += x >> 4;
        jst_sam_cigar_spans(w.data(), n, q, r);
        EXPECT_TRUE(q == total && r == total);
        EXPECT_STR(cigar_text(w, false), plain);
        EXPECT_STR(cigar_text(w, true), std::to_string(total) + "M");
        uint64_t left = 0;
        for (uint32_t i = 0; i < 64 && i < n; ++i)
            left += w[i] >> 4;
        if (n > 64) { // an insertion right behind the 64th word: the run that ends at a wave's last lane
            std::vector<uint32_t> v(w);
            v.insert(v.begin() + 64, word(2, IN));
            EXPECT_STR(cigar_text(v, true), std::to_string(left) + "M2I" + std::to_string(total - left) + "M");
            jst_sam_cigar_spans(v.data(), n + 1, q, r);
            EXPECT_TRUE(q == total + 2 && r == total);
            v[64] = word(2, DE);
            jst_sam_cigar_spans(v.data(), n + 1, q, r);
            EXPECT_TRUE(q == total && r == total + 2);
        }
    }
}

// ---- MAPQ ----
static void mapq_cases()
{
    const jst_sam_mapq_tables D = jst_sam_default_tables();
    const uint8_t unique[4] = {60, 40, 30, 20}, multi[4] = {3, 1, 1, 0};
    for (uint32_t n_next : {0u, 1u, 2u, 3u, 4u, 1000u, 0xFFFFFFFFu}) {
        EXPECT_TRUE(jst_sam_mapq(D, 0, n_next) == 0);
        EXPECT_TRUE(jst_sam_mapq(D, 1, n_next) == unique[n_next < 3 ? n_next : 3]);
        for (uint32_t n_best : {2u, 3u, 4u, 5u, 6u, 1000u, 0xFFFFFFFFu})
            EXPECT_TRUE(jst_sam_mapq(D, n_best, n_next) == multi[(n_best < 5 ? n_best : 5) - 2]);
    }
    spm_sam_opts o{};
    const uint8_t u2[4] = {9, 8, 7, 6}, m2[4] = {5, 4, 250, 2};
    std::memcpy(o.mapq_unique, u2, 4);
    std::memcpy(o.mapq_multi, m2, 4);
    jst_sam_mapq_tables T = jst_sam_tables_of(o);
    for (uint32_t i = 0; i < 4; ++i) {
        EXPECT_TRUE(jst_sam_mapq(T, 1, i) == u2[i]);
        EXPECT_TRUE(jst_sam_mapq(T, i + 2, 77) == m2[i]);
    }
    EXPECT_TRUE(jst_sam_mapq(T, 0xFFFFFFFFu, 0xFFFFFFFFu) == 2 && jst_sam_mapq(T, 1, 0xFFFFFFFFu) == 6 && jst_sam_mapq(T, 0, 0) == 0);
    o.mapq_defaults = 1; // the tables of the opts are not read
    T = jst_sam_tables_of(o);
    EXPECT_TRUE(jst_sam_mapq(T, 1, 0) == 60 && jst_sam_mapq(T, 2, 0) == 3);
}

// ---- a paired fixture: five pairs, reads of 30 symbols ----
struct fixture
{
    std::vector<spm_jst_ref_locus> loci;
    std::vector<uint32_t> ops, rescue_ops;
    std::vector<spm_jst_read> reads;
    std::vector<spm_jst_pair> pairs;
    std::vector<spm_jst_rescue> rescues;
    std::vector<uint32_t> first;
    std::vector<uint8_t> ranks;
    std::vector<uint32_t> offsets;
    std::vector<int32_t> m;
    std::string names;
    std::vector<uint64_t> name_off;
    jst_sam_src S;

    void locus(uint32_t pattern, uint64_t b, int32_t score, std::vector<uint32_t> words, uint32_t n_hap = 2)
    {
        spm_jst_ref_locus L{};
        uint64_t q, r;
        jst_sam_cigar_spans(words.data(), (uint32_t)words.size(), q, r);
        L.pattern = pattern;
        L.ref_begin = b;
        L.ref_end = b + r;
        L.score = score;
        L.cigar_off = (uint32_t)ops.size();
        L.cigar_len = (uint32_t)words.size();
        L.n_haplotypes = n_hap;
        L.n_records = n_hap;
        for (uint32_t w : words) {
            ops.push_back(w);
            const uint32_t op = w & 15u;
            L.ref_score += op == EQ ? 0 : (int32_t)(w >> 4);
        }
        loci.push_back(L);
    }
    void read(uint32_t first_locus, uint32_t n, uint32_t n_forward, uint32_t primary, uint32_t n_best, uint32_t n_next)
    {
        spm_jst_read R{};
        R.first_locus = first_locus;
        R.n_loci = n;
        R.n_forward = n_forward;
        R.primary = primary;
        R.best = primary == X ? -1 : loci[primary].score;
        R.best_ref_score = primary == X ? -1 : loci[primary].ref_score;
        R.n_best = n_best;
        R.n_next = n_next;
        reads.push_back(R);
    }
    void pair(uint32_t l1, uint32_t l2, bool proper, int32_t tlen, uint32_t n_best, uint32_t n_next)
    {
        spm_jst_pair R{};
        const bool un1 = l1 == X, un2 = l2 == X;
        const bool rev1 = !un1 && (loci[l1].pattern & 1), rev2 = !un2 && (loci[l2].pattern & 1);
        R.locus1 = l1;
        R.locus2 = l2;
        R.tlen = tlen;
        R.best = proper ? loci[l1].score + loci[l2].score : -1;
        R.n_pairs = R.n_best = proper ? n_best : 0;
        R.n_next = n_next;
        R.flag1 = jst_pairs_flag(false, proper, un1, un2, rev1, rev2);
        R.flag2 = jst_pairs_flag(true, proper, un2, un1, rev2, rev1);
        pairs.push_back(R);
    }
    fixture()
    {
        locus(0, 1000, 0, {word(30, EQ)});                            // 0  pair 0 mate 1 forward
        locus(3, 1170, 1, {word(20, EQ), word(1, MM), word(9, EQ)});  // 1  pair 0 mate 2 reverse: the proper partner
        locus(3, 7000, 0, {word(30, EQ)});                            // 2  ... its own primary, far away
        locus(4, 500, 0, {word(30, EQ)});                             // 3  pair 1 mate 1 forward, mate 2 unmapped
        locus(12, 2000, 0, {word(30, EQ)});                           // 4  pair 3 mate 1 forward
        locus(14, 5000, 1, {word(10, EQ), word(1, IN), word(19, EQ)}); // 5  pair 3 mate 2 forward: discordant
        locus(19, 720, 0, {word(30, EQ)});                            // 6  pair 4 mate 2 reverse, mate 1 unmapped
        read(0, 1, 1, 0, 1, 0);
        read(1, 2, 0, 2, 1, 1);
        read(3, 1, 1, 3, 1, 0);
        read(4, 0, 0, X, 0, 0);
        read(4, 0, 0, X, 0, 0);
        read(4, 0, 0, X, 0, 0);
        read(4, 1, 1, 4, 2, 0);
        read(5, 1, 1, 5, 1, 2);
        read(6, 0, 0, X, 0, 0);
        read(6, 1, 0, 6, 3, 0);
        pair(0, 1, true, 200, 1, 0);
        pair(3, X, false, 0, 0, 0);
        pair(X, X, false, 0, 0, 0);
        pair(4, 5, false, 0, 0, 0);
        pair(X, 6, false, 0, 0, 0);
        for (uint32_t p = 0; p < 20; ++p) {
            offsets.push_back((uint32_t)ranks.size());
            m.push_back(30);
            for (uint32_t i = 0; i < 30; ++i)
                ranks.push_back((uint8_t)((p + i * i) % 4));
        }
        m[14] = 30; // (10= 1I 19=: 30 query symbols)
        bind();
        S.rname = "chr";
        S.rname_len = 3;
        S.symbols = "ACGT";
        S.tables = jst_sam_default_tables();
    }
    void bind()
    {
        first.assign(pairs.size(), X);
        for (size_t j = rescues.size(); j-- > 0;)
            if (rescues[j].pair < pairs.size())
                first[rescues[j].pair] = (uint32_t)j;
        S.loci = loci.data();
        S.n_loci = (uint32_t)loci.size();
        S.ops = ops.data();
        S.n_ops = ops.size();
        S.reads = reads.data();
        S.n_reads = (uint32_t)reads.size();
        S.strands = 2;
        S.pairs = pairs.data();
        S.n_pairs = (uint32_t)pairs.size();
        S.rescues = rescues.empty() ? nullptr : rescues.data();
        S.n_rescues = (uint32_t)rescues.size();
        S.rescue_ops = rescue_ops.data();
        S.n_rescue_ops = rescue_ops.size();
        S.first_rescue = rescues.empty() ? nullptr : first.data();
        S.ranks = ranks.data();
        S.offsets = offsets.data();
        S.m = m.data();
        S.n_needles = (uint32_t)m.size();
        S.sigma = 4;
    }
    // a rescue record of `pair` that rescues mate `y` (0: mate 1) beside the pair's locus of the other mate
    void rescue(uint32_t pair_, uint32_t y, uint16_t status, int32_t score, uint64_t b, int32_t tlen)
    {
        const spm_jst_pair &P = pairs[pair_];
        spm_jst_rescue R{};
        const uint32_t anchor = y ? P.locus1 : P.locus2;
        const bool a_rev = loci[anchor].pattern & 1;
        R.pair = pair_;
        R.anchor = anchor;
        R.pattern = jst_rescue_needle(pair_, y ^ 1u, loci[anchor].pattern);
        R.status = status;
        R.score = -1;
        if (status != SPM_RESCUE_NONE) {
            R.ref_begin = b;
            R.ref_end = b + 30;
            R.score = score;
            R.cigar_off = (uint32_t)rescue_ops.size();
            R.cigar_len = 3;
            for (uint32_t w : {word(10, EQ), word((uint32_t)score, MM), word(20 - (uint32_t)score, EQ)})
                rescue_ops.push_back(w);
            R.tlen = status == SPM_RESCUE_RESCUED ? tlen : 0;
        }
        R.flag = jst_pairs_flag(y == 1, status == SPM_RESCUE_RESCUED, status == SPM_RESCUE_NONE, false, status != SPM_RESCUE_NONE && !a_rev, a_rev);
        rescues.push_back(R);
        bind();
    }
};

static std::string line_text(const jst_sam_src &S, const spm_sam_line &L, const jst_sam_aux &A)
{
    jst_sam_fields F;
    ++checks;
    if (!jst_sam_resolve(S, L, A, F, true)) {
        ++failures;
        std::printf("FAILED: a line does not resolve (read %u, kind %u)\n", L.read, L.kind);
        return "";
    }
    std::string s = through([&](auto &k) { jst_sam_compose(S, F, k); });
    EXPECT_TRUE(!s.empty() && s.back() == '\n');
    for (char &c : s)
        c = c == '\t' ? ' ' : c;
    s.pop_back();
    return s;
}

// all lines of the fixture, in line order
static std::vector<std::string> all_lines(const fixture &f, bool *ok = nullptr)
{
    std::vector<std::string> out;
    if (ok)
        *ok = true;
    for (uint32_t r = 0; r < f.S.n_reads; ++r) {
        jst_sam_reported own, other;
        int32_t tlen = 0;
        bool good = true;
        if (f.S.pairs) {
            const jst_sam_pair_plan plan = jst_sam_plan_pair(f.S, r / 2);
            good = plan.ok;
            own = plan.mate[r & 1];
            other = plan.mate[(r & 1) ^ 1];
            tlen = r & 1 ? -plan.tlen : plan.tlen;
        } else {
            own = jst_sam_plan_single(f.S, r, good);
        }
        if (!good) {
            if (ok)
                *ok = false;
            continue;
        }
        const uint32_t n = jst_sam_line_count(f.S.reads[r], own, f.S.flags);
        std::vector<spm_sam_line> lines(n);
        std::vector<jst_sam_aux> aux(n);
        jst_sam_read_lines(f.S, r, own, f.S.pairs ? &other : nullptr, tlen, lines.data(), aux.data(), n);
        for (uint32_t i = 0; i < n; ++i)
            out.push_back(line_text(f.S, lines[i], aux[i]));
    }
    return out;
}

static std::string seq_of(const fixture &f, uint32_t pattern)
{
    std::string s;
    for (uint32_t i = 0; i < 30; ++i)
        s += "ACGT"[f.ranks[f.offsets[pattern] + i]];
    return s;
}

static void pair_cases()
{
    fixture f;
    std::vector<std::string> L = all_lines(f);
    EXPECT_TRUE(L.size() == 10);
    // the worked cases of spm_hip.h: a proper pair, one mate only, nobody mapped
    EXPECT_STR(L[0], "0 99 chr 1001 60 30= = 1171 200 " + seq_of(f, 0) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:1 X1:i:0");
    EXPECT_STR(L[1], "0 147 chr 1171 60 20=1X9= = 1001 -200 " + seq_of(f, 3) + " * NM:i:1 XH:i:1 XN:i:2 X0:i:1 X1:i:0");
    EXPECT_STR(L[2], "1 73 chr 501 60 30= = 501 0 " + seq_of(f, 4) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:1 X1:i:0");
    EXPECT_STR(L[3], "1 133 chr 501 0 * = 501 0 " + seq_of(f, 6) + " *");
    EXPECT_STR(L[4], "2 77 * 0 0 * * 0 0 " + seq_of(f, 8) + " *");
    EXPECT_STR(L[5], "2 141 * 0 0 * * 0 0 " + seq_of(f, 10) + " *");
    // discordant: each mate's own read counts (n_best 2 -> multi[0]; n_best 1, n_next 2 -> unique[2])
    EXPECT_STR(L[6], "3 65 chr 2001 3 30= = 5001 0 " + seq_of(f, 12) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:2 X1:i:0");
    EXPECT_STR(L[7], "3 129 chr 5001 30 10=1I19= = 2001 0 " + seq_of(f, 14) + " * NM:i:1 XH:i:1 XN:i:2 X0:i:1 X1:i:2");
    EXPECT_STR(L[8], "4 101 chr 721 0 * = 721 0 " + seq_of(f, 16) + " *");
    EXPECT_STR(L[9], "4 153 chr 721 1 30= = 721 0 " + seq_of(f, 19) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:3 X1:i:0");
    // names, M, secondaries
    f.names = "ab@c!~";
    f.name_off = {0, 1, 2, 4, 5, 6};
    f.S.names = f.names.data();
    f.S.name_off = f.name_off.data();
    f.S.flags = SPM_SAM_CIGAR_M | SPM_SAM_SECONDARY;
    L = all_lines(f);
    EXPECT_TRUE(L.size() == 11);
    EXPECT_STR(L[1], "a 147 chr 1171 60 30M = 1001 -200 " + seq_of(f, 3) + " * NM:i:1 XH:i:1 XN:i:2 X0:i:1 X1:i:0");
    EXPECT_STR(L[2], "a 401 chr 7001 255 30M = 1001 0 * * NM:i:0 XH:i:0 XN:i:2"); // 0x100 0x10 0x1 0x80; the mate is forward
    EXPECT_STR(L[5], "@c 77 * 0 0 * * 0 0 " + seq_of(f, 8) + " *");
    EXPECT_STR(L[8], "! 129 chr 5001 30 10M1I19M = 2001 0 " + seq_of(f, 14) + " * NM:i:1 XH:i:1 XN:i:2 X0:i:1 X1:i:2");
    f.S.names = nullptr;
    f.S.flags = 0;

    // ---- pair 1 (mate 1 mapped) crossed with the status of its one rescue record ----
    for (uint16_t status : {SPM_RESCUE_RESCUED, SPM_RESCUE_NONE, SPM_RESCUE_NOT_CONCORDANT}) {
        fixture g;
        g.rescue(1, 1, status, 4, 670, 200);
        jst_sam_pair_plan P = jst_sam_plan_pair(g.S, 1);
        EXPECT_TRUE(P.ok);
        if (status != SPM_RESCUE_RESCUED) { // changes nothing
            const jst_sam_pair_plan Q = jst_sam_plan_pair(f.S, 1);
            EXPECT_TRUE(P.mate[0].kind == SPM_SAM_LOCUS && P.mate[1].kind == SPM_SAM_UNMAPPED && P.tlen == 0);
            EXPECT_TRUE(P.mate[0].flag == Q.mate[0].flag && P.mate[1].flag == Q.mate[1].flag && P.mate[0].mapq == Q.mate[0].mapq);
            EXPECT_TRUE(all_lines(g) == all_lines(f));
            continue;
        }
        EXPECT_TRUE(P.mate[0].kind == SPM_SAM_LOCUS && P.mate[0].source == 3 && P.mate[0].flag == 0x63);
        EXPECT_TRUE(P.mate[1].kind == SPM_SAM_RESCUE && P.mate[1].source == 0 && P.mate[1].flag == 0x93 && P.tlen == 200);
        EXPECT_TRUE(P.mate[0].mapq == 60 && P.mate[1].mapq == 60 && P.mate[1].x0 == 1 && P.mate[1].x1 == 0);
        L = all_lines(g);
        EXPECT_STR(L[2], "1 99 chr 501 60 30= = 671 200 " + seq_of(g, 4) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:1 X1:i:0");
        EXPECT_STR(L[3], "1 147 chr 671 60 10=4X16= = 501 -200 " + seq_of(g, 7) + " * NM:i:4 XR:i:1 X0:i:1 X1:i:0");
    }
    { // pair 4: mate 2 reverse mapped, mate 1 rescued forward; the anchor read has n_best 3 -> both MAPQ 1
        fixture g;
        g.rescue(4, 0, SPM_RESCUE_RESCUED, 2, 500, 250);
        const jst_sam_pair_plan P = jst_sam_plan_pair(g.S, 4);
        EXPECT_TRUE(P.ok && P.mate[0].kind == SPM_SAM_RESCUE && P.mate[0].flag == 0x63 && P.mate[1].flag == 0x93 && P.tlen == 250);
        EXPECT_TRUE(P.mate[0].mapq == 1 && P.mate[1].mapq == 1 && P.mate[0].x0 == 3);
        L = all_lines(g);
        EXPECT_STR(L[8], "4 99 chr 501 1 10=2X18= = 721 250 " + seq_of(g, 16) + " * NM:i:2 XR:i:1 X0:i:3 X1:i:0");
        EXPECT_STR(L[9], "4 147 chr 721 1 30= = 501 -250 " + seq_of(g, 19) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:3 X1:i:0");
    }
    // ---- pair 3 (discordant): two records, every combination of statuses; two RESCUED with unequal and equal scores ----
    for (uint16_t s0 : {SPM_RESCUE_RESCUED, SPM_RESCUE_NONE, SPM_RESCUE_NOT_CONCORDANT})
        for (uint16_t s1 : {SPM_RESCUE_RESCUED, SPM_RESCUE_NONE, SPM_RESCUE_NOT_CONCORDANT})
            for (int32_t score0 : {3, 5, 7}) {
                fixture g;
                g.rescue(3, 0, s0, score0, 5100, -130); // rescues mate 1 (reverse) beside mate 2 forward at 5000
                g.rescue(3, 1, s1, 5, 2120, 150);       // rescues mate 2 (reverse) beside mate 1 forward at 2000
                const jst_sam_pair_plan P = jst_sam_plan_pair(g.S, 3);
                EXPECT_TRUE(P.ok);
                const bool r0 = s0 == SPM_RESCUE_RESCUED, r1 = s1 == SPM_RESCUE_RESCUED;
                const int used = r0 && r1 ? (score0 <= 5 ? 0 : 1) : r0 ? 0 : r1 ? 1 : -1;
                if (used < 0) {
                    EXPECT_TRUE(P.mate[0].kind == SPM_SAM_LOCUS && P.mate[1].kind == SPM_SAM_LOCUS && P.tlen == 0 && P.mate[0].flag == 0x41);
                    EXPECT_TRUE(all_lines(g) == all_lines(f));
                } else if (used == 0) { // mate 1 rescued: both lines take mate 2's counts (1, 2) -> 30
                    EXPECT_TRUE(P.mate[0].kind == SPM_SAM_RESCUE && P.mate[0].source == 0 && P.mate[0].flag == 0x53 && P.tlen == -130);
                    EXPECT_TRUE(P.mate[1].kind == SPM_SAM_LOCUS && P.mate[1].source == 5 && P.mate[1].flag == (0x81 | 0x2 | 0x20));
                    EXPECT_TRUE(P.mate[0].mapq == 30 && P.mate[1].mapq == 30 && P.mate[0].x1 == 2 && P.mate[0].pos == 5101);
                } else { // mate 2 rescued: mate 1's counts (2, 0) -> 3
                    EXPECT_TRUE(P.mate[1].kind == SPM_SAM_RESCUE && P.mate[1].source == 1 && P.mate[1].flag == 0x93 && P.tlen == 150);
                    EXPECT_TRUE(P.mate[0].kind == SPM_SAM_LOCUS && P.mate[0].source == 4 && P.mate[0].flag == 0x63 && P.mate[0].mapq == 3);
                }
                if (used == 0) { // with secondaries the rescued mate's own locus becomes a secondary line behind it
                    g.S.flags = SPM_SAM_SECONDARY;
                    L = all_lines(g);
                    EXPECT_TRUE(L.size() == 12);
                    EXPECT_STR(L[8], "3 321 chr 2001 255 30= = 5001 0 * * NM:i:0 XH:i:0 XN:i:2"); // 0x100 0x1 0x40, mate forward
                    EXPECT_TRUE(L[7].rfind("3 83 chr 5101 30 ", 0) == 0 && L[9].rfind("3 163 chr 5001 30 10=1I19= = 5101 130 ", 0) == 0);
                }
            }
    // ---- a rescue record where there cannot be one: a proper pair, an unmapped pair ----
    for (uint32_t p : {0u, 2u}) {
        fixture g;
        spm_jst_rescue R{};
        R.pair = p;
        R.pattern = 4 * p + 3;
        R.anchor = p == 0 ? 0 : X;
        R.status = SPM_RESCUE_NONE;
        g.rescues.push_back(R);
        g.bind();
        EXPECT_TRUE(!jst_sam_plan_pair(g.S, p).ok);
    }
    // ---- the flag fix-up of the anchor ----
    EXPECT_TRUE(jst_sam_anchor_flag(0x49, 0x93) == 0x63);        // mate 1 forward, mate 2 rescued reverse
    EXPECT_TRUE(jst_sam_anchor_flag(0x99, 0x63) == 0x93);        // mate 2 reverse, mate 1 rescued forward: no 0x20
    EXPECT_TRUE(jst_sam_anchor_flag(0x41 | 0x20, 0x63) == 0x43); // a discordant anchor whose old mate was reverse: 0x20 is the rescue's
    EXPECT_TRUE(jst_sam_anchor_flag(0x81, 0x53) == 0xA3);
    // ---- choosing among a pair's records ----
    spm_jst_rescue c[2] = {};
    c[0].status = c[1].status = SPM_RESCUE_RESCUED;
    c[0].score = 4;
    c[1].score = 3;
    EXPECT_TRUE(jst_sam_choose_rescue(c, 2) == 1 && jst_sam_choose_rescue(c, 1) == 0 && jst_sam_choose_rescue(c, 0) == -1);
    c[1].score = 4;
    EXPECT_TRUE(jst_sam_choose_rescue(c, 2) == 0);
    c[0].status = SPM_RESCUE_NOT_CONCORDANT;
    EXPECT_TRUE(jst_sam_choose_rescue(c, 2) == 1);
    c[1].status = SPM_RESCUE_NONE;
    EXPECT_TRUE(jst_sam_choose_rescue(c, 2) == -1);
}

// ---- single-end ----
static void single_cases()
{
    fixture f;
    f.S.pairs = nullptr;
    f.S.n_pairs = 0;
    std::vector<std::string> L = all_lines(f);
    EXPECT_TRUE(L.size() == 10);
    EXPECT_STR(L[0], "0 0 chr 1001 60 30= * 0 0 " + seq_of(f, 0) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:1 X1:i:0");
    EXPECT_STR(L[1], "1 16 chr 7001 40 30= * 0 0 " + seq_of(f, 3) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:1 X1:i:1");
    EXPECT_STR(L[3], "3 4 * 0 0 * * 0 0 " + seq_of(f, 6) + " *");
    f.S.flags = SPM_SAM_SECONDARY;
    L = all_lines(f);
    EXPECT_TRUE(L.size() == 11);
    EXPECT_STR(L[1], "1 16 chr 7001 40 30= * 0 0 " + seq_of(f, 3) + " * NM:i:0 XH:i:0 XN:i:2 X0:i:1 X1:i:1");
    EXPECT_STR(L[2], "1 272 chr 1171 255 20=1X9= * 0 0 * * NM:i:1 XH:i:1 XN:i:2");
    // inside an insertion: printed as it is
    fixture g;
    g.loci[3].ref_end = g.loci[3].ref_begin;
    g.ops[g.loci[3].cigar_off] = word(30, IN);
    g.loci[3].ref_score = 30;
    g.S.pairs = nullptr;
    EXPECT_STR(all_lines(g)[2], "2 0 chr 501 60 30I * 0 0 " + seq_of(g, 4) + " * NM:i:30 XH:i:0 XN:i:2 X0:i:1 X1:i:0");
}

// ---- the agreement predicates, one field wrong at a time ----
static void predicate_cases()
{
    {
        fixture f;
        for (uint32_t r = 0; r < 10; ++r)
            EXPECT_TRUE(jst_sam_read_ok(f.S.loci, f.S.n_loci, f.reads[r], r, 2));
        spm_jst_read R = f.reads[1];
        R.first_locus = 6;
        EXPECT_TRUE(!jst_sam_read_ok(f.S.loci, f.S.n_loci, R, 1, 2)); // the run leaves the loci
        R = f.reads[1];
        R.n_loci = 3;
        EXPECT_TRUE(!jst_sam_read_ok(f.S.loci, f.S.n_loci, R, 1, 2)); // its tail names another read
        R = f.reads[1];
        R.first_locus = 0;
        EXPECT_TRUE(!jst_sam_read_ok(f.S.loci, f.S.n_loci, R, 1, 2)); // its head does
        R = f.reads[1];
        R.primary = 3;
        EXPECT_TRUE(!jst_sam_read_ok(f.S.loci, f.S.n_loci, R, 1, 2)); // the primary lies outside the run
        R = f.reads[1];
        R.n_forward = 3;
        EXPECT_TRUE(!jst_sam_read_ok(f.S.loci, f.S.n_loci, R, 1, 2));
        R = f.reads[3];
        R.primary = 0;
        EXPECT_TRUE(!jst_sam_read_ok(f.S.loci, f.S.n_loci, R, 3, 2)); // no loci, but a primary
        EXPECT_TRUE(jst_sam_read_ok(f.S.loci, f.S.n_loci, f.reads[1], 3, 1) && !jst_sam_read_ok(f.S.loci, f.S.n_loci, f.reads[1], 1, 1));
        EXPECT_TRUE(jst_sam_in_run(f.reads[1], 1) && jst_sam_in_run(f.reads[1], 2) && !jst_sam_in_run(f.reads[1], 0) && !jst_sam_in_run(f.reads[1], 3));
        EXPECT_TRUE(!jst_sam_in_run(f.reads[3], 4));
    }
    // a pair record against the plan: a locus outside the loci, in another read's run, a flag that disagrees
    for (int wrong = 0; wrong < 6; ++wrong) {
        fixture f;
        spm_jst_pair &P = f.pairs[0];
        if (wrong == 0)
            P.locus1 = 7;
        else if (wrong == 1)
            P.locus2 = 3;
        else if (wrong == 2)
            P.flag1 ^= 0x10;
        else if (wrong == 3)
            P.flag2 ^= 0x2;
        else if (wrong == 4)
            P.locus2 = X;
        else
            f.reads[0].n_loci = 9;
        EXPECT_TRUE(!jst_sam_plan_pair(f.S, 0).ok);
        EXPECT_TRUE(jst_sam_plan_pair(f.S, 1).ok);
    }
    {
        fixture f;
        f.pairs[3].locus1 = X; // a pair that is not proper reports the read summary's primaries
        EXPECT_TRUE(!jst_sam_plan_pair(f.S, 3).ok);
    }
    // a rescue record: one field wrong at a time
    {
        fixture f;
        f.rescue(1, 1, SPM_RESCUE_RESCUED, 4, 670, 200);
        const spm_jst_rescue good = f.rescues[0];
        EXPECT_TRUE(jst_sam_rescue_ok(good, f.pairs[1], 1, 5) && jst_sam_rescue_names_pair(good, 5));
        spm_jst_rescue R = good;
        R.pair = 5;
        EXPECT_TRUE(!jst_sam_rescue_names_pair(R, 5) && !jst_sam_rescue_ok(R, f.pairs[1], 1, 5)); // a pair outside the pairs
        R = good;
        R.pattern = 11;
        EXPECT_TRUE(!jst_sam_rescue_names_pair(R, 5));                                          // a needle of another pair
        R = good;
        R.anchor = 4;
        EXPECT_TRUE(!jst_sam_rescue_ok(R, f.pairs[1], 1, 5));                                   // an anchor that is not the pair's locus
        R = good;
        R.pattern = 5; // rescues mate 1: the anchor would be locus2, which the pair does not have
        EXPECT_TRUE(!jst_sam_rescue_ok(R, f.pairs[1], 1, 5));
        R = good;
        R.status = 3;
        EXPECT_TRUE(!jst_sam_rescue_ok(R, f.pairs[1], 1, 5));
        EXPECT_TRUE(!jst_sam_rescue_ok(good, f.pairs[1], 2, 5));
        spm_jst_pair proper = f.pairs[1];
        proper.flag1 |= 0x2;
        EXPECT_TRUE(!jst_sam_rescue_ok(good, proper, 1, 5));
        f.rescues[0].anchor = 4;
        EXPECT_TRUE(!jst_sam_plan_pair(f.S, 1).ok);
    }
    {   // the order of the records: (pair, mate rescued), strictly
        fixture f;
        f.rescue(3, 0, SPM_RESCUE_NONE, 0, 0, 0);
        f.rescue(3, 1, SPM_RESCUE_NONE, 0, 0, 0);
        f.rescue(4, 0, SPM_RESCUE_NONE, 0, 0, 0);
        EXPECT_TRUE(jst_sam_rescues_ordered(f.rescues[0], f.rescues[1]) && jst_sam_rescues_ordered(f.rescues[1], f.rescues[2]));
        EXPECT_TRUE(!jst_sam_rescues_ordered(f.rescues[1], f.rescues[0]) && !jst_sam_rescues_ordered(f.rescues[0], f.rescues[0]));
        EXPECT_TRUE(!jst_sam_rescues_ordered(f.rescues[2], f.rescues[1]));
    }
    // a transcript inside its pool
    EXPECT_TRUE(jst_sam_transcript_ok(0, 1, 1) && jst_sam_transcript_ok(7, 3, 10) && !jst_sam_transcript_ok(8, 3, 10));
    EXPECT_TRUE(!jst_sam_transcript_ok(0, 0, 10) && !jst_sam_transcript_ok(0xFFFFFFFFu, 0xFFFFFFFFu, 10) && !jst_sam_transcript_ok(0, 1, 0));
    // a line record against its sources
    {
        fixture f;
        f.rescue(1, 1, SPM_RESCUE_RESCUED, 4, 670, 200);
        jst_sam_fields F;
        const jst_sam_aux A{671, 200, 1, 0, 0};
        spm_sam_line L{};
        L.read = 2;
        L.source = 3;
        L.flag = 0x63;
        L.mapq = 60;
        L.kind = SPM_SAM_LOCUS;
        EXPECT_TRUE(jst_sam_resolve(f.S, L, A, F, true));
        spm_sam_line B = L;
        B.read = 10;
        EXPECT_TRUE(!jst_sam_resolve(f.S, B, A, F, true));
        B = L;
        B.source = 7;
        EXPECT_TRUE(!jst_sam_resolve(f.S, B, A, F, true));
        B = L;
        B.source = 2; // a locus of another read
        EXPECT_TRUE(!jst_sam_resolve(f.S, B, A, F, true));
        B = L;
        B.kind = 4;
        EXPECT_TRUE(!jst_sam_resolve(f.S, B, A, F, true));
        f.loci[3].cigar_off = (uint32_t)f.ops.size();
        EXPECT_TRUE(!jst_sam_resolve(f.S, L, A, F, true)); // the transcript leaves the pool
        f.loci[3].cigar_off = 7;                            // 10= of locus 5: 10 query symbols, the needle has 30
        f.loci[3].cigar_len = 1;
        EXPECT_TRUE(!jst_sam_resolve(f.S, L, A, F, true) && jst_sam_resolve(f.S, L, A, F, false));
        f.loci[3].cigar_off = 4;
        f.m[4] = 31;
        EXPECT_TRUE(!jst_sam_resolve(f.S, L, A, F, true));
        f.m[4] = 30;
        EXPECT_TRUE(jst_sam_resolve(f.S, L, A, F, true));
        f.loci[3].ref_end = f.loci[3].ref_begin - 1;
        EXPECT_TRUE(!jst_sam_resolve(f.S, L, A, F, true));
        spm_sam_line R{};
        R.read = 3;
        R.source = 0;
        R.flag = 0x93;
        R.kind = SPM_SAM_RESCUE;
        EXPECT_TRUE(jst_sam_resolve(f.S, R, A, F, true));
        B = R;
        B.source = 1;
        EXPECT_TRUE(!jst_sam_resolve(f.S, B, A, F, true));
        B = R;
        B.read = 2;
        EXPECT_TRUE(!jst_sam_resolve(f.S, B, A, F, true));
        f.rescues[0].cigar_len = 4;
        EXPECT_TRUE(!jst_sam_resolve(f.S, R, A, F, true));
        f.rescues[0].cigar_len = 2; // 10= 4X: 14 query symbols
        EXPECT_TRUE(!jst_sam_resolve(f.S, R, A, F, true));
        f.S.n_needles = 6;
        spm_sam_line U{};
        U.read = 3;
        U.source = X;
        U.flag = 0x85;
        EXPECT_TRUE(!jst_sam_resolve(f.S, U, A, F, true)); // needle 6 of an unmapped read 3
        f.S.n_needles = 20;
        EXPECT_TRUE(jst_sam_resolve(f.S, U, A, F, true));
    }
    // names
    EXPECT_TRUE(jst_sam_name_ok("a", 1) && jst_sam_name_ok("@", 1) && jst_sam_name_ok("**", 2) && jst_sam_name_ok("!~", 2));
    EXPECT_TRUE(!jst_sam_name_ok("*", 1) && !jst_sam_name_ok("", 0) && !jst_sam_name_ok("a b", 3) && !jst_sam_name_ok("a\tb", 3));
    EXPECT_TRUE(!jst_sam_name_ok("a\x7f", 2) && !jst_sam_name_ok("\xc3\xa4", 2));
    const std::string long_name(255, 'x');
    EXPECT_TRUE(jst_sam_name_ok(long_name.data(), 254) && !jst_sam_name_ok(long_name.data(), 255));
}

int main()
{
    number_cases();
    field_cases();
    mapq_cases();
    pair_cases();
    single_cases();
    predicate_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
