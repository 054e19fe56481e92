// pileup_vcf_core_cases.cpp -- the genotyping rule and the VCF text on the host (libspm_amd/csrc/pileup_vcf_core.hpp): the three
// default cost literals and the two priors against the formula of spm_hip.h, computed here with std::log10 and nowhere else;
// the decimal writer at 0, 9, 10, 2^31 - 1 and 2^32 - 1 and at every power of ten, through the counting sink and the storing
// one; the worked table; where a run splits into head bytes, dwords and tail bytes, for every shift and every length up to 40:
// each byte once, the dwords on 4-byte borders; the line bound against the longest line a site can have; and, on random site
// sets, the serial text builder against a host emulation of the device's scheme -- every site's length, the exclusive sum, per
// group of G sites the lines formatted into a run buffer shifted by the low bits of the run's address, the run copied by head
// bytes, dwords and tail bytes -- with groups of 1, 2, 3, 5, 8 and 128 sites, site counts around the group size, and the text
// at all four alignments: every byte behind the header written exactly once, the bytes those of the serial builder.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/pileup_vcf_core.hpp"

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

static spm_pileup_site site(uint32_t pos, uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint32_t depth, uint8_t ref)
{
    spm_pileup_site S{};
    S.pos = pos;
    S.depth = depth;
    S.counts[0] = a;
    S.counts[1] = c;
    S.counts[2] = g;
    S.counts[3] = t;
    S.ref = ref;
    return S;
}

static std::string line_of(const spm_pileup_site &S, const std::string &rname, const vc_opts &O)
{
    vc_eval E;
    vc_call(S, O, E);
    const uint32_t len = vc_line_len((uint32_t)rname.size(), S, E, O);
    if (!len)
        return "";
    std::vector<uint8_t> buf(len + 1, 0xEE);
    vc_store_sink out{buf.data()};
    vc_line_emit(out, rname.data(), (uint32_t)rname.size(), S, E, O);
    EXPECT_TRUE(out.p == buf.data() + len && buf[len] == 0xEE); // the counting sink and the storing one agree
    EXPECT_TRUE(len <= kVcMaxLine);
    return std::string(buf.begin(), buf.begin() + len);
}

static void literals()
{
    const double e = 0.01, theta = 1e-3;
    auto milli = [](double p) { return (uint32_t)std::llround(-10000.0 * std::log10(p)); };
    EXPECT_TRUE(kVcCostMatch == milli(1 - e) && kVcCostMatch == 44);
    EXPECT_TRUE(kVcCostHet == milli((1 - e) / 2 + e / 6) && kVcCostHet == 3039);
    EXPECT_TRUE(kVcCostMiss == milli(e / 3) && kVcCostMiss == 24771);
    EXPECT_TRUE(kVcPriorHet == milli(theta) && kVcPriorHet == 30000);
    EXPECT_TRUE(kVcPriorHomAlt == milli(theta / 2) && kVcPriorHomAlt == 33010);
    vc_opts O;
    EXPECT_TRUE(vc_opts_of(nullptr, O) == nullptr && O.ploidy == 2 && O.min_qual == 20 && O.cost_miss == 24771);
}

static void decimals()
{
    std::vector<uint32_t> values = {0u, 9u, 10u, 0x7FFFFFFFu, 0xFFFFFFFFu, 1u, 99u, 100u, 4294967294u};
    for (uint32_t p = 1; p < 1000000000u; p *= 10) {
        values.push_back(p * 10 - 1);
        values.push_back(p * 10);
        values.push_back(p * 10 + 1);
    }
    for (uint32_t v : values) {
        uint8_t buf[12];
        std::memset(buf, 0xEE, sizeof buf);
        vc_store_sink out{buf};
        vc_put_u32(out, v);
        vc_count_sink n;
        vc_put_u32(n, v);
        const std::string want = std::to_string(v);
        EXPECT_TRUE(n.n == want.size() && out.p == buf + want.size() && std::memcmp(buf, want.data(), want.size()) == 0 && buf[want.size()] == 0xEE);
    }
}

static void worked_table()
{
    vc_opts O;
    const std::string rname = "chr1";
    EXPECT_TRUE(line_of(site(0, 10, 10, 0, 0, 20, 0), rname, O) == "chr1\t1\t.\tA\tC\t157\tPASS\tDP=20\tGT:AD:GQ:PL\t0/1:10,10:99:157,0,190\n");
    EXPECT_TRUE(line_of(site(5, 0, 0, 3, 0, 3, 0), rname, O) == "chr1\t6\t.\tA\tG\t41\tPASS\tDP=3\tGT:AD:GQ:PL\t1/1:0,3:6:41,6,0\n");
    EXPECT_TRUE(line_of(site(9, 0, 8, 0, 8, 16, 0), rname, O) == "chr1\t10\t.\tA\tC,T\t288\tPASS\tDP=16\tGT:AD:GQ:PL\t1/2:0,8,8:99:288,144,123,144,0,123\n");
    EXPECT_TRUE(line_of(site(12, 19, 1, 0, 0, 20, 0), rname, O).empty());
    const uint32_t row1[4] = {10, 10, 0, 0}, row4[4] = {19, 1, 0, 0};
    EXPECT_TRUE(vc_cost(row1, 0, 0, 0, O) == 248150 && vc_cost(row1, 0, 1, 0, O) == 90780 && vc_cost(row1, 1, 1, 0, O) == 281160);
    EXPECT_TRUE(vc_cost(row4, 0, 0, 0, O) == 25607 && vc_cost(row4, 0, 1, 0, O) == 90780);
    EXPECT_TRUE(line_of(site(3, 0, 9, 0, 0, 9, 4), rname, O).empty()); // a reference rank above 3: no call
    vc_eval E;
    vc_call(site(3, 0, 9, 0, 0, 9, 200), O, E);
    EXPECT_TRUE(E.status == SPM_CALL_REF_N);
    // the longest line: every number ten digits, two ALTs; LowQual cannot stand beside a ten-digit QUAL, and the AD of REF and
    // the best PL are one digit, so the bound is not met, by some twenty bytes
    const uint32_t top = 0xFFFFFFFFu;
    const std::string name(kSamMaxName, 'n');
    const std::string longest = line_of(site(top - 1, 0, top, 0, top, top, 0), name, O);
    EXPECT_TRUE(!longest.empty() && longest.size() <= kVcMaxLine && longest.size() + 24 > kVcMaxLine);
    O.ploidy = 1;
    EXPECT_TRUE(line_of(site(5, 0, 0, 3, 0, 3, 0), rname, O) == "chr1\t6\t.\tA\tG\t41\tPASS\tDP=3\tGT:AD:GQ:PL\t1:0,3:41:41,0\n");
    O = vc_opts{};
    O.min_qual = 42;
    EXPECT_TRUE(line_of(site(5, 0, 0, 3, 0, 3, 0), rname, O) == "chr1\t6\t.\tA\tG\t41\tLowQual\tDP=3\tGT:AD:GQ:PL\t1/1:0,3:6:41,6,0\n");
}

static void run_splits()
{
    for (uint32_t shift = 0; shift < 4; ++shift)
        for (uint32_t B = 0; B <= 40; ++B) {
            uint32_t a = 99, b = 99;
            vc_run_split(shift, B, a, b);
            EXPECT_TRUE(shift <= a && a <= b && b <= shift + B);
            EXPECT_TRUE(a == b || (a % 4 == 0 && b % 4 == 0));
            EXPECT_TRUE(a - shift < 4 && shift + B - b < 4); // at most three head bytes, three tail bytes
            EXPECT_TRUE(!(a > shift && shift == 0));         // no head on a border
        }
}

// the device's scheme over n sites with groups of G: -> the text behind a header of `header` bytes, the buffer `misalign`
// bytes off a 4-byte border
static void emulate(const std::vector<spm_pileup_site> &sites, const std::string &rname, const vc_opts &O, uint32_t G, uint32_t header,
                    uint32_t misalign, const std::string &want)
{
    const uint32_t n = (uint32_t)sites.size();
    std::vector<uint32_t> lens(n), offs(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) { // the call stage and the exclusive sum
        vc_eval E;
        vc_call(sites[i], O, E);
        lens[i] = vc_line_len((uint32_t)rname.size(), sites[i], E, O);
        offs[i] = (uint32_t)total;
        total += lens[i];
    }
    EXPECT_TRUE(total == want.size());
    if (total != want.size())
        return;
    std::vector<uint8_t> text(header + total + 8, 0xEE);
    std::vector<uint8_t> writes(text.size(), 0);
    std::vector<uint32_t> run((G * kVcMaxLine + 3 + 3) / 4);
    bool aligned = true, inside = true;
    for (uint32_t first = 0; first < n; first += G) {
        const uint32_t last = (n - first < G ? n : first + G) - 1;
        const uint32_t r0 = offs[first], B = offs[last] + lens[last] - r0;
        const uint64_t at = (uint64_t)header + r0;
        const uint32_t shift = (uint32_t)((misalign + at) & 3u);
        uint8_t *bytes = reinterpret_cast<uint8_t *>(run.data());
        std::memset(bytes, 0xDD, run.size() * 4);
        inside = inside && shift + B <= run.size() * 4;
        for (uint32_t i = first; i <= last; ++i) { // the lanes
            if (!lens[i])
                continue;
            vc_eval E;
            vc_call(sites[i], O, E);
            vc_store_sink out{bytes + shift + (offs[i] - r0)};
            vc_line_emit(out, rname.data(), (uint32_t)rname.size(), sites[i], E, O);
            inside = inside && out.p == bytes + shift + (offs[i] - r0) + lens[i];
        }
        uint8_t *dst = text.data() + at - shift;
        uint32_t a, b;
        vc_run_split(shift, B, a, b);
        for (uint32_t p = shift; p < a; ++p) {
            dst[p] = bytes[p];
            ++writes[at - shift + p];
        }
        for (uint32_t w = a / 4; w < b / 4; ++w) {
            aligned = aligned && (misalign + at - shift + 4ull * w) % 4 == 0;
            std::memcpy(dst + 4 * w, &run[w], 4);
            for (uint32_t k = 0; k < 4; ++k)
                ++writes[at - shift + 4 * w + k];
        }
        for (uint32_t p = b; p < shift + B; ++p) {
            dst[p] = bytes[p];
            ++writes[at - shift + p];
        }
    }
    bool once = true, untouched = true;
    for (size_t k = 0; k < text.size(); ++k) {
        const bool line_byte = k >= header && k < header + total;
        once = once && writes[k] == (line_byte ? 1 : 0);
        untouched = untouched && (line_byte || text[k] == 0xEE);
    }
    EXPECT_TRUE(aligned && inside);
    EXPECT_TRUE(once && untouched);
    EXPECT_TRUE(std::memcmp(text.data() + header, want.data(), total) == 0);
}

static void schemes()
{
    std::mt19937_64 rng(20261021);
    auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const uint32_t group_sizes[] = {1, 2, 3, 5, 8, 128};
    for (uint32_t round = 0; round < 60; ++round) {
        const uint32_t G = group_sizes[round % 6];
        const uint32_t shapes[] = {0, 1, G - 1, G, G + 1, 2 * G + 1, 3 * G - 1};
        const std::string rname = std::string(1 + pick(round % 7 == 0 ? kSamMaxName : 6), 'c');
        vc_opts O;
        O.ploidy = 1 + round % 2;
        O.min_qual = pick(60);
        for (uint32_t n : shapes) {
            std::vector<spm_pileup_site> sites;
            const uint32_t kind = pick(4); // mixed; no site yields a line; every site yields one; huge numbers
            uint32_t pos = kind == 3 ? 1999999990u + pick(20) : pick(3);
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t c[4];
                const uint8_t ref = (uint8_t)pick(kind == 0 ? 5 : 4);
                for (uint32_t x = 0; x < 4; ++x)
                    c[x] = kind == 1 ? (x == ref ? 9 : 0) : kind == 2 ? (x == ref ? 0 : x == (ref + 1u) % 4 ? 9 + pick(90) : 0) : kind == 3 ? (pick(2) ? 0xFFFFFFFFu - pick(5) : pick(3)) : pick(5) * pick(2);
                sites.push_back(site(pos, c[0], c[1], c[2], c[3], kind == 3 ? 0xFFFFFFFFu : c[0] + c[1] + c[2] + c[3] + pick(2), ref));
                pos += 1 + (kind == 3 ? pick(5000000) : pick(1200));
            }
            std::string want;
            vc_serial(sites.data(), n, rname.data(), (uint32_t)rname.size(), O, 0, true, nullptr, &want);
            std::vector<spm_variant_call> calls(n);
            vc_serial(sites.data(), n, rname.data(), (uint32_t)rname.size(), O, 77, true, calls.data(), nullptr);
            uint64_t at = 77;
            bool records = true;
            for (uint32_t i = 0; i < n; ++i) {
                records = records && calls[i].offset == at && calls[i].pos == sites[i].pos && calls[i].reserved == 0 &&
                          (calls[i].len == 0) == (calls[i].status != SPM_CALL_VARIANT) &&
                          (calls[i].len == 0 || want.compare(at - 77, calls[i].len, line_of(sites[i], rname, O)) == 0);
                at += calls[i].len;
            }
            EXPECT_TRUE(records && at == 77 + want.size());
            if (kind == 1)
                EXPECT_TRUE(want.empty());
            if (kind == 2)
                EXPECT_TRUE(std::count(want.begin(), want.end(), '\n') == (long)n);
            for (uint32_t misalign = 0; misalign < 4; ++misalign)
                emulate(sites, rname, O, G, 100 + pick(4), misalign, want);
        }
    }
}

int main()
{
    literals();
    decimals();
    worked_table();
    run_splits();
    schemes();
    EXPECT_TRUE(vc_sites_in_order(nullptr, 0, 0));
    const spm_pileup_site two[2] = {site(4, 0, 0, 0, 0, 0, 0), site(4, 0, 0, 0, 0, 0, 0)};
    EXPECT_TRUE(vc_sites_in_order(two, 1, 5) && !vc_sites_in_order(two, 1, 4) && !vc_sites_in_order(two, 2, 9));
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
