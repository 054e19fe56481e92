// bgzf_core_cases.cpp -- the container of spm_hip_bgzf_frame on the host (libspm_amd/csrc/bgzf_core.hpp): CRC-32 by chunks plus
// combine against the serial byte-wise CRC, the identities the kernel's lane scheme rests on, the lane scheme itself at every
// source alignment, the geometry at the block borders, the bytes around a block, and the serial framer against bytes written
// out by hand.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/bgzf_core.hpp"

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

static std::string hex(const std::vector<uint8_t> &v)
{
    std::string s;
    char b[4];
    for (uint8_t c : v) {
        std::snprintf(b, sizeof(b), "%02x", c);
        s += b;
    }
    return s;
}

// a CRC-32 that shares nothing with the header: bit by bit, straight from the definition
static uint32_t crc32_plain(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k)
            c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return c ^ 0xFFFFFFFFu;
}

static std::vector<uint8_t> input(int kind, size_t n)
{
    std::vector<uint8_t> v(n, kind == 0 ? 0x00 : 0xff);
    if (kind == 2)
        for (size_t i = 0; i < n; ++i)
            v[i] = (uint8_t)(mix64(0xB6F2 + i) >> 17);
    return v;
}

// ---- CRC: the known value, the arithmetic, chunks plus combine ----
static void crc_cases()
{
    const char *digits = "123456789";
    EXPECT_TRUE(crc32_serial(reinterpret_cast<const uint8_t *>(digits), 9) == 0xCBF43926u);
    EXPECT_TRUE(crc32_plain(reinterpret_cast<const uint8_t *>(digits), 9) == 0xCBF43926u);
    EXPECT_TRUE(crc32_serial(nullptr, 0) == 0 && crc32_of_pure(0, 0) == 0);
    // x^0 is the unit, x^8 shifts by a byte, powers add up
    EXPECT_TRUE(crc_xpow_bytes(0) == 0x80000000u && crc_xpow_bytes(1) == 0x00800000u && crc_xpow_bytes(3) == 0x00000080u);
    for (uint32_t a : {0u, 1u, 0x80000000u, 0xDEADBEEFu, 0xFFFFFFFFu}) {
        EXPECT_TRUE(crc_mulmod(a, 0x80000000u) == a && crc_mulmod(0x80000000u, a) == a && crc_mulmod(a, 0) == 0);
        EXPECT_TRUE(crc_mulmod(a, 0x40000000u) == crc_step(a));
        EXPECT_TRUE(crc_mulmod(a, 0x12345678u) == crc_mulmod(0x12345678u, a));
        uint32_t by_steps = a;
        for (int i = 0; i < 8 * 5; ++i)
            by_steps = crc_step(by_steps);
        EXPECT_TRUE(crc_shift_bytes(a, 5) == by_steps);
        EXPECT_TRUE(crc_dword(a, 0x04030201u) == crc_byte(crc_byte(crc_byte(crc_byte(a, 1), 2), 3), 4));
    }
    for (uint64_t n : {0ull, 1ull, 2ull, 255ull, 256ull, 65280ull, 1ull << 20, (1ull << 40) + 12345})
        for (uint64_t m : {0ull, 1ull, 77ull, 65279ull, 1ull << 33})
            EXPECT_TRUE(crc_mulmod(crc_xpow_bytes(n), crc_xpow_bytes(m)) == crc_xpow_bytes(n + m));

    std::vector<size_t> lens;
    for (size_t n = 0; n <= 1100; ++n)
        lens.push_back(n);
    lens.push_back(65279);
    lens.push_back(65280);
    for (int kind = 0; kind < 3; ++kind)
        for (size_t n : lens) {
            const std::vector<uint8_t> v = input(kind, n);
            const uint32_t want = crc32_plain(v.data(), n);
            EXPECT_TRUE(crc32_serial(v.data(), n) == want);
            EXPECT_TRUE(crc32_of_pure(crc_pure(v.data(), n), n) == want);
            // leading zero bytes do not change R
            if (n && kind == 2 && n <= 1100) {
                std::vector<uint8_t> z(n + 37, 0);
                memcpy(z.data() + 37, v.data(), n);
                EXPECT_TRUE(crc_pure(z.data(), z.size()) == crc_pure(v.data(), n));
            }
            for (size_t chunks : {1u, 2u, 63u, 64u, 65u, 256u}) {
                const size_t per = (n + chunks - 1) / chunks;
                uint32_t r = 0;
                size_t seen = 0;
                for (size_t c = 0; c < chunks; ++c) {
                    const size_t lo = std::min(n, c * per), hi = std::min(n, lo + per);
                    r = crc_combine(r, crc_pure(v.data() + lo, hi - lo), hi - lo);
                    seen += hi - lo;
                }
                EXPECT_TRUE(seen == n && crc32_of_pure(r, n) == want);
            }
        }
}

// ---- the lanes of the frame kernel: their ranges tile the body at every source alignment, and their tree gives the CRC ----
static void lane_cases()
{
    for (uint32_t D : {1u, 7u, 64u, 255u, 256u, 257u, 1000u, 4080u, 4081u, 65279u, 65280u}) {
        const bgzf_lane_plan L = bgzf_plan_lanes(D);
        EXPECT_TRUE(L.chunk % 16 == 0 && (uint64_t)L.chunk * kBgzfLanes >= D + 15 && L.chunk >= 16);
        EXPECT_TRUE(L.pw[0] == crc_xpow_bytes(L.chunk) && L.pw[6] == crc_xpow_bytes(64ull * L.chunk));
        std::vector<uint32_t> ds = {1, 2, 15, 16, 17, 31, 32, 33, D / 2, D - 1, D};
        for (uint32_t d : ds) {
            if (d == 0 || d > D)
                continue;
            const std::vector<uint8_t> v = input(2, d);
            const uint32_t want = crc32_plain(v.data(), d);
            for (uint64_t a0 = 4096; a0 < 4096 + 16; ++a0) {
                const uint32_t body = bgzf_body(a0, d);
                bool ok = body <= d && d - body < 16 && (body == 0 || (a0 + body) % 16 == 0);
                uint32_t at = 0;
                for (uint32_t t = 0; t < kBgzfLanes; ++t) {
                    uint32_t lo, hi;
                    bgzf_lane_range(body, L.chunk, t, lo, hi);
                    if (hi <= lo)
                        continue;
                    // in order, gapless, whole 16-byte pieces of the source behind the first border
                    ok = ok && lo == at && hi <= body && (a0 + hi) % 16 == 0 && (lo == 0 || (a0 + lo) % 16 == 0);
                    at = hi;
                }
                ok = ok && at == body;
                EXPECT_TRUE(ok);
                EXPECT_TRUE(bgzf_crc_by_lanes(v.data(), a0, d, L) == want);
            }
        }
    }
    // all-zero and all-ff blocks of full length
    for (int kind = 0; kind < 2; ++kind) {
        const std::vector<uint8_t> v = input(kind, 65280);
        EXPECT_TRUE(bgzf_crc_by_lanes(v.data(), 4099, 65280, bgzf_plan_lanes(65280)) == crc32_plain(v.data(), 65280));
    }
}

// ---- geometry ----
static void geometry_cases()
{
    EXPECT_TRUE(bgzf_block_data(0) == 65280 && bgzf_block_data(1) == 1 && bgzf_block_data(65280) == 65280);
    for (uint32_t D : {1u, 7u, 256u, 65280u}) {
        const uint64_t ns[] = {0, 1, (uint64_t)D - 1, D, (uint64_t)D + 1, 2ull * D};
        for (uint64_t n : ns) {
            const uint64_t nb = bgzf_n_blocks(n, D);
            EXPECT_TRUE(nb == (n + D - 1) / D);
            uint64_t sum = 0;
            for (uint64_t b = 0; b < nb; ++b) {
                const uint32_t d = bgzf_block_len(n, D, b);
                EXPECT_TRUE(d >= 1 && d <= D && (b + 1 < nb ? d == D : d == n - b * D));
                EXPECT_TRUE(bgzf_block_offset(D, b) == b * (D + 31ull));
                sum += d;
            }
            EXPECT_TRUE(sum == n);
            EXPECT_TRUE(bgzf_framed_size(n, D, false) == n + 31 * nb && bgzf_framed_size(n, D, true) == n + 31 * nb + 28);
            EXPECT_TRUE(!bgzf_size_overflows(n, D));
            for (uint64_t u = 0; u < n; u += (n > 64 ? n / 7 : 1))
                EXPECT_TRUE(bgzf_data_offset(D, u) == (u / D) * (D + 31ull) + 23 + u % D);
            if (n)
                EXPECT_TRUE(bgzf_data_offset(D, n - 1) + 9 == bgzf_framed_size(n, D, false));
        }
    }
    EXPECT_TRUE(bgzf_n_blocks(0, 65280) == 0 && bgzf_framed_size(0, 65280, false) == 0 && bgzf_framed_size(0, 1, true) == 28);
    EXPECT_TRUE(bgzf_size_overflows(~0ull, 65280) && bgzf_size_overflows(~0ull / 16, 1) && !bgzf_size_overflows(1ull << 50, 1));
}

// ---- the bytes around a block ----
static void frame_byte_cases()
{
    auto head = [](uint32_t d) {
        std::vector<uint8_t> h(kBgzfHead);
        for (uint32_t i = 0; i < kBgzfHead; ++i)
            h[i] = bgzf_head_byte(d, i);
        return hex(h);
    };
    EXPECT_TRUE(head(1) == "1f8b08040000000000ff0600424302001f000101" "00feff");
    EXPECT_TRUE(head(4) == "1f8b08040000000000ff06004243020022000104" "00fbff");
    EXPECT_TRUE(head(65280) == "1f8b08040000000000ff0600424302001eff0100" "ffff00");
    EXPECT_TRUE(head(0x1234) == "1f8b08040000000000ff0600424302005212013412cbed");
    std::vector<uint8_t> t(kBgzfTail), e(kBgzfEof);
    for (uint32_t i = 0; i < kBgzfTail; ++i)
        t[i] = bgzf_tail_byte(0xff00, 0xCBF43926u, i);
    EXPECT_TRUE(hex(t) == "2639f4cb00ff0000");
    for (uint32_t i = 0; i < kBgzfEof; ++i)
        e[i] = bgzf_eof_byte(i);
    EXPECT_TRUE(hex(e) == "1f8b08040000000000ff0600424302001b0003000000000000000000");
    EXPECT_TRUE(kBgzfHead + kBgzfTail == 31 && kBgzfFrame == 31);
}

// ---- the serial framer ----
static void framer_cases()
{
    const uint8_t abc[] = {'a', 'b', 'c', 'd', 'e', 'f'};
    const std::string eof = "1f8b08040000000000ff0600424302001b0003000000000000000000";
    auto frame = [&](uint64_t n, uint32_t D, bool with_eof) {
        std::vector<uint8_t> out(bgzf_framed_size(n, D, with_eof) + 8, 0xAA);
        bgzf_frame_serial(abc, n, D, with_eof, out.data());
        for (size_t i = out.size() - 8; i < out.size(); ++i)
            EXPECT_TRUE(out[i] == 0xAA); // nothing beyond the framed size
        out.resize(out.size() - 8);
        return hex(out);
    };
    // crc32("abcdef") = 0x4b8e39ef, crc32("abcd") = 0xed82cd11, crc32("ef") = 0xfd824970
    EXPECT_TRUE(crc32_plain(abc, 6) == 0x4b8e39efu && crc32_plain(abc, 4) == 0xed82cd11u && crc32_plain(abc + 4, 2) == 0xfd824970u);
    EXPECT_TRUE(frame(6, 65280, false) == "1f8b08040000000000ff0600424302002400" "01" "0600" "f9ff" "616263646566" "ef398e4b" "06000000");
    EXPECT_TRUE(frame(6, 4, true) == "1f8b08040000000000ff0600424302002200" "01" "0400" "fbff" "61626364" "11cd82ed" "04000000"
                                     "1f8b08040000000000ff0600424302002000" "01" "0200" "fdff" "6566" "704982fd" "02000000" + eof);
    EXPECT_TRUE(frame(6, 6, true) == "1f8b08040000000000ff0600424302002400" "01" "0600" "f9ff" "616263646566" "ef398e4b" "06000000" + eof);
    EXPECT_TRUE(frame(0, 4, true) == eof && frame(0, 4, false).empty());
    // a long input, block by block
    const std::vector<uint8_t> v = input(2, 2 * 65280 + 5);
    std::vector<uint8_t> out(bgzf_framed_size(v.size(), 65280, true));
    bgzf_frame_serial(v.data(), v.size(), 65280, true, out.data());
    for (uint64_t b = 0; b < 3; ++b) {
        const uint32_t d = bgzf_block_len(v.size(), 65280, b);
        const uint8_t *blk = out.data() + bgzf_block_offset(65280, b);
        bool ok = memcmp(blk + 23, v.data() + b * 65280, d) == 0;
        const uint32_t crc = crc32_plain(v.data() + b * 65280, d);
        for (uint32_t i = 0; i < 23; ++i)
            ok = ok && blk[i] == bgzf_head_byte(d, i);
        for (uint32_t i = 0; i < 8; ++i)
            ok = ok && blk[23 + d + i] == bgzf_tail_byte(d, crc, i);
        EXPECT_TRUE(ok && (blk[16] | blk[17] << 8) == (int)d + 30);
    }
}

int main()
{
    crc_cases();
    lane_cases();
    geometry_cases();
    frame_byte_cases();
    framer_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
