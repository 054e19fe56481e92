// scan_plan_cases.cpp -- the host-side decisions of one scan (libspm_amd/csrc/scan_plan.hpp) without a device: the tile
// tables of the brute-force kernel and the span-local fallback's ranges on generated inputs, the retry policy row by row,
// the clean predicate against the status expression of the device-side fused copy, the filter's buffer sizes, the chunk
// geometry of a streaming pass.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../libspm_amd/csrc/scan_plan.hpp"

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

using table = std::vector<uint64_t>;

// every tile {cold, lo, hi} of `tab` lies in one haystack of `segs` (n + 1 offsets), starts cold `warm` symbols early
// wherever the haystack allows, and owns at most `tile` end positions; owners[p - base] counts the tiles that own p
static void check_tiles(const table &tab, const table &segs, uint64_t warm, uint64_t tile, uint64_t base, std::vector<int> &owners)
{
    EXPECT_TRUE(tab.size() % 3 == 0);
    for (size_t t = 0; t + 2 < tab.size(); t += 3) {
        const uint64_t cold = tab[t], lo = tab[t + 1], hi = tab[t + 2];
        EXPECT_TRUE(cold <= lo && lo < hi && hi - lo <= tile);
        size_t s = 0;
        while (s + 1 < segs.size() && !(segs[s] <= lo && lo < segs[s + 1]))
            ++s;
        EXPECT_TRUE(s + 1 < segs.size());
        if (s + 1 >= segs.size())
            continue;
        EXPECT_TRUE(hi <= segs[s + 1]);                                          // no tile crosses a haystack's end
        EXPECT_TRUE(cold == (lo - segs[s] >= warm ? lo - warm : segs[s]));       // ... and no warm-up its begin
        for (uint64_t p = lo; p < hi; ++p)
            if (p >= base && p - base < owners.size())
                ++owners[p - base];
            else
                EXPECT_TRUE(false);
    }
}

static void tiler_cases()
{
    std::mt19937_64 rng(0x5CA9F1A9);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int round = 0; round < 400; ++round) {
        // a scan [begin, end) of a text, with left context from ctx_begin; every third round segmented (ctx_begin = begin)
        const bool segmented = round % 3 == 2;
        const uint64_t ctx_begin = pick(0, 3000), begin = segmented || round % 3 == 0 ? ctx_begin : ctx_begin + pick(0, 5000);
        const uint64_t end = begin + pick(1, round % 7 == 0 ? 300000 : 40000);
        const uint32_t max_window = (uint32_t)pick(0, 300);
        table segs = {begin};
        if (segmented) {
            while (segs.back() < end) {
                const uint64_t kind = rng() % 5; // empty and one-symbol segments among ordinary ones
                segs.push_back(std::min(end, segs.back() + (kind == 0 ? 0 : kind == 1 ? 1 : pick(2, 9000))));
            }
            if (rng() % 2)
                segs.push_back(end); // a trailing empty segment
        } else
            segs.push_back(end);
        const table hay = segmented ? segs : table{ctx_begin, end};
        // spans that gave up: inside, across the borders of, and (the streaming kernel reads whole chunks) outside the range
        const uint64_t n_ovf = pick(0, 12);
        table ov;
        std::vector<int> want(end - begin, 0);
        for (uint64_t i = 0; i < n_ovf; ++i) {
            const uint64_t b = pick(ctx_begin > 2000 ? ctx_begin - 2000 : 0, end + 1500), len = pick(1, 6000);
            ov.push_back(b);
            ov.push_back(len);
            for (uint64_t p = std::max(begin, b >= 16 ? b - 16 : 0); p < std::min(end, b + len + max_window); ++p)
                want[p - begin] = 1;
        }
        const fallback_plan F = plan_fallback(ov.data(), n_ovf, begin, end, max_window, 256, (uint32_t)pick(1, 40));
        EXPECT_TRUE(F.warm == (max_window ? max_window - 1 : 0) && F.tile >= 1024 && F.tile % 256 == 0 && F.tile <= (1u << 20));
        std::vector<int> got(end - begin, 0);
        uint64_t total = 0;
        for (size_t r = 0; r < F.ranges.size(); ++r) {
            EXPECT_TRUE(begin <= F.ranges[r].first && F.ranges[r].first < F.ranges[r].second && F.ranges[r].second <= end); // clipped
            EXPECT_TRUE(r == 0 || F.ranges[r - 1].second < F.ranges[r].first);                                          // merged
            for (uint64_t p = F.ranges[r].first; p < F.ranges[r].second; ++p)
                got[p - begin] = 1;
            total += F.ranges[r].second - F.ranges[r].first;
        }
        EXPECT_TRUE(got == want && total == F.total);
        table tab;
        fallback_tiles(F, ctx_begin, segmented ? segs.data() : nullptr, segmented ? segs.size() - 1 : 0, tab);
        std::vector<int> owners(end - begin, 0);
        check_tiles(tab, hay, F.warm, F.tile, begin, owners);
        EXPECT_TRUE(owners == want); // every end position of a range has exactly one owner, no other position has one
        // the segmented brute-force scan: every segment tiled, with tile lengths down to a few symbols
        const uint64_t warm = pick(0, 200), tile = round % 2 ? pick(1, 64) * 4 : pick(256, 4096);
        table all;
        for (size_t s = 0; s + 1 < hay.size(); ++s)
            append_tiles(all, s == 0 ? begin : hay[s], hay[s + 1], hay[s], warm, tile);
        std::fill(owners.begin(), owners.end(), 0);
        check_tiles(all, hay, warm, tile, begin, owners);
        EXPECT_TRUE(owners == std::vector<int>(end - begin, 1));
    }
    // touching ranges are merged, overlapping ones too; a span wholly outside the range leaves nothing
    const uint64_t ov[] = {1000, 100, 1100 + 50 + 16, 10, 5000, 10, 90000, 5};
    const fallback_plan F = plan_fallback(ov, 4, 0, 80000, 50, 256, 1);
    using range = std::pair<uint64_t, uint64_t>;
    EXPECT_TRUE(F.ranges.size() == 2 && F.ranges[0] == range(984, 1226) && F.ranges[1] == range(4984, 5060) && F.total == 242 + 76);
}

// ---- the retry policy: expected values written down from the driver's rules ----
struct counters
{
    unsigned long long c[kCntBlock] = {};
    counters(unsigned long long hits, unsigned long long surv, unsigned long long overflow, unsigned long long bands,
             unsigned long long gave_up)
    {
        c[kCntHits] = hits;
        c[kCntSurvSlots] = surv;
        c[kCntVoid] = overflow;
        c[kCntBandSlots] = bands;
        c[kCntSpansGaveUp] = gave_up;
    }
};

static bool same(const retry_state &a, const retry_state &b)
{
    return a.cand_cap_override == b.cand_cap_override && a.band_scale == b.band_scale && a.seen_full == b.seen_full &&
           a.need_seen == b.need_seen;
}

static void policy_cases()
{
    using O = scan_outcome;
    filter_result cap; // survivor list 1000, band list 500, hit buffer 100, dedupe set 65536 slots (nearly full: > 8192 hits)
    cap.cand_cap = 1000, cap.band_cap = 500, cap.seen_mask = 0xFFFF;
    const uint64_t hit_cap = 100;
    const retry_state fresh;
    scan_decision d;
    // nothing happened
    d = decide_scan(counters(10, 800, 0, 100, 0).c, cap, hit_cap, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::final_hits && same(d.next, fresh) && !d.more_surv && !d.more_bands && !d.more_seen);
    // hit overflow wins over everything: no retry, no fallback
    d = decide_scan(counters(101, 5000, 1, 900, 7).c, cap, hit_cap, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::caller_overflow && same(d.next, fresh) && !d.more_surv && !d.more_bands && !d.more_seen);
    // survivor list too small: what was counted + an eighth + 4096 ...
    d = decide_scan(counters(10, 2000, 0, 100, 3).c, cap, hit_cap, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::more_room && d.more_surv && !d.more_bands && !d.more_seen && d.next.cand_cap_override == 6346 &&
                d.next.band_scale == 0 && !d.next.seen_full && !d.next.need_seen);
    // ... or four times the list, whichever is more; never beyond 2^27
    filter_result big = cap; uint64_t big_hits = 100;
    big.cand_cap = 1000000;
    d = decide_scan(counters(10, 1000001, 0, 100, 0).c, big, big_hits, fresh, 1, 0);
    EXPECT_TRUE(d.what == O::more_room && d.next.cand_cap_override == 4000000);
    big.cand_cap = (1ull << 27) - 1;
    d = decide_scan(counters(10, 1ull << 28, 0, 100, 0).c, big, big_hits, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::more_room && d.next.cand_cap_override == 1ull << 27);
    big.cand_cap = 1ull << 27; // the largest list: its overflow is the spans' business
    d = decide_scan(counters(10, 1ull << 28, 0, 100, 5).c, big, big_hits, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::span_fallback && same(d.next, fresh));
    // the cand_cap knob pins the list: no survivor retry, the spans that gave up go to the fallback
    d = decide_scan(counters(10, 2000, 0, 100, 3).c, cap, hit_cap, fresh, 0, 1000);
    EXPECT_TRUE(d.what == O::span_fallback && !d.more_surv && same(d.next, fresh));
    // band list too small: scale by ceil(drawn / cap) + 1, at least 2; it suppresses the dedupe retry
    d = decide_scan(counters(10, 800, 1, 1200, 0).c, cap, hit_cap, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::more_room && d.more_bands && !d.more_seen && !d.more_surv && d.next.band_scale == 4 && !d.next.seen_full);
    retry_state scaled;
    scaled.band_scale = 4;
    d = decide_scan(counters(10, 800, 2, 501, 0).c, cap, hit_cap, scaled, 1, 0);
    EXPECT_TRUE(d.what == O::more_room && d.next.band_scale == 4 * 3);
    big = cap;
    big.band_cap = 1ull << 28; // the largest band list: nothing left to retry with
    d = decide_scan(counters(10, 800, 1, (1ull << 28) + 1, 0).c, big, big_hits, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::brute_fallback && same(d.next, fresh));
    // overflow with room in the band list: the dedupe set (or the table) -- once with the full set, then brute force
    d = decide_scan(counters(10, 800, 1, 100, 0).c, cap, hit_cap, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::more_room && d.more_seen && !d.more_bands && d.next.seen_full && d.next.band_scale == 0);
    retry_state full;
    full.seen_full = true;
    d = decide_scan(counters(10, 800, 1, 100, 4).c, cap, hit_cap, full, 1, 0);
    EXPECT_TRUE(d.what == O::brute_fallback && same(d.next, full));
    // a nearly full dedupe set in an attempt cut short by its lists promotes seen_full
    big = cap;
    big_hits = 1 << 20;
    d = decide_scan(counters(8193, 2000, 0, 100, 0).c, big, big_hits, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::more_room && d.more_surv && !d.more_seen && d.next.seen_full);
    d = decide_scan(counters(8192, 2000, 0, 100, 0).c, big, big_hits, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::more_room && !d.next.seen_full);
    // the third attempt never repeats: it ends in one of the final outcomes
    d = decide_scan(counters(10, 2000, 0, 100, 3).c, cap, hit_cap, fresh, 2, 0);
    EXPECT_TRUE(d.what == O::span_fallback && !d.more_surv && same(d.next, fresh));
    d = decide_scan(counters(10, 800, 1, 1200, 0).c, cap, hit_cap, fresh, 2, 0);
    EXPECT_TRUE(d.what == O::brute_fallback && !d.more_bands);
    d = decide_scan(counters(10, 2000, 0, 100, 0).c, cap, hit_cap, fresh, 2, 0);
    EXPECT_TRUE(d.what == O::final_hits);
    // spans gave up in a run that reported without the dedupe set: once more with it; with it: the span-local fallback
    filter_result skipped = cap;
    skipped.seen_skipped = true;
    d = decide_scan(counters(10, 800, 0, 100, 2).c, skipped, hit_cap, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::with_seen && d.next.need_seen && !d.next.seen_full && d.next.cand_cap_override == 0);
    d = decide_scan(counters(10, 800, 0, 100, 2).c, cap, hit_cap, fresh, 0, 0);
    EXPECT_TRUE(d.what == O::span_fallback && same(d.next, fresh));
    // after the fallback's re-scan
    d = decide_scan(counters(50, 800, 0, 100, 2).c, cap, hit_cap, fresh, 0, 0, true);
    EXPECT_TRUE(d.what == O::final_hits && same(d.next, fresh));
    d = decide_scan(counters(50, 800, 1, 100, 2).c, cap, hit_cap, fresh, 0, 0, true);
    EXPECT_TRUE(d.what == O::with_full_seen && d.next.seen_full && !d.next.need_seen && !d.more_seen);
    d = decide_scan(counters(50, 800, 1, 100, 2).c, cap, hit_cap, full, 0, 0, true);
    EXPECT_TRUE(d.what == O::brute_fallback && same(d.next, full));
    d = decide_scan(counters(101, 800, 1, 100, 2).c, cap, hit_cap, fresh, 0, 0, true);
    EXPECT_TRUE(d.what == O::caller_overflow && same(d.next, fresh));
}

// the clean predicate against the status word of hits_fused_copy_device_kernel, as that kernel spelt it out
static void clean_cases()
{
    const unsigned long long cand_cap = 1000, hit_cap = 100;
    for (int bits = 0; bits < 16; ++bits) {
        const counters k(bits & 8 ? hit_cap + 1 : hit_cap, bits & 4 ? cand_cap + 1 : cand_cap, bits & 1, 77, (bits & 2) ? 3 : 0);
        const unsigned long long *c = k.c, n = c[0];
        const bool status = c[2] != 0 || c[6] != 0 || c[1] > cand_cap || n > hit_cap;
        EXPECT_TRUE(scan_needs_host(c, cand_cap, n, hit_cap) == status);
        EXPECT_TRUE(scan_clean(c, cand_cap) == !(c[2] != 0 || c[6] != 0 || c[1] > cand_cap));
        EXPECT_TRUE(scan_needs_host(c, cand_cap) == !scan_clean(c, cand_cap));
    }
    struct
    {
        mutable uint64_t cand_hint = 5, hit_hint = 500, band_hint = 0;
        mutable bool scanned = false;
    } set;
    raise_hints(set, counters(70, 60, 0, 50, 0).c);
    EXPECT_TRUE(set.cand_hint == 60 && set.hit_hint == 500 && set.band_hint == 50 && set.scanned);
}

// the sizes of a first scan (no hints) follow the inputs alone; the scratch buffer is laid out without gaps or overlaps
static void sizing_cases()
{
    struct pass
    {
        uint32_t stride, n_keys, key_len;
    };
    struct
    {
        uint32_t n = 1000, max_k = 3, max_m = 100, sigma = 4;
        bool scanned = false;
        uint64_t cand_hint = 0, band_hint = 0, hit_hint = 0;
        const void *d_peq_bot = nullptr, *d_surplus = nullptr;
        std::vector<pass> fidx = {{4, 4000, 16}};
    } set;
    struct
    {
        int cand_cap = 0, band_cap = 0, verify_wave_min_words = 8;
    } tune;
    const retry_state fresh;
    filter_sizes Z = size_filter(set, tune, 1ull << 30, 256, 1ull << 20, fresh);
    // est = max(4096, 8 * 1000 * 4, 2^30 / 2048) = 524288; survivors 2 est + 256 * 16 * 32; bands a quarter + 256 * 32 * 32
    EXPECT_TRUE(Z.surv_cap == 2 * 524288 + 131072 && Z.band_cap == Z.surv_cap / 4 + 262144 && Z.band_slots == 1u << 21);
    EXPECT_TRUE(Z.nwn == 4 && !Z.use_wave && !Z.overlap && Z.Bw == 32 && Z.max_span == 31);
    EXPECT_TRUE(Z.seen_slots == 1u << 21); // min(bands x 38 end positions, hit buffer, 4 M for a first scan), twice, rounded up
    EXPECT_TRUE(Z.surv_bytes == Z.surv_cap * 16 && Z.seen_bytes == Z.seen_slots * 8 && Z.band_bytes == Z.band_cap * 32 &&
                Z.ovf_bytes == kOvfCap * 16);
    retry_state again;
    again.cand_cap_override = 5000000, again.band_scale = 3, again.seen_full = true;
    tune.band_cap = 77; // (a repeated attempt sizes its band list itself)
    Z = size_filter(set, tune, 1ull << 30, 256, 1ull << 24, again);
    EXPECT_TRUE(Z.surv_cap == 5000000 && Z.band_cap == 3 * 1250000 + 262144 && Z.seen_slots == 1u << 25);
    tune.cand_cap = 4096;
    Z = size_filter(set, tune, 1ull << 30, 256, 1ull << 20, fresh);
    EXPECT_TRUE(Z.surv_cap == 4096 && Z.band_cap == 77 && Z.band_slots == 1u << 12);
    set.max_k = 64, set.max_m = 1024, set.d_peq_bot = &set, set.d_surplus = &set; // surplus seeds, wave-per-band kernel
    Z = size_filter(set, tune, 1ull << 30, 256, 1ull << 20, fresh);
    EXPECT_TRUE(Z.use_wave && Z.overlap && Z.nwn == 32 && Z.Bw == 260 && Z.max_span == 259 + 65);
}

// the span of a streaming pass: values worked out by hand from the rule (256 CUs; 512-thread workgroups, two per CU:
// 4096 waves; 1024-thread workgroups, two per CU: 8192 waves)
static void span_cases()
{
    auto is = [](span_plan s, uint32_t chunks, uint32_t dynamic) { return s.span_chunks == chunks && s.dynamic == dynamic; };
    // a small text, 64 Ki symbols: 64 / (4096 * 32) + 1 = 1; the 64 KiB rule offers min(64, 64 / 16384 + 1) = 1; minimum 8
    EXPECT_TRUE(is(plan_span(64, 4096, 1024), 8, 2));
    EXPECT_TRUE(is(plan_span(0, 4096, 1024), 8, 2) && is(plan_span(1, 1, 1024), 8, 2));
    // ... its 16 p-chunks: 16 / (8192 * 8) + 1 = 1; minimum 4
    EXPECT_TRUE(is(plan_span(16, 8192, 4096), 4, 2));
    // 4 Mi symbols: 4096 / 131072 + 1 = 1 -> max(1, min(64, 4096 / 16384 + 1 = 1)) = 1 -> 8
    EXPECT_TRUE(is(plan_span(4096, 4096, 1024), 8, 2));
    // 256 Mi symbols: 262144 / 131072 + 1 = 3 -> max(3, min(64, 262144 / 16384 + 1 = 17)) = 17 -> rounded up to 24
    EXPECT_TRUE(is(plan_span(262144, 4096, 1024), 24, 2));
    // 1 GiB: 2^20 / 2^17 + 1 = 9 -> max(9, min(64, 2^20 / 2^14 + 1 = 65)) = 64
    EXPECT_TRUE(is(plan_span(1u << 20, 4096, 1024), 64, 2));
    // ... in p-chunks on 8192 waves: 2^18 / 2^16 + 1 = 5 -> 8
    EXPECT_TRUE(is(plan_span(1u << 18, 8192, 4096), 8, 2));
    // 16 GiB: 2^24 / 2^17 + 1 = 129 (>= 64: the small-text rule is out) -> 136; below 192: per workgroup
    EXPECT_TRUE(is(plan_span(1u << 24, 4096, 1024), 136, 2));
    // ... on 8192 waves: 2^24 / 2^18 + 1 = 65 -> 72;  packed: 2^22 / 2^16 + 1 = 65 -> 68, >= 48: per wave
    EXPECT_TRUE(is(plan_span(1u << 24, 8192, 1024), 72, 2));
    EXPECT_TRUE(is(plan_span(1u << 22, 8192, 4096), 68, 1));
    // the dequeue threshold: 191 * 2^17 chunks give 192 (per wave), one chunk less 191 -> 192 as well
    EXPECT_TRUE(is(plan_span(191ull << 17, 4096, 1024), 192, 1) && is(plan_span((191ull << 17) - 1, 4096, 1024), 192, 1));
    EXPECT_TRUE(is(plan_span(183ull << 17, 4096, 1024), 184, 2)); // 183 + 1 = 184, a multiple of 8: per workgroup
    EXPECT_TRUE(is(plan_span(47ull << 16, 8192, 4096), 48, 1) && is(plan_span(43ull << 16, 8192, 4096), 44, 2));
    // the caps: 4096 chunks (and p-chunks) per span
    EXPECT_TRUE(is(plan_span(1ull << 40, 4096, 1024), 4096, 1) && is(plan_span(1ull << 40, 8192, 4096), 4096, 1));
    // few waves (a small device): 64 chunks on 64 waves: 64 / 2048 + 1 = 1 -> max(1, min(64, 64 / 256 + 1)) = 1 -> 8;
    // 2^16 chunks: 2^16 / 2^11 + 1 = 33 -> max(33, min(64, 2^16 / 2^8 + 1)) = 64
    EXPECT_TRUE(is(plan_span(64, 64, 1024), 8, 2) && is(plan_span(1u << 16, 64, 1024), 64, 2));
}

// the chunks and spans of a streaming pass: values worked out by hand (chunk 0 begins at the unit border at or below lo)
static void geometry_cases()
{
    auto is = [](stream_geometry g, uint64_t base0, uint64_t n_chunks, uint64_t n_whole, uint64_t n_spans) {
        return g.base0 == base0 && g.n_chunks == n_chunks && g.n_whole == n_whole && g.n_spans == n_spans;
    };
    // lo inside chunk 1 of the 1-byte text, hi inside chunk 9: chunks 1..9 = 9, the last one ragged; spans of 8: 2
    EXPECT_TRUE(is(stream_geometry_of(1500, 10000, 1024, 8), 1024, 9, 8, 2));
    // ... in p-chunks: lo and hi inside p-chunks 0 and 2: 3 p-chunks, 2 whole; spans of 4: 1
    EXPECT_TRUE(is(stream_geometry_of(1500, 10000, 4096, 4), 0, 3, 2, 1));
    // hi exactly on a chunk border: no ragged chunk; 8 chunks are one span of 8 and two spans of 4
    EXPECT_TRUE(is(stream_geometry_of(1024, 9 * 1024, 1024, 8), 1024, 8, 8, 1));
    EXPECT_TRUE(is(stream_geometry_of(1030, 9 * 1024, 1024, 4), 1024, 8, 8, 2));
    EXPECT_TRUE(is(stream_geometry_of(5000, 3 * 4096, 4096, 4), 4096, 2, 2, 1));
    // ... one symbol further: a ragged chunk, and with it a ninth chunk and a second span
    EXPECT_TRUE(is(stream_geometry_of(1024, 9 * 1024 + 1, 1024, 8), 1024, 9, 8, 2));
    EXPECT_TRUE(is(stream_geometry_of(5000, 3 * 4096 + 1, 4096, 4), 4096, 3, 2, 1));
    // less than one chunk: inside one chunk (no whole chunk), and across a border (one ragged chunk behind a whole one)
    EXPECT_TRUE(is(stream_geometry_of(100, 200, 1024, 8), 0, 1, 0, 1));
    EXPECT_TRUE(is(stream_geometry_of(1000, 1100, 1024, 8), 0, 2, 1, 1));
    EXPECT_TRUE(is(stream_geometry_of(4000, 4200, 4096, 4), 0, 2, 1, 1));
    EXPECT_TRUE(is(stream_geometry_of(4097, 4100, 4096, 4), 4096, 1, 0, 1));
    // lo on a border; a text beyond 2^32 symbols; the driver's count of chunks (spans of one chunk)
    EXPECT_TRUE(is(stream_geometry_of(0, 1ull << 34, 1024, 136), 0, 1ull << 24, 1ull << 24, ((1ull << 24) + 135) / 136));
    EXPECT_TRUE(is(stream_geometry_of((1ull << 33) + 7, (1ull << 34) + 5, 4096, 68), 1ull << 33, (1ull << 21) + 1, 1ull << 21,
                   ((1ull << 21) + 1 + 67) / 68));
    EXPECT_TRUE(is(stream_geometry_of(1500, 10000, 1024), 1024, 9, 8, 9) && is(stream_geometry_of(1500, 10000, 4096), 0, 3, 2, 3));
}

int main()
{
    span_cases();
    geometry_cases();
    tiler_cases();
    policy_cases();
    clean_cases();
    sizing_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
