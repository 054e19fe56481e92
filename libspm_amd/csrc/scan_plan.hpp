// scan_plan.hpp -- what one scan decides on the host, as pure functions (plain C++17, no HIP: the kernels, the scan driver,
// the sanitizer build and tests/cpp/scan_plan_cases.cpp all compile it): the legend of the counter block, what its
// values mean for the scan (clean / retry / fallback), the tile tables of the brute-force kernel, the span of a streaming
// pass, and the buffer sizes of the seed filter.  The driver (scan.hip, scan_filter.hip, scan_brute.hip) keeps the HIP
// calls and acts on the answers.
#pragma once

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

#include "hd.hpp"

namespace spm_hip
{

// ---- the counter block of one scan (spm_hits::d_count): kCntBlock 64-bit words, cleared before the scan ----
enum scan_counter : int
{
    kCntHits = 0,          // hits reported (may exceed the hit buffer: the count goes on, the records stop)
    kCntSurvSlots = 1,     // survivor slots drawn by the streaming passes (this pass: resolve_kernel adds up)
    kCntVoid = 2,          // hard overflow: band list / band table / dedupe set / overflow list full, or a poisoned table
    kCntBandSlots = 3,     // band-list slots drawn by resolve_kernel
    kCntSpanHead = 4,      // the span queue's head (cleared in front of every streaming pass)
    kCntPairs = 5,         // seed-checked (survivor, entry) pairs: spm_scan_stats::n_candidates
    kCntSpansGaveUp = 6,   // spans that gave up (entries of the overflow list)
    kCntBandsVerified = 7, // bands the verification looked at: spm_scan_stats::n_bands
    // resolve_kernel writes these two and nobody reads them.  Removing the writes changes resolve_kernel and belongs to
    // a change that measures.
    kCntUnreadSurvSum = 8, // survivors over all passes
    kCntUnreadSurvMax = 9, // largest survivor demand of a pass
    kCntBandsSelected = 10, // entries of the list band_select_kernel kept (sets with surplus seeds)
    kCntRunHeads = 11,      // entries of the list of run heads (band_runs_kernel)
    kCntFanOut = 12,        // records of the journaled-sequence fan-out launched behind the scan (jst_search.hpp)
    kCntStateOnly = 13,     // where a state-only brute-force pass counts the hits it does not report
    kCntTicket = 15,        // the device-side fused copy: workgroups that have read the block (the last one clears it)
};
constexpr int kCntBlock = 16;    // words allocated and cleared
constexpr int kCntReadBack = 13; // words the host reads after a filter scan: everything up to kCntFanOut
constexpr int kCntReadBackRescan = 8; // ... after the span-local fallback's re-scan: up to kCntBandsVerified
constexpr int kCntReadBackCount = 4;  // ... when only the hit count is missing
// spm_ctx::h_counters is the pinned landing block of those read-backs; a fan-out that runs on its own lands its count
// behind them.  (A device slot, a host index and a length: that kCntStateOnly, kLandFanOut and kCntReadBack are all
// 13 is a coincidence -- each is simply the first word the read-back leaves alone.)
constexpr int kLandFanOut = 13;

// Clean: nothing overflowed, no span gave up, the survivor list sufficed -- the hit list is final and the host has
// nothing to do.  The device-side fused copy adds a reason of its own: more hits `n` than the buffer's `hit_cap` (n by
// reference: by value the compiler tests it ahead of the counters, and that kernel's code is meant to stay as it was;
// so is `!scan_clean(..) || n > hit_cap`, which compiles to a different branch order).
SPM_HD inline bool scan_needs_host(const unsigned long long *c, unsigned long long cand_cap, const unsigned long long &n = 0,
                                   unsigned long long hit_cap = 0)
{
    return c[kCntVoid] != 0 || c[kCntSpansGaveUp] != 0 || c[kCntSurvSlots] > cand_cap || n > hit_cap;
}
SPM_HD inline bool scan_clean(const unsigned long long *c, unsigned long long cand_cap) { return !scan_needs_host(c, cand_cap); }

// a clean scan teaches the needle set what its lists have to hold (Set: spm_patterns, whose hints are mutable)
template <typename Set>
inline void raise_hints(const Set &ps, const unsigned long long *c)
{
    ps.cand_hint = std::max<uint64_t>(ps.cand_hint, c[kCntSurvSlots]);
    ps.hit_hint = std::max<uint64_t>(ps.hit_hint, c[kCntHits]);
    ps.band_hint = std::max<uint64_t>(ps.band_hint, c[kCntBandSlots]);
    ps.scanned = true;
}

// ---- the retry policy ----
struct retry_state // what scan_impl carries from one filter attempt to the next
{
    uint64_t cand_cap_override = 0; // after a survivor overflow: the count the first attempt needed
    uint64_t band_scale = 0;        // after a band list / table overflow: that much more room
    bool seen_full = false;         // after a dedupe-set overflow: size it for the caller's hit buffer
    bool need_seen = false;         // sets that report without the dedupe set: with it after all (spans gave up)
};
struct filter_result // what one filter run tells the driver: what it ran with, and where the fallback finds its lists
{
    unsigned long long *d_seen = nullptr; // the dedupe set in the scratch buffer (the brute-force re-scan reports through it)
    uint32_t seen_mask = 0;               // ... its slots - 1
    uint64_t *d_ovf = nullptr;            // overflow list in the scratch buffer: {begin, symbols} per span that gave up
    bool seen_skipped = false;            // this run reported (some of) its hits without asking the dedupe set
    uint64_t cand_cap = 0, band_cap = 0;  // the capacities of its survivor and band lists
};
enum class scan_outcome
{
    final_hits,      // the hit list is complete
    caller_overflow, // more hits than the caller's buffer takes: SPM_E_OVERFLOW from the views, not a reason to scan again
    more_room,       // the same attempt again, with the retry state of scan_decision::next (at most two repeats)
    with_seen,       // spans gave up in a scan that ran without the dedupe set: a new round with it (next.need_seen)
    with_full_seen,  // the dedupe set ran out during the fallback's re-scan (it was sized for what earlier scans reported):
                     // a new round with the set sized for the caller's hit buffer (next.seen_full)
    span_fallback,   // only the spans that gave up are scanned again, by the brute-force kernel
    brute_fallback,  // lists still too small: the whole range again, brute force
};
struct scan_decision
{
    scan_outcome what = scan_outcome::final_hits;
    retry_state next;
    bool more_surv = false, more_bands = false, more_seen = false; // why more_room (the trace line)
};
constexpr uint64_t kSurvMax = 1ull << 27; // 2 GiB of survivors: beyond that spans give up (brute-force re-scan)
constexpr uint64_t kBandMax = 1ull << 28;

// After attempt `attempt` (0, 1, 2: the third never repeats) of a round of filter runs; `rescanned`: after the span-local
// fallback's re-scan that followed it.  `cand_cap_knob`: scan_tuning::cand_cap, which pins the survivor list.
inline scan_decision decide_scan(const unsigned long long *c, const filter_result &ran, uint64_t hit_cap, const retry_state &rs,
                                 int attempt, int cand_cap_knob, bool rescanned = false)
{
    scan_decision d;
    d.next = rs;
    if (c[kCntHits] <= hit_cap && attempt < 2 && !rescanned) {
        // Start over with more room when the lists were too small for this text (the first attempt counted the
        // demand): survivor buffer full -- spans gave up for that reason, not for their own budget --, or band list /
        // band table / dedupe set full.
        d.more_surv = c[kCntSurvSlots] > ran.cand_cap && ran.cand_cap < kSurvMax && !cand_cap_knob;
        d.more_bands = c[kCntVoid] != 0 && c[kCntBandSlots] > ran.band_cap && ran.band_cap < kBandMax;
        d.more_seen = c[kCntVoid] != 0 && !rs.seen_full && !d.more_bands && c[kCntBandSlots] <= ran.band_cap;
        if (d.more_surv || d.more_bands || d.more_seen) {
            d.what = scan_outcome::more_room;
            if (d.more_surv)
                d.next.cand_cap_override = std::min<uint64_t>(
                    kSurvMax, std::max<uint64_t>(c[kCntSurvSlots] + c[kCntSurvSlots] / 8 + 4096, 4 * ran.cand_cap));
            if (d.more_bands)
                d.next.band_scale = std::max<uint64_t>(1, rs.band_scale) *
                                    std::max<uint64_t>(2, (c[kCntBandSlots] + ran.band_cap - 1) / ran.band_cap + 1);
            if (d.more_seen || c[kCntHits] > ((uint64_t)ran.seen_mask + 1) / 8)
                d.next.seen_full = true; // (an attempt cut short by its lists that nearly filled the set: the full one will not fit)
            return d;
        }
    }
    if (c[kCntHits] > hit_cap)
        d.what = scan_outcome::caller_overflow;
    else if (c[kCntVoid] != 0 && rescanned && !rs.seen_full) {
        d.what = scan_outcome::with_full_seen;
        d.next.seen_full = true;
    } else if (c[kCntVoid] != 0)
        d.what = scan_outcome::brute_fallback;
    else if (c[kCntSpansGaveUp] != 0 && !rescanned) {
        d.what = ran.seen_skipped ? scan_outcome::with_seen : scan_outcome::span_fallback;
        d.next.need_seen |= ran.seen_skipped;
    }
    return d;
}

// ---- tile tables of the brute-force kernel: {cold start, own_lo, own_hi} per tile ----
// The tiles of [lo, hi) inside a haystack that begins at hay_lo: each owns `tile` end positions and starts cold `warm`
// symbols early, or at the haystack's first symbol.
inline void append_tiles(std::vector<uint64_t> &tab, uint64_t lo, uint64_t hi, uint64_t hay_lo, uint64_t warm, uint64_t tile)
{
    for (; lo < hi; lo += tile) {
        tab.push_back(lo >= hay_lo + warm ? lo - warm : hay_lo);
        tab.push_back(lo);
        tab.push_back(std::min(lo + tile, hi));
    }
}

constexpr uint64_t kOvfCap = 1ull << 17; // spans the overflow list holds (2 MiB); beyond: whole-scan fallback

struct fallback_plan // the span-local fallback: what the brute-force kernel scans again
{
    std::vector<std::pair<uint64_t, uint64_t>> ranges; // end positions, sorted, disjoint, not touching
    uint64_t total = 0;                                // ... how many
    uint64_t warm = 0, tile = 0;
};
// ov: {begin, symbols} of the n_ovf spans that gave up; [begin, end): the owned end positions of the filter's scan
inline fallback_plan plan_fallback(const uint64_t *ov, uint64_t n_ovf, uint64_t begin, uint64_t end, uint32_t max_window,
                                   uint64_t n_cu, uint32_t n_groups)
{
    fallback_plan F;
    // a window that starts in span [b, b + len) belongs to occurrences whose last symbol lies in
    // [b - 16, b + len + max_window): those are scanned again (clipped to the owned range), merged where they touch
    std::vector<std::pair<uint64_t, uint64_t>> rg;
    rg.reserve(n_ovf);
    for (uint64_t i = 0; i < n_ovf; ++i) {
        const uint64_t b = ov[2 * i], len = ov[2 * i + 1];
        const uint64_t lo = std::max<uint64_t>(begin, b >= 16 ? b - 16 : 0);
        const uint64_t hi = std::min<uint64_t>(end, b + len + max_window);
        if (lo < hi)
            rg.emplace_back(lo, hi);
    }
    std::sort(rg.begin(), rg.end());
    for (const auto &r : rg) {
        if (!F.ranges.empty() && r.first <= F.ranges.back().second)
            F.ranges.back().second = std::max(F.ranges.back().second, r.second);
        else
            F.ranges.push_back(r);
    }
    for (const auto &r : F.ranges)
        F.total += r.second - r.first;
    F.warm = max_window > 0 ? max_window - 1 : 0;
    // tile length: enough tiles to fill the machine, long enough that the warm-up stays a small share
    const uint64_t want_tiles = n_cu * 32 / std::max(1u, n_groups) + 1;
    F.tile = std::max<uint64_t>(std::max<uint64_t>(1024, (F.warm * 8 + 255) & ~255ull), (F.total / want_tiles + 255) & ~255ull);
    F.tile = std::min<uint64_t>(F.tile, 1u << 20);
    return F;
}
// its tile table; segs (n_segments + 1 offsets) or nullptr: one haystack that begins at ctx_begin
inline void fallback_tiles(const fallback_plan &F, uint64_t ctx_begin, const uint64_t *segs, uint64_t n_segments,
                           std::vector<uint64_t> &tab)
{
    for (const auto &r : F.ranges) {
        if (!segs) {
            append_tiles(tab, r.first, r.second, ctx_begin, F.warm, F.tile);
            continue;
        }
        // every segment is a haystack of its own: the segments that meet [r.first, r.second), the one holding r.first, then on
        uint64_t sidx = (uint64_t)(std::upper_bound(segs, segs + n_segments + 1, r.first) - segs);
        sidx = sidx ? sidx - 1 : 0;
        for (; sidx < n_segments && segs[sidx] < r.second; ++sidx) // (cold starts inside the segment)
            append_tiles(tab, std::max(r.first, segs[sidx]), std::min(r.second, segs[sidx + 1]), segs[sidx], F.warm, F.tile);
    }
}

// ---- the chunks and spans of a streaming pass over the windows inside [lo, hi): the kernels and the driver ask here ----
struct stream_geometry
{
    uint64_t base0;    // first symbol of chunk 0: chunks are aligned to `unit` symbols relative to text[0]
    uint64_t n_chunks; // chunks that hold a symbol in front of hi
    uint64_t n_whole;  // ... that lie fully in front of hi
    uint64_t n_spans;  // spans of span_chunks chunks (the last one may be short)
};
// unit: symbols per chunk, 1024 (the 1-byte text) or 4096 (the p-chunks of the 2-bit shadow); lo < hi.  The driver counts
// the chunks before it has planned the span: spans of one chunk.
SPM_HD inline stream_geometry stream_geometry_of(uint64_t lo, uint64_t hi, uint32_t unit, uint32_t span_chunks = 1)
{
    stream_geometry G;
    G.base0 = lo & ~(uint64_t)(unit - 1);
    G.n_chunks = (hi - G.base0 + (unit - 1)) / unit;
    G.n_whole = (hi - G.base0) / unit;
    G.n_spans = (G.n_chunks + span_chunks - 1) / span_chunks;
    return G;
}

// ---- the span of a streaming pass: how many chunks a wave (or workgroup) takes off the span queue at a time ----
struct span_plan
{
    uint32_t span_chunks = 0; // chunks per span: whole groups of chunks (8 of 1 KiB, 4 p-chunks of the packed shadow)
    uint32_t dynamic = 0;     // span dequeue: 1 per wave, 2 per workgroup
};
// n_chunks: chunks of `unit` symbols the pass covers; n_waves: waves of its grid.  unit 1024: the 1-byte text; unit 4096:
// the p-chunks of the 2-bit shadow.
inline span_plan plan_span(uint64_t n_chunks, uint64_t n_waves, uint32_t unit)
{
    assert(unit == 1024 || unit == 4096);
    span_plan S;
    if (unit == 4096) {
        uint64_t pspan = n_chunks / (n_waves * 8) + 1;
        pspan = std::min<uint64_t>(std::max<uint64_t>(pspan, 4), 4096);
        pspan = (pspan + 3) & ~3ull;
        S.span_chunks = (uint32_t)pspan;
        S.dynamic = pspan >= 48 ? 1u : 2u;
        assert(S.dynamic == 1 || S.dynamic == 2);
        return S;
    }
    uint64_t span = n_chunks / (n_waves * 32) + 1;
    // small texts: at least 64 KiB per dequeue as long as every wave still gets ~4 spans (a 1 GiB text ran 14 % faster
    // with 64-chunk spans than with the 24 the rule above gives: fewer dequeue rounds, each a workgroup barrier)
    if (span < 64)
        span = std::max<uint64_t>(span, std::min<uint64_t>(64, n_chunks / (n_waves * 4) + 1));
    span = std::min<uint64_t>(std::max<uint64_t>(span, 8), 4096);
    span = (span + 7) & ~7ull; // whole groups of chunks
    S.span_chunks = (uint32_t)span;
    // span dequeue: per wave while the dequeue rate stays far below what one atomic word sustains (~88/us, i.e.
    // spans >= 192 KiB at 7 TB/s), per workgroup otherwise (measured: C3 2.52 vs 2.59 ms, C2 0.88 vs 0.20 ms)
    S.dynamic = span >= 192 ? 1u : 2u;
    assert(S.dynamic == 1 || S.dynamic == 2); // (the kernels know no other way to draw a span)
    return S;
}

// ---- sizes of one filter run: survivor list, band list, band table, band width, dedupe set, scratch layout ----
constexpr uint32_t kChunkMin = 32; // first chunk of list slots a wave draws (filter.hpp: chunk_grow)
constexpr size_t kSurvivorBytes = 16, kBandRecBytes = 16; // sizeof(survivor), sizeof(band_rec): scan_filter.hip asserts it

struct filter_sizes
{
    uint64_t surv_cap = 0, band_cap = 0, band_slots = 0, seen_slots = 0;
    uint32_t nwn = 1, Bw = 32, max_span = 31;
    bool use_wave = false; // verification by the wave-per-band kernel
    bool overlap = false;  // the set's needles carry surplus seeds: bands overlap
    size_t surv_bytes = 0, seen_bytes = 0, band_bytes = 0, ovf_bytes = 0; // the scratch buffer, in this order
};

// Set: the needle set (spm_patterns: its shape, its seed index `fidx`, what earlier scans taught it); Tune: scan_tuning
template <typename Set, typename Tune>
inline filter_sizes size_filter(const Set &ps, const Tune &tune, uint64_t symbols, uint64_t n_cu, uint64_t hit_cap, const retry_state &R)
{
    filter_sizes Z;
    const uint64_t kmax = ps.max_k;
    uint64_t est = std::max<uint64_t>(4096, 8ull * ps.n * (kmax + 1)); // a handful of true seed hits per needle
    // real texts are not uniform: room for the seed hits of repeat stretches -- one survivor per 2048 symbols (1 % of a
    // text in repeats needs one per 2800; a scan that outgrows its lists is repeated once with room for what it counted, and
    // the needle set remembers).  The first scan on a context pays for these buffers: sized for one survivor per 512
    // symbols (and as many bands) they were 2 GB of lists and a 4 GB band table to clear for a 16 GiB text -- 1.6 ms in
    // front of a 2.7 ms scan.
    est = std::max<uint64_t>(est, symbols / (ps.scanned ? 4096 : 2048));
    // chance hits of short keys: windows looked at x keys / 4^key_len, per pass (negligible for 16-symbol keys)
    double chance = 0;
    for (const auto &F : ps.fidx)
        chance += (double)symbols / std::max(1u, F.stride) * (double)F.n_keys / std::pow(4.0, (double)F.key_len);
    est = std::max<uint64_t>(est, (uint64_t)(2.0 * chance));
    est = std::max<uint64_t>(est, ps.cand_hint + ps.cand_hint / 4);
    // slots are drawn in growing chunks per wave (unused tails stay invalid): twice the estimate + the first chunks
    Z.surv_cap = std::min(2 * est + n_cu * 16 * kChunkMin, kSurvMax);
    if (R.cand_cap_override)
        Z.surv_cap = R.cand_cap_override;
    if (tune.cand_cap > 0)
        Z.surv_cap = (uint64_t)tune.cand_cap;
    // (+ the first chunk of every wave of resolve_kernel: n_cu x 8 workgroups of 4 waves)
    // bands: at most one per candidate pair, usually far fewer (uniform text: 1 000 for 20 000 survivors; 1 % repeats: 1.6 M
    // for 6 M; 5 %: as many as survivors) -- a quarter of the survivor slots unless earlier scans needed more
    const uint64_t band_want = std::max<uint64_t>(Z.surv_cap / 4, 2 * ps.band_hint);
    Z.band_cap = std::max<uint64_t>(band_want, 4096) * (R.band_scale ? R.band_scale : 1) + n_cu * 32 * kChunkMin;
    if (tune.band_cap > 0 && !R.band_scale) // (tests force the band-list-full path with it; a repeated attempt sizes itself)
        Z.band_cap = (uint64_t)tune.band_cap;
    Z.band_slots = 1u << 12;
    while (Z.band_slots < 2 * Z.band_cap)
        Z.band_slots <<= 1;
    // bands: Bw diagonals each.  Sets with surplus seeds: 4(k+1), overlapping by k + 1 (wider bands mean fewer occurrences
    // whose seeds straddle two of them at the price of more end positions per verification; 4(k+1) measured best for
    // |P| = 1024, k = 64; the lane-per-band kernel keeps its end-position slots per thread: k + 1 there).
    // Other sets: 32 diagonals, no overlap -- every band with a seed hit is verified.
    Z.nwn = std::max(1u, (ps.max_m + 31) / 32);
    const int wave_min = tune.verify_wave_min_words; // 0 = never use the wave-per-band kernel
    // (the wave-per-band kernel keeps the match masks of <= 5 symbols in registers: dna15 sets use the lane-per-band one)
    Z.use_wave = ps.d_peq_bot && wave_min > 0 && Z.nwn >= (uint32_t)wave_min && ps.sigma <= 5;
    Z.overlap = ps.d_surplus != nullptr;
    Z.Bw = 32; // (one mask bit per diagonal)
    if (Z.overlap) {
        Z.Bw = (ps.max_k + 1) * (Z.use_wave ? 4 : 1);
        if (Z.Bw + ps.max_k > 2047)
            Z.Bw = ps.max_k + 1;
    }
    Z.max_span = Z.Bw - 1 + (Z.overlap ? ps.max_k + 1 : 0);
    // dedupe set: one key per reported hit, so twice the hit capacity is room enough; a caller with a huge hit buffer
    // (repeat-rich texts) pays for what earlier scans of this needle set actually reported
    uint64_t want_seen = std::min<uint64_t>(Z.band_cap * (2 * kmax + 1 + Z.max_span), std::max<uint64_t>(hit_cap, 1));
    if (!R.seen_full)
        // (the first scan of a needle set knows nothing yet: room for 4 M hits -- a 64 MiB memset, 10 us -- rather than a
        // set that a repeat-rich text fills up, which costs a second run of the whole scan)
        want_seen = std::min<uint64_t>(want_seen, ps.scanned ? std::max<uint64_t>(1u << 18, 4 * ps.hit_hint) : (1ull << 22));
    Z.seen_slots = 1u << 16;
    while (Z.seen_slots < 2 * want_seen)
        Z.seen_slots <<= 1;
    Z.surv_bytes = Z.surv_cap * kSurvivorBytes;
    Z.seen_bytes = Z.seen_slots * sizeof(unsigned long long);
    Z.band_bytes = Z.band_cap * kBandRecBytes * 2; // (+ the selected bands of overlapping sets / the heads of runs)
    Z.ovf_bytes = kOvfCap * 2 * sizeof(uint64_t);
    return Z;
}

} // namespace spm_hip
