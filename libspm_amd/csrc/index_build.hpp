// index_build.hpp -- host side of the seed filter: which windows of which needles are indexed, and the tables the
// kernels of filter.hpp and its filter_*.hpp stages read.  PURE HOST C++17 (no HIP): spm_hip.hip includes it for the product, index_host.cpp compiles
// it with plain g++ for the sanitizer build and the host self-check.
//
// This header is the planner -- build_filter_index, a sequence of named stages -- and the name everybody includes for the
// whole index build: index_types.hpp (knobs, views, the index, seeds and keys; host_util.hpp under it), index_tables.hpp (the
// levels of one pass, build_one_index), index_dense.hpp (the dense pass, build_dense_index), index_selftest.hpp (host_selftest).
//
// What the reference does at this point is O(|P|) per needle: its matcher constructors build one SeqAn pattern each
// (/root/reference/libspm/libspm/matcher/myers_matcher.hpp:40-43, shiftor_matcher.hpp:38-40).  A set of 100 000 needles
// is 400 000+ seeds here, so the build is threaded (index_tuning::threads).
#pragma once

#include <cmath>

#include "index_dense.hpp"

namespace spm_hip
{

// a set that needs more passes than this is left to the brute-force engine
constexpr size_t kMaxPasses = 256;

struct seed_census
{
    bool in_range;  // false: a needle is empty or longer than 2047 symbols -- no seed filter, and the layout stops there
    bool sparse_ok; // every needle has a layout with seeds of >= kKeyMin symbols
    uint32_t qmin;  // shortest seed
    uint64_t n_seeds;
};

// the seeds of every needle, into X.seed_q / seed_n / seed_first / seed_off
inline seed_census layout_all_seeds(const needle_view &nv, seed_index &X)
{
    seed_census L{true, true, 0xFFFFFFFFu, 0};
    X.seed_q.assign(nv.n, 0);
    X.seed_n.assign(nv.n, 0);
    X.seed_first.assign(nv.n + 1, 0);
    std::vector<uint16_t> off;
    for (uint32_t p = 0; p < nv.n; ++p) {
        const uint32_t m = (uint32_t)nv.m[p];
        if (m == 0 || m > 2047) {
            L.in_range = false;
            return L;
        }
        uint32_t n = 0, q = 0;
        if (!layout_seeds(nv, p, kKeyMin, n, q, off)) {
            L.sparse_ok = false; // (one needle without a layout keeps the whole set off the sparse passes)
            break;
        }
        X.seed_q[p] = (uint16_t)q;
        X.seed_n[p] = (uint16_t)n;
        X.seed_first[p] = (uint32_t)X.seed_off.size();
        X.seed_off.insert(X.seed_off.end(), off.begin(), off.end());
        L.qmin = std::min(L.qmin, q);
        L.n_seeds += n;
    }
    X.seed_first[nv.n] = (uint32_t)X.seed_off.size();
    return L;
}

struct key_plan
{
    bool ok = false; // false: the sparse passes do not apply
    uint32_t H = kKeyMax, Smax = 1;
};

// Key length H and the largest stride: a window of H symbols at every S-th text position needs S <= q - H + 1.
// Seeds of >= 17 symbols use full 32-bit keys; shorter seeds give up one or two symbols of key for stride 2
// (half the windows), which costs far less than the extra spurious key matches it lets through.
// Seeds of <= 12 symbols: the whole seed is the key (stride 1) -- every symbol of key divides the chance matches by 4.
inline key_plan choose_key_and_stride(uint32_t qmin, uint64_t n_seeds, const index_tuning &T)
{
    key_plan K;
    if (qmin < kKeyMin)
        return K;
    if (qmin < kKeyMax + 1)
        K.H = qmin <= 12 ? qmin : qmin - 1;
    if ((double)n_seeds / std::pow(4.0, (double)K.H) > kMaxSurvivorShare)
        return K; // too many keys for their length: most text windows would match one by chance
    while (K.Smax * 2 <= 16 && K.Smax * 2 <= qmin - (K.H - 1))
        K.Smax *= 2;
    if (T.force_stride > 0 && (uint32_t)T.force_stride <= K.Smax)
        K.Smax = (uint32_t)T.force_stride;
    K.ok = true;
    return K;
}

struct stride_choice
{
    uint32_t stride;
    uint64_t passes; // of at most `cap` keys each
};

// The stride of the sparse passes: the largest one when a single pass suffices; otherwise the one minimising passes x cost
// per pass (a pass with stride S looks at 16/S windows per 16 symbols; measured cost grows ~0.3x per doubling).
inline stride_choice best_stride(uint64_t n_seeds, uint32_t Smax, uint64_t cap)
{
    uint32_t S = Smax;
    double best = 1e300;
    for (uint32_t s = Smax; s >= 1; s >>= 1) {
        const double passes = (double)((n_seeds * s + cap - 1) / cap);
        const double cost = passes * (1.0 + 0.3 * ((double)Smax / s - 1.0));
        if (cost < best) {
            best = cost;
            S = s;
        }
    }
    return {S, (n_seeds * S + cap - 1) / cap};
}

// The dense pass instead?  A sparse pass streams the text at the HBM rate as long as it looks at <= 4 windows per 16
// symbols of ONE table.  A set that needs several such passes, or stride 1 (16 windows per 16 symbols: LDS- and VALU-bound
// at ~3x the HBM time), is better off with the one dense pass (~2x the HBM time whatever the number of keys).
inline bool wants_dense_pass(const needle_view &nv, const index_tuning &T, const key_plan &K, uint64_t n_seeds)
{
    if (T.dense == 0 || !dense_eligible(nv))
        return false;
    if (T.dense >= 2 || !K.ok)
        return true;
    const stride_choice c = best_stride(n_seeds, K.Smax, (uint64_t)T.max_keys);
    return c.passes >= 2 || c.stride == 1;
}

struct pass_plan // which windows are indexed, and in which pass
{
    std::vector<std::vector<seed_key>> items;
    std::vector<uint32_t> anchor; // c | cm << 4; 0: no bit of the dimer is compared, every window is looked up
};

// Anchored keys.  A set this large gets ONE key per seed (stride 1: every text window is looked up, in every
// pass) -- but which of the seed's q - H + 1 windows that is, is ours to choose.  Pass i takes only keys whose
// first two symbols (a "dimer", 4 bits: sym0 | sym1 << 2) match ITS anchor pattern: (dimer ^ c) & cm == 0, at
// first one dimer per pass (cm = 15).  The streaming kernel then looks up only the text windows that begin
// with the anchor -- 1 in 16 -- instead of all: a window beginning with anything else cannot equal a key of the
// pass.  Lossless: an intact seed still has its key window in the text.  Each seed goes to a pass in which it
// has such a window among its first 32 (fewest choices first, least-loaded pass).  A seed that finds no place
// (seeds of 37 symbols, 22 windows, 7 passes: a few in a million) widens a pass's pattern by one don't-care bit
// -- that pass looks up 2 in 16 windows.
struct anchor_candidate
{
    uint32_t p, o, dimers, n_ok; // dimers: bit d set = one of the windows r <= min(31, q - H) begins with d
};
constexpr uint32_t kAnchorWindows = 32; // (an entry records where its window sits in the seed in 5 bits)

// the seeds over np passes of at most `cap` keys; false: some seed finds no pass even with a widened pattern
inline bool assign_anchored_np(const needle_view &nv, const seed_index &X, std::vector<anchor_candidate> &seeds, uint32_t np,
                               uint64_t cap, pass_plan &P)
{
    std::vector<uint32_t> pc(np), pcm(np, 15u), sets(np);
    for (uint32_t i = 0; i < np; ++i) {
        pc[i] = (5u * i + 3u) & 15u; // (a fixed shuffle of the dimers: neighbouring passes differ in both symbols)
        sets[i] = dimer_mask_of(pc[i], pcm[i]);
    }
    for (anchor_candidate &c : seeds) {
        c.n_ok = 0;
        for (uint32_t i = 0; i < np; ++i)
            c.n_ok += (c.dimers & sets[i]) ? 1u : 0u;
    }
    std::vector<uint32_t> order(seeds.size());
    for (uint32_t i = 0; i < order.size(); ++i)
        order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return seeds[x].n_ok < seeds[y].n_ok; });
    std::vector<std::vector<uint32_t>> members(np);
    for (uint32_t idx : order) {
        const anchor_candidate &c = seeds[idx];
        uint32_t best = np;
        for (uint32_t i = 0; i < np; ++i)
            if ((c.dimers & sets[i]) && members[i].size() < cap && (best == np || members[i].size() < members[best].size()))
                best = i;
        if (best == np) { // no place: widen the narrowest pattern that then takes this seed
            uint32_t bbit = 0;
            for (uint32_t i = 0; i < np; ++i) {
                if (members[i].size() >= cap)
                    continue;
                for (uint32_t bit = 1; bit < 16; bit <<= 1)
                    if ((pcm[i] & bit) && (c.dimers & dimer_mask_of(pc[i], pcm[i] & ~bit)) &&
                        (best == np || __builtin_popcount(pcm[i]) > __builtin_popcount(pcm[best]))) {
                        best = i;
                        bbit = bit;
                    }
            }
            if (best == np)
                return false;
            pcm[best] &= ~bbit;
            sets[best] = dimer_mask_of(pc[best], pcm[best]);
        }
        members[best].push_back(idx);
    }
    P.items.resize(np);
    for (uint32_t i = 0; i < np; ++i) {
        std::vector<seed_key> &items = P.items[i];
        for (uint32_t idx : members[i]) {
            const anchor_candidate &c = seeds[idx];
            const uint8_t *pat = nv.needle(c.p);
            uint32_t r = 0;
            while (!((sets[i] >> dimer_at(pat, c.o + r)) & 1u))
                ++r;
            items.push_back({c.p, c.o, r, X.seed_q[c.p]});
        }
        P.anchor.push_back(pc[i] | (pcm[i] << 4));
    }
    return true;
}

// with the fewest passes that hold the seeds, or one more; false: neither works out, P is untouched
inline bool assign_anchored_passes(const needle_view &nv, const seed_index &X, uint32_t H, uint64_t n_seeds, uint64_t cap,
                                   pass_plan &P)
{
    std::vector<anchor_candidate> seeds;
    seeds.reserve(n_seeds);
    for (uint32_t p = 0; p < nv.n; ++p) {
        const uint8_t *pat = nv.needle(p);
        const uint32_t q = X.seed_q[p];
        for (uint32_t j = 0; j < X.seed_n[p]; ++j) {
            const uint32_t o = X.seed_off[X.seed_first[p] + j];
            uint32_t dm = 0;
            for (uint32_t r = 0; r <= std::min<uint32_t>(kAnchorWindows - 1, q - H); ++r)
                dm |= 1u << dimer_at(pat, o + r);
            seeds.push_back({p, o, dm, 0});
        }
    }
    const uint32_t np_min = (uint32_t)((n_seeds + cap - 1) / cap);
    return assign_anchored_np(nv, X, seeds, np_min, cap, P) || assign_anchored_np(nv, X, seeds, np_min + 1, cap, P);
}

// unanchored passes: the needles in order, as many per pass as `cap` keys hold, every seed with its first S windows
inline void partition_passes(const needle_view &nv, const seed_index &X, uint32_t S, uint64_t cap, pass_plan &P)
{
    uint32_t p0 = 0;
    while (p0 < nv.n) {
        uint64_t keys = 0;
        uint32_t p1 = p0;
        while (p1 < nv.n) {
            const uint64_t add = (uint64_t)X.seed_n[p1] * S;
            if (keys + add > cap && p1 > p0)
                break;
            keys += add;
            ++p1;
        }
        P.items.emplace_back();
        P.anchor.push_back(0u);
        for (uint32_t p = p0; p < p1; ++p)
            for (uint32_t j = 0; j < X.seed_n[p]; ++j)
                for (uint32_t r = 0; r < S; ++r)
                    P.items.back().push_back({p, X.seed_off[X.seed_first[p] + j], r, X.seed_q[p]});
        p0 = p1;
    }
}

struct built_pass
{
    filter_index F;
    std::vector<u32x4> entries; // numbered from 0
    int rc = SPM_OK;
};

// the passes are independent: built side by side (they are of about one size: a slice of them per thread), each into its
// own slot
inline std::vector<built_pass> build_passes(const needle_view &nv, const index_tuning &T, const pass_plan &P, uint32_t H,
                                            uint32_t S)
{
    const size_t np = P.items.size();
    std::vector<built_pass> B(np);
    parallel_slices(np, (unsigned)std::min<size_t>(T.n_threads(), np), [&](size_t b, size_t e, unsigned) {
        for (size_t pi = b; pi < e; ++pi) {
            filter_index &F = B[pi].F;
            F.key_len = H;
            F.anchor_c = P.anchor[pi] & 15u;
            F.anchor_cm = P.anchor[pi] >> 4;
            F.dimer_set = dimer_mask_of(F.anchor_c, F.anchor_cm);
            B[pi].rc = build_one_index(nv, T, P.items[pi], S, F, B[pi].entries);
        }
    });
    return B;
}

// the passes' entries, appended in pass order (a pass numbered its entries from 0: its directory moves to where they land)
inline void append_passes(std::vector<built_pass> &B, seed_index &X)
{
    X.filter_max_range = 0;
    for (built_pass &b : B) {
        const uint32_t base = (uint32_t)X.h_entries.size();
        if (base)
            for (u32x4 &d : b.F.h_ht)
                if (d.z != 0)
                    d.y += base;
        X.h_entries.insert(X.h_entries.end(), b.entries.begin(), b.entries.end());
        X.filter_max_range = std::max(X.filter_max_range, b.F.max_range);
        X.fidx.push_back(std::move(b.F));
    }
}

// Seed filter applicability + partition of the needle set into passes whose keys fit one LDS table (or the one dense pass).
inline int build_filter_index(const needle_view &nv, const index_tuning &T, seed_index &X)
{
    X = seed_index();
    if ((nv.sigma != 4 && nv.sigma != 5 && nv.sigma != 15) || nv.algo == SPM_ALGO_MYERS_PREFIX || nv.n == 0 ||
        nv.n >= (1u << 21))
        return SPM_OK;
    const seed_census L = layout_all_seeds(nv, X);
    if (!L.in_range)
        return SPM_OK;
    const key_plan K = L.sparse_ok ? choose_key_and_stride(L.qmin, L.n_seeds, T) : key_plan();
    if (wants_dense_pass(nv, T, K, L.n_seeds)) {
        seed_index D;
        const int rc = build_dense_index(nv, T, D);
        if (rc != SPM_OK)
            return rc;
        if (!D.fidx.empty()) {
            X = std::move(D);
            return SPM_OK;
        }
    }
    if (!K.ok) {
        X = seed_index();
        return SPM_OK;
    }
    // keys per pass: the fingerprint table has 65536 slots; the hash-and-displace build succeeds up to ~88 % load
    // (57 344 keys).  If a pass's key set turns out too dense for the table, the whole set is re-partitioned with smaller
    // batches rather than dropping to the Bloom cascade.
    const uint64_t cap0 = (uint64_t)T.max_keys;
    const uint64_t caps[3] = {cap0, cap0 * 7 / 8, cap0 * 3 / 4};
    for (int attempt = 0; attempt < 3; ++attempt) {
        const uint64_t cap = caps[attempt];
        const uint32_t H = K.H, S = T.force_stride > 0 ? K.Smax : best_stride(L.n_seeds, K.Smax, cap).stride;
        X.filter_stride = S;
        X.filter_key_len = H;
        pass_plan P;
        const bool anchorable =
            S == 1 && (L.n_seeds + cap - 1) / cap > 1 && nv.sigma == 4 && H == 16 && L.qmin > H && T.anchor != 0;
        X.filter_anchored = anchorable && assign_anchored_passes(nv, X, H, L.n_seeds, cap, P);
        if (!X.filter_anchored)
            partition_passes(nv, X, S, cap, P);
        if (P.items.size() > kMaxPasses) {
            X = seed_index();
            return SPM_OK; // too many passes to be worth it: brute force
        }
        std::vector<built_pass> B = build_passes(nv, T, P, H, S);
        bool all_ok = true, table_overfull = false; // table_overfull: a pass's key set was too dense for the fingerprint table
        for (const built_pass &b : B) {
            if (b.rc != SPM_OK)
                return b.rc;
            all_ok = all_ok && b.F.ok;
            table_overfull = table_overfull || (T.hash == 2 && b.F.hash_variant != 2 && b.F.hash_variant != 4);
        }
        if (!all_ok) {
            X = seed_index();
            return SPM_OK;
        }
        if (table_overfull && attempt < 2)
            continue; // once more, with fewer keys per pass
        append_passes(B, X);
        return SPM_OK;
    }
    return SPM_OK;
}

} // namespace spm_hip

#include "index_selftest.hpp"
