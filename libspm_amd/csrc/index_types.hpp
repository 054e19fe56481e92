// index_types.hpp -- what the stages of the seed index build (index_build.hpp) hand to each other and to the library: the
// knobs, the needle set as a view, one pass (filter_index), the whole index (seed_index), and how a needle is cut into seeds
// and a window of a seed becomes a key with its entry fields.  PURE HOST C++17 (no HIP).
#pragma once

#include <algorithm>
#include <cstdint>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/spm_hip.h"
#include "filter_shared.hpp"
#include "host_util.hpp"

namespace spm_hip
{

// every knob of the index build, read from the environment in ONE place (spm_hip_patterns_create / the self-check).  Apart
// from the thread count, each one is set by a test to reach a path that some needle set also takes by default.
struct index_tuning
{
    int force_stride = 0;
    int max_keys = 57344; // keys per LDS fingerprint table
    int hash = 2;           // 2: perfect-hash fingerprint table (Bloom cascade where it cannot be built), 1: Bloom cascade
    int anchor = 1;
    int dedupe = 1;
    int dense = 1;          // 0: never, 1: when the sparse plan needs several passes or stride 1, 2: whenever the set admits it
    int dense_min_density = 0; // force at least this many sixteenths of the dimers as anchors
    int threads = 0;        // 0: hardware concurrency, at most 16
    static index_tuning from_env()
    {
        index_tuning T;
        T.force_stride = env_int("SPM_HIP_FILTER_STRIDE", 0);
        T.max_keys = std::max(1024, env_int("SPM_HIP_FILTER_MAX_KEYS", 57344));
        T.hash = std::max(1, std::min(2, env_int("SPM_HIP_FILTER_HASH", 2)));
        T.anchor = env_int("SPM_HIP_FILTER_ANCHOR", 1);
        T.dedupe = env_int("SPM_HIP_FILTER_DEDUPE", 1);
        T.dense = env_int("SPM_HIP_FILTER_DENSE", 1);
        T.dense_min_density = env_int("SPM_HIP_FILTER_DENSE_MIN_DENSITY", 0);
        T.threads = env_int("SPM_HIP_BUILD_THREADS", 0);
        return T;
    }
    unsigned n_threads() const
    {
        if (threads > 0)
            return (unsigned)std::min(threads, 64);
        const unsigned hc = std::thread::hardware_concurrency();
        return std::max(1u, std::min(16u, hc ? hc : 1u));
    }
};

// the needle set as the index build sees it (views; owned by the caller)
struct needle_view
{
    int algo = 0;
    uint32_t n = 0, sigma = 4;
    const uint8_t *ranks = nullptr;
    const uint32_t *offsets = nullptr; // n + 1
    const int32_t *m = nullptr, *k = nullptr;
    uint32_t max_k = 0;
    bool is_myers() const { return algo == SPM_ALGO_MYERS || algo == SPM_ALGO_MYERS_PREFIX; }
    const uint8_t *needle(size_t p) const { return ranks + offsets[p]; }
    uint32_t errors(size_t p) const { return is_myers() ? (uint32_t)k[p] : 0; } // (exact matchers: no errors)
};

// one pass over the text: the level-1 image every workgroup stages into LDS, the exact key directory, and (dense passes)
// the bucketed fingerprint table in between
struct filter_index
{
    // anchored passes: every key begins with a dimer d (sym0 | sym1 << 2) with (d ^ anchor_c) & anchor_cm == 0; cm = 0: unanchored
    uint32_t anchor_c = 0, anchor_cm = 0;
    bool ok = false;
    uint32_t dense = 0;      // 1: presence bits in LDS + fingerprint buckets in L2, anchors = union of n_pat patterns
    uint32_t n_pat = 0, pat_c[kDensePatterns] = {0, 0, 0}, pat_cm[kDensePatterns] = {0, 0, 0};
    uint32_t dimer_set = 0xFFFF; // bit d set: windows beginning with dimer d are looked up
    uint32_t bucket_shift = 0;   // bucket = (key * C) >> bucket_shift
    uint32_t stride = 0;
    uint32_t key_len = 16;
    uint32_t bitmap_words = 0;
    uint32_t n_probes = 0;
    uint32_t hash_variant = 0;
    uint32_t lds_words = 0;
    uint32_t chd_slot_mask = 0, chd_bucket_shift = 0, chd_disp_off = 0;
    uint32_t ht_mask = 0;
    uint64_t n_keys = 0;
    uint64_t n_entries = 0; // entries of the exact table after identical (key, needle) pairs were merged
    uint32_t max_range = 0; // largest diagonal range of a merged entry
    // host images (dropped after the upload unless the caller keeps them: the self-check does)
    std::vector<uint32_t> h_image;
    std::vector<u32x4> h_ht; // the directory: {key, first entry, entries, -}, open addressing, an empty slot has .z == 0
    std::vector<uint16_t> h_buckets; // dense: kDenseSlots 16-bit slots per bucket
    // device copies (spm_hip.hip)
    uint32_t *d_bitmap = nullptr;
    u32x4 *d_ht = nullptr;
    u32x4 *d_buckets = nullptr;
};

struct seed_index
{
    std::vector<filter_index> fidx; // one per pass; empty = the seed filter does not apply
    uint32_t filter_stride = 0;
    uint32_t filter_key_len = 16;
    bool filter_anchored = false; // stride 1, one key per seed, chosen to begin with an anchor dimer of its pass
    bool filter_dense = false;    // one dense pass (fidx.size() == 1)
    uint32_t filter_max_range = 0; // largest diagonal range over all passes
    // seed layout: needle p has seed_n[p] seeds at seed_off[seed_first[p] + j]; sparse passes: all seed_q[p] symbols long;
    // dense pass: seed_len[seed_first[p] + j] symbols, and they may overlap seed_c[p] deep (seed_n[p] >= seed_c[p] k + 1)
    std::vector<uint16_t> seed_q, seed_n, seed_off, seed_len;
    std::vector<uint8_t> seed_c;
    std::vector<uint32_t> seed_first;
    std::vector<u32x4> h_entries; // exact entries of all passes, grouped by key: {val = needle << 11 | offset, seed
                                  // signature, range code, key}
};

struct seed_key // one indexed window: needle p, seed at offset o of the needle, window starting r symbols into the seed
{
    uint32_t p, o, r;
    uint32_t q; // length of the seed
};

// A symbol the 2-bit keys can hold: A, C, G, T.  dna5 (seqan3 ranks A0 C1 G2 N3 T4): everything but N; dna15 (A0 B1 C2 D3
// G4 H5 K6 M7 N8 R9 S10 T11 V12 W13 Y14): A, C, G, T only.
inline bool key_symbol(uint32_t sigma, uint8_t c)
{
    return sigma == 4 ? c < 4 : sigma == 5 ? (c < 5 && c != 3) : (c == 0 || c == 2 || c == 4 || c == 11);
}
inline uint32_t key_code(uint32_t sigma, uint8_t c) // 2-bit code of a key symbol
{
    return sigma == 4 ? (c & 3u) : sigma == 5 ? (c == 4 ? 3u : c) : (c == 11 ? 3u : (uint32_t)c >> 1);
}

// the key of the H-symbol window pat[at, at + H): 2 bits per symbol, the first symbol lowest
inline uint32_t window_key(uint32_t sigma, const uint8_t *pat, uint32_t at, uint32_t H)
{
    uint32_t key = 0;
    for (uint32_t i = 0; i < H; ++i)
        key |= key_code(sigma, pat[at + i]) << (2 * i);
    return key;
}

// dimer d = sym0 | sym1 << 2 of the dna4 window that begins at pat[at]: the lowest four bits of its key
inline uint32_t dimer_at(const uint8_t *pat, uint32_t at) { return (pat[at] & 3u) | ((uint32_t)(pat[at + 1] & 3u) << 2); }

// the dimers d with (d ^ c) & cm == 0, one bit each
inline uint32_t dimer_mask_of(uint32_t c, uint32_t cm)
{
    uint32_t set = 0;
    for (uint32_t d = 0; d < 16; ++d)
        set |= (((d ^ c) & cm) == 0 ? 1u : 0u) << d;
    return set;
}

// Seeds of one needle.  The pigeonhole argument needs n DISJOINT pieces of the needle (n = k + 1, or k + 2 for needles
// with many errors: two intact pieces on nearby diagonals) -- they need not tile it.  A needle of key symbols only is cut
// into n pieces of q = floor(m / n) at offsets j * q.  A needle with an N (or, in dna15, any other ambiguity code) takes
// its pieces from its stretches of key symbols -- the n first pieces of the largest length q that yields n of them --,
// because a piece with an N can only occur where the text has an N too, and the filter never looks there: an intact
// piece WITHOUT one is found like any other seed.  false: the needle has no such layout with q >= q_floor.
inline bool layout_seeds(const needle_view &nv, uint32_t p, uint32_t q_floor, uint32_t &n_out, uint32_t &q_out,
                         std::vector<uint16_t> &off)
{
    const uint32_t m = (uint32_t)nv.m[p], k = nv.errors(p);
    const uint8_t *pat = nv.needle(p);
    bool clean = true;
    for (uint32_t i = 0; i < m; ++i)
        clean = clean && key_symbol(nv.sigma, pat[i]);
    const seed_plan sp = plan_seeds(m, k);
    off.clear();
    if (clean) {
        n_out = sp.n;
        q_out = sp.q;
        for (uint32_t j = 0; j < sp.n; ++j)
            off.push_back((uint16_t)(j * sp.q));
        return sp.q >= q_floor;
    }
    std::vector<std::pair<uint32_t, uint32_t>> runs; // (begin, length) of the stretches of key symbols
    for (uint32_t i = 0; i < m;) {
        if (!key_symbol(nv.sigma, pat[i])) {
            ++i;
            continue;
        }
        uint32_t j = i;
        while (j < m && key_symbol(nv.sigma, pat[j]))
            ++j;
        runs.emplace_back(i, j - i);
        i = j;
    }
    for (uint32_t n : {sp.n, k + 1}) { // (a needle that cannot afford the surplus seed keeps k + 1)
        for (uint32_t q = m / n; q >= q_floor && q > 0; --q) {
            uint64_t have = 0;
            for (const auto &r : runs)
                have += r.second / q;
            if (have < n)
                continue;
            for (const auto &r : runs)
                for (uint32_t j = 0; j + q <= r.second && off.size() < n; j += q)
                    off.push_back((uint16_t)(r.first + j));
            n_out = n;
            q_out = q;
            return true;
        }
        if (sp.n == k + 1)
            break;
    }
    return false;
}

struct index_kv // one indexed window on its way into the tables: the entry {val, sig, meta = range code, key}
{
    uint32_t key, val, sig, meta;
};

// key of the window seed[r, r + H) and the entry fields that go with it (filter_resolve.hpp: seed_sig_ok, kRngSingle)
inline index_kv make_kv(const needle_view &nv, const seed_key &it, uint32_t H)
{
    const uint32_t p = it.p, o = it.o, r = it.r, q = it.q;
    const uint8_t *pat = nv.needle(p);
    const uint32_t key = window_key(nv.sigma, pat, o + r, H);
    // signature: the REST of the seed -- its r symbols before the key window, then those after it --, the first 16 of
    // them, 2 bits each.  With the key that is the whole seed when q <= key_len + 16, so the resolve kernel checks "the
    // seed occurs here unchanged" in registers
    uint32_t sig = 0, ns = 0;
    for (uint32_t i = r > 16 ? r - 16 : 0; i < r && ns < 16; ++i, ++ns) // (the 16 symbols next to the window)
        sig |= key_code(nv.sigma, pat[o + i]) << (2 * ns);
    for (uint32_t i = r + H; i < q && ns < 16; ++i, ++ns)
        sig |= key_code(nv.sigma, pat[o + i]) << (2 * ns);
    // range code of a single entry: where the window sits in its seed (r), how many rest symbols the signature holds
    // (ns), and whether that is the whole rest
    const uint32_t meta = kRngSingle | (r & 0x1F) | (ns << 5) | (ns == q - H ? kRngWhole : 0u);
    return {key, (p << 11) | (o + r), sig, meta};
}

} // namespace spm_hip
