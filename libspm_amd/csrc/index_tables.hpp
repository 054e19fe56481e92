// index_tables.hpp -- the levels of ONE pass of the seed filter, each built from the pass's keys by a function of its own:
// runs of identical entries merged, then level 1 (perfect-hash fingerprint table, Bloom cascade, or presence bits with
// fingerprint buckets), then the exact directory.  build_one_index calls them in order.  PURE HOST C++17 (no HIP).
#pragma once

#include <cstring>

#include "index_types.hpp"

namespace spm_hip
{

// identical (key, needle) entries beyond this many are merged into one with a diagonal range.  (Measured on the 1 % repeat
// text, 16 / 128 needles across a stretch: > 4: 6.4 / 12.2 ms, > 8: 5.0 / 9.2, > 12: 5.0 / 8.4, > 24: 5.1 / 8.7, never: 5.1 /
// 9.4 -- merged entries skip the per-offset checks and cost bands, single ones cost checks.)
constexpr size_t kMergeRun = 12;

// A periodic seed puts the same key at several offsets of one needle (a homopolymer run: at every shift of every
// seed).  More than kMergeRun such entries -- the needle IS a repeat there -- are merged into one with a diagonal
// range: a text window then yields ONE pair per needle, counted into the bands of all the offsets, without per-offset
// checks (they would pass wherever the text carries the same repeat).  Shorter runs -- a needle that merely ends in a
// repeat -- stay apart, each with its own seed signature.  `keys` comes back sorted by (key, val), a merged entry with
// its range code in .meta; returns the largest span of a merged run.
inline uint32_t merge_entry_runs(std::vector<index_kv> &keys)
{
    uint32_t max_span = 0;
    std::sort(keys.begin(), keys.end(),
              [](const index_kv &a, const index_kv &b) { return a.key != b.key ? a.key < b.key : a.val < b.val; });
    size_t w = 0;
    for (size_t i = 0; i < keys.size();) {
        size_t j = i + 1;
        while (j < keys.size() && keys[j].key == keys[i].key && (keys[j].val >> 11) == (keys[i].val >> 11))
            ++j;
        if (j - i > kMergeRun) {
            const uint32_t span = (keys[j - 1].val & 0x7FF) - (keys[i].val & 0x7FF);
            keys[w] = keys[i];
            keys[w++].meta = kRngRun | span;
            max_span = std::max(max_span, span);
        } else {
            for (size_t q = i; q < j; ++q)
                keys[w++] = keys[q];
        }
        i = j;
    }
    keys.resize(w);
    return max_span;
}

// Exact level: a directory key -> (first entry, count) with open addressing, and the entries of a key side by side in
// one array (all passes share it).  A survivor costs one short directory probe; its entries -- a key that twenty needles
// share has twenty -- are then dealt to the lanes of the wave one pair each (resolve_kernel), instead of one lane walking a
// probe sequence while 63 wait.  `keys` comes back sorted by key.
inline void build_directory(std::vector<index_kv> &keys, filter_index &F, std::vector<u32x4> &entries)
{
    {
        // stable LSD radix sort by key (3 passes of 11 bits) of (key, index) pairs -- the passes read and write 8-byte pairs
        // in sequence; sorting an index array THROUGH the 16-byte records was six passes of cache misses --, then one gather
        const size_t n = keys.size();
        std::vector<uint64_t> pa(n), pb(n);
        for (size_t i = 0; i < n; ++i)
            pa[i] = ((uint64_t)keys[i].key << 32) | (uint64_t)i;
        for (uint32_t shift = 0; shift < 32; shift += 11) {
            uint32_t count[2049] = {0};
            for (size_t i = 0; i < n; ++i)
                ++count[((pa[i] >> (32 + shift)) & 2047u) + 1];
            for (uint32_t b = 0; b < 2048; ++b)
                count[b + 1] += count[b];
            for (size_t i = 0; i < n; ++i)
                pb[count[(pa[i] >> (32 + shift)) & 2047u]++] = pa[i];
            pa.swap(pb);
        }
        std::vector<uint32_t> order(n);
        for (size_t i = 0; i < n; ++i)
            order[i] = (uint32_t)pa[i];
        std::vector<index_kv> k2(n);
        for (size_t i = 0; i < n; ++i)
            k2[i] = keys[order[i]];
        keys.swap(k2);
    }
    size_t n_distinct = 0;
    for (size_t i = 0; i < keys.size(); ++i)
        n_distinct += (i == 0 || keys[i].key != keys[i - 1].key) ? 1 : 0;
    const uint32_t ht_size = next_pow2((uint32_t)std::max<uint64_t>(1024, n_distinct * 2));
    F.ht_mask = ht_size - 1;
    F.h_ht.assign(ht_size, u32x4{0, 0, 0, 0});
    entries.reserve(entries.size() + keys.size());
    for (size_t i = 0; i < keys.size();) {
        size_t j = i;
        while (j < keys.size() && keys[j].key == keys[i].key)
            ++j;
        // (the directory of 400 000 keys is 16 MB of 16-byte slots hit at random: ask for the slots of the keys a few steps
        // ahead while this one is placed -- the inserts were 20 ms of a 100 ms build as a chain of cache misses)
        if (j + 12 < keys.size())
            __builtin_prefetch(&F.h_ht[ht_hash(keys[j + 12].key) & F.ht_mask], 1, 0);
        uint32_t slot = ht_hash(keys[i].key) & F.ht_mask;
        while (F.h_ht[slot].z != 0)
            slot = (slot + 1) & F.ht_mask;
        F.h_ht[slot] = u32x4{keys[i].key, (uint32_t)entries.size(), (uint32_t)(j - i), 0};
        for (size_t q = i; q < j; ++q)
            entries.push_back(u32x4{keys[q].val, keys[q].sig, keys[q].meta, keys[q].key});
        i = j;
    }
}

// level 1 of a dense pass -- and of sparse passes that look at 8 or 16 windows per 16 symbols, where two LDS reads and two
// multiplies per window (the fingerprint table) cost more than the pass can hide: one presence bit per key in LDS, then a
// bucketed fingerprint table in L2 for the windows whose bit is set (filter_shared.hpp)
inline void build_bits_level1(const std::vector<index_kv> &keys, filter_index &F)
{
    F.h_image.assign((1u << kDenseBloomBits) / 32, 0);
    for (const index_kv &e : keys) {
        const uint32_t b = dense_bloom_index(e.key);
        F.h_image[b >> 5] |= 1u << (b & 31);
    }
    F.bitmap_words = F.lds_words = (uint32_t)F.h_image.size();
    uint32_t lg = 12; // about two keys per bucket of kDenseSlots
    while ((1ull << lg) * 2 < keys.size() && lg < 24)
        ++lg;
    F.bucket_shift = 32 - lg;
    F.h_buckets.assign((size_t)kDenseSlots << lg, 0);
    for (const index_kv &e : keys) {
        uint16_t *bk = F.h_buckets.data() + (size_t)dense_bucket(e.key, F.bucket_shift) * kDenseSlots;
        const uint16_t fp = (uint16_t)dense_fp(e.key);
        uint32_t s = 0;
        while (s < kDenseSlots && bk[s] != 0 && bk[s] != fp)
            ++s;
        if (s < kDenseSlots)
            bk[s] = fp;
        else
            bk[kDenseSlots - 1] = (uint16_t)kDenseAcceptAll; // overflow: this bucket lets every window through
    }
}

constexpr uint32_t kChdMaxBucket = 64; // keys of one bucket of the fingerprint table, at most

// the smallest displacement that sends the nb keys of one bucket to free slots, all different; the slots are taken and get
// the keys' fingerprints.  false: there is none
inline bool chd_place_bucket(const uint32_t *bucket_keys, uint32_t nb, uint32_t slot_mask, uint8_t *used, uint16_t *fp,
                             uint16_t &disp)
{
    chd_hashes hh[kChdMaxBucket];
    uint32_t slots[kChdMaxBucket];
    for (uint32_t i = 0; i < nb; ++i)
        hh[i] = chd_hash(bucket_keys[i]);
    for (uint32_t d = 0; d < 65536; ++d) {
        bool good = true;
        for (uint32_t i = 0; i < nb && good; ++i) {
            const uint32_t sl = chd_slot(hh[i], d, slot_mask);
            if (used[sl])
                good = false;
            for (uint32_t j = 0; j < i && good; ++j)
                if (slots[j] == sl)
                    good = false;
            slots[i] = sl;
        }
        if (!good)
            continue;
        for (uint32_t i = 0; i < nb; ++i) {
            used[slots[i]] = 1;
            fp[slots[i]] = (uint16_t)hh[i].f;
        }
        disp = (uint16_t)d;
        return true;
    }
    return false;
}

// Level 1 as a perfect-hash fingerprint table (hash-and-displace, see filter_shared.hpp): the image is the slots'
// fingerprints, then the buckets' displacements.  Buckets are placed fullest first.  false, and F untouched: the key set
// is too dense for the table (more than 96 % of 65536 slots, a bucket of more than kChdMaxBucket keys, or a bucket that no
// displacement places).
inline bool build_fingerprint_table(const std::vector<index_kv> &keys, filter_index &F)
{
    std::vector<uint32_t> uniq;
    uniq.reserve(keys.size());
    for (const index_kv &e : keys)
        uniq.push_back(e.key);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    uint32_t n_slots = 1024;
    while (n_slots < 2 * uniq.size() && n_slots < 65536)
        n_slots <<= 1;
    if (uniq.size() > (size_t)(0.96 * n_slots))
        return false;
    const uint32_t n_buckets = std::max(64u, n_slots / 8);
    uint32_t lg = 0;
    while ((1u << lg) < n_buckets)
        ++lg;
    const uint32_t shift = 32 - lg;
    // bucket the keys (counting sort: no per-bucket vectors)
    std::vector<uint32_t> b_begin(n_buckets + 1, 0), b_keys(uniq.size());
    for (uint32_t k : uniq)
        ++b_begin[(chd_hash(k).x >> shift) + 1];
    for (uint32_t b = 0; b < n_buckets; ++b)
        b_begin[b + 1] += b_begin[b];
    {
        std::vector<uint32_t> fill(b_begin.begin(), b_begin.end() - 1);
        for (uint32_t k : uniq)
            b_keys[fill[chd_hash(k).x >> shift]++] = k;
    }
    std::vector<uint32_t> order(n_buckets);
    for (uint32_t b = 0; b < n_buckets; ++b)
        order[b] = b;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return b_begin[a + 1] - b_begin[a] > b_begin[b + 1] - b_begin[b]; });
    std::vector<uint16_t> fp(n_slots, 0xFFFF), disp(n_buckets, 0);
    std::vector<uint8_t> used(n_slots, 0);
    for (uint32_t b : order) {
        const uint32_t nb = b_begin[b + 1] - b_begin[b];
        if (nb == 0)
            break;
        if (nb > kChdMaxBucket || !chd_place_bucket(b_keys.data() + b_begin[b], nb, n_slots - 1, used.data(), fp.data(), disp[b]))
            return false;
    }
    F.chd_slot_mask = n_slots - 1;
    F.chd_bucket_shift = shift;
    F.chd_disp_off = n_slots * 2;
    F.h_image.resize((n_slots * 2 + n_buckets * 2) / 4);
    memcpy(F.h_image.data(), fp.data(), n_slots * 2);
    memcpy((uint8_t *)F.h_image.data() + n_slots * 2, disp.data(), n_buckets * 2);
    F.bitmap_words = (uint32_t)F.h_image.size();
    return true;
}

// Level 1 as a Bloom cascade: F.n_probes bits per key in a bitmap of 32 bits per key (1024 .. 32768 words)
inline void build_bloom_image(const std::vector<index_kv> &keys, filter_index &F)
{
    const uint64_t want_bits = F.n_keys * 32;
    uint32_t words = 1024;
    while ((uint64_t)words * 32 < want_bits && words < 32768)
        words <<= 1;
    F.bitmap_words = words;
    F.h_image.assign(words, 0);
    const uint32_t idx_mask = words * 32 - 1;
    for (const index_kv &e : keys)
        for (uint32_t pr = 0; pr < F.n_probes; ++pr) {
            const uint32_t hh = bloom_hash(e.key, pr) & idx_mask;
            F.h_image[hh >> 5] |= 1u << (hh & 31);
        }
}

// One sparse pass: the windows `items` at stride S, with F.key_len and F.anchor_* set by the caller.  F.hash_variant says
// which level 1 came out: 4 (presence bits), 2 (fingerprint table) or 1 (Bloom cascade -- asked for, or the key set was too
// dense for the table).  F.ok stays false where the kernels have no such level 1 (dna5 / dna15 without a table).
inline int build_one_index(const needle_view &nv, const index_tuning &T, const std::vector<seed_key> &items, uint32_t S,
                           filter_index &F, std::vector<u32x4> &entries)
{
    F.ok = false;
    std::vector<index_kv> keys;
    keys.reserve(items.size());
    for (const seed_key &it : items)
        keys.push_back(make_kv(nv, it, F.key_len)); // window seed[r, r+H) -- inside the seed because r <= q - H
    F.n_keys = keys.size();
    if (F.n_keys == 0)
        return SPM_OK;
    // (runs are not merged in sets whose bands count seed hits: the count works on single diagonals)
    const bool band_merging = nv.max_k >= kMergeMinK && nv.max_k <= 1000;
    if (!band_merging && T.dedupe != 0)
        F.max_range = std::max(F.max_range, merge_entry_runs(keys));
    F.n_entries = keys.size();
    F.stride = S;
    F.n_probes = kBloomProbes;
    F.hash_variant = (uint32_t)T.hash;
    F.h_image.clear(); // what every workgroup stages into LDS
    if (T.hash == 2 && nv.sigma == 4 && S <= 2 && F.anchor_cm == 0) {
        // 8 or 16 windows of every 16 symbols are looked up: presence bits (one LDS read, no multiply) + L2 buckets
        F.hash_variant = 4;
        build_bits_level1(keys, F);
    } else {
        if (F.hash_variant == 2 && !build_fingerprint_table(keys, F))
            F.hash_variant = 1; // key set too dense for the fingerprint table: Bloom cascade
        if (nv.sigma != 4 && F.hash_variant != 2)
            return SPM_OK; // the dna5 kernel is built for the fingerprint table only
        if (F.hash_variant != 2)
            build_bloom_image(keys, F);
        F.lds_words = (uint32_t)F.h_image.size();
    }
    build_directory(keys, F, entries);
    F.ok = true;
    return SPM_OK;
}

} // namespace spm_hip
