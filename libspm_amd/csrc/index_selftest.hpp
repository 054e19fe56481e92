// index_selftest.hpp -- host-only self-check of the seed index (no device): builds the tables exactly as
// spm_hip_patterns_create does and verifies the properties the filter's losslessness rests on.  level1_accepts and
// directory_holds are the host statement of what the kernels evaluate.  stats: see include/spm_hip.h.  Part of
// index_build.hpp, which includes it below the planner it checks.
#pragma once

#include <cstring>

namespace spm_hip
{

// level-1 membership test, exactly as the kernels evaluate it
inline bool level1_accepts(const filter_index &F, uint32_t key)
{
    if (F.dense || F.hash_variant == 4) {
        if (F.dense && !((F.dimer_set >> (key & 15u)) & 1u))
            return false; // the streaming kernel does not look this window up
        const uint32_t b = dense_bloom_index(key);
        if (!((F.h_image[b >> 5] >> (b & 31)) & 1u))
            return false;
        const uint16_t *bk = F.h_buckets.data() + (size_t)dense_bucket(key, F.bucket_shift) * kDenseSlots;
        if (bk[kDenseSlots - 1] == kDenseAcceptAll)
            return true;
        for (uint32_t s = 0; s < kDenseSlots; ++s)
            if (bk[s] == dense_fp(key))
                return true;
        return false;
    }
    if (F.hash_variant == 2) {
        const uint16_t *fp = reinterpret_cast<const uint16_t *>(F.h_image.data());
        const uint16_t *disp = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(F.h_image.data()) + F.chd_disp_off);
        const chd_hashes hh = chd_hash(key);
        const uint32_t d = disp[hh.x >> F.chd_bucket_shift];
        return fp[chd_slot(hh, d, F.chd_slot_mask)] == hh.f;
    }
    const uint32_t idx_mask = F.bitmap_words * 32 - 1;
    for (uint32_t pr = 0; pr < F.n_probes; ++pr) {
        const uint32_t x = bloom_hash(key, pr) & idx_mask;
        if (!((F.h_image[x >> 5] >> (x & 31)) & 1))
            return false;
    }
    return true;
}

// the exact level: pass F's directory has `key`, and among its entries one for val = needle << 11 | offset
inline bool directory_holds(const seed_index &X, const filter_index &F, uint32_t key, uint32_t val)
{
    uint32_t slot = ht_hash(key) & F.ht_mask;
    for (;;) {
        const u32x4 d = F.h_ht[slot];
        if (d.z == 0)
            return false;
        if (d.x == key) {
            for (uint32_t q = 0; q < d.z; ++q) {
                const u32x4 e = X.h_entries[d.y + q];
                if (e.w != key)
                    return false; // the entries of a key lie side by side
                if ((e.x >> 11) == (val >> 11)) {
                    // the entry itself, or a run whose diagonal range covers this offset
                    const uint32_t x0 = e.x & 0x7FF, x = val & 0x7FF;
                    if (!(e.z & kRngRun) ? x == x0 : (x >= x0 && x <= x0 + (e.z & 0x7FF)))
                        return true;
                }
            }
            return false;
        }
        slot = (slot + 1) & F.ht_mask;
    }
}

// the window of needle p at offset `at` is found at every level of pass F
inline bool window_indexed(const needle_view &nv, const seed_index &X, const filter_index &F, uint32_t p, uint32_t at)
{
    const uint32_t key = window_key(nv.sigma, nv.needle(p), at, F.key_len);
    return level1_accepts(F, key) && directory_holds(X, F, key, (p << 11) | at);
}

// false-positive rate of level 1 on pseudo-random keys: stats[5] of stats[6]
inline void selftest_false_positives(const filter_index &F, uint64_t *stats)
{
    const uint32_t key_mask = F.key_len >= 16 ? 0xFFFFFFFFu : ((1u << (2 * F.key_len)) - 1);
    const uint64_t trials = 1 << 20;
    uint64_t fp = 0;
    for (uint64_t t = 0; t < trials; ++t)
        fp += level1_accepts(F, (uint32_t)mix64(0xC0FFEE + t) & key_mask) ? 1 : 0;
    stats[5] = fp;
    stats[6] = trials;
}

// Dense pass.  Every needle: c k + 1 pieces, no position in more than c of them, each piece inside the needle and holding
// its key window, which begins with an anchor and is found at all three levels with the piece's entry
inline int selftest_dense(const needle_view &nv, const seed_index &X, uint64_t *stats)
{
    const filter_index &F = X.fidx[0];
    uint64_t checked = 0, missing = 0, deep = 0; // deep: needles with c > 1
    for (uint32_t p = 0; p < nv.n; ++p) {
        const uint32_t m = (uint32_t)nv.m[p], c = X.seed_c[p], sn = X.seed_n[p];
        if (c == 0 || sn < c * (uint32_t)nv.k[p] + 1)
            return SPM_E_INVALID;
        deep += c > 1 ? 1 : 0;
        std::vector<uint8_t> cover(m, 0);
        for (uint32_t j = 0; j < sn; ++j) {
            const uint32_t o = X.seed_off[X.seed_first[p] + j], q = X.seed_len[X.seed_first[p] + j];
            if (q < kKeyMax || o + q > m)
                return SPM_E_INVALID;
            for (uint32_t i = 0; i < q; ++i)
                if (++cover[o + i] > c)
                    return SPM_E_INVALID;
            // the piece's entry: some window of the piece, anchored, with val = (p, window offset)
            uint32_t found = 0;
            for (uint32_t r = 0; r + kKeyMax <= q; ++r)
                found += window_indexed(nv, X, F, p, o + r) ? 1 : 0;
            ++checked;
            missing += found < 1 ? 1 : 0;
        }
    }
    stats[3] = checked;
    stats[4] = missing;
    selftest_false_positives(F, stats);
    stats[7] = 3u | ((uint64_t)__builtin_popcount(F.dimer_set & 0xFFFFu) << 8) | (deep << 16);
    return missing ? SPM_E_INVALID : SPM_OK;
}

// sparse passes, needle p: the stride reaches every occurrence, k + 1 seeds, each inside the needle, disjoint, of key symbols
inline bool selftest_seeds_sound(const needle_view &nv, const seed_index &X, uint32_t p)
{
    const uint32_t q = X.seed_q[p], sn = X.seed_n[p];
    if (X.filter_stride > q - (X.filter_key_len - 1) || sn < (uint32_t)nv.k[p] + 1)
        return false; // sampling would miss occurrences / too few seeds for the pigeonhole argument
    for (uint32_t j = 0; j < sn; ++j) {
        const uint32_t o = X.seed_off[X.seed_first[p] + j];
        if (o + q > (uint32_t)nv.m[p] || (j && o < (uint32_t)X.seed_off[X.seed_first[p] + j - 1] + q))
            return false;
        for (uint32_t i = 0; i < q; ++i)
            if (!key_symbol(nv.sigma, nv.needle(p)[o + i]))
                return false;
    }
    return true;
}

struct selftest_counts
{
    uint64_t checked = 0, missing = 0;
    size_t pass = 0;      // plain passes: the pass the current needle belongs to ...
    uint64_t in_pass = 0; // ... and the keys of the needles before it in that pass
};

// Anchored passes, needle p: every seed has ONE key, in one pass, and that key begins with an anchor dimer of the pass (so
// the streaming kernel, which looks up only such windows, meets it)
inline void selftest_anchored_needle(const needle_view &nv, const seed_index &X, uint32_t p, selftest_counts &C)
{
    const uint32_t q = X.seed_q[p];
    for (uint32_t j = 0; j < X.seed_n[p]; ++j) {
        const uint32_t o = X.seed_off[X.seed_first[p] + j];
        uint32_t found = 0;
        for (const filter_index &F : X.fidx)
            for (uint32_t r = 0; r + X.filter_key_len <= q && r < 32; ++r)
                if (((dimer_at(nv.needle(p), o + r) ^ F.anchor_c) & F.anchor_cm) == 0 && window_indexed(nv, X, F, p, o + r))
                    ++found;
        ++C.checked;
        C.missing += found < 1 ? 1 : 0;
    }
}

// Plain passes, needle p: it belongs to exactly one pass (the passes take the needles in order), and every indexed window
// of every seed is found at both levels.  false: the passes' key counts do not add up
inline bool selftest_plain_needle(const needle_view &nv, const seed_index &X, uint32_t p, selftest_counts &C)
{
    const uint32_t S = X.filter_stride, sn = X.seed_n[p];
    const uint64_t mine = (uint64_t)sn * S;
    while (C.pass < X.fidx.size() && C.in_pass + mine > X.fidx[C.pass].n_keys) {
        if (C.in_pass != X.fidx[C.pass].n_keys)
            return false;
        ++C.pass;
        C.in_pass = 0;
    }
    if (C.pass >= X.fidx.size())
        return false;
    C.in_pass += mine;
    for (uint32_t j = 0; j < sn; ++j)
        for (uint32_t r = 0; r < S; ++r) {
            ++C.checked;
            C.missing += window_indexed(nv, X, X.fidx[C.pass], p, X.seed_off[X.seed_first[p] + j] + r) ? 0 : 1;
        }
    return true;
}

inline int selftest_sparse(const needle_view &nv, const seed_index &X, uint64_t keys_total, uint64_t *stats)
{
    uint64_t expect = 0;
    for (uint32_t p = 0; p < nv.n; ++p)
        expect += (uint64_t)X.seed_n[p] * X.filter_stride;
    if (expect != keys_total)
        return SPM_E_INVALID;
    selftest_counts C;
    for (uint32_t p = 0; p < nv.n; ++p) {
        if (!selftest_seeds_sound(nv, X, p))
            return SPM_E_INVALID;
        if (X.filter_anchored)
            selftest_anchored_needle(nv, X, p, C);
        else if (!selftest_plain_needle(nv, X, p, C))
            return SPM_E_INVALID;
    }
    uint64_t anchor_sum = 0; // dimers looked up, over all passes
    for (const filter_index &F : X.fidx)
        anchor_sum += 1ull << (4 - __builtin_popcount(F.anchor_cm));
    stats[3] = C.checked;
    stats[4] = C.missing;
    selftest_false_positives(X.fidx[0], stats);
    stats[7] = X.fidx[0].hash_variant | (X.filter_anchored ? anchor_sum << 8 : 0);
    return C.missing ? SPM_E_INVALID : SPM_OK;
}

inline int host_selftest(int algo, const uint8_t *ranks_concat, const uint32_t *offsets, uint32_t n_patterns,
                         const uint16_t *k, uint32_t sigma, uint64_t *stats)
{
    if (!ranks_concat || !offsets || !stats || n_patterns == 0)
        return SPM_E_INVALID;
    std::vector<int32_t> mm(n_patterns, 0), kk(n_patterns, 0);
    needle_view nv;
    nv.algo = algo;
    nv.n = n_patterns;
    nv.sigma = sigma;
    nv.ranks = ranks_concat;
    nv.offsets = offsets;
    for (uint32_t p = 0; p < n_patterns; ++p) {
        mm[p] = (int32_t)(offsets[p + 1] - offsets[p]);
        kk[p] = (nv.is_myers() && k) ? k[p] : 0;
        nv.max_k = std::max<uint32_t>(nv.max_k, (uint32_t)kk[p]);
    }
    nv.m = mm.data();
    nv.k = kk.data();
    seed_index X;
    const int rc = build_filter_index(nv, index_tuning::from_env(), X);
    memset(stats, 0, 8 * sizeof(uint64_t));
    if (rc != SPM_OK)
        return rc;
    stats[0] = X.fidx.size();   // passes (0 = the seed filter does not apply)
    stats[1] = X.filter_stride | ((uint64_t)X.filter_key_len << 32); // S | H << 32
    if (X.fidx.empty())
        return SPM_OK;
    uint64_t keys_total = 0;
    for (const filter_index &F : X.fidx)
        keys_total += F.n_keys;
    stats[2] = keys_total;
    return X.filter_dense ? selftest_dense(nv, X, stats) : selftest_sparse(nv, X, keys_total, stats);
}

} // namespace spm_hip
