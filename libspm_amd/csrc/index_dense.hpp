// index_dense.hpp -- the dense pass of the seed filter, host side: which dimers are anchors, where every needle's keys lie,
// and the pass's tables.  PURE HOST C++17 (no HIP).
//
// Dense pass: ONE pass for a needle set of any size (filter_shared.hpp says how the kernel looks windows up).
//
// Pieces.  The pigeonhole argument in its general form: if no needle POSITION lies in more than c pieces, k edits destroy
// at most c k pieces (an edit touches one position, or the gap between two, and a piece holding a gap holds its left
// position), so c k + 1 pieces leave one intact.  c = 1 is the usual "k + 1 disjoint pieces".  Every piece is a 16-symbol
// key window that begins with an anchor dimer, plus (c = 1 only) up to 16 neighbouring symbols that no other piece claims
// -- they go into the entry's signature, so a chance match of the key dies in registers.  Keys are taken greedily from
// the left: position p is taken if it is anchored and p >= (the c-th last one taken) + 16.  A needle that cannot fill
// k + 1 pieces tries c = 2, 3, .. kDenseCmax; if one needle still fails, the anchor set grows.
//
// Anchors.  A union of <= kDensePatterns dimer patterns.  Densities are tried in ascending order (1/8, 3/16, 1/4, 5/16,
// 3/8, 1/2, 3/4, 1); at every density the candidate sets are ranked on a sample of the needles by how many of them they
// leave without a layout, and the best one is tried on all.  (Random 150-symbol needles, k = 3: 1/8 leaves 0.2 % of them
// to c >= 2 and none uncovered; 100-symbol ones need 3/16.)
#pragma once

#include <chrono>
#include <cstdio>

#include "index_tables.hpp"

namespace spm_hip
{

struct dense_anchor_set
{
    uint32_t n_pat = 0, c[kDensePatterns] = {0, 0, 0}, cm[kDensePatterns] = {0, 0, 0};
    uint32_t dimers = 0; // bit d set: dimer d is an anchor
    uint32_t sixteenths() const { return (uint32_t)__builtin_popcount(dimers); }
};

inline dense_anchor_set anchor_union(const dense_anchor_set &a, uint32_t c, uint32_t cm)
{
    dense_anchor_set r = a;
    r.c[r.n_pat] = c & cm;
    r.cm[r.n_pat] = cm;
    ++r.n_pat;
    r.dimers |= dimer_mask_of(c, cm);
    return r;
}

// greedy key positions of one needle for overlap depth c; returns how many were found (at most `want`)
inline uint32_t dense_pick(const uint8_t *pat, uint32_t m, uint32_t dimers, uint32_t c, uint32_t want, uint16_t *pos)
{
    if (m < kKeyMax)
        return 0;
    uint32_t n = 0;
    for (uint32_t i = 0; i + kKeyMax <= m && n < want; ++i) {
        if (!((dimers >> dimer_at(pat, i)) & 1u))
            continue;
        if (n >= c && i < (uint32_t)pos[n - c] + kKeyMax)
            continue;
        pos[n++] = (uint16_t)i;
    }
    return n;
}

constexpr uint32_t kDenseCmax = 4; // pieces of a needle may overlap up to this many deep (c k + 1 pieces then)

// smallest overlap depth with which the needle gets its c k + 1 pieces (0: none up to kDenseCmax)
inline uint32_t dense_layout(const uint8_t *pat, uint32_t m, uint32_t k, uint32_t dimers, uint16_t *pos, uint32_t &n_out)
{
    for (uint32_t c = 1; c <= kDenseCmax; ++c) {
        const uint32_t want = c * k + 1;
        if (want > 255)
            break;
        if (dense_pick(pat, m, dimers, c, want, pos) == want) {
            n_out = want;
            return c;
        }
    }
    return 0;
}

constexpr uint32_t kDenseMaxPieces = kDenseCmax * 7 + 1; // k <= 7

inline bool dense_eligible(const needle_view &nv)
{
    if (nv.sigma != 4 || nv.max_k >= kMergeMinK || nv.n == 0)
        return false;
    for (uint32_t p = 0; p < nv.n; ++p) {
        const uint32_t m = (uint32_t)nv.m[p];
        if (m < kKeyMax * (nv.errors(p) + 1) || m > 2047)
            return false; // (k + 1 disjoint 16-symbol keys must fit whatever the anchors)
    }
    return true;
}

// the needles of [begin, end) (every step-th one) that have no layout with this anchor set: counted, and listed up to `cap`
inline uint64_t dense_uncovered(const needle_view &nv, uint32_t dimers, size_t begin, size_t end, size_t step,
                                std::vector<uint32_t> *list = nullptr, size_t cap = 0)
{
    uint64_t bad = 0;
    uint16_t pos[kDenseMaxPieces];
    for (size_t p = begin; p < end; p += step) {
        uint32_t n = 0;
        if (dense_layout(nv.needle(p), (uint32_t)nv.m[p], nv.errors(p), dimers, pos, n) == 0) {
            ++bad;
            if (list && list->size() < cap)
                list->push_back((uint32_t)p);
        }
    }
    return bad;
}

// ---- the anchor choice ----
// Densities are tried in ascending order.  At every rung the candidate sets are ranked by how many needles they leave
// without a layout -- on a sample of the set and on the HARD needles, those that a set tried earlier could not place (a
// poly-A needle only ever begins with AA: one such needle decides which sets are worth trying at all) --, and the best one
// is tried on all needles; what it fails on joins the hard list and the rung is ranked once more before the next one.
struct anchor_search
{
    const needle_view &nv;
    unsigned nt;
    size_t sample_step;
    std::vector<uint32_t> hard; // needles that a set tried on all of them left without a layout, 256 at most
};

// How many needles of the whole set this anchor set leaves without a layout; some of them join the hard list.  Every thread
// lists the first 8 of ITS slice, so which needles become hard -- and through them, in principle, which anchors are chosen
// -- can depend on the number of build threads (index_tuning::threads).  Known, and left as it is.
inline uint64_t uncovered_all(anchor_search &S, uint32_t dimers)
{
    std::vector<uint64_t> part(S.nt, 0);
    std::vector<std::vector<uint32_t>> lists(S.nt);
    parallel_slices(S.nv.n, S.nt,
                    [&](size_t b, size_t e, unsigned t) { part[t] = dense_uncovered(S.nv, dimers, b, e, 1, &lists[t], 8); });
    uint64_t s = 0;
    for (unsigned t = 0; t < S.nt; ++t) {
        s += part[t];
        for (uint32_t p : lists[t])
            if (S.hard.size() < 256)
                S.hard.push_back(p);
    }
    return s;
}

// rank the candidates of one rung (sample: once; hard needles: at every attempt) and try the best untried one on all
// needles, a few times; best_seen: the tried set that failed on the fewest; true: it covers every needle
inline bool try_rung(anchor_search &S, const std::vector<dense_anchor_set> &cands, dense_anchor_set &best_seen)
{
    const needle_view &nv = S.nv;
    std::vector<uint64_t> base(cands.size(), 0);
    parallel_slices(cands.size(), S.nt, [&](size_t b, size_t e, unsigned) {
        for (size_t i = b; i < e; ++i)
            base[i] = dense_uncovered(nv, cands[i].dimers, 0, nv.n, S.sample_step);
    });
    std::vector<uint8_t> tried(cands.size(), 0);
    uint64_t best_fail = ~0ull;
    for (int attempt = 0; attempt < 4; ++attempt) {
        size_t best = cands.size();
        uint64_t best_bad = ~0ull;
        for (size_t i = 0; i < cands.size(); ++i) {
            if (tried[i])
                continue;
            uint64_t bad = base[i];
            for (uint32_t p : S.hard)
                bad += 4096 * dense_uncovered(nv, cands[i].dimers, p, (size_t)p + 1, 1);
            if (bad < best_bad) {
                best_bad = bad;
                best = i;
            }
        }
        if (best == cands.size())
            break;
        tried[best] = 1;
        const size_t hard_before = S.hard.size();
        const uint64_t fail = uncovered_all(S, cands[best].dimers);
        if (fail < best_fail) {
            best_fail = fail;
            best_seen = cands[best];
        }
        if (fail == 0)
            return true;
        if (S.hard.size() == hard_before || fail > nv.n / 2000 + 4)
            break; // (nothing new to learn from / this density is far from enough: the next rung)
        // The needles it failed on: if most other sets of this rung place them, the failure is a matter of numbers (a
        // hundred thousand needles, each set unlucky with one or two) and the next set will meet its own: the next
        // rung.  If few sets place them (a poly-A needle wants AA), they now steer the ranking: once more.
        uint64_t placed = 0, asked = 0;
        for (size_t h = hard_before; h < S.hard.size(); ++h)
            for (size_t i = 0; i < cands.size(); i += 3) {
                ++asked;
                placed += dense_uncovered(nv, cands[i].dimers, S.hard[h], (size_t)S.hard[h] + 1, 1) == 0 ? 1 : 0;
            }
        if (2 * placed > asked)
            break;
    }
    return false;
}

// `base` with one more pattern, for every pattern with `care` compared bits that has none of the dimers of `base`
// (disjoint: the density really grows by the pattern's share)
inline std::vector<dense_anchor_set> anchor_extensions(const dense_anchor_set &base, uint32_t care)
{
    std::vector<dense_anchor_set> r;
    for (uint32_t cm = 0; cm < 16; ++cm) {
        if ((uint32_t)__builtin_popcount(cm) != care)
            continue;
        for (uint32_t c = 0; c < 16; ++c)
            if ((c & ~cm) == 0 && (dimer_mask_of(c, cm) & base.dimers) == 0)
                r.push_back(anchor_union(base, c, cm));
    }
    return r;
}

// The ladder: 2, 3, 4, 5, 6, 8, 12, 16 sixteenths of the dimers are anchors (a rung is built only if the ones below it
// leave a needle without a layout).  A rung's candidates are the best set seen at an earlier rung (`extends`; -1: the
// empty set) plus one more pattern with `care` compared bits.
struct anchor_rung
{
    int extends;
    uint32_t care;
    bool dimer_pairs; // also any two single dimers (two patterns: ~5 VALU more per 16 windows)
};
constexpr anchor_rung kAnchorLadder[] = {
    {-1, 3, true}, // 2/16: one pattern with a don't-care bit, or two dimers
    {0, 4, false}, // 3/16
    {-1, 2, false}, // 4/16
    {2, 4, false}, // 5/16
    {2, 3, false}, // 6/16
    {-1, 1, false}, // 8/16
    {5, 2, false}, // 12/16
    {-1, 0, false}, // every window
};
constexpr size_t kAnchorRungs = sizeof(kAnchorLadder) / sizeof(kAnchorLadder[0]);

inline std::vector<dense_anchor_set> rung_candidates(const anchor_rung &R, const dense_anchor_set *best_of_rung)
{
    const dense_anchor_set none;
    std::vector<dense_anchor_set> c = anchor_extensions(R.extends < 0 ? none : best_of_rung[R.extends], R.care);
    if (R.dimer_pairs)
        for (uint32_t d0 = 0; d0 < 16; ++d0)
            for (uint32_t d1 = d0 + 1; d1 < 16; ++d1)
                if (__builtin_popcount(d0 ^ d1) != 1) // (those are the single patterns)
                    c.push_back(anchor_union(anchor_union(none, d0, 15), d1, 15));
    return c;
}

inline bool choose_dense_anchors(const needle_view &nv, const index_tuning &T, dense_anchor_set &out)
{
    anchor_search S{nv, T.n_threads(), std::max<size_t>(1, nv.n / 1024), {}};
    const int max_density = T.dense >= 2 ? 16 : 8; // beyond 8 sixteenths the set is not worth a dense pass (unless forced)
    dense_anchor_set best_of_rung[kAnchorRungs];
    for (size_t rung = 0; rung < kAnchorRungs; ++rung) {
        const std::vector<dense_anchor_set> c = rung_candidates(kAnchorLadder[rung], best_of_rung);
        if (c.empty() || (int)c[0].sixteenths() < T.dense_min_density)
            continue;
        if ((int)c[0].sixteenths() > max_density)
            return false;
        if (try_rung(S, c, best_of_rung[rung])) {
            out = best_of_rung[rung];
            return true;
        }
    }
    return false;
}

// ---- the layouts ----
struct dense_layouts // per needle p: overlap depth c[p], n[p] keys at pos[first[p] ..] (positions in the needle)
{
    std::vector<uint8_t> c, n;
    std::vector<uint32_t> first;
    std::vector<uint16_t> pos;
};

// first fit, per needle (threads), the positions laid out back to back
inline dense_layouts dense_first_fit(const needle_view &nv, unsigned nt, uint32_t dimers)
{
    dense_layouts L;
    L.c.assign(nv.n, 0);
    L.n.assign(nv.n, 0);
    L.first.assign(nv.n + 1, 0);
    std::vector<std::vector<uint16_t>> pos_of(nt); // thread t: the positions of its slice of needles, back to back
    parallel_slices(nv.n, nt, [&](size_t b, size_t e, unsigned t) {
        uint16_t pos[kDenseMaxPieces];
        std::vector<uint16_t> &out = pos_of[t];
        out.reserve((e - b) * 5);
        for (size_t p = b; p < e; ++p) {
            uint32_t n = 0;
            L.c[p] = (uint8_t)dense_layout(nv.needle(p), (uint32_t)nv.m[p], nv.errors(p), dimers, pos, n);
            L.n[p] = (uint8_t)n;
            out.insert(out.end(), pos, pos + n);
        }
    });
    for (uint32_t p = 0; p < nv.n; ++p)
        L.first[p + 1] = L.first[p] + L.n[p];
    L.pos.reserve(L.first[nv.n]);
    for (unsigned t = 0; t < nt; ++t) // (the slices of parallel_slices are contiguous and ascending)
        L.pos.insert(L.pos.end(), pos_of[t].begin(), pos_of[t].end());
    return L;
}

// Which windows become keys decides how many presence bits are set, i.e. how many text windows pass level 1 and cost a
// gather from L2 -- the resource the dense pass runs out of first.  A needle usually has several layouts (150 symbols, 3/16
// of the dimers: ~25 anchored windows for 4 keys), so every needle with disjoint pieces (c = 1) takes the layout whose keys
// hit the most bits that OTHER needles have set already (dynamic programme over its anchored windows: best number of shared
// bits with j keys from window i on).  Needles are taken in rounds of n / 32: a round reads the bit counts the rounds before it
// left (and its own needles' previous choice, which does not count), then its changes are applied -- the result does not
// depend on the number of threads.  Two sweeps (the first needles chose when the table was empty): random 150-symbol
// needles, k = 3, 100 000 of them: 31.7 % of the 2^20 bits set with first-fit keys, 18.4 % after one sweep, 16.0 % after two.
inline void dense_share_bits(const needle_view &nv, const index_tuning &T, uint32_t dimers, const std::vector<uint8_t> &cc,
                             const std::vector<uint32_t> &first, std::vector<uint16_t> &pos_flat)
{
    thread_team team(T.n_threads());
    std::vector<uint16_t> ref(1u << kDenseBloomBits, 0); // keys per presence bit
    std::vector<uint8_t> placed(nv.n, 0); // the needle's keys are counted in ref
    std::vector<uint32_t> bit_of(pos_flat.size(), 0), fresh_bit(pos_flat.size(), 0); // presence bit of every chosen key
    for (uint32_t p = 0; p < nv.n; ++p)
        if (cc[p] != 1) { // (overlapping pieces keep their first-fit keys)
            for (uint32_t s = first[p]; s < first[p + 1]; ++s)
                ++ref[bit_of[s] = dense_bloom_index(window_key(4, nv.needle(p), pos_flat[s], kKeyMax))];
            placed[p] = 1;
        }
    constexpr uint32_t kRounds = 24;
    std::vector<uint16_t> fresh(pos_flat.size());
    // The round's changes to the counters, bucketed by counter range: thread t files its needles' changes under the range
    // they fall in, then thread r applies everything filed under range r -- every change read once, every counter touched
    // by one thread (no atomics, the same result whatever the thread count), and that thread's 1/nt of the 2 MB of counters
    // stays in its cache (the updates are random: done by one thread they were a third of this function's time).
    const unsigned nt = team.size();
    std::vector<std::vector<std::vector<uint32_t>>> upd(nt, std::vector<std::vector<uint32_t>>(nt));
    auto range_of = [&](uint32_t bit) { return (unsigned)(((uint64_t)bit * nt) >> kDenseBloomBits); };
    for (int sweep = 0; sweep < 2; ++sweep)
        for (uint32_t round = 0; round < kRounds; ++round) {
            const size_t rb = (size_t)nv.n * round / kRounds, re = (size_t)nv.n * (round + 1) / kRounds;
            for (auto &per_thread : upd) // (every thread's files, also of threads that get no slice this round)
                for (auto &v : per_thread)
                    v.clear();
            team.run(re - rb, [&](size_t b, size_t e, unsigned tid) {
                std::vector<uint16_t> cpos;
                std::vector<uint32_t> cbit, nxt;
                std::vector<uint8_t> shared;
                std::vector<int16_t> dp;
                for (size_t p = rb + b; p < rb + e; ++p) {
                    const uint32_t need = first[p + 1] - first[p];
                    if (cc[p] != 1 || need == 0)
                        continue;
                    const uint8_t *pat = nv.needle(p);
                    const uint32_t m = (uint32_t)nv.m[p];
                    uint32_t own[kDenseMaxPieces];
                    for (uint32_t j = 0; j < need; ++j)
                        own[j] = placed[p] ? bit_of[first[p] + j] : 0xFFFFFFFFu;
                    // the anchored windows, their bits, and whether somebody else has set them
                    cpos.clear();
                    cbit.clear();
                    shared.clear();
                    uint32_t key = window_key(4, pat, 0, kKeyMax);
                    for (uint32_t i = 0; i + kKeyMax <= m; ++i) {
                        if (i)
                            key = (key >> 2) | ((uint32_t)(pat[i + kKeyMax - 1] & 3u) << 30);
                        if (!((dimers >> (key & 15u)) & 1u))
                            continue;
                        const uint32_t bit = dense_bloom_index(key);
                        uint32_t mine = 0;
                        for (uint32_t j = 0; j < need; ++j)
                            mine += own[j] == bit ? 1u : 0u;
                        cpos.push_back((uint16_t)i);
                        cbit.push_back(bit);
                        shared.push_back(ref[bit] > mine ? 1 : 0);
                    }
                    const uint32_t nc = (uint32_t)cpos.size();
                    nxt.assign(nc + 1, nc); // first candidate that does not overlap candidate i
                    for (uint32_t i = 0, t = 0; i < nc; ++i) {
                        while (t < nc && cpos[t] < cpos[i] + kKeyMax)
                            ++t;
                        nxt[i] = t;
                    }
                    // dp[j][i]: most shared bits with j keys among candidates i.., -1: no such layout
                    dp.assign((size_t)(need + 1) * (nc + 1), -1);
                    for (uint32_t i = 0; i <= nc; ++i)
                        dp[i] = 0;
                    for (uint32_t j = 1; j <= need; ++j)
                        for (uint32_t i = nc; i-- > 0;) {
                            const int16_t skip = dp[(size_t)j * (nc + 1) + i + 1];
                            const int16_t rest = dp[(size_t)(j - 1) * (nc + 1) + nxt[i]];
                            const int16_t take = rest < 0 ? (int16_t)-1 : (int16_t)(rest + shared[i]);
                            dp[(size_t)j * (nc + 1) + i] = take >= skip ? take : skip;
                        }
                    if (dp[(size_t)need * (nc + 1)] < 0) { // (cannot happen: first fit found a layout)
                        for (uint32_t j = 0; j < need; ++j) {
                            fresh[first[p] + j] = pos_flat[first[p] + j];
                            fresh_bit[first[p] + j] = dense_bloom_index(window_key(4, pat, pos_flat[first[p] + j], kKeyMax));
                        }
                    } else
                    for (uint32_t i = 0, j = need; j >= 1;) {
                        const int16_t rest = dp[(size_t)(j - 1) * (nc + 1) + nxt[i]];
                        const int16_t take = rest < 0 ? (int16_t)-1 : (int16_t)(rest + shared[i]);
                        if (take >= 0 && take == dp[(size_t)j * (nc + 1) + i] && take >= dp[(size_t)j * (nc + 1) + i + 1]) {
                            fresh[first[p] + (need - j)] = cpos[i];
                            fresh_bit[first[p] + (need - j)] = cbit[i];
                            i = nxt[i];
                            --j;
                        } else {
                            ++i;
                        }
                    }
                    // this needle's changes: filed for the counters (bit | 1 << 31: one key less), written back for the needle
                    // (nobody else reads a needle's own positions and bits)
                    for (uint32_t s2 = first[p]; s2 < first[p + 1]; ++s2) {
                        if (placed[p])
                            upd[tid][range_of(bit_of[s2])].push_back(bit_of[s2] | 0x80000000u);
                        upd[tid][range_of(fresh_bit[s2])].push_back(fresh_bit[s2]);
                        pos_flat[s2] = fresh[s2];
                        bit_of[s2] = fresh_bit[s2];
                    }
                    placed[p] = 1;
                }
            });
            team.run(nt, [&](size_t b, size_t e, unsigned) {
                for (size_t r = b; r < e; ++r)
                    for (unsigned t2 = 0; t2 < nt; ++t2)
                        for (uint32_t u : upd[t2][r]) {
                            if (u & 0x80000000u)
                                --ref[u & 0x7FFFFFFFu];
                            else
                                ++ref[u];
                        }
            });
        }
}

// The piece around every key and its entry.  c = 1: the key plus what lies between it and its neighbours' halves of the
// gaps, at most 8 symbols before and 16 in all; c > 1: the key alone.  Fills the seed layout of X and returns the entries
// on their way into the tables, needle by needle.
inline std::vector<index_kv> dense_pieces(const needle_view &nv, unsigned nt, const dense_layouts &L, seed_index &X)
{
    const size_t n_keys = L.pos.size();
    X.seed_q.assign(nv.n, 0);
    X.seed_n.assign(nv.n, 0);
    X.seed_c.assign(nv.n, 1);
    X.seed_first = L.first;
    X.seed_off.assign(n_keys, 0);
    X.seed_len.assign(n_keys, 0);
    std::vector<index_kv> keys(n_keys);
    parallel_slices(nv.n, nt, [&](size_t b, size_t e, unsigned) {
        for (size_t p = b; p < e; ++p) {
            const uint16_t *pos = L.pos.data() + L.first[p];
            const uint32_t m = (uint32_t)nv.m[p], c = L.c[p], n = L.n[p];
            X.seed_n[p] = (uint16_t)n;
            X.seed_c[p] = (uint8_t)c;
            for (uint32_t j = 0; j < n; ++j) {
                uint32_t lo = pos[j], hi = pos[j] + kKeyMax;
                if (c == 1) {
                    const uint32_t gap_l = j == 0 ? pos[j] : (pos[j] - (pos[j - 1] + kKeyMax)) / 2;
                    const uint32_t gap_r = j + 1 == n ? m - hi : (pos[j + 1] - hi + 1) / 2;
                    const uint32_t before = std::min<uint32_t>(8, gap_l);
                    const uint32_t after = std::min<uint32_t>(16 - before, gap_r);
                    lo -= before;
                    hi += after;
                }
                const size_t s = (size_t)L.first[p] + j;
                X.seed_off[s] = (uint16_t)lo;
                X.seed_len[s] = (uint16_t)(hi - lo);
                keys[s] = make_kv(nv, seed_key{(uint32_t)p, lo, pos[j] - lo, hi - lo}, kKeyMax);
            }
        }
    });
    return keys;
}

// the dense pass's header: 16-symbol keys at every anchored window
inline filter_index dense_pass_header(const dense_anchor_set &A, size_t n_keys)
{
    filter_index F;
    F.dense = 1;
    F.key_len = kKeyMax;
    F.stride = 1;
    F.n_pat = A.n_pat;
    for (uint32_t i = 0; i < A.n_pat; ++i) {
        F.pat_c[i] = A.c[i];
        F.pat_cm[i] = A.cm[i];
    }
    F.dimer_set = A.dimers;
    F.n_keys = n_keys;
    F.n_entries = n_keys;
    F.hash_variant = 3;
    return F;
}

// X.fidx stays empty where some needle has no layout even with the densest anchor set allowed: not a dense set
inline int build_dense_index(const needle_view &nv, const index_tuning &T, seed_index &X)
{
    using iclk = std::chrono::steady_clock;
    auto ms = [&](iclk::time_point a) { return std::chrono::duration<double, std::milli>(iclk::now() - a).count(); };
    const unsigned nt = T.n_threads();
    const auto t0 = iclk::now();
    dense_anchor_set A;
    if (!choose_dense_anchors(nv, T, A))
        return SPM_OK;
    const double ms_anchors = ms(t0);
    const auto t1 = iclk::now();
    dense_layouts L = dense_first_fit(nv, nt, A.dimers);
    const double ms_first_fit = ms(t1);
    dense_share_bits(nv, T, A.dimers, L.c, L.first, L.pos);
    const double ms_share = ms(t1) - ms_first_fit;
    std::vector<index_kv> keys = dense_pieces(nv, nt, L, X);
    const double ms_layout = ms(t1);
    const auto t2 = iclk::now();
    filter_index F = dense_pass_header(A, keys.size());
    build_bits_level1(keys, F); // level 1: presence bits; level 1b: fingerprint buckets (about two keys per bucket)
    const double ms_level1 = ms(t2);
    const auto t3 = iclk::now();
    build_directory(keys, F, X.h_entries); // the exact level
    if (trace_on()) {
        uint64_t set = 0;
        for (uint32_t w : F.h_image)
            set += (uint64_t)__builtin_popcount(w);
        fprintf(stderr, "[spm_hip] dense index: %zu keys, anchors %u/16 (%u pattern(s)), %.1f %% of the presence bits set; anchors %.2f ms, "
                        "layouts %.2f (first fit %.2f, shared bits %.2f), bits + buckets %.2f, directory %.2f (%u threads)\n",
                keys.size(), A.sixteenths(), A.n_pat, 100.0 * (double)set / (double)(1u << kDenseBloomBits), ms_anchors, ms_layout,
                ms_first_fit, ms_share, ms_level1, ms(t3), nt);
    }
    F.ok = true;
    X.fidx.push_back(std::move(F));
    X.filter_stride = 1;
    X.filter_key_len = kKeyMax;
    X.filter_anchored = false;
    X.filter_dense = true;
    X.filter_max_range = 0;
    return SPM_OK;
}

} // namespace spm_hip
