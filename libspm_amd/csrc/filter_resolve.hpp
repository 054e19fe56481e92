// filter_resolve.hpp -- the resolve stage of the seed filter (filter.hpp): resolve_kernel with its checks and its queues.
// The kernel is no template: exactly one translation unit (filter_resolve.hip) includes this header.
#pragma once

#include "filter_params.hpp"
#include "pack.hpp"
#include "wave.hpp"

namespace spm_hip
{

// ---------------------------------------------------------------------------------------------------
// resolve: survivors -> (needle, offset) through the exact key directory -> whole-seed check, piece count -> diagonal bands
// ---------------------------------------------------------------------------------------------------
// One lane per survivor, a full grid: the L2 round trips of the table probes overlap across thousands of waves instead of
// stalling the streaming kernel.
//   * A survivor says: the key window at needle offset x matches the text at t.  The pigeonhole argument needs a seed
//     that occurs in the text UNCHANGED, and such a seed yields a survivor of its own -- so a (survivor, entry) pair whose
//     whole seed does not match exactly is dropped without losing an occurrence.  On long texts most pairs are chance
//     matches of the key (C4: 800 000 of 1 140 000; C3: 16 000 of 20 000); they fail after ~1.3 symbols.
//   * What is left is counted into a hash table keyed (needle, haystack, diagonal band); the first arrival of a band
//     appends it to the band list.  A band is verified ONCE, over every end position its diagonals can produce -- the 17
//     sampled windows of one needle inside one 136-base microsatellite are one or two verifications, not 17; the 65
//     seeds of a |P| = 1024, k = 64 occurrence one, not 65.
//   * Sets whose needles carry k + 2 seeds (k >= kMergeMinK): an occurrence keeps >= 2 seeds intact, on diagonals <= k
//     apart; bands overlap by k + 1 diagonals so that those seeds always share a band, and a band is verified only if it
//     collected as many seed hits as the needle has surplus seeds.

// 16 bytes from an arbitrary address with ONE load: gfx950 under amdhsa runs with unaligned access enabled, so an
// align-1 copy of 16 bytes is a single global_load_dwordx4.  (Byte loads would cost the memory pipe 16 instructions, each
// as expensive as this one; the checks below run for 10^7..10^8 (survivor, entry) pairs on a repeat-rich text.)
__device__ __forceinline__ uint4 load_bytes16(const uint8_t *p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// the same near the end of a buffer: bytes at or beyond `limit` read as 0xFF (never equal to a symbol)
__device__ __forceinline__ uint4 load_bytes16_guarded(const uint8_t *base, uint64_t idx, uint64_t limit)
{
    if (idx + 16 <= limit)
        return load_bytes16(base + idx);
    uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (int b = 0; b < 16; ++b)
        if (idx + b < limit)
            w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)base[idx + b] << (8 * (b & 3)));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t diff16(const uint4 a, const uint4 b, uint32_t n) // n <= 16 leading bytes compared
{
    const uint32_t d[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
    uint32_t r = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t have = n > 4 * i ? n - 4 * i : 0; // bytes of this dword that count
        const uint32_t mask = have >= 4 ? 0xFFFFFFFFu : (have == 0 ? 0u : (1u << (8 * have)) - 1);
        r |= d[i] & mask;
    }
    return r;
}

// r = offset of the key window inside its seed (the seeds of a needle with an N do not sit at multiples of q)
// q_whole: the seed's length when the entry spells it (kRngWhole: key + signature are the whole seed; the pieces of a
// dense pass differ in length), 0: all seeds of the needle are seed_q[needle] long
__device__ __forceinline__ bool seed_intact(const resolve_params &P, uint64_t t, uint32_t val, uint32_t r, uint32_t q_whole,
                                            int64_t hay_b, int64_t hay_e)
{
    if (!P.needle_ranks)
        return true;
    const uint32_t pat = val >> 11, x = val & 0x7FF;
    struct
    {
        uint32_t q;
    } sp{q_whole ? q_whole : P.seed_q[pat]};
    const uint32_t o = x - r; // start of the seed inside the needle
    const int64_t ts = (int64_t)t - (int64_t)r; // where the seed would start in the text
    if (ts < hay_b || ts + (int64_t)sp.q > hay_e)
        return false; // it would stick out of the haystack
    const uint8_t *nd = P.needle_ranks + P.needle_offsets[pat] + o; // (the needle buffer is padded: no guard)
    // (the key window itself already matched; comparing it again costs less than skipping it.)  16 symbols per round: a
    // chance match of the key fails in the first
    for (uint32_t i = 0; i < sp.q; i += 16) {
        const uint32_t n = sp.q - i < 16 ? sp.q - i : 16;
        if (diff16(load_bytes16_guarded(P.text, (uint64_t)ts + i, P.text_alloc), load_bytes16(nd + i), n))
            return false;
    }
    return true;
}

// Piece count (dna4 sets without surplus seeds, i.e. k < kMergeMinK) -- the q-gram lemma on aligned pieces.  The seed
// sits unchanged on diagonal d (needle position y <-> text index d + y).  Cut the needle into pieces of 8 symbols: an
// occurrence with <= k edits leaves all but k of them unchanged, each displaced by at most k from its place on the
// diagonal (the indels between it and the seed).  So if more than k pieces are found nowhere within +-k of their place,
// no occurrence contains this seed here -- and an occurrence always has an intact seed whose pieces pass.  What this
// removes: the seed hits of needles that merely END in a microsatellite or a poly-A run, in every stretch of the same
// unit (their unique part fails after two or three blocks); each would have cost a band and a verification of ~170
// columns.  Needles that ARE a repeat pass, as they must: they occur there.  A pair whose needle would stick out of the
// haystack is not checked.
//
// The count runs two rounds (32 needle symbols, four pieces) per visit, starting at the end of the needle that is far
// from the seed -- the seed sits in the part the needle shares with the text, what differs is at the other end -- and a
// pair that is neither rejected nor through goes back into the wave's queue: on a repeat-rich text 85 % of the pairs are
// rejected in the first visit, and the other lanes of the wave do not wait for the 15 % that need all the rounds.
// Progress lives in the pair's `rng` word: rounds done (bits 21..27), pieces missing (28..30).
constexpr uint32_t kPieceRoundsShift = 21, kPieceMissingShift = 28;

__device__ __forceinline__ bool pieces_apply(const resolve_params &P, uint64_t t, uint32_t val, uint32_t m, uint32_t k, int64_t hay_b,
                                             int64_t hay_e)
{
    if (!P.pieces_check || k == 0 || k > 7 || m < 32)
        return false;
    const int64_t d = (int64_t)t - (int64_t)(val & 0x7FF);
    return d - (int64_t)k >= hay_b && d + (int64_t)(m + k) <= hay_e;
}

// one visit; returns 0: rejected, 1: more rounds to go (rng updated), 2: through
__device__ __forceinline__ uint32_t pieces_visit(const resolve_params &P, uint64_t t, uint32_t val, uint32_t &rng, uint32_t m, uint32_t k)
{
    const uint32_t pat = val >> 11, x = val & 0x7FF;
    const uint32_t n_rounds = m >> 4; // two pieces per 16 needle symbols
    uint32_t done = (rng >> kPieceRoundsShift) & 0x7F, missing = (rng >> kPieceMissingShift) & 7;
    const bool ascending = 2 * x >= m; // seed in the right half: start at the left end
    const uint32_t todo = n_rounds - done < 2 ? n_rounds - done : 2;
    // rounds `done`, `done + 1` in visiting order are the needle words r_lo, r_lo + 1 (if todo == 2)
    const uint32_t r_lo = ascending ? done : n_rounds - done - todo;
    const uint32_t *pk = P.needle_pk + P.pk_offsets[pat] + r_lo;
    const uint32_t nw0 = pk[0], nw1 = todo == 2 ? pk[1] : 0;
    // text [d + 16 r_lo - k, ... + 48): 16 + 2k <= 30 symbols per round, the two rounds share the middle load
    const uint64_t w0 = (uint64_t)((int64_t)t - (int64_t)x + (int64_t)(16 * r_lo) - (int64_t)k);
    const uint32_t c0 = pack16(load_bytes16_guarded(P.text, w0, P.text_alloc));
    const uint32_t c1 = pack16(load_bytes16_guarded(P.text, w0 + 16, P.text_alloc));
    const uint32_t c2 = todo == 2 ? pack16(load_bytes16_guarded(P.text, w0 + 32, P.text_alloc)) : 0;
#pragma unroll
    for (uint32_t rr = 0; rr < 2; ++rr) {
        if (rr < todo) {
            const uint32_t two = rr ? nw1 : nw0;
            const uint64_t win = rr ? ((uint64_t)c1 | ((uint64_t)c2 << 32)) : ((uint64_t)c0 | ((uint64_t)c1 << 32));
#pragma unroll
            for (uint32_t j = 0; j < 2; ++j) {
                const uint32_t piece = (two >> (16 * j)) & 0xFFFFu;
                bool found = false;
                for (uint32_t sh = 0; sh <= 2 * k; ++sh) // displacement sh - k
                    found = found || (((uint32_t)(win >> (2 * (8 * j + sh))) & 0xFFFFu) == piece);
                missing += found ? 0u : 1u;
            }
        }
    }
    if (missing > k)
        return 0;
    done += todo;
    if (done >= n_rounds)
        return 2;
    rng = (rng & ~((0x7Fu << kPieceRoundsShift) | (7u << kPieceMissingShift))) | (done << kPieceRoundsShift) |
          (missing << kPieceMissingShift);
    return 1;
}

// The 64 text symbols around a survivor's key window, [t - 16, t + 48), 2 bits each: every entry of the key is checked
// against them in registers ("does the REST of the seed match too?") instead of with loads per entry -- 73 % of the
// (survivor, entry) pairs of a repeat-rich text die here.
struct text64
{
    uint64_t lo, hi; // symbols 0..31, 32..63
    bool ok;         // false: the window is not wholly inside the haystack (no signature check then)
};

__device__ __forceinline__ uint32_t syms16(const text64 &W, uint32_t first) // 16 symbols from index `first` (<= 48)
{
    if (first >= 32)
        return (uint32_t)(W.hi >> (2 * (first - 32)));
    return (uint32_t)(W.lo >> (2 * first)) | (first ? (uint32_t)(W.hi << (2 * (32 - first)) ) : 0u);
}

// the first n (<= 16) symbols of the seed's rest -- the (up to 16) symbols right before the key window, r of them if the
// window starts r < 16 symbols into its seed, then those after it -- against the text
__device__ __forceinline__ bool seed_sig_ok(const text64 &W, uint32_t sig, uint32_t r, uint32_t n, uint32_t H)
{
    if (n == 0)
        return true;
    const uint32_t rb = r < 16 ? r : 16; // symbols of the seed before the window that the signature starts with
    const uint32_t nl = rb < n ? rb : n; // ... of which it holds the first nl: text [t - rb, t - rb + nl)
    uint32_t got = nl ? syms16(W, 16 - rb) : 0u;
    if (nl < 16) {
        got &= (1u << (2 * nl)) - 1;
        got |= syms16(W, 16 + H) << (2 * nl);
    }
    const uint32_t mask = n >= 16 ? 0xFFFFFFFFu : ((1u << (2 * n)) - 1);
    return ((got ^ sig) & mask) == 0;
}

// Work waits in LDS until a wave has 64 items of a kind: a key shared by twenty needles, a pair that needs all its
// piece rounds, a seed hit that counts into four bands would otherwise keep one lane busy while 63 idle -- and the band
// table's atomics, whose round trips to HBM are the longest latency in this kernel, would be issued a few lanes at a time.
constexpr uint32_t kPairCap = 128;
struct pair_queue // per wave: (survivor, entry) pairs on their way through the checks
{
    uint32_t t_lo[kPairCap], t_hi[kPairCap], val[kPairCap], rng[kPairCap], seg[kPairCap];
};
struct band_queue // per wave: (band key, diagonals hit) on their way into the band table
{
    uint32_t key_lo[kPairCap], key_hi[kPairCap], run_lo[kPairCap], run_hi[kPairCap];
    uint32_t elect[128]; // insert_bands: which lane of the batch speaks for a band
};

struct band_chunk // this wave's chunk of the band list (wave-uniform registers)
{
    uint64_t base;
    uint32_t used, size, draws;
};
// The first draws of a wave take exactly what it needs, so a scan with few bands (the usual case; and the long-needle
// sets whose wave-per-band verification wants every wave busy) leaves a dense list; later draws take growing chunks.
constexpr uint32_t kDenseDraws = 4;

// n (<= 64) queued band hits, one per lane: into the band table; the first arrival of a band appends it to the list
__device__ __forceinline__ void insert_bands(const resolve_params &R, band_queue &B, uint32_t first, uint32_t n,
                                             uint32_t lane, band_chunk &C)
{
    bool act = lane < n;
    unsigned long long bkey = 0, run = 0;
    if (act)
        bkey = ((unsigned long long)B.key_hi[first + lane] << 32) | B.key_lo[first + lane];
    // Hits of the same band inside the batch (the sampled windows of one needle in one repeat stretch) go to the table
    // as ONE: every lane names itself in a small LDS table under its band's hash, whoever is left standing there speaks
    // for the lanes with the same band, which OR their diagonals into its queue entry.  (Worth 2 % on a text with many
    // needles inside repeats; the table's compare-and-swap round trips are the longest waits of this kernel.)
    if (!R.overlap) {
        const uint32_t h = (uint32_t)mix64(bkey) & 127u;
        if (act)
            B.elect[h] = lane;
        queue_sync();
        const uint32_t w = act ? B.elect[h] : lane;
        const unsigned long long wkey = ((unsigned long long)B.key_hi[first + w] << 32) | B.key_lo[first + w];
        const bool follower = act && w != lane && wkey == bkey;
        if (follower) {
            atomicOr(&B.run_lo[first + w], B.run_lo[first + lane]);
            atomicOr(&B.run_hi[first + w], B.run_hi[first + lane]);
            act = false;
        }
        queue_sync();
    }
    if (act)
        run = ((unsigned long long)B.run_hi[first + lane] << 32) | B.run_lo[first + lane];
    bool claimed = false;
    uint32_t s2 = (uint32_t)mix64(bkey) & R.table_mask;
    if (act) {
        bool placed = false;
        for (uint32_t tries = 0; tries < 8192 && !placed; ++tries) {
            // (a table that has overflowed is lost -- the host repeats the scan with a larger one: do not walk a full table
            // 8192 slots per band, which cost 5 s on a text with 5 % repeats whose first attempt was sized for 1 %)
            if ((tries & 31u) == 31u && __hip_atomic_load(&R.counters[kCntVoid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
                break;
            const unsigned long long o = atomicCAS(&R.band_tab[s2].x, kBandEmpty, bkey);
            if (o == kBandEmpty) {
                claimed = true;
                placed = true;
            } else if (o == bkey) {
                placed = true;
            } else {
                s2 = (s2 + 1) & R.table_mask;
            }
        }
        if (!placed) {
            atomicAdd(&R.counters[kCntVoid], 1ull); // table full: the host starts over with more room
            *R.table_poison = 1u;
        }
        else if (R.overlap)
            atomicAdd(&R.band_tab[s2].y, 1ull);
        else
            atomicAnd(&R.band_tab[s2].y, ~run);
    }
    const uint64_t mm = __ballot(claimed);
    if (mm == 0)
        return;
    const uint32_t nn = __popcll(mm);
    if (C.used + nn > C.size) { // close this chunk (unused tail invalid), draw the next
        for (uint32_t q = C.used + lane; q < C.size; q += 64)
            if (C.base + q < R.band_cap)
                R.bands[C.base + q].val = kBandInvalid;
        uint32_t next = chunk_grow(C.size, nn);
        if (C.draws < kDenseDraws) {
            next = nn;
            ++C.draws;
        }
        unsigned long long b = 0;
        if (lane == 0)
            b = atomicAdd(&R.counters[kCntBandSlots], (unsigned long long)next);
        C.base = uniform_u64(b);
        C.used = 0;
        C.size = next;
    }
    if (claimed) {
        const uint64_t idx = C.base + C.used + __popcll(mm & ((1ull << lane) - 1));
        if (idx < R.band_cap) {
            band_rec br;
            br.slot = s2;
            br.val = (uint32_t)(bkey >> 43) << 11;
            br.seg = (uint32_t)((bkey & ((1ull << 43) - 1)) >> R.band_bits);
            br.band = (uint32_t)(bkey & ((1ull << R.band_bits) - 1));
            R.bands[idx] = br;
        } else {
            atomicAdd(&R.counters[kCntVoid], 1ull); // band list full: the slot this lane claimed is never given back
            *R.table_poison = 1u;
        }
    }
    C.used += nn;
}

struct resolve_wave // what a wave of resolve_kernel carries (wave-uniform)
{
    pair_queue *Q;
    band_queue *B;
    uint32_t qn, bn;
    band_chunk C;
    uint32_t n_cand;
};

// n (<= 64) pairs from the top of the queue, one per lane: one visit of the checks; pairs with rounds to go return to the
// queue, pairs that are through become band hits
__device__ __forceinline__ void check_pairs(const resolve_params &R, resolve_wave &S, uint32_t n, uint32_t lane)
{
    pair_queue &Q = *S.Q;
    band_queue &B = *S.B;
    S.qn -= n;
    const uint32_t first = S.qn;
    bool live = lane < n;
    uint64_t t = 0, seg = 0;
    uint32_t val = 0, rng = 0;
    int64_t sb = (int64_t)R.hay_begin, se = (int64_t)R.hay_end;
    if (live) {
        const uint32_t i = first + lane;
        t = ((uint64_t)Q.t_hi[i] << 32) | Q.t_lo[i];
        val = Q.val[i];
        rng = Q.rng[i];
        seg = Q.seg[i];
        if (R.seg_offsets) {
            sb = (int64_t)R.seg_offsets[seg];
            se = (int64_t)R.seg_offsets[seg + 1];
        }
    }
    queue_sync(); // (every lane holds its pair before anything is written back)
    bool through = live;
    const uint32_t pat = val >> 11;
    if (live && !(rng & kRngRun)) {
        if (!(rng & kSeedChecked)) {
            live = seed_intact(R, t, val, (rng >> 16) & 0x1F, (rng & kRngWhole) ? R.key_len + ((rng >> 5) & 0x1F) : 0u, sb, se);
            rng |= kSeedChecked;
        }
        through = live;
        if (live && R.pieces_check) {
            const uint32_t m = (uint32_t)R.m[pat], k = (uint32_t)R.k[pat];
            if (pieces_apply(R, t, val, m, k, sb, se)) {
                const uint32_t v = pieces_visit(R, t, val, rng, m, k);
                live = v != 0;
                through = v == 2;
            }
        }
    }
    // back into the queue: alive, not through
    {
        const bool back = live && !through;
        const uint64_t mm = __ballot(back);
        if (back) {
            const uint32_t q = S.qn + __popcll(mm & ((1ull << lane) - 1));
            Q.t_lo[q] = (uint32_t)t;
            Q.t_hi[q] = (uint32_t)(t >> 32);
            Q.val[q] = val;
            Q.rng[q] = rng;
            Q.seg[q] = (uint32_t)seg;
        }
        S.qn += __popcll(mm);
    }
    // bands this pair counts into: those holding a diagonal of [d_lo, d_hi]; with overlapping bands also the one
    // before, if d_lo still lies in its k-wide extension
    int64_t b_cur = 0, b_last = -1, d_lo = 0, d_hi = 0;
    if (R.exact_hits) { // (wave-uniform; such sets have no merged run entries)
        bool fresh = false;
        int64_t e = 0;
        if (live && through) {
            ++S.n_cand;
            e = (int64_t)t - (int64_t)(val & 0x7FF) + (int64_t)R.m[pat]; // exclusive end of the occurrence
            int64_t own_b = (int64_t)R.scan_begin, own_e = (int64_t)R.scan_end;
            if (R.seg_offsets) {
                own_b = R.seg_owned ? sb + (int64_t)R.seg_owned[seg] : sb;
                own_e = se;
            }
            // (R.seen == nullptr: every occurrence has exactly one sampled window and one entry, so nothing is reported
            // twice -- unless spans give up and the brute-force kernel re-scans them: then the host runs the scan again
            // with the dedupe set)
            fresh = e >= own_b + 1 && e <= own_e && (!R.seen || seen_insert_raw(R.seen, R.seen_mask, R.overflow, pat, e));
        }
        const unsigned long long idx = wave_reserve_hits(R.hit_counter, fresh ? 1u : 0u);
        if (fresh && idx < R.hit_cap) {
            spm_hit h;
            h.pos = (R.report_begin ? (uint64_t)(e - (int64_t)R.m[pat]) : (uint64_t)e) + R.pos_offset;
            h.pattern = pat;
            h.score = 0;
            R.hits[idx] = h;
        }
        queue_sync();
        return;
    }
    if (live && through) {
        ++S.n_cand;
        d_hi = (int64_t)t - (int64_t)(val & 0x7FF) - sb + (int64_t)R.max_m;
        d_lo = d_hi - (int64_t)((rng & kRngRun) ? (rng & 0x7FF) : 0u);
        b_cur = d_lo / (int64_t)R.Bw;
        b_last = d_hi / (int64_t)R.Bw;
        if (R.overlap && b_cur > 0 && d_lo - b_cur * (int64_t)R.Bw <= (int64_t)R.k[pat])
            --b_cur;
        if ((uint64_t)b_last >> R.band_bits) {
            atomicAdd(&R.counters[kCntVoid], 1ull); // a haystack too long for the key layout: the host falls back
            b_last = b_cur - 1;
        }
    }
    for (;;) {
        const bool have = b_cur <= b_last;
        const uint64_t mm = __ballot(have);
        if (mm == 0)
            break;
        if (have) {
            const unsigned long long bkey =
                ((unsigned long long)pat << 43) | ((unsigned long long)seg << R.band_bits) | (unsigned long long)b_cur;
            // which diagonals of the band (Bw <= 64) are hit: the verification covers just those
            const int64_t b0 = b_cur * (int64_t)R.Bw;
            const uint32_t o_lo = (uint32_t)(d_lo > b0 ? d_lo - b0 : 0);
            const uint32_t o_hi = (uint32_t)(d_hi < b0 + (int64_t)R.Bw - 1 ? d_hi - b0 : (int64_t)R.Bw - 1);
            const unsigned long long run = (o_hi - o_lo >= 63 ? ~0ull : ((1ull << (o_hi - o_lo + 1)) - 1)) << o_lo;
            const uint32_t q = S.bn + __popcll(mm & ((1ull << lane) - 1));
            B.key_lo[q] = (uint32_t)bkey;
            B.key_hi[q] = (uint32_t)(bkey >> 32);
            B.run_lo[q] = (uint32_t)run;
            B.run_hi[q] = (uint32_t)(run >> 32);
        }
        S.bn += __popcll(mm);
        queue_sync();
        if (S.bn >= 64) {
            S.bn -= 64;
            insert_bands(R, B, S.bn, 64, lane, S.C);
            queue_sync();
        }
        ++b_cur;
    }
    queue_sync();
}

__global__ __launch_bounds__(256) void resolve_kernel(const resolve_params R)
{
    __shared__ pair_queue pair_queues[4];
    __shared__ band_queue band_queues[4];
    unsigned long long n = R.counters[kCntSurvSlots];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&R.counters[kCntUnreadSurvSum], n);
        atomicMax(&R.counters[kCntUnreadSurvMax], n);
    }
    if (n > R.surv_cap)
        n = R.surv_cap;
    if (!R.exact_hits && __hip_atomic_load(R.table_poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        // an earlier scan left slots in the band table and the host has not emptied it yet: this scan is void
        if (blockIdx.x == 0 && threadIdx.x == 0)
            atomicAdd(&R.counters[kCntVoid], 1ull);
        return;
    }
    const uint32_t lane = threadIdx.x & 63;
    resolve_wave S;
    S.Q = &pair_queues[threadIdx.x >> 6];
    S.B = &band_queues[threadIdx.x >> 6];
    S.qn = 0;
    S.bn = 0;
    S.C.base = 0;
    S.C.used = 0;
    S.C.size = 0;
    S.C.draws = 0;
    S.n_cand = 0;
    pair_queue &Q = *S.Q;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride; // wave-uniform trip count: the queue and the appends are wave-collective
    for (uint64_t r = 0; r < rounds; ++r) {
        // a list or table of this attempt has overflowed: its results are void (the host starts over), stop feeding it
        if ((r & 7u) == 7u &&
            __builtin_amdgcn_readfirstlane((uint32_t)(__hip_atomic_load(&R.counters[kCntVoid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)))
            break;
        const uint64_t i = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool probing = false;
        uint32_t key = 0;
        uint64_t t = 0, seg = 0;
        pass_entry T = R.passes[0];
        if (i < n) {
            const survivor sv = R.surv[i];
            if (sv.t_hi != kSurvInvalid) {
                probing = true;
                key = sv.key;
                t = ((uint64_t)sv.t_hi << 32) | sv.t_lo;
                if (sv.pad != 0)
                    T = R.passes[sv.pad];
            }
        }
        if (probing && R.seg_offsets) {
            uint64_t lo = 0, hi = R.n_segments; // invariant: seg_offsets[lo] <= t < seg_offsets[hi]
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (R.seg_offsets[mid] <= t)
                    lo = mid;
                else
                    hi = mid;
            }
            seg = lo;
            if ((int64_t)t + (int64_t)R.key_len > (int64_t)R.seg_offsets[lo + 1])
                probing = false; // the key window straddles two haystacks
        }
        // the text around the key window, once per survivor
        text64 W;
        W.lo = 0;
        W.hi = 0;
        W.ok = false;
        if (probing && R.flank_check) { // (dna4 sets: 2-bit codes)
            int64_t sb = (int64_t)R.hay_begin, se = (int64_t)R.hay_end;
            if (R.seg_offsets) {
                sb = (int64_t)R.seg_offsets[seg];
                se = (int64_t)R.seg_offsets[seg + 1];
            }
            if ((int64_t)t - 16 >= sb && (int64_t)t + 48 <= se && t + 48 <= R.text_alloc) {
                const uint8_t *p = R.text + (t - 16);
                W.lo = (uint64_t)pack16(load_bytes16(p)) | ((uint64_t)pack16(load_bytes16(p + 16)) << 32);
                W.hi = (uint64_t)pack16(load_bytes16(p + 32)) | ((uint64_t)pack16(load_bytes16(p + 48)) << 32);
                W.ok = true;
            }
        }
        // the key's entries: one short directory probe per survivor ...
        uint32_t first = 0, cnt = 0;
        {
            uint32_t slot = ht_hash(key) & T.ht_mask;
            while (__ballot(probing) != 0) {
                if (probing) {
                    const uint4 d = T.ht[slot];
                    if (d.z == 0) {
                        probing = false; // (a level-1 false positive: no such key)
                    } else if (d.x == key) {
                        first = d.y;
                        cnt = d.z;
                        probing = false;
                    } else {
                        slot = (slot + 1) & T.ht_mask;
                    }
                }
            }
        }
        // ... then the (survivor, entry) pairs of the whole wave are dealt to its lanes, 64 at a time: pair i belongs to the
        // lane whose inclusive prefix sum of `cnt` is the first one above i
        uint32_t incl = cnt; // (flat: through wave_prefix_incl the branch behind it comes out inverted)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= (uint32_t)o)
                incl += up;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)incl, 63));
        for (uint32_t p0 = 0; p0 < total; p0 += 64) {
            const uint32_t i = p0 + lane;
            bool have = i < total;
            uint32_t owner = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const uint32_t v = (uint32_t)__shfl((int)incl, (int)(owner + step - 1));
                if (v <= i)
                    owner += step;
            }
            owner = owner > 63 ? 63 : owner;
            const uint32_t o_incl = (uint32_t)__shfl((int)incl, (int)owner), o_cnt = (uint32_t)__shfl((int)cnt, (int)owner);
            const uint32_t o_first = (uint32_t)__shfl((int)first, (int)owner);
            const uint64_t o_t = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(t >> 32), (int)owner) << 32) |
                                 (uint32_t)__shfl((int)(uint32_t)t, (int)owner);
            const uint32_t o_seg = (uint32_t)__shfl((int)(uint32_t)seg, (int)owner);
            text64 OW;
            OW.lo = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(W.lo >> 32), (int)owner) << 32) |
                    (uint32_t)__shfl((int)(uint32_t)W.lo, (int)owner);
            OW.hi = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(W.hi >> 32), (int)owner) << 32) |
                    (uint32_t)__shfl((int)(uint32_t)W.hi, (int)owner);
            OW.ok = __shfl((int)W.ok, (int)owner) != 0;
            uint32_t val = 0, rng = 0;
            if (have) {
                const uint4 e = R.entries[o_first + (i - (o_incl - o_cnt))];
                val = e.x;
                rng = e.z;
                if (!(rng & kRngRun)) {
                    const uint32_t r0 = rng & 0x1F, ns = (rng >> 5) & 0x1F;
                    const bool whole = (rng & kRngWhole) != 0;
                    // (queued with the pair: where the key window sits in its seed, and the seed's length if the entry knows it)
                    rng = (r0 << 16) | (whole ? (ns << 5) | kRngWhole : 0u);
                    if (OW.ok) { // does the rest of the seed match?  (registers only)
                        if (!seed_sig_ok(OW, e.y, r0, ns, R.key_len))
                            have = false;
                        else if (whole)
                            rng |= kSeedChecked;
                    }
                }
            }
            // queue the pairs that are left; 64 waiting pairs are resolved at once
            const uint64_t mm = __ballot(have);
            if (mm != 0) {
                if (have) {
                    const uint32_t q = S.qn + __popcll(mm & ((1ull << lane) - 1));
                    Q.t_lo[q] = (uint32_t)o_t;
                    Q.t_hi[q] = (uint32_t)(o_t >> 32);
                    Q.val[q] = val;
                    Q.rng[q] = rng;
                    Q.seg[q] = o_seg;
                }
                S.qn += __popcll(mm);
                queue_sync();
                while (S.qn >= 64)
                    check_pairs(R, S, 64, lane);
            }
        }
    }
    while (S.qn != 0)
        check_pairs(R, S, S.qn < 64 ? S.qn : 64, lane);
    if (S.bn != 0)
        insert_bands(R, *S.B, 0, S.bn, lane, S.C);
    for (uint32_t q = S.C.used + lane; q < S.C.size; q += 64)
        if (S.C.base + q < R.band_cap)
            R.bands[S.C.base + q].val = kBandInvalid;
    wave_count_add(R.counters + kCntPairs, S.n_cand);
}

} // namespace spm_hip
