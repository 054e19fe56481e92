// filter_stream.hpp -- level 1 of the seed filter (filter.hpp): the survivor chunks of a wave, the window look-ups, the
// skeleton of a streaming pass, and the two kernels that stream sparse passes -- seed_filter_kernel over the 1-byte text,
// seed_filter_packed_kernel over the 2-bit shadow.  (The dense pass builds on the same skeleton: filter_dense.hpp.)
#pragma once

#include "brute.hpp" // alignbit
#include "filter_params.hpp"
#include "pack.hpp"

namespace spm_hip
{

// this wave's chunk record in LDS
__device__ __forceinline__ uint32_t *cand_chunk_of(const filter_params &P, const uint32_t *lds)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return const_cast<uint32_t *>(lds) + P.lds_words + kCandLdsSlot + kCandRec * wave;
}

// A wave starts a span: fresh budget (wave-uniform call).
__device__ __forceinline__ void span_open(const filter_params &P, const uint32_t *lds, uint32_t lane, uint64_t begin)
{
    if (lane == 0) {
        uint32_t *ck = cand_chunk_of(P, lds);
        ck[4] = 0;
        ck[5] = 0;
        ck[6] = (uint32_t)begin;
        ck[7] = (uint32_t)(begin >> 32);
    }
}

// the current span gives up (wave-uniform call)
__device__ __forceinline__ void span_give_up(const filter_params &P, uint32_t *ck, uint32_t lane)
{
    if (lane == 0) {
        ck[5] = 1;
        const unsigned long long i = atomicAdd(&P.counters[kCntSpansGaveUp], 1ull);
        if (i < P.ovf_cap) {
            P.ovf_spans[2 * i] = ((uint64_t)ck[7] << 32) | ck[6];
            P.ovf_spans[2 * i + 1] = (uint64_t)P.span_chunks * (uint64_t)P.span_unit;
        } else {
            atomicAdd(&P.counters[kCntVoid], 1ull); // no room to remember it: the host re-runs the whole scan
        }
    }
    queue_sync();
}

// mark the unused tail of a wave's chunk invalid (wave-uniform call)
__device__ __forceinline__ void surv_close(const filter_params &P, const uint32_t *ck, uint32_t lane)
{
    const uint32_t used = ck[2], size = ck[3];
    const uint64_t base = ((uint64_t)ck[1] << 32) | ck[0];
    for (uint32_t i = used + lane; i < size; i += 64)
        if (base + i < P.surv_cap) {
            survivor sv;
            sv.key = 0;
            sv.t_lo = 0;
            sv.t_hi = kSurvInvalid;
            sv.pad = 0;
            P.surv[base + i] = sv;
        }
}

// Record the survivors of one wave step (wave-uniform call; `has` marks the lanes that hold one).
__device__ __forceinline__ void emit_survivors(const filter_params &P, bool has, uint32_t key, uint64_t t, uint32_t lane,
                                               const uint32_t *lds)
{
    const uint64_t m = __ballot(has);
    if (m == 0)
        return;
    uint32_t *ck = cand_chunk_of(P, lds);
    const uint32_t n = __popcll(m);
    uint32_t used = (uint32_t)__builtin_amdgcn_readfirstlane(ck[2]);
    const uint32_t size = (uint32_t)__builtin_amdgcn_readfirstlane(ck[3]);
    const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane(ck[4]) + n;
    if (cnt > P.span_budget) {
        span_give_up(P, ck, lane);
        return;
    }
    if (used + n > size) { // close this chunk, draw the next (twice as large, up to kChunkMax)
        surv_close(P, ck, lane);
        const uint32_t next = chunk_grow(size, n);
        if (lane == 0) {
            const unsigned long long b = atomicAdd(&P.counters[kCntSurvSlots], (unsigned long long)next);
            ck[0] = (uint32_t)b;
            ck[1] = (uint32_t)(b >> 32);
            ck[2] = 0;
            ck[3] = next;
        }
        used = 0;
        queue_sync();
    }
    const uint64_t cbase = uniform_u64(((uint64_t)ck[1] << 32) | ck[0]);
    if (cbase + used + n > P.surv_cap) { // the survivor buffer is full
        span_give_up(P, ck, lane);
        return;
    }
    if (has) {
        survivor sv;
        sv.key = key;
        sv.t_lo = (uint32_t)t;
        sv.t_hi = (uint32_t)(t >> 32);
        sv.pad = P.pass;
        P.surv[cbase + used + __popcll(m & ((1ull << lane) - 1))] = sv;
    }
    if (lane == 0) {
        ck[2] = used + n;
        ck[4] = cnt;
    }
    queue_sync();
}

// Level 1 + level 2 on NWD 2-bit-packed words per lane (w[j] = 16 bases, prev[j] = the 16 bases before them).
// PK selects how word j maps to a text position (1-byte text vs. packed shadow).
// KM: keys shorter than 16 symbols (masked); only strides 1 and 2 ever carry such keys.
template <int S, int NWD, int HV, int SIG, bool PK, bool KM>
__device__ __forceinline__ void filter_words(const filter_params &P, const uint32_t (&w)[NWD],
                                             const uint32_t (&prev)[NWD], const uint32_t (&nv)[SIG != 4 ? NWD : 1],
                                             uint64_t gbase, uint32_t lane, const uint32_t *lds, uint32_t idx_mask)
{
    constexpr int NWIN = 16 / S; // windows per word
    const uint32_t kmask = KM ? P.key_mask : 0xFFFFFFFFu;
    static_assert(NWD * NWIN <= 32, "one mask bit per window of a group");
    // windows d = S, 2S, .., 16 of chunk u: text start t = L_u - 16 + d, key = bits [2d, 2d+32) of (w:prev)
    uint32_t pos_mask = 0;
    if constexpr (HV == 2) {
        // perfect-hash fingerprints: round 1 reads the displacement of every window's bucket, round 2 the
        // fingerprint at the displaced slot -- two LDS round trips per group, all windows in flight together
        const uint16_t *fp_tab = reinterpret_cast<const uint16_t *>(lds);
        const uint16_t *disp_tab = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(lds) + P.chd_disp_off);
        uint32_t xs[NWD * NWIN], ds[NWD * NWIN];
#pragma unroll
        for (int u = 0; u < NWD; ++u) {
#pragma unroll
            for (int i = 0; i < NWIN; ++i) {
                const int d = S * (i + 1);
                const uint32_t key = (d == 16 ? w[u] : alignbit(w[u], prev[u], (2 * d) & 31)) & kmask;
                const uint32_t x = chd_hash(key).x;
                xs[u * NWIN + i] = x;
                ds[u * NWIN + i] = disp_tab[x >> P.chd_bucket_shift];
            }
        }
#pragma unroll
        for (int u = 0; u < NWD; ++u) {
#pragma unroll
            for (int i = 0; i < NWIN; ++i) {
                const int d = S * (i + 1);
                const uint32_t key = (d == 16 ? w[u] : alignbit(w[u], prev[u], (2 * d) & 31)) & kmask;
                const uint32_t slot = ((xs[u * NWIN + i] >> 3) + ds[u * NWIN + i] * ((key | 1u) & 0xFFFFFFu)) &
                                      P.chd_slot_mask;
                ds[u * NWIN + i] = fp_tab[slot];
            }
        }
#pragma unroll
        for (int u = 0; u < NWD; ++u) {
#pragma unroll
            for (int i = 0; i < NWIN; ++i) {
                const int d = S * (i + 1);
                const uint32_t key = (d == 16 ? w[u] : alignbit(w[u], prev[u], (2 * d) & 31)) & kmask;
                const uint32_t miss = (ds[u * NWIN + i] ^ key ^ (key >> 16)) & 0xFFFFu;
                pos_mask |= (miss == 0 ? 1u : 0u) << (u * NWIN + i);
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < NWD; ++u) {
#pragma unroll
            for (int i = 0; i < NWIN; ++i) {
                const int d = S * (i + 1);
                const uint32_t key = (d == 16 ? w[u] : alignbit(w[u], prev[u], (2 * d) & 31)) & kmask;
                const uint32_t h = bloom_hash(key, 0) & idx_mask;
                const uint32_t word = lds[h >> 5];
                pos_mask |= __builtin_amdgcn_ubfe(word, h, 1) << (u * NWIN + i);
            }
        }
        // cascade: further probes only for survivors
        for (uint32_t pr = 1; pr < P.n_probes; ++pr) {
            if (__ballot(pos_mask != 0) == 0)
                break;
            uint32_t keep = 0;
#pragma unroll
            for (int u = 0; u < NWD; ++u) {
#pragma unroll
                for (int i = 0; i < NWIN; ++i) {
                    if (pos_mask & (1u << (u * NWIN + i))) {
                        const int d = S * (i + 1);
                        const uint32_t key = (d == 16 ? w[u] : alignbit(w[u], prev[u], (2 * d) & 31)) & kmask;
                        const uint32_t h = bloom_hash(key, pr) & idx_mask;
                        const uint32_t word = lds[h >> 5];
                        keep |= __builtin_amdgcn_ubfe(word, h, 1) << (u * NWIN + i);
                    }
                }
            }
            pos_mask = keep;
        }
    }
    if constexpr (SIG != 4) {
        if (__ballot(pos_mask != 0) != 0) {
#pragma unroll
            for (int u = 0; u < NWD; ++u) {
#pragma unroll
                for (int i = 0; i < NWIN; ++i) {
                    const int d = S * (i + 1);
                    if (__builtin_amdgcn_ubfe(nv[u], d, P.key_len) != 0) // an N inside the window
                        pos_mask &= ~(1u << (u * NWIN + i));
                }
            }
        }
    }
    // survivors: recorded for resolve_kernel (one per wave step and lane until every lane's mask is empty)
    while (__ballot(pos_mask != 0) != 0) {
        if (__builtin_amdgcn_readfirstlane(cand_chunk_of(P, lds)[5]) != 0)
            break; // the span has given up
        uint64_t t = 0;
        uint32_t key = 0;
        bool has = false;
        if (pos_mask != 0) {
            const int bit = __ffs(pos_mask) - 1;
            pos_mask &= pos_mask - 1;
            const int u = bit / NWIN, i = bit % NWIN;
            const int d = S * (i + 1);
            uint32_t wu = w[0], pu = prev[0];
#pragma unroll
            for (int q = 1; q < NWD; ++q)
                if (u == q) {
                    wu = w[q];
                    pu = prev[q];
                }
            key = (d == 16 ? wu : alignbit(wu, pu, (uint32_t)(2 * d) & 31u)) & kmask;
            // first base of word u of this lane: 1-byte text = chunk u, 16 bytes per lane; packed shadow = load u>>2
            // (4096 bases), 64 bases per lane, word u&3
            const uint64_t wpos = PK ? gbase + (uint64_t)(u >> 2) * 4096 + (uint64_t)lane * 64 + (uint64_t)(u & 3) * 16
                                     : gbase + (uint64_t)u * 1024 + (uint64_t)lane * 16;
            const int64_t ts = (int64_t)wpos - 16 + d;
            if (ts >= (int64_t)P.lo && (uint64_t)ts + P.key_len <= P.hi) {
                t = (uint64_t)ts;
                has = true;
            }
        }
        emit_survivors(P, has, key, t, lane, lds);
    }
}


// ---- anchored passes (stride 1, needle sets of several passes) ------------------------------------------------------
// The keys of the pass all begin with its anchor dimer (the host chose each seed's key window that way; a few passes
// carry a pattern with a don't-care bit, i.e. two dimers), so only the text windows that begin with it -- 1 in 16 -- can
// equal a key.  Which of a lane's 16 windows those are is computed bit-parallel on the packed word (9 VALU for 16
// windows); the hash and the two LDS reads then run for the selected windows only, in a per-lane loop.  The unanchored
// stride-1 kernel spends 14 VALU and two conflict-ridden LDS reads on EVERY window and saturates both the VALU and the
// LDS.

// bit 2 (d - 1) set: window d (1..16) of this word -- it starts at symbol d of (prev, w) -- begins with the anchor
__device__ __forceinline__ uint32_t anchor_select(uint32_t w, uint32_t prev, uint32_t c, uint32_t cm)
{
    // (wave-uniform) the pattern's bits for the first and the second symbol, repeated for every symbol of a word
    const uint32_t C0 = (c & 3u) * 0x55555555u, M0 = (cm & 3u) * 0x55555555u;
    const uint32_t C1 = (c >> 2) * 0x55555555u, M1 = (cm >> 2) * 0x55555555u;
    const uint32_t X = alignbit(w, prev, 2); // symbols 1..16: where the windows start
    const uint32_t Y = alignbit(w, prev, 4); // symbols 2..17: their second symbols
    uint32_t t = ((X ^ C0) & M0) | ((Y ^ C1) & M1); // a set bit: that bit of that symbol differs from the pattern
    t |= t >> 1;
    return ~t & 0x55555555u;
}

template <int NWD>
__device__ __forceinline__ void filter_words_anchored(const filter_params &P, const uint32_t (&w)[NWD], const uint32_t (&prev)[NWD],
                                                      uint64_t gbase, uint32_t lane, const uint32_t *lds)
{
    static_assert(NWD % 2 == 0 || NWD == 1, "words are taken in pairs");
    const uint16_t *fp_tab = reinterpret_cast<const uint16_t *>(lds);
    const uint16_t *disp_tab = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(lds) + P.chd_disp_off);
#pragma unroll
    for (int j = 0; j < NWD; j += 2) {
        // the selected windows of two words in one mask: bit b = word j + (b & 1), window (b >> 1) + 1
        uint32_t todo = anchor_select(w[j], prev[j], P.anchor_c, P.anchor_cm);
        if (j + 1 < NWD)
            todo |= anchor_select(w[j + 1 < NWD ? j + 1 : j], prev[j + 1 < NWD ? j + 1 : j], P.anchor_c, P.anchor_cm) << 1;
        while (__ballot(todo != 0) != 0) {
            const bool act = todo != 0;
            const uint32_t b = act ? (uint32_t)__ffs(todo) - 1u : 0u;
            todo &= todo - 1;
            const uint32_t u = b & 1u, d = (b >> 1) + 1u;
            const uint32_t wu = (j + 1 < NWD && u) ? w[j + 1 < NWD ? j + 1 : j] : w[j];
            const uint32_t pu = (j + 1 < NWD && u) ? prev[j + 1 < NWD ? j + 1 : j] : prev[j];
            const uint32_t key = (uint32_t)((((uint64_t)wu << 32) | pu) >> (2 * d));
            const uint32_t x = chd_hash(key).x;
            const uint32_t dsp = disp_tab[x >> P.chd_bucket_shift];
            const uint32_t slot = ((x >> 3) + dsp * ((key | 1u) & 0xFFFFFFu)) & P.chd_slot_mask;
            const uint32_t f = fp_tab[slot];
            const bool hit = act && ((f ^ key ^ (key >> 16)) & 0xFFFFu) == 0;
            if (__ballot(hit) != 0) { // rare: a survivor for resolve_kernel
                if (__builtin_amdgcn_readfirstlane(cand_chunk_of(P, lds)[5]) != 0)
                    return; // the span has given up
                const uint64_t wpos = gbase + (uint64_t)(j + u) * 1024 + (uint64_t)lane * 16;
                const int64_t ts = (int64_t)wpos - 16 + (int64_t)d;
                const bool has = hit && ts >= (int64_t)P.lo && (uint64_t)ts + P.key_len <= P.hi;
                emit_survivors(P, has, key, has ? (uint64_t)ts : 0, lane, lds);
            }
        }
    }
}

// ---- the skeleton of a streaming pass: what seed_filter_kernel, seed_filter_dense_kernel and seed_filter_packed_kernel
// share (stage, draw a span, its chunks, the word in front of it, every word's predecessor) ----

// Prologue: stage the level-1 table in LDS (once per workgroup; the grid is persistent) and clear the waves' chunk records.
__device__ __forceinline__ void stream_stage(const filter_params &P, uint32_t *lds)
{
    for (uint32_t i = threadIdx.x; i < P.lds_words; i += blockDim.x)
        lds[i] = P.bitmap[i];
    if ((threadIdx.x & 63) == 0) { // this wave's candidate chunk: none drawn yet
        uint32_t *ck = lds + P.lds_words + kCandLdsSlot + kCandRec * (threadIdx.x >> 6);
        for (uint32_t i = 0; i < kCandRec; ++i)
            ck[i] = 0; // size 0: the first survivor draws a chunk; no span open yet
    }
    __syncthreads();
}

enum class span_draw
{
    run,  // `sp` is this wave's next span
    idle, // the workgroup's last round has no span for this wave: draw again, to keep meeting the barriers
    done, // the queue is empty
};

// Spans are drawn from a queue, counters[kCntSpanHead] (evens out the tail; a static round-robin measured 15-20 % slower
// on 16 GiB and is gone):
//   dynamic == 1: every wave draws its next span with one returning atomic;
//   dynamic == 2: one atomic per WORKGROUP hands one span to each of its waves (waves_per_wg times fewer
//                 atomics at the same granularity; a single head saturates near 88 dequeues/us, which a 1 GiB
//                 text with 16 KiB spans would exceed).  Sharding the head per XCD group was slower (no
//                 balancing across shards).
// Every wave of the workgroup calls it in step (dynamic == 2 meets two workgroup barriers); `done` is then uniform over
// the workgroup.
__device__ __forceinline__ span_draw draw_span(const filter_params &P, uint32_t *lds, uint32_t lane, uint32_t wave_in_wg,
                                               uint32_t waves_per_wg, uint64_t n_spans, uint64_t &sp)
{
    if (P.dynamic == 1) {
        unsigned long long t = 0;
        if (lane == 0)
            t = atomicAdd(&P.counters[kCntSpanHead], 1ull);
        sp = uniform_u64(t);
        return sp >= n_spans ? span_draw::done : span_draw::run;
    }
    __syncthreads(); // every wave has read the previous base
    if (threadIdx.x == 0) {
        const unsigned long long t = atomicAdd(&P.counters[kCntSpanHead], (unsigned long long)waves_per_wg);
        lds[P.lds_words] = (uint32_t)t;
        lds[P.lds_words + 1] = (uint32_t)(t >> 32);
    }
    __syncthreads();
    const uint64_t base = uniform_u64(((uint64_t)lds[P.lds_words + 1] << 32) | lds[P.lds_words]);
    if (base >= n_spans)
        return span_draw::done; // uniform over the workgroup
    sp = base + wave_in_wg;
    return sp >= n_spans ? span_draw::idle : span_draw::run;
}

// The word in front of a span that begins at text index span_base of the 1-byte text (the word of the lane "before lane
// 0": the last 16 bytes of the previous chunk), and its N mask; wave-uniform.
template <int SIG>
__device__ __forceinline__ uint32_t span_carry_in(const filter_params &P, uint64_t span_base, uint32_t lane, uint32_t &carry_n)
{
    uint32_t carry_in = 0;
    carry_n = 0;
    if (span_base >= 16 && lane == 0) {
        const uint4 before = load_text16(P.text, span_base - 16, P.hi);
        carry_in = pack16_sig<SIG>(before, carry_n);
    }
    carry_n = __builtin_amdgcn_readfirstlane(carry_n);
    return __builtin_amdgcn_readfirstlane(carry_in);
}

__device__ __forceinline__ uint32_t span_carry_in(const filter_params &P, uint64_t span_base, uint32_t lane) // dna4: no N mask
{
    uint32_t no_n;
    return span_carry_in<4>(P, span_base, lane, no_n);
}

// dna4: pack this lane's 16 text bytes into w and give it its predecessor -- the previous lane's word through DPP, lane 0
// takes the carry; the carry becomes lane 63's word.  (dna5 / dna15 keep the sequence, interleaved with its twin on the N
// masks, flat in filter_group: shared, the compiler schedules their packing differently.)
__device__ __forceinline__ void pack_with_prev(const uint4 &cur, uint32_t lane, uint32_t &carry_in, uint32_t &w, uint32_t &prev)
{
    w = pack16(cur);
    prev = __builtin_amdgcn_update_dpp(0u, w, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
    if (lane == 0)
        prev = carry_in;
    carry_in = __builtin_amdgcn_readlane(w, 63);
}

// One group of UU consecutive 1-KiB chunks, already in registers.  chunk u of the group starts at text index
// gbase + 1024*u; this lane holds its bytes [16*lane, 16*lane+16).
template <int S, int UU, int HV, int SIG, bool KM, bool AN = false>
__device__ __forceinline__ void filter_group(const filter_params &P, const uint4 (&cur)[UU], uint64_t gbase,
                                             uint32_t &carry_in, uint32_t &carry_n, uint32_t lane,
                                             const uint32_t *lds, uint32_t idx_mask)
{
    uint32_t w[UU], prev[UU];
    uint32_t nv[SIG != 4 ? UU : 1]; // dna5 / dna15: (this lane's N mask << 16) | previous lane's N mask
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        if constexpr (SIG == 4) {
            pack_with_prev(cur[u], lane, carry_in, w[u], prev[u]);
        } else {
            uint32_t nm = 0;
            w[u] = pack16_sig<SIG>(cur[u], nm);
            prev[u] = __builtin_amdgcn_update_dpp(0u, w[u], 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            if (lane == 0)
                prev[u] = carry_in;
            carry_in = __builtin_amdgcn_readlane(w[u], 63);
            uint32_t np = __builtin_amdgcn_update_dpp(0u, nm, 0x138, 0xF, 0xF, false);
            if (lane == 0)
                np = carry_n;
            carry_n = __builtin_amdgcn_readlane(nm, 63);
            nv[u] = (nm << 16) | np;
        }
    }
    if constexpr (AN)
        filter_words_anchored<UU>(P, w, prev, gbase, lane, lds);
    else
        filter_words<S, UU, HV, SIG, false, KM>(P, w, prev, nv, gbase, lane, lds, idx_mask);
}

// Streaming structure: a wave owns spans of consecutive 1-KiB chunks; per iteration it works on a GROUP of U chunks
// (U KiB contiguous per wave) while the unconditional 16-byte loads of the next group are already in flight, so
// each wave keeps 2*U KiB outstanding.  Only groups that lie fully inside the text take this path; the ragged end
// of the text goes through a guarded one-chunk loop (bytes past the end read as 0).
// 512 threads: 8 waves per CU is the measured best for the HBM-bound 1-byte text, and a bound of 1024 leaves 128 VGPRs,
// which made the masked-key stride-2 variant spill to scratch inside the streaming loop (+31 % kernel time).
// Stride 1 without key masks (C4-sized needle sets: LDS-bound at 16 windows per lane, see DESIGN) fits 128 VGPRs and may run
// 16 waves per CU.
template <int S, int U, int HV, int SIG, bool KM, bool AN = false>
__global__ __launch_bounds__(((S == 1 && !KM && SIG == 4) || (S == 2 && U == 2)) ? 1024 : 512) void seed_filter_kernel(const filter_params P)
{
    extern __shared__ uint32_t lds[];
    stream_stage(P, lds);

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t waves_per_wg = blockDim.x >> 6;
    const uint32_t wave_in_wg = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t idx_mask = P.bitmap_words * 32 - 1;

    const stream_geometry G = stream_geometry_of(P.lo, P.hi, 1024, P.span_chunks);
    const uint64_t span = P.span_chunks; // multiple of U (host guarantees)
    const uint8_t *lane_text = P.text + G.base0 + (uint64_t)lane * 16;

    uint64_t sp;
    for (;;) {
        const span_draw drawn = draw_span(P, lds, lane, wave_in_wg, waves_per_wg, G.n_spans, sp);
        if (drawn == span_draw::done)
            break;
        if (drawn == span_draw::idle)
            continue;
        const uint64_t c_begin = sp * span;
        const uint64_t c_end = c_begin + span < G.n_chunks ? c_begin + span : G.n_chunks;
        span_open(P, lds, lane, G.base0 + c_begin * 1024);
        uint32_t carry_n;
        uint32_t carry_in = span_carry_in<SIG>(P, G.base0 + c_begin * 1024, lane, carry_n);
        // ---- fast path: whole groups ----
        uint64_t ch = c_begin;
        const uint64_t whole_end = c_end < G.n_whole ? c_end : G.n_whole;
        const uint64_t fast_end = c_begin + (whole_end > c_begin ? (whole_end - c_begin) / U * U : 0);
        if (ch < fast_end) {
            uint4 nxt[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                nxt[u] = load16_stream(lane_text + (ch + u) * 1024);
            for (; ch < fast_end; ch += U) {
                uint4 cur[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    cur[u] = nxt[u];
                // prefetch unconditionally (no branch around the loads); past the last group of the span re-read
                // one chunk of the current group -- in bounds, L2-resident, 1/U of a group
                const bool more = ch + U < fast_end;
                const uint64_t pf = more ? ch + U : ch;
                const uint64_t ustride = more ? 1024 : 0;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    nxt[u] = load16_stream(lane_text + pf * 1024 + (uint64_t)u * ustride);
                // strides 1 and 2: keep the loads here -- left alone, the scheduler sinks them to the very end of the
                // group's work and the next iteration waits out the whole HBM latency.  (The larger strides are
                // scheduled well as they are; a barrier there only forces the packing to wait for all eight loads.)
                if constexpr (S <= 2)
                    __builtin_amdgcn_sched_barrier(0);
                filter_group<S, U, HV, SIG, KM, AN>(P, cur, G.base0 + ch * 1024, carry_in, carry_n, lane, lds, idx_mask);
            }
        }
        // ---- ragged end ----
        for (; ch < c_end; ++ch) {
            uint4 one[1];
            // (chunks are 1 KiB aligned: the lane's offset is OR-ed in, which keeps this address apart from lane_text's sum)
            one[0] = load_text16(P.text, (G.base0 + ch * 1024) | ((uint64_t)lane * 16), P.hi);
            filter_group<S, 1, HV, SIG, KM, AN>(P, one, G.base0 + ch * 1024, carry_in, carry_n, lane, lds, idx_mask);
        }
    }
    surv_close(P, cand_chunk_of(P, lds), lane);
}

// Same filter, fed from the shadow: one 16-byte load per lane = 4 words = 64 symbols; a wave-load ("p-chunk") covers
// 4096 symbols.  U2 p-chunks per group, the next group's loads in flight.  The shadow is zero-padded to whole
// p-chunks, so every load is unconditional; windows reaching past the text are dropped by the range check.
template <int S, int U2, int HV, bool KM>
__global__ __launch_bounds__(1024) void seed_filter_packed_kernel(const filter_params P, const uint4 *__restrict__ shadow)
{
    extern __shared__ uint32_t lds[];
    stream_stage(P, lds);

    constexpr int NWD = 4 * U2;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t waves_per_wg = blockDim.x >> 6;
    const uint32_t wave_in_wg = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t idx_mask = P.bitmap_words * 32 - 1;

    const stream_geometry G = stream_geometry_of(P.lo, P.hi, 4096, P.span_chunks); // p-chunks
    const uint64_t span = P.span_chunks;                    // multiple of U2
    const uint4 *lane_src = shadow + (G.base0 / 64) + lane; // one uint4 = 64 symbols

    uint64_t sp;
    for (;;) {
        const span_draw drawn = draw_span(P, lds, lane, wave_in_wg, waves_per_wg, G.n_spans, sp);
        if (drawn == span_draw::done)
            break;
        if (drawn == span_draw::idle)
            continue;
        const uint64_t c_begin = sp * span;
        const uint64_t c_end = c_begin + span < G.n_chunks ? c_begin + span : G.n_chunks;
        const uint64_t fast_end = c_begin + (c_end - c_begin + U2 - 1) / U2 * U2; // whole groups (shadow is padded)
        span_open(P, lds, lane, G.base0 + c_begin * 4096);
        // the word in front of this span's first word
        uint32_t carry_in = 0;
        {
            const uint64_t first_word = (G.base0 + c_begin * 4096) / 16;
            if (first_word > 0 && lane == 0)
                carry_in = reinterpret_cast<const uint32_t *>(shadow)[first_word - 1];
            carry_in = __builtin_amdgcn_readfirstlane(carry_in);
        }
        uint4 nxt[U2];
#pragma unroll
        for (int u = 0; u < U2; ++u)
            nxt[u] = load16_stream(reinterpret_cast<const uint8_t *>(lane_src + (c_begin + u) * 64));
        for (uint64_t ch = c_begin; ch < fast_end; ch += U2) {
            uint4 cur[U2];
#pragma unroll
            for (int u = 0; u < U2; ++u)
                cur[u] = nxt[u];
            const bool more = ch + U2 < fast_end;
            const uint64_t pf = more ? ch + U2 : ch;
            const uint64_t ustride = more ? 64 : 0;
#pragma unroll
            for (int u = 0; u < U2; ++u)
                nxt[u] = load16_stream(reinterpret_cast<const uint8_t *>(lane_src + pf * 64 + (uint64_t)u * ustride));
            __builtin_amdgcn_sched_barrier(0); // as in seed_filter_kernel: the prefetch stays ahead of the group's work
            uint32_t w[NWD], prev[NWD];
            const uint32_t nv[1] = {0};
#pragma unroll
            for (int u = 0; u < U2; ++u) {
                w[4 * u + 0] = cur[u].x;
                w[4 * u + 1] = cur[u].y;
                w[4 * u + 2] = cur[u].z;
                w[4 * u + 3] = cur[u].w;
                uint32_t p0 = __builtin_amdgcn_update_dpp(0u, cur[u].w, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
                if (lane == 0)
                    p0 = carry_in;
                carry_in = __builtin_amdgcn_readlane(cur[u].w, 63);
                prev[4 * u + 0] = p0;
                prev[4 * u + 1] = cur[u].x;
                prev[4 * u + 2] = cur[u].y;
                prev[4 * u + 3] = cur[u].z;
            }
            filter_words<S, NWD, HV, 4, true, KM>(P, w, prev, nv, G.base0 + ch * 4096, lane, lds, idx_mask);
        }
    }
    surv_close(P, cand_chunk_of(P, lds), lane);
}

} // namespace spm_hip
