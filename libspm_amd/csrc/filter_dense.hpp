// filter_dense.hpp -- the dense pass of the seed filter (filter.hpp), on the skeleton of filter_stream.hpp.
#pragma once

#include "filter_stream.hpp"

namespace spm_hip
{

// ---------------------------------------------------------------------------------------------------
// Dense pass: every key of a needle set of any size in ONE pass over the text (filter_shared.hpp, index_dense.hpp).
//   level 0   which of a lane's 16 windows per word begin with an anchor dimer: bit-parallel on the packed word
//             (dense_select: ~6 VALU per pattern and word); 1/8 .. 3/16 of the windows for the usual sets;
//   level 1   one presence bit per key in LDS (2^20 bits), looked up for the anchored windows in a per-lane loop over the
//             set bits of two words; about a third of them pass with 400 000 keys;
//   level 1b  those wait in a per-wave LDS queue {key, offset in the span} until 64 or more are there; then the wave takes
//             them one per lane, gathers each one's 16-byte fingerprint bucket from L2 (up to kDenseBatches batches in
//             flight together: the chip serves ~2.7e11 such gathers per second, tools/l2_gather_probe.hip, so the queue
//             exists to issue them 64 lanes wide and to keep several round trips overlapping), and compares the 15-bit
//             fingerprint with the bucket's eight slots;
//   what matches is a survivor like those of the sparse passes: recorded for resolve_kernel.
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t kDenseQueueCap = 192; // entries per wave
constexpr int kDenseBatches = 3;

template <int NP>
__device__ __forceinline__ uint32_t dense_select(const filter_params &P, uint32_t w, uint32_t prev)
{
    const uint32_t X = alignbit(w, prev, 2); // symbols 1..16: where the windows start
    const uint32_t Y = alignbit(w, prev, 4); // symbols 2..17: their second symbols
    uint32_t sel = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        // (wave-uniform) the pattern's bits for the first and the second symbol, repeated for every symbol of a word
        const uint32_t C0 = (P.pat_c[i] & 3u) * 0x55555555u, M0 = (P.pat_cm[i] & 3u) * 0x55555555u;
        const uint32_t C1 = (P.pat_c[i] >> 2) * 0x55555555u, M1 = (P.pat_cm[i] >> 2) * 0x55555555u;
        uint32_t t = ((X ^ C0) & M0) | ((Y ^ C1) & M1); // a set bit: that bit of that symbol differs from the pattern
        t |= t >> 1;
        sel |= ~t;
    }
    return sel & 0x55555555u; // bit 2 (d - 1): window d (1..16) of this word begins with an anchor
}

struct dense_queue // per wave, in LDS behind the survivor-chunk records
{
    uint32_t key[kDenseQueueCap];
    uint32_t off[kDenseQueueCap]; // window start - span begin + 16
};
static_assert(sizeof(dense_queue) == kDenseQueueBytes, "filter_params.hpp sizes the launch's LDS");

// Take queued windows through level 1b: full batches of 64 (`all`: the rest too).  Wave-uniform call.
__device__ __forceinline__ void dense_drain(const filter_params &P, dense_queue &Q, uint32_t &qn, bool all, uint64_t span_base,
                                            uint32_t lane, const uint32_t *lds)
{
    while (qn >= 64 || (all && qn != 0)) {
        const uint32_t nb_full = qn >> 6;
        uint32_t nb = all ? (qn + 63) >> 6 : nb_full;
        nb = nb > (uint32_t)kDenseBatches ? (uint32_t)kDenseBatches : nb;
        uint32_t key[kDenseBatches], off[kDenseBatches];
        uint4 bk[kDenseBatches];
        bool v[kDenseBatches];
#pragma unroll
        for (int b = 0; b < kDenseBatches; ++b) { // entries [qn - 64 (b + 1), qn - 64 b), from the top of the queue
            const int32_t e = (int32_t)qn - 64 * b - 1 - (int32_t)lane;
            v[b] = (uint32_t)b < nb && e >= 0;
            key[b] = 0;
            off[b] = 0;
            bk[b] = make_uint4(0, 0, 0, 0);
            if (v[b]) {
                key[b] = Q.key[e];
                off[b] = Q.off[e];
                bk[b] = P.buckets[dense_bucket(key[b], P.bucket_shift)];
            }
        }
        qn = qn > 64 * nb ? qn - 64 * nb : 0;
#pragma unroll
        for (int b = 0; b < kDenseBatches; ++b) {
            if ((uint32_t)b >= nb)
                break; // (wave-uniform)
            const uint32_t f2 = dense_fp(key[b]) * 0x00010001u;
            // a 16-bit slot equal to the fingerprint <=> a zero halfword in slot ^ fingerprint
            const uint32_t x0 = bk[b].x ^ f2, x1 = bk[b].y ^ f2, x2 = bk[b].z ^ f2, x3 = bk[b].w ^ f2;
            const uint32_t z = ((x0 - 0x00010001u) & ~x0) | ((x1 - 0x00010001u) & ~x1) | ((x2 - 0x00010001u) & ~x2) |
                               ((x3 - 0x00010001u) & ~x3);
            const bool hit = v[b] && ((z & 0x80008000u) != 0 || (bk[b].w >> 16) == kDenseAcceptAll);
            if (__ballot(hit) != 0) { // rare: a survivor for resolve_kernel
                if (__builtin_amdgcn_readfirstlane(cand_chunk_of(P, lds)[5]) == 0) { // (unless the span has given up)
                    const int64_t ts = (int64_t)span_base + (int64_t)off[b] - 16;
                    const bool has = hit && ts >= (int64_t)P.lo && (uint64_t)ts + P.key_len <= P.hi;
                    emit_survivors(P, has, key[b], has ? (uint64_t)ts : 0, lane, lds);
                }
            }
        }
    }
}

// S == 0: the anchored windows of a dense pass (NP patterns).  S = 1, 2: EVERY S-th window of a sparse pass whose level 1 is
// the presence table (hash variant 4): the same number for every lane, at fixed places -- unrolled, no search for set bits.
template <int UU, int NP, int S, bool KM>
__device__ __forceinline__ void dense_group(const filter_params &P, const uint4 (&cur)[UU], uint64_t gbase, uint64_t span_base,
                                            uint32_t &carry_in, uint32_t lane, const uint32_t *lds, dense_queue &Q, uint32_t &qn)
{
    static_assert(UU % 2 == 0 || UU == 1, "words are taken in pairs");
    uint32_t w[UU], prev[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u)
        pack_with_prev(cur[u], lane, carry_in, w[u], prev[u]);
    const uint32_t goff = (uint32_t)(gbase - span_base) + lane * 16; // (this lane's first base of chunk 0) - span begin
#pragma unroll
    for (int j = 0; j < UU; j += 2) {
        constexpr bool pair = UU > 1;
        const uint32_t w0 = w[j], p0 = prev[j], w1 = w[pair ? j + 1 : j], p1 = prev[pair ? j + 1 : j];
        const uint32_t kmask = KM ? P.key_mask : 0xFFFFFFFFu;
        static_assert(kDenseBloomBits == 20, "the word address below takes bits 5..19 of the index");
        // pm: bit b = word j + (b & 1), window (b >> 1) + 1 has its presence bit set
        uint32_t pm = 0;
        if constexpr (S == 0) {
            // the anchored windows of two words in one mask
            uint32_t todo = dense_select<NP>(P, w0, p0);
            if (pair)
                todo |= dense_select<NP>(P, w1, p1) << 1;
            // level 1, every lane for itself (a lane runs as long as it has anchored windows -- no wave-wide steps in
            // here, the loop is what this kernel spends its time in): which of them have their presence bit set
            while (todo != 0) {
                const uint32_t b = (uint32_t)__ffs(todo) - 1u;
                todo &= todo - 1;
                const bool odd = (b & 1u) != 0;
                const uint64_t both = ((uint64_t)(odd ? w1 : w0) << 32) | (odd ? p1 : p0);
                const uint32_t key = (uint32_t)(both >> ((b & ~1u) + 2u)); // window d = (b >> 1) + 1 starts 2 d bits in
                const uint32_t h = key ^ (key >> 13); // dense_bloom_index(key) = h & (2^20 - 1): word h >> 5, bit h & 31
                const uint32_t word = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(lds) + ((h >> 3) & 0x1FFFCu));
                pm |= __builtin_amdgcn_ubfe(word, h, 1) << b;
            }
        } else {
#pragma unroll
            for (int u = 0; u < (pair ? 2 : 1); ++u) {
#pragma unroll
                for (int d = S; d <= 16; d += S) {
                    const uint32_t wu = u ? w1 : w0, pu = u ? p1 : p0;
                    const uint32_t key = (d == 16 ? wu : alignbit(wu, pu, (2 * d) & 31)) & kmask;
                    const uint32_t h = key ^ (key >> 13);
                    const uint32_t word = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(lds) + ((h >> 3) & 0x1FFFCu));
                    pm |= __builtin_amdgcn_ubfe(word, h, 1) << (2 * (d - 1) + u);
                }
            }
        }
        // level 1b: those that do wait in the queue until the wave has a batch of them (wave-wide steps from here on)
        while (__ballot(pm != 0) != 0) {
            const bool pos = pm != 0;
            const uint32_t b = pos ? (uint32_t)__ffs(pm) - 1u : 0u;
            pm &= pm - 1;
            const bool odd = (b & 1u) != 0;
            const uint64_t both = ((uint64_t)(odd ? w1 : w0) << 32) | (odd ? p1 : p0);
            const uint32_t key = (uint32_t)(both >> ((b & ~1u) + 2u)) & kmask;
            const uint64_t mm = __ballot(pos);
            if (pos) {
                const uint32_t q = qn + __popcll(mm & ((1ull << lane) - 1));
                Q.key[q] = key;
                Q.off[q] = goff + (uint32_t)j * 1024u + (odd ? 1024u : 0u) + (b >> 1) + 1u; // = window start - span begin + 16
            }
            qn += __popcll(mm);
            queue_sync();
            if (qn > kDenseQueueCap - 64)
                dense_drain(P, Q, qn, false, span_base, lane, lds);
        }
    }
}

template <int U, int NP, int S = 0, bool KM = false>
__global__ __launch_bounds__(1024) void seed_filter_dense_kernel(const filter_params P)
{
    extern __shared__ uint32_t lds[];
    stream_stage(P, lds);

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t waves_per_wg = blockDim.x >> 6;
    const uint32_t wave_in_wg = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    dense_queue &Q = *reinterpret_cast<dense_queue *>(lds + P.lds_words + kCandLdsSlot + kCandRec * 16 +
                                                      (sizeof(dense_queue) / 4) * wave_in_wg);
    uint32_t qn = 0;

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
        const uint64_t span_base = G.base0 + c_begin * 1024;
        span_open(P, lds, lane, span_base);
        uint32_t carry_in = span_carry_in(P, span_base, lane);
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
                const bool more = ch + U < fast_end;
                const uint64_t pf = more ? ch + U : ch;
                const uint64_t ustride = more ? 1024 : 0;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    nxt[u] = load16_stream(lane_text + pf * 1024 + (uint64_t)u * ustride);
                __builtin_amdgcn_sched_barrier(0); // the prefetch stays ahead of the group's work
                dense_group<U, NP, S, KM>(P, cur, G.base0 + ch * 1024, span_base, carry_in, lane, lds, Q, qn);
            }
        }
        for (; ch < c_end; ++ch) { // ragged end
            uint4 one[1];
            one[0] = load_text16(P.text, G.base0 + ch * 1024 + (uint64_t)lane * 16, P.hi);
            dense_group<1, NP, S, KM>(P, one, G.base0 + ch * 1024, span_base, carry_in, lane, lds, Q, qn);
        }
        dense_drain(P, Q, qn, true, span_base, lane, lds); // (offsets in the queue are relative to this span)
    }
    surv_close(P, cand_chunk_of(P, lds), lane);
}

} // namespace spm_hip
