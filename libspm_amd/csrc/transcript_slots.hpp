// transcript_slots.hpp -- the distinct transcript slots of a "records + CIGAR pool" object, numbered in pool order.  gfx950.
// Unit: jst_ref.hip, where jst_project.hpp, jst_normalize.hpp and jst_collapse.hpp include it: all three begin with this
// stage, and the collapse is right only if it numbers the slots of the projection's records the way the projection numbered
// its own, so the stage is written once and its two kernels that are no templates are compiled once.
//   slot_rep_kernel      one lane per record: atomicMin of the record index into rep[cigar_off] -- the smallest record index
//                        represents its slot; a record its caller's predicate calls unusable is counted, not entered
//   (hipcub exclusive sum of rep[w] != none over the pool: the number of every slot, in pool order)
//   slot_compact_kernel  one lane per pool word: slot number -> representative record; the last lane writes the slot count
// and on the host: the temp bytes the sum needs, the stage enqueued in that order, and the downloaded numbering for the loop
// that sends the records of a host view to their slots.  The sum and the launches are device_order.hpp's, the count of the
// flagged lanes is wave.hpp's.
// Also what the callers would otherwise each write again: slot_count (the clamp every later kernel runs under),
// ref_aln_unusable (the collapse's and the normalisation's test of a projected record), slot_total_kernel (the words of all
// slots, for the projection and the normalisation).
#pragma once

#include <vector>

#include "device_order.hpp"
#include "wave.hpp"

namespace spm_hip
{

constexpr uint32_t kSlotNone = 0xFFFFFFFFu;
enum { kSlotCntSlots = 0, kSlotCntBad = 1 }; // the first two counters of every caller

// The tables of the stage.  The callers' kernel parameter blocks hold the same fields (their kernels read them too) and
// hand them out as one of these: slots().
struct slot_tables
{
    uint32_t *rep;              // [n_ops] smallest record index whose transcript starts at this word, or none
    uint32_t *sid;              // [n_ops] exclusive sum of rep != none: the slot's number
    uint32_t *slot_rec;         // [cap] representative record of slot s
    uint64_t n_ops;             // words of the source's pool
    uint32_t cap;               // slots the per-slot tables hold: min(records, n_ops)
    unsigned long long *counts; // the caller's counters; kSlotCnt* are this stage's
};

// the slots the stage counted, as far as the per-slot tables hold them: what every later kernel of a caller runs over
__device__ __forceinline__ uint32_t slot_count(const unsigned long long *counts, uint32_t cap)
{
    return (uint32_t)min(counts[kSlotCntSlots], (unsigned long long)cap);
}

// What makes a projected record (the collapse's and the normalisation's input) unusable: tested before any of its fields
// indexes a table.  Limits: ref_aln_limits, or a kernel's parameter block, which holds the same three fields.
struct ref_aln_limits
{
    uint64_t n_ops;      // words of the source's pool
    uint32_t n_patterns; // needles of the set
    uint64_t n_ref;      // symbols of the reference
};

template <class Limits> __device__ __forceinline__ bool ref_aln_unusable(const Limits &P, const spm_jst_ref_aln &a)
{
    return a.cigar_len == 0 || (uint64_t)a.cigar_off + a.cigar_len > P.n_ops || a.pattern >= P.n_patterns ||
           a.ref_begin > a.ref_end || a.ref_end > P.n_ref;
}

struct ref_aln_unusable_op // the predicate as the slot stage takes it
{
    ref_aln_limits lim;
    __device__ __forceinline__ bool operator()(const spm_jst_ref_aln &a) const { return ref_aln_unusable(lim, a); }
};

// unusable(record): true if the record must not index a table -- tested before any of its fields does
template <class Rec, class Unusable>
__global__ __launch_bounds__(256) void slot_rep_kernel(const Rec *recs, uint32_t n, const slot_tables T, const Unusable unusable)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const Rec a = recs[i];
        bad = unusable(a);
        if (!bad)
            atomicMin(&T.rep[a.cigar_off], (uint32_t)i);
    }
    count_flagged(&T.counts[kSlotCntBad], bad);
}

__global__ __launch_bounds__(256) void slot_compact_kernel(const slot_tables T)
{
    const unsigned long long w = blockIdx.x * 256ull + threadIdx.x;
    if (w >= T.n_ops)
        return;
    const uint32_t r = T.rep[w];
    const uint32_t s = T.sid[w];
    if (r != kSlotNone && s < T.cap)
        T.slot_rec[s] = r;
    if (w == T.n_ops - 1)
        T.counts[kSlotCntSlots] = (unsigned long long)s + (r != kSlotNone ? 1ull : 0ull);
}

// one lane: the words of all slots -- slot_off is the exclusive sum of slot_words -- into the caller's counter `words`
__global__ void slot_total_kernel(unsigned long long *counts, uint32_t cap, const unsigned long long *slot_off,
                                  const uint32_t *slot_words, uint32_t words)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t n_slots = slot_count(counts, cap);
        counts[words] = n_slots ? slot_off[n_slots - 1] + slot_words[n_slots - 1] : 0ull;
    }
}

// what the exclusive sums of the callers add up: "this word starts a slot", a table of bytes, a table of words widened
struct slot_flag_op
{
    const uint32_t *rep;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return rep[w] != kSlotNone ? 1u : 0u; }
};

struct byte_op
{
    const uint8_t *v;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return v[i]; }
};

struct widen_op
{
    const uint32_t *v;
    __device__ __forceinline__ unsigned long long operator()(uint32_t i) const { return v[i]; }
};

inline hipError_t slot_stage_tmp_bytes(spm_ctx *ctx, uint64_t n_ops, size_t *tmp_bytes)
{
    return exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(slot_flag_op{nullptr}), n_ops, tmp_bytes);
}

// the stage on the context's stream.  T.counts is zero already; n > 0 and T.n_ops > 0.
template <class Rec, class Unusable>
hipError_t slot_stage_enqueue(spm_ctx *ctx, const Rec *recs, uint32_t n, const slot_tables &T, Unusable unusable, void *tmp,
                              size_t tmp_bytes)
{
    hipError_t e = hipMemsetAsync(T.rep, 0xFF, T.n_ops * 4, ctx->stream);
    if (e != hipSuccess)
        return e;
    if ((e = launch_1d(ctx, slot_rep_kernel<Rec, Unusable>, n, recs, n, T, unusable)) != hipSuccess)
        return e;
    if ((e = exclusive_sum(ctx, tmp, tmp_bytes, counted<uint32_t>(slot_flag_op{T.rep}), T.sid, T.n_ops)) != hipSuccess)
        return e;
    return launch_1d(ctx, slot_compact_kernel, T.n_ops, T);
}

// the numbering on the host: download() enqueues the copy (the caller synchronises), of() answers for one record
struct slot_host_map
{
    std::vector<uint32_t> sid;
    explicit slot_host_map(uint64_t n_ops) : sid(n_ops) {}
    hipError_t download(spm_ctx *ctx, const slot_tables &T)
    {
        return hipMemcpyAsync(sid.data(), T.sid, sid.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
    }
    uint32_t of(uint32_t cigar_off) const { return cigar_off < sid.size() ? sid[cigar_off] : kSlotNone; }
};

} // namespace spm_hip
