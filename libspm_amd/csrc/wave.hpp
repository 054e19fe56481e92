// wave.hpp -- what the 64 lanes of a wave settle among themselves before one of them goes to memory, written once for the
// kernels of the result chain (select.hpp, jst_select.hpp, jst_locate.hpp, transcript_slots.hpp and the stages behind it,
// jst_reads.hpp, jst_pairs.hpp, jst_sam.hpp, jst_bam.hpp) and of the seed filter (filter_resolve.hpp, filter_verify.hpp).
// gfx950.  Shuffles and one ballot: no LDS, no barrier.  All 64 lanes call every function here.
//   count_flagged   one atomicAdd per wave for the lanes that raise a flag
//   wave_count_add  one atomicAdd per wave for the sum of the lanes' counts
//   wave_prefix_incl   the inclusive prefix sum over the lanes
//   wave_reserve    one atomicAdd per wave for the output slots its lanes ask for (the fan-outs of jst_fanout.hpp)
//   wave_reserve_hits   the same for the seed filter's hit list
//   wave_run_scan   segmented inclusive scan over runs of equal id: the last lane of a run holds the run's combined value
//   run_min, run_sum   the values the callers carry through it, alone or as the members of a struct of their own (scalar
//                   members only: an array member sends the scan through scratch memory)
//   wave_max, wave_sum   the maximum and the sum of the wave, in every lane
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp" // uniform_u64

namespace spm_hip
{

// one atomicAdd per wave: the lanes of it that raise `flag`
__device__ __forceinline__ void count_flagged(unsigned long long *counter, bool flag)
{
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(counter, (unsigned long long)__popcll(m));
}

// the inclusive prefix sum of v over the lanes: lane l holds v of lanes 0..l
__device__ __forceinline__ uint32_t wave_prefix_incl(uint32_t v)
{
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, o);
        if (lane >= (uint32_t)o)
            v += up;
    }
    return v;
}

// One atomicAdd per wave for slots in an output array: every lane asks for n of them (0: none) and receives the number of its
// first, the lanes' slots in lane order -- the exclusive prefix of n over the lanes on top of what the counter held.
// (its prefix stays flat: through wave_prefix_incl the fan-out kernels of jst_fanout.hpp are scheduled differently)
__device__ __forceinline__ unsigned long long wave_reserve(unsigned long long *counter, uint32_t n)
{
    const uint32_t lane = threadIdx.x & 63;
    uint32_t incl = n;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if ((int)lane >= o)
            incl += up;
    }
    const uint32_t total = __shfl(incl, 63);
    unsigned long long base = 0;
    if (lane == 0 && total)
        base = atomicAdd(counter, (unsigned long long)total);
    return __shfl(base, 0) + (incl - n);
}

// Reserve hit slots for a whole wave with ONE atomic: lane l gets `mine` consecutive slots starting at the returned index.
// (One atomic per end-position slot and wave, as the brute-force kernels do it, serialises on the counter's address at
// ~100/us: a repeat-rich text reports millions of hits.)  Call with the wave converged.
// The seed filter's wave_reserve (filter_resolve.hpp, filter_verify.hpp): it skips the broadcast when no lane asks and takes
// the base through a scalar register.  (With wave_reserve's body in its place resolve_kernel takes one VGPR more and the four
// verify_wave kernels come out different, so the two stay apart.)
__device__ __forceinline__ unsigned long long wave_reserve_hits(unsigned long long *counter, uint32_t mine)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t incl = wave_prefix_incl(mine);
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    unsigned long long base = 0;
    if (total != 0) {
        if (lane == 0)
            base = atomicAdd(counter, (unsigned long long)total);
        base = uniform_u64(base);
    }
    return base + (incl - mine);
}

// one atomic per wave: add the lanes' counts to a statistics counter (call with the wave converged)
template <class T> __device__ __forceinline__ void wave_count_add(unsigned long long *counter, T v)
{
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(counter, (unsigned long long)v);
}

// Lanes of one id are contiguous.  Inclusive segmented scan over the wave: the last lane of every run of equal `id` (the
// return value: the wave's last lane, or the next lane's id differs) holds the run's combined value in v.  A value says how
// it travels and how it takes in what stands to its left:
//   V up(int d) const                 the value d lanes below
//   void join(const V &left, bool take)   combine with `left` if `take` -- a select, not a branch: every step of the scan
//                                     stays straight-line code
template <class Id, class V> __device__ __forceinline__ bool wave_run_scan(Id id, V &v)
{
    const uint32_t lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const V left = v.up(d);
        const Id id2 = __shfl_up(id, d);
        v.join(left, lane >= (uint32_t)d && id2 == id);
    }
    const Id id_next = __shfl_down(id, 1);
    return lane == 63 || id_next != id;
}

template <class T> struct run_min
{
    T v;
    __device__ __forceinline__ run_min up(int d) const { return run_min{__shfl_up(v, d)}; }
    __device__ __forceinline__ void join(const run_min &l, bool take) { v = take && l.v < v ? l.v : v; }
};

template <class T> struct run_sum
{
    T v;
    __device__ __forceinline__ run_sum up(int d) const { return run_sum{__shfl_up(v, d)}; }
    __device__ __forceinline__ void join(const run_sum &l, bool take) { v += take ? l.v : T(0); }
};

template <class T> __device__ __forceinline__ T wave_max(T v)
{
    for (int d = 32; d; d >>= 1) {
        const T v2 = __shfl_xor(v, d);
        v = v2 > v ? v2 : v;
    }
    return v;
}

template <class T> __device__ __forceinline__ T wave_sum(T v)
{
    for (int d = 32; d; d >>= 1)
        v += __shfl_xor(v, d);
    return v;
}

} // namespace spm_hip
