// wave.hpp -- what the 64 lanes of a wave settle among themselves before one of them goes to memory, written once for the
// kernels of the result chain (select.hpp, jst_select.hpp, jst_locate.hpp, transcript_slots.hpp and the stages behind it,
// jst_reads.hpp, jst_pairs.hpp).  gfx950.  Shuffles and one ballot: no LDS, no barrier.  All 64 lanes call every function here.
//   count_flagged   one atomicAdd per wave for the lanes that raise a flag
//   wave_reserve    one atomicAdd per wave for the output slots its lanes ask for (the fan-outs of jst_fanout.hpp)
//   wave_run_scan   segmented inclusive scan over runs of equal id: the last lane of a run holds the run's combined value
//   run_min, run_sum   the values the callers carry through it, alone or as the members of a struct of their own (scalar
//                   members only: an array member sends the scan through scratch memory)
//   wave_max        the maximum of the wave, in every lane
#pragma once

#include <hip/hip_runtime.h>

namespace spm_hip
{

// one atomicAdd per wave: the lanes of it that raise `flag`
__device__ __forceinline__ void count_flagged(unsigned long long *counter, bool flag)
{
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(counter, (unsigned long long)__popcll(m));
}

// One atomicAdd per wave for slots in an output array: every lane asks for n of them (0: none) and receives the number of its
// first, the lanes' slots in lane order -- the exclusive prefix of n over the lanes on top of what the counter held.
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

} // namespace spm_hip
