// device_order.hpp -- the host side of "order the records, then compact them", written once for the drivers that do it:
// select.hip, jst_select.hip, jst_locate.hpp, transcript_slots.hpp (the slot stage of jst_project.hpp, jst_normalize.hpp
// and jst_collapse.hpp), those three themselves, jst_reads.hpp and jst_pairs.hpp.  Here are
//   the launch of a one-lane-per-item kernel on the context's stream,
//   the radix sort of (64-bit key, 32-bit index) pairs over the key's low bits: declared here, compiled once in
//   device_order.hip (hipcub's sort is 234 kernels; defined inline here, every unit that included this header compiled them),
//   the running maximum and the exclusive sum over 32-bit values, compiled there too (bam_pileup.hpp),
//   the hipcub exclusive sum over any input iterator,
//   the read-back of a call's counts,
//   the events a call times its stages with,
//   the handle of a result that is records alone (no pool).
// HIP, host code only: the sums are templates, so hipcub instantiates for the callers' own iterator types what a direct call
// would.  Every function returns the first hipError_t that is not hipSuccess, for the caller's SPM_HIP_CHECK.
#pragma once

#include <vector>

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "common.hpp"

namespace spm_hip
{

// ---- kernel(args...) with one lane per item, in workgroups of Block lanes; n_items > 0.  The arguments are converted to
// the kernel's own parameter types, as a direct call would convert them ----
template <unsigned Block = 256, class... Params, class... Args>
hipError_t launch_1d(spm_ctx *ctx, void (*kernel)(Params...), uint64_t n_items, Args &&...args)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_items + Block - 1) / Block)), dim3(Block), 0, ctx->stream,
                       static_cast<Params>(args)...);
    return hipGetLastError();
}

// ---- the sort: keys_in/idx_in -> keys_out/idx_out, stable, by bits [0, key_bits) of the key (device_order.hip) ----
#pragma GCC visibility push(hidden) // calls between the library's own units, not part of its surface
hipError_t sort_pairs_tmp_bytes(spm_ctx *ctx, size_t n, uint32_t key_bits, size_t *tmp_bytes);
hipError_t sort_pairs(spm_ctx *ctx, void *tmp, size_t tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out,
                      const uint32_t *idx_in, uint32_t *idx_out, size_t n, uint32_t key_bits);
// ---- two scans over n 32-bit values, compiled once in device_order.hip: the inclusive running maximum and the exclusive sum;
// in and out may be the same array.  One temporary size serves both ----
hipError_t scan_u32_tmp_bytes(spm_ctx *ctx, size_t n, size_t *tmp_bytes);
hipError_t inclusive_max_u32(spm_ctx *ctx, void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, size_t n);
hipError_t exclusive_sum_u32(spm_ctx *ctx, void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, size_t n);
#pragma GCC visibility pop

// ---- the exclusive sum of n items of `in` into out[0..n) ----
template <class Out, class Iter> hipError_t exclusive_sum_tmp_bytes(spm_ctx *ctx, Iter in, size_t n, size_t *tmp_bytes)
{
    *tmp_bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *tmp_bytes, in, (Out *)nullptr, n, ctx->stream);
}

template <class Iter, class Out> hipError_t exclusive_sum(spm_ctx *ctx, void *tmp, size_t tmp_bytes, Iter in, Out *out, size_t n)
{
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, n, ctx->stream);
}

// f(0), f(1), ... as an input iterator: what the sums above add up
template <class T, class Op> using counted_iter = hipcub::TransformInputIterator<T, Op, hipcub::CountingInputIterator<uint32_t>>;
template <class T, class Op> counted_iter<T, Op> counted(Op op)
{
    return counted_iter<T, Op>(hipcub::CountingInputIterator<uint32_t>(0), op);
}

// ---- the one read-back of a call: n_words counters into ctx->h_counters, and the synchronisation ----
inline hipError_t read_counts(spm_ctx *ctx, const unsigned long long *d_counts, size_t n_words)
{
    const hipError_t e = hipMemcpyAsync(ctx->h_counters, d_counts, n_words * 8, hipMemcpyDeviceToHost, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}

// ---- N events that live as long as the call that times its stages with them ----
template <int N> struct hip_events
{
    hipEvent_t e[N] = {};
    hip_events() = default;
    hip_events(const hip_events &) = delete; // (e is an array of handles this object destroys)
    hip_events &operator=(const hip_events &) = delete;
    ~hip_events()
    {
        for (hipEvent_t x : e)
            if (x)
                hipEventDestroy(x);
    }
    hipError_t create()
    {
        hipError_t r = hipSuccess;
        for (int i = 0; i < N && r == hipSuccess; ++i)
            r = hipEventCreate(&e[i]);
        return r;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
};

// ---- what a "records only" result handle is made of, and what its C accessors answer.  The handle derives from this ----
template <class Rec, class Stats> struct device_records
{
    spm_ctx *ctx = nullptr;
    Rec *d = nullptr; // [n]
    uint64_t n = 0;
    std::vector<Rec> host;
    Stats stats{};

    // h: the deriving handle (or null); work of the context's stream may still read its records
    template <class Handle> static void destroy(Handle *h)
    {
        if (!h)
            return;
        if (h->ctx && h->d)
            hipStreamSynchronize(h->ctx->stream);
        hipFree(h->d);
        delete h;
    }
    int view(const Rec **records, uint64_t *n_out) const { return out<Rec>(host.data(), records, n_out); }
    int device(const void **records, uint64_t *n_out) const { return out<void>(d, records, n_out); }
    int stats_out(Stats *s) const
    {
        if (!s)
            return SPM_E_INVALID;
        *s = stats;
        return SPM_OK;
    }

  private:
    template <class P> int out(const P *from, const P **records, uint64_t *n_out) const
    {
        if (!records || !n_out)
            return SPM_E_INVALID;
        *records = from;
        *n_out = n;
        return SPM_OK;
    }
};

} // namespace spm_hip
