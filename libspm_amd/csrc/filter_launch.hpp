// filter_launch.hpp -- what the seed filter's driver (scan_filter.hip) calls in the units that hold its kernels, one per stage:
// filter_stream.hip, filter_dense.hip, filter_resolve.hip, filter_verify.hip.  Each unit owns its kernels' selection tables and
// launch geometry; the driver owns the buffers, the parameter blocks and the order of the launches.  Host code only.
#pragma once

#include "internal.hpp"
#include "filter_params.hpp"

// raise the kernel's dynamic LDS limit to what this launch asks for, then launch it
template <typename K, typename... Args>
static void launch(K kernel, dim3 grid, uint32_t threads, size_t lds, hipStream_t s, Args... args)
{
    hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, args...);
}

using filter_kernel = void (*)(filter_params);

#pragma GCC visibility push(hidden) // calls between the library's own units, not part of its surface

// ---- filter_stream.hip ----
// One streaming pass of the seed index: P holds what the passes of a scan share; the pass's tables, its launch geometry and
// span plan are set here.  SPM_E_UNSUPPORTED (and the context's message) if no kernel streams such a pass.
int launch_stream_pass(const scan_args &A, filter_params P, uint32_t pass);
void warm_stream_kernels();

// ---- filter_dense.hip ----
// the kernel of a dense pass, or of a sparse pass whose level 1 is the presence table (hash variant 4); nullptr: none
filter_kernel select_dense_kernel(const filter_index &F, bool km);
void warm_dense_kernels();

// ---- filter_resolve.hip ----
// surv_expect: the survivors the scan is expected to leave (sizes the grid; a scan that leaves more simply loops)
void launch_resolve(const resolve_params &R, uint64_t surv_expect, uint32_t n_cu, hipStream_t s);

// ---- filter_verify.hip ----
void launch_band_runs(const verify_params &V, band_rec *bands, band_rec *heads, unsigned long long *head_count, uint32_t n_cu,
                      hipStream_t s);
void launch_band_select(const verify_params &V, band_rec *out, unsigned long long *out_count, uint32_t n_cu, hipStream_t s);
void launch_band_release(const verify_params &V, const band_rec *bands, uint32_t n_cu, hipStream_t s);
// nwn = 32-bit words that can hold needle rows = ceil(max |P| / 32), rounded up to an instantiated width; band_expect: the
// bands the scan is expected to leave (sizes the grid)
void launch_verify(uint32_t nwn, const verify_params &V, uint64_t band_expect, uint32_t n_cu, hipStream_t s);
// long needles: one 32-row block per lane, G = lanes per band >= blocks of the longest needle
void launch_verify_wave(uint32_t n_blocks, const verify_params &V, const uint32_t *peq_bot, uint32_t max_m, uint32_t n_cu,
                        hipStream_t s);
void warm_verify_kernels();

#pragma GCC visibility pop
