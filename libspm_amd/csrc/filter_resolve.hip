// filter_resolve.hip -- resolve_kernel of the seed filter (filter_resolve.hpp) and its launch.
#include "filter_launch.hpp"
#include "filter_resolve.hpp"

void launch_resolve(const resolve_params &R, uint64_t surv_expect, uint32_t n_cu, hipStream_t s)
{
    // (5 workgroups per CU are resident at once -- LDS queues, 84 VGPRs --: a larger grid only adds a second, partly filled
    // round.  A lane takes ~4 survivors in turn: measured on C5, whose survivors are few and cheap, 0.137 -> 0.10 ms;
    // c3r 1.33 -> 1.25 ms with the cap alone.)
    const uint64_t rmax = (uint64_t)n_cu * 5;
    // (a short survivor list: one survivor per lane, its latency is the kernel's; a long one: four per lane)
    const uint64_t per_wg = (surv_expect + 255) / 256 <= rmax ? 256 : 1024;
    const uint32_t rgrid = (uint32_t)std::min<uint64_t>(rmax, std::max<uint64_t>(n_cu / 2, (surv_expect + per_wg - 1) / per_wg));
    hipLaunchKernelGGL(resolve_kernel, dim3(rgrid), dim3(256), 0, s, R);
}

// (the code objects of the filter's other units are loaded with this one's)
void spm_warm_filter_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)resolve_kernel);
    warm_stream_kernels();
    warm_dense_kernels();
    warm_verify_kernels();
}
