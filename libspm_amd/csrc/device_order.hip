// device_order.hip -- the radix sort of device_order.hpp, instantiated once for the library: (64-bit key, 32-bit index) pairs.
// Every driver that orders records calls these two; no other unit names hipcub's sort.  Beside it the two scans over 32-bit
// values that the pileup takes (bam_pileup.hpp): the running maximum and the exclusive sum.
#include "internal.hpp"
#include "device_order.hpp"

namespace spm_hip
{

hipError_t sort_pairs_tmp_bytes(spm_ctx *ctx, size_t n, uint32_t key_bits, size_t *tmp_bytes)
{
    *tmp_bytes = 0;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, *tmp_bytes, (const unsigned long long *)nullptr,
                                              (unsigned long long *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0,
                                              (int)key_bits, ctx->stream);
}

hipError_t sort_pairs(spm_ctx *ctx, void *tmp, size_t tmp_bytes, const unsigned long long *keys_in,
                      unsigned long long *keys_out, const uint32_t *idx_in, uint32_t *idx_out, size_t n,
                      uint32_t key_bits)
{
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys_in, keys_out, idx_in, idx_out, n, 0, (int)key_bits,
                                              ctx->stream);
}

hipError_t scan_u32_tmp_bytes(spm_ctx *ctx, size_t n, size_t *tmp_bytes)
{
    size_t a = 0, b = 0;
    hipError_t e = hipcub::DeviceScan::InclusiveScan(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, hipcub::Max(), n, ctx->stream);
    if (e == hipSuccess)
        e = hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, n, ctx->stream);
    *tmp_bytes = a > b ? a : b;
    return e;
}

hipError_t inclusive_max_u32(spm_ctx *ctx, void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, size_t n)
{
    return hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, in, out, hipcub::Max(), n, ctx->stream);
}

hipError_t exclusive_sum_u32(spm_ctx *ctx, void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, size_t n)
{
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, n, ctx->stream);
}

} // namespace spm_hip

// hipcub's kernels have no name to ask the runtime about, so the unit's code object is loaded by what loads it in a call: a
// sort, of one pair, in the first bytes of the context's scratch (nothing else is enqueued yet).
void spm_warm_device_order_kernels(spm_ctx *ctx)
{
    size_t tmp_bytes = 0;
    if (!ctx->d_scratch || spm_hip::sort_pairs_tmp_bytes(ctx, 1, 1, &tmp_bytes) != hipSuccess || 64 + tmp_bytes > ctx->scratch_bytes)
        return;
    uint8_t *s = static_cast<uint8_t *>(ctx->d_scratch);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(s);
    uint32_t *idx = reinterpret_cast<uint32_t *>(s + 16);
    (void)spm_hip::sort_pairs(ctx, s + 64, tmp_bytes, keys, keys + 1, idx, idx + 1, 1, 1);
}
