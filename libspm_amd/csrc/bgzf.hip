// bgzf.hip -- BGZF framing behind the C ABI: spm_hip_bgzf_frame over a device buffer that no handle owns (bgzf.hpp has the
// kernel), its view / device / stats / destroy, and the two host-only calls over the serial framer of bgzf_core.hpp,
// spm_hip_bgzf_frame_host and spm_hip_bgzf_framed_size.
#include "internal.hpp"
#include "bgzf.hpp"

// the frame stage on the context's stream: n bytes at d_src into d_dst, which has room for bgzf_framed_size bytes
hipError_t bgzf_frame_enqueue(spm_ctx *ctx, const void *d_src, uint64_t n, uint32_t D, bool eof, void *d_dst)
{
    bgzf_params P;
    P.src = static_cast<const uint8_t *>(d_src);
    P.dst = static_cast<uint8_t *>(d_dst);
    P.n = n;
    P.n_blocks = bgzf_n_blocks(n, D);
    P.D = D;
    P.L = bgzf_plan_lanes(D);
    const uint64_t grid = P.n_blocks + (eof ? 1 : 0);
    if (!grid)
        return hipSuccess;
    hipLaunchKernelGGL(bgzf_frame_kernel, dim3((unsigned)grid), dim3(kBgzfLanes), 0, ctx->stream, P);
    return hipGetLastError();
}

extern "C" void spm_hip_bgzf_destroy(spm_bgzf *z)
{
    if (!z)
        return;
    if (z->ctx && z->d)
        hipStreamSynchronize(z->ctx->stream);
    hipFree(z->d);
    delete z;
}

extern "C" int spm_hip_bgzf_framed_size(uint64_t n, const spm_bgzf_opts *opts, uint64_t *len)
{
    static const char *const who = "spm_hip_bgzf_framed_size";
    if (!opts || !len) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL %s", who, !opts ? "opts" : "len");
        return SPM_E_INVALID;
    }
    const char *why = nullptr;
    if (bgzf_check_opts(*opts, why) != SPM_OK) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %s (block_data %u, flags 0x%x, reserved %llu)", who, why, opts->block_data, opts->flags,
                    (unsigned long long)opts->reserved);
        return SPM_E_INVALID;
    }
    const uint32_t D = bgzf_block_data(opts->block_data);
    if (bgzf_size_overflows(n, D)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %llu bytes in blocks of %u do not fit 64 bits once framed (not supported)", who,
                    (unsigned long long)n, D);
        return SPM_E_UNSUPPORTED;
    }
    *len = bgzf_framed_size(n, D, (opts->flags & SPM_BGZF_EOF) != 0);
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_frame_host(const void *src, uint64_t n, const spm_bgzf_opts *opts, void *dst, uint64_t cap, uint64_t *len)
{
    static const char *const who = "spm_hip_bgzf_frame_host";
    if ((!src && n) || !len || (!dst && cap)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL %s", who, !len ? "len" : !src ? "src with n > 0" : "dst with cap > 0");
        return SPM_E_INVALID;
    }
    uint64_t need = 0;
    SPM_TRY(spm_hip_bgzf_framed_size(n, opts, &need));
    *len = need;
    if (need > cap)
        return SPM_E_OVERFLOW;
    bgzf_frame_serial(static_cast<const uint8_t *>(src), n, bgzf_block_data(opts->block_data), (opts->flags & SPM_BGZF_EOF) != 0,
                      static_cast<uint8_t *>(dst));
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_frame(spm_ctx *ctx, const void *device_src, uint64_t n, const spm_bgzf_opts *opts, spm_bgzf **out)
{
    static const char *const who = "spm_hip_bgzf_frame";
    if (out)
        *out = nullptr;
    if (!ctx || !opts || !out) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !ctx ? "ctx" : !opts ? "opts" : "out");
        return SPM_E_INVALID;
    }
    const auto t_call = clk::now();
    if (!device_src && n) {
        SPM_SET_ERR(ctx, "%s: NULL device_src with n = %llu", who, (unsigned long long)n);
        return SPM_E_INVALID;
    }
    const char *why = nullptr;
    if (bgzf_check_opts(*opts, why) != SPM_OK) {
        SPM_SET_ERR(ctx, "%s: %s (block_data %u, flags 0x%x, reserved %llu)", who, why, opts->block_data, opts->flags,
                    (unsigned long long)opts->reserved);
        return SPM_E_INVALID;
    }
    const uint32_t D = bgzf_block_data(opts->block_data);
    const bool eof = (opts->flags & SPM_BGZF_EOF) != 0;
    const uint64_t n_blocks = bgzf_n_blocks(n, D);
    if (n_blocks > kBgzfMaxBlocks) {
        SPM_SET_ERR(ctx, "%s: %llu bytes in blocks of %u are more than 2^31 - 2 blocks (not supported)", who, (unsigned long long)n, D);
        return SPM_E_UNSUPPORTED;
    }
    std::unique_ptr<spm_bgzf, void (*)(spm_bgzf *)> Z(new spm_bgzf, spm_hip_bgzf_destroy);
    Z->ctx = ctx;
    Z->n = bgzf_framed_size(n, D, eof);
    Z->stats.n_in = n;
    Z->stats.n_out = Z->n;
    Z->stats.n_blocks = n_blocks;
    if (Z->n) {
        SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        hip_events<2> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        SPM_HIP_CHECK(ctx, hipMalloc(&Z->d, Z->n));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], ctx->stream));
        SPM_HIP_CHECK(ctx, bgzf_frame_enqueue(ctx, device_src, n, D, eof, Z->d));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], ctx->stream));
        SPM_HIP_CHECK(ctx, hipEventSynchronize(ev[1])); // (the source is the caller's again when the call returns)
        hipEventElapsedTime(&Z->stats.ms_frame, ev[0], ev[1]);
    }
    Z->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] bgzf frame: %llu bytes -> %llu blocks of %u%s, %llu bytes: device %.3f ms, %.3f ms in all\n",
                (unsigned long long)n, (unsigned long long)n_blocks, D, eof ? " + EOF" : "", (unsigned long long)Z->n, Z->stats.ms_frame,
                Z->stats.ms_host);
    *out = Z.release();
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_view(spm_bgzf *z, const void **bytes, uint64_t *n)
{
    if (!z)
        return SPM_E_INVALID;
    if (!z->have_host && z->n) {
        spm_ctx *ctx = z->ctx;
        SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        z->host.resize(z->n);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(z->host.data(), z->d, z->n, hipMemcpyDeviceToHost, ctx->stream));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    z->have_host = true;
    if (bytes)
        *bytes = z->host.data();
    if (n)
        *n = z->n;
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_device(spm_bgzf *z, const void **bytes, uint64_t *n)
{
    if (!z)
        return SPM_E_INVALID;
    if (bytes)
        *bytes = z->d;
    if (n)
        *n = z->n;
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_stats(const spm_bgzf *z, spm_bgzf_stats *out)
{
    if (!z || !out)
        return SPM_E_INVALID;
    *out = z->stats;
    return SPM_OK;
}

void spm_warm_bgzf_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)bgzf_frame_kernel);
}
