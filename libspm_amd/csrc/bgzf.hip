// bgzf.hip -- BGZF framing behind the C ABI: spm_hip_bgzf_frame over a device buffer that no handle owns (bgzf.hpp has the
// kernel), its view / device / stats / destroy, and the two host-only calls over the serial framer of bgzf_core.hpp,
// spm_hip_bgzf_frame_host and spm_hip_bgzf_framed_size; spm_hip_bgzf_deflate (bgzf_deflate.hpp has the kernels), the stages
// behind it for spm_hip_bam_deflate, the blocks' offsets of either kind of handle, and the host-only calls over the serial
// deflater of bgzf_deflate_core.hpp; spm_hip_bam_deflate, the deflated file of a BAM handle (output_handles.hpp).
#include "internal.hpp"
#include "bgzf.hpp"
#include "bgzf_deflate.hpp"

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
    if (z)
        handle_destroy(z, {z->d, z->d_offsets_alloc});
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
    SPM_TRY(bgzf_check_n_blocks(who, ctx, n, D, "bytes"));
    std::unique_ptr<spm_bgzf, void (*)(spm_bgzf *)> Z(new spm_bgzf, spm_hip_bgzf_destroy);
    Z->ctx = ctx;
    Z->n = bgzf_framed_size(n, D, eof);
    Z->stats.n_in = n;
    Z->stats.n_out = Z->n;
    Z->stats.n_blocks = n_blocks;
    Z->D = D;
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
    Z->deflate.ms_place = Z->stats.ms_frame;
    Z->deflate.ms_host = Z->stats.ms_host;
    Z->deflate.n_in = n;
    Z->deflate.n_out = Z->n;
    Z->deflate.n_blocks = Z->deflate.n_stored_blocks = n_blocks;
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
    SPM_TRY(handle_download(z->ctx, z->have_host, view_part{z->d, z->n, z->host}));
    out_if(bytes, z->host.data());
    out_if(n, z->n);
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_device(spm_bgzf *z, const void **bytes, uint64_t *n)
{
    if (!z)
        return SPM_E_INVALID;
    out_if(bytes, z->d);
    out_if(n, z->n);
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_stats(const spm_bgzf *z, spm_bgzf_stats *out) { return stats_out(z ? &z->stats : nullptr, out); }

// ---- deflated blocks (bgzf_deflate.hpp, bgzf_deflate_core.hpp) ----
static int deflate_check_opts(const char *who, spm_ctx *ctx, const spm_bgzf_deflate_opts *o)
{
    const char *why = !o                                ? "NULL opts"
                      : o->block_data > kBgzfBlockData  ? "block_data above 65280"
                      : (o->flags & ~(SPM_BGZF_EOF | SPM_BGZF_DYNAMIC)) ? "unknown flag bits"
                      : o->level != 1                   ? "level is not 1 (the greedy parse, the one there is)"
                      : o->reserved                     ? "reserved is not 0"
                                                        : nullptr;
    if (!why)
        return SPM_OK;
    if (o)
        SPM_SET_ERR(ctx, "%s: %s (block_data %u, flags 0x%x, level %u, reserved %u)", who, why, o->block_data, o->flags, o->level, o->reserved);
    else
        SPM_SET_ERR(ctx, "%s: %s", who, why);
    return SPM_E_INVALID;
}

extern "C" int spm_hip_bgzf_deflate_bound(uint64_t n, const spm_bgzf_deflate_opts *opts, uint64_t *len)
{
    SPM_TRY(deflate_check_opts("spm_hip_bgzf_deflate_bound", nullptr, opts));
    const spm_bgzf_opts o{opts->block_data, opts->flags & SPM_BGZF_EOF, 0};
    return spm_hip_bgzf_framed_size(n, &o, len);
}

extern "C" int spm_hip_bgzf_deflate_host(const void *src, uint64_t n, const spm_bgzf_deflate_opts *opts, void *dst, uint64_t cap,
                                         uint64_t *len)
{
    static const char *const who = "spm_hip_bgzf_deflate_host";
    if ((!src && n) || !len || (!dst && cap)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL %s", who, !len ? "len" : !src ? "src with n > 0" : "dst with cap > 0");
        return SPM_E_INVALID;
    }
    uint64_t bound = 0;
    SPM_TRY(spm_hip_bgzf_deflate_bound(n, opts, &bound));
    std::vector<uint8_t> file(bound);
    *len = bgzf_deflate_serial(static_cast<const uint8_t *>(src), n, bgzf_block_data(opts->block_data), (opts->flags & SPM_BGZF_EOF) != 0,
                               file.data(), nullptr, nullptr, (opts->flags & SPM_BGZF_DYNAMIC) != 0);
    if (*len > cap)
        return SPM_E_OVERFLOW;
    if (*len)
        memcpy(dst, file.data(), *len);
    return SPM_OK;
}

// The deflate stages on the context's stream: n bytes at d_src, behind `prefix` (bytes that are blocks already), into a new handle.
int bgzf_deflate_run(const char *who, spm_ctx *ctx, const void *d_src, uint64_t n, const spm_bgzf_deflate_opts *opts,
                     const std::vector<uint8_t> &prefix, spm_bgzf **out)
{
    const auto t_call = clk::now();
    const uint32_t D = bgzf_block_data(opts->block_data);
    const bool eof = (opts->flags & SPM_BGZF_EOF) != 0, dynamic = (opts->flags & SPM_BGZF_DYNAMIC) != 0;
    const uint64_t n_blocks = bgzf_n_blocks(n, D);
    SPM_TRY(bgzf_check_n_blocks(who, ctx, n, D, "bytes"));
    std::unique_ptr<spm_bgzf, void (*)(spm_bgzf *)> Z(new spm_bgzf, spm_hip_bgzf_destroy);
    Z->ctx = ctx;
    Z->D = D;
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hip_events<4> ev;
    SPM_HIP_CHECK(ctx, ev.create());
    dev_scratch keep;
    bgzf_deflate_params P;
    P.src = static_cast<const uint8_t *>(d_src);
    P.n = n;
    P.n_blocks = n_blocks;
    P.D = D;
    P.stage_words = deflate_stage_words(D);
    P.L = bgzf_plan_lanes(D);
    // the offsets stay with the handle: [0] unused, [1 .. n_blocks + 1] the blocks and their end, then the counters
    unsigned long long *sums = nullptr;
    SPM_HIP_CHECK(ctx, hipMalloc(&sums, (n_blocks + 2 + kDefCnts) * 8));
    Z->d_offsets_alloc = sums;
    Z->d_offsets = sums + 1;
    P.offsets = Z->d_offsets;
    P.counts = sums + n_blocks + 2;
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kDefCnts * 8, st));
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    const auto sizes = counted<unsigned long long>(deflate_size_op{nullptr, 0, 0});
    SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<unsigned long long>(ctx, sizes, n_blocks + 2, &tmp_bytes));
    SPM_HIP_CHECK(ctx, keep.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 1)));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.size, std::max<uint64_t>(n_blocks, 1) * 4));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    if (n_blocks) {
        SPM_HIP_CHECK(ctx, keep.alloc(&P.slots, n * 2));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.stage, n_blocks * P.stage_words * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.crc, n_blocks * 4));
        hipLaunchKernelGGL(dynamic ? bgzf_deflate_kernel<true> : bgzf_deflate_kernel<false>, dim3((unsigned)n_blocks), dim3(kBgzfLanes), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<unsigned long long>(deflate_size_op{P.size, n_blocks, prefix.size()}), sums,
                                     n_blocks + 2));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    SPM_HIP_CHECK(ctx, read_counts(ctx, sums + n_blocks + 1, 1 + kDefCnts)); // the one read-back: the end of the blocks, the counts
    const uint64_t end = ctx->h_counters[0];
    Z->n = end + (eof ? kBgzfEof : 0);
    if (Z->n) {
        SPM_HIP_CHECK(ctx, hipMalloc(&Z->d, Z->n));
        P.dst = Z->d;
        if (!prefix.empty())
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(Z->d, prefix.data(), prefix.size(), hipMemcpyHostToDevice, st));
    }
    if (n_blocks + (eof ? 1 : 0)) {
        hipLaunchKernelGGL(bgzf_place_kernel, dim3((unsigned)(n_blocks + (eof ? 1 : 0))), dim3(kBgzfLanes), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
    SPM_HIP_CHECK(ctx, hipEventSynchronize(ev[3])); // (source and prefix are the caller's again when the call returns)
    spm_bgzf_deflate_stats &S = Z->deflate;
    hipEventElapsedTime(&S.ms_parse, ev[0], ev[1]);
    hipEventElapsedTime(&S.ms_scan, ev[1], ev[2]);
    hipEventElapsedTime(&S.ms_place, ev[2], ev[3]);
    S.n_in = n;
    S.n_out = Z->n;
    S.n_blocks = n_blocks;
    S.n_stored_blocks = ctx->h_counters[1 + kDefCntStored];
    S.n_matches = ctx->h_counters[1 + kDefCntMatches];
    S.n_literals = ctx->h_counters[1 + kDefCntLiterals];
    S.n_prefix_bytes = prefix.size();
    Z->n_dynamic_blocks = ctx->h_counters[1 + kDefCntDynamic];
    S.ms_host = ms_since(t_call);
    Z->stats.ms_frame = S.ms_parse + S.ms_scan + S.ms_place;
    Z->stats.ms_host = S.ms_host;
    Z->stats.n_in = n;
    Z->stats.n_out = Z->n;
    Z->stats.n_blocks = n_blocks;
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] bgzf deflate: %llu bytes -> %llu blocks of %u (%llu stored, %llu dynamic)%s, %llu bytes: parse %.3f, scan "
                        "%.3f, place %.3f ms, %.3f ms in all\n", (unsigned long long)n, (unsigned long long)n_blocks, D,
                (unsigned long long)S.n_stored_blocks, (unsigned long long)Z->n_dynamic_blocks, eof ? " + EOF" : "", (unsigned long long)Z->n, S.ms_parse, S.ms_scan, S.ms_place,
                S.ms_host);
    *out = Z.release();
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_deflate(spm_ctx *ctx, const void *device_src, uint64_t n, const spm_bgzf_deflate_opts *opts, spm_bgzf **out)
{
    static const char *const who = "spm_hip_bgzf_deflate";
    if (out)
        *out = nullptr;
    if (!ctx || !opts || !out) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !ctx ? "ctx" : !opts ? "opts" : "out");
        return SPM_E_INVALID;
    }
    if (!device_src && n) {
        SPM_SET_ERR(ctx, "%s: NULL device_src with n = %llu", who, (unsigned long long)n);
        return SPM_E_INVALID;
    }
    SPM_TRY(deflate_check_opts(who, ctx, opts));
    return bgzf_deflate_run(who, ctx, device_src, n, opts, std::vector<uint8_t>(), out);
}

// The whole BAM file deflated: the header section by the host deflater, without an EOF block, the record stream behind it.
extern "C" int spm_hip_bam_deflate(spm_bam *b, const spm_bgzf_deflate_opts *opts, spm_bgzf **out)
{
    static const char *const who = "spm_hip_bam_deflate";
    if (out)
        *out = nullptr;
    if (!b)
        return SPM_E_INVALID;
    spm_ctx *ctx = b->ctx;
    if (!opts || !out) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !opts ? "opts" : "out");
        return SPM_E_INVALID;
    }
    SPM_TRY(deflate_check_opts(who, ctx, opts));
    const uint32_t D = bgzf_block_data(opts->block_data);
    std::vector<uint8_t> header(bgzf_framed_size(b->plain_header.size(), D, false)); // (a bound: a block never grows past stored)
    header.resize(bgzf_deflate_serial(b->plain_header.data(), b->plain_header.size(), D, false, header.data(), nullptr, nullptr,
                                      (opts->flags & SPM_BGZF_DYNAMIC) != 0));
    return bgzf_deflate_run(who, ctx, b->d_records, b->n_record_bytes, opts, header, out);
}

// the offsets of a framed handle are the closed form: made, and uploaded, when first asked for (spm_hip_bam_index asks too)
int bgzf_offsets_ready(spm_bgzf *z, bool on_device)
{
    spm_ctx *ctx = z->ctx;
    const uint64_t n_offsets = z->stats.n_blocks + 1;
    if (!z->have_host_offsets) {
        z->host_offsets.resize(n_offsets);
        if (z->d_offsets) {
            SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(z->host_offsets.data(), z->d_offsets, n_offsets * 8, hipMemcpyDeviceToHost, ctx->stream));
            SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        } else {
            for (uint64_t b = 0; b + 1 < n_offsets; ++b)
                z->host_offsets[b] = bgzf_block_offset(z->D, b);
            z->host_offsets[n_offsets - 1] = bgzf_framed_size(z->stats.n_in, z->D, false);
        }
        z->have_host_offsets = true;
    }
    if (on_device && !z->d_offsets) {
        SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        SPM_HIP_CHECK(ctx, hipMalloc(&z->d_offsets_alloc, n_offsets * 8));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(z->d_offsets_alloc, z->host_offsets.data(), n_offsets * 8, hipMemcpyHostToDevice, ctx->stream));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        z->d_offsets = static_cast<unsigned long long *>(z->d_offsets_alloc);
    }
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_blocks(spm_bgzf *z, const uint64_t **offsets, uint64_t *n_blocks)
{
    if (!z)
        return SPM_E_INVALID;
    SPM_TRY(bgzf_offsets_ready(z, false));
    out_if(offsets, z->host_offsets.data());
    out_if(n_blocks, z->stats.n_blocks);
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_blocks_device(spm_bgzf *z, const void **offsets, uint64_t *n_blocks)
{
    if (!z)
        return SPM_E_INVALID;
    SPM_TRY(bgzf_offsets_ready(z, true));
    out_if(offsets, z->d_offsets);
    out_if(n_blocks, z->stats.n_blocks);
    return SPM_OK;
}

extern "C" int spm_hip_bgzf_deflate_stats(const spm_bgzf *z, spm_bgzf_deflate_stats *out)
{
    return stats_out(z ? &z->deflate : nullptr, out);
}

extern "C" int spm_hip_bgzf_block_types(const spm_bgzf *z, uint64_t n[3])
{
    if (!z || !n)
        return SPM_E_INVALID;
    n[0] = z->deflate.n_stored_blocks;
    n[2] = z->n_dynamic_blocks;
    n[1] = z->deflate.n_blocks - n[0] - n[2];
    return SPM_OK;
}

void spm_warm_bgzf_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)bgzf_frame_kernel);
    (void)hipFuncGetAttributes(&a, (const void *)bgzf_deflate_kernel<false>);
    (void)hipFuncGetAttributes(&a, (const void *)bgzf_deflate_kernel<true>);
    (void)hipFuncGetAttributes(&a, (const void *)bgzf_place_kernel);
}
