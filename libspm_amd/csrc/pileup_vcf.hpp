// pileup_vcf.hpp -- genotype calls for pileup sites and the VCF text of the variant ones (spm_hip_pileup_sites_vcf,
// spm_hip_pileup_sites_vcf_records, spm_hip_pileup_sites_calls_host, spm_hip_pileup_sites_vcf_host, spm_hip_vcf_header; contract
// and rule in spm_hip.h, scheme in DESIGN.md 4.12f, the rule's functions in pileup_vcf_core.hpp).  gfx950.  Unit: pileup_vcf.hip.
// It reads and makes the handles of output_handles.hpp.
//   vc_call_kernel      one lane per site: the ten costs in registers, the call record (its offset comes later), the line's
//                       length, the order test against the left neighbour and against ref_len, the counters, the sum of the lengths;
//   (device_order.hip)  the exclusive sum of the lengths: the lines' offsets behind the header;
//   vc_write_kernel     one workgroup per run of kVcGroup consecutive sites.  A lane formats its site's line into LDS at the
//                       place the line has inside the run, the run shifted by the low two bits of its address in the text, so a
//                       dword of LDS is a dword of the text.  Behind a barrier the group stores the run: the head bytes up to
//                       the first 4-byte border, whole dwords, the tail bytes.  Every byte of the text behind the header is
//                       written by exactly one group: no memset.  The lane also stores its call record's offset.
// The header is built on the host and copied to the front of the text on the stream.  Vector stores only; the only global atomics
// go to the counters.
#pragma once

#include <algorithm>
#include <memory>
#include <string>

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "pileup_vcf_core.hpp"
#include "device_order.hpp"
#include "output_handles.hpp"
#include "wave.hpp"

namespace spm_hip
{

// Sites per workgroup of the write stage, one lane each.  The run's bytes lie packed in LDS, so what bounds them is the number
// of sites times the longest line a site can have (kVcMaxLine: every number ten digits, a name of 254 bytes), plus the shift.
constexpr uint32_t kVcGroup = 128;
constexpr uint32_t kVcLdsWords = (kVcGroup * kVcMaxLine + 3 + 3) / 4;
static_assert(kVcLdsWords * 4 <= 64 * 1024, "a group's run of longest lines fits the LDS a workgroup may take");
enum { kVcCntBad, kVcCntVariant, kVcCntRef, kVcCntRefN, kVcCntLowQual, kVcCntLineBytes, kVcCnts };

struct vcf_params
{
    const spm_pileup_site *sites = nullptr;
    uint32_t n = 0;
    uint64_t ref_len = 0;
    vc_opts O;
    const char *rname = nullptr; // device copy
    uint32_t rname_len = 0;
    uint32_t *lens = nullptr, *offs = nullptr; // [n]
    spm_variant_call *calls = nullptr;         // [n]
    uint8_t *text = nullptr;
    uint64_t header_bytes = 0, n_text = 0;
    unsigned long long *counts = nullptr;
};

__global__ __launch_bounds__(256) void vc_call_kernel(const vcf_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false, variant = false, ref = false, ref_n = false, low = false;
    uint32_t len = 0;
    if (i < P.n) {
        const spm_pileup_site S = P.sites[i];
        bad = S.pos >= P.ref_len || (i > 0 && P.sites[i - 1].pos >= S.pos);
        vc_eval E;
        vc_call(S, P.O, E);
        len = vc_line_len(P.rname_len, S, E, P.O);
        spm_variant_call C;
        vc_record(S, E, len, 0, C);
        P.calls[i] = C;
        P.lens[i] = len;
        variant = E.status == SPM_CALL_VARIANT;
        ref = E.status == SPM_CALL_REF;
        ref_n = E.status == SPM_CALL_REF_N;
        low = variant && E.qual < P.O.min_qual;
    }
    count_flagged(&P.counts[kVcCntBad], bad);
    count_flagged(&P.counts[kVcCntVariant], variant);
    count_flagged(&P.counts[kVcCntRef], ref);
    count_flagged(&P.counts[kVcCntRefN], ref_n);
    count_flagged(&P.counts[kVcCntLowQual], low);
    (void)wave_reserve(&P.counts[kVcCntLineBytes], len); // (one atomic per wave; 64 bits, where offs[] would wrap)
}

// The driver has refused a text of 2^32 bytes or more before this runs, so offs[] did not wrap; lens[] are vc_call_kernel's, each
// kVcMaxLine at most, so a run fits `run`; header_bytes + offs[i] + lens[i] <= n_text.
__global__ __launch_bounds__(kVcGroup) void vc_write_kernel(const vcf_params P)
{
    __shared__ uint32_t run[kVcLdsWords];
    uint8_t *const bytes = reinterpret_cast<uint8_t *>(run);
    const uint32_t first = blockIdx.x * kVcGroup; // (the grid is ceil(n / kVcGroup): first < n)
    const uint32_t last = (P.n - first < kVcGroup ? P.n : first + kVcGroup) - 1;
    const uint32_t r0 = P.offs[first], B = P.offs[last] + P.lens[last] - r0;
    const uint64_t at = P.header_bytes + r0; // of the run in the text
    const uint32_t shift = (uint32_t)((reinterpret_cast<uint64_t>(P.text) + at) & 3u);
    const uint32_t i = first + threadIdx.x;
    if (i < P.n) {
        const uint32_t off = P.offs[i], len = P.lens[i];
        P.calls[i].offset = P.header_bytes + off;
        if (len) {
            const spm_pileup_site S = P.sites[i];
            vc_eval E;
            vc_call(S, P.O, E);
            vc_store_sink out{bytes + shift + (off - r0)};
            vc_line_emit(out, P.rname, P.rname_len, S, E, P.O);
        }
    }
    __syncthreads();
    uint8_t *const dst = P.text + at - shift; // on a 4-byte border; byte p of `bytes` belongs at dst + p
    uint32_t a, b;
    vc_run_split(shift, B, a, b);
    for (uint32_t p = shift + threadIdx.x; p < a; p += kVcGroup)
        dst[p] = bytes[p];
    for (uint32_t w = a / 4 + threadIdx.x; w < b / 4; w += kVcGroup)
        reinterpret_cast<uint32_t *>(dst)[w] = run[w];
    for (uint32_t p = b + threadIdx.x; p < shift + B; p += kVcGroup)
        dst[p] = bytes[p];
}

using vcf_ptr = std::unique_ptr<spm_vcf, void (*)(spm_vcf *)>;

static const char *const kVcNameRule = "is empty, longer than 254 bytes or holds a byte outside '!' .. '~' (rname: or is \"*\")";

// what every form refuses before anything is read; O: the options the rule takes
static int vcf_check_args(const char *who, spm_ctx *ctx, const void *sites, uint64_t n, const char *rname, const char *sample, uint64_t ref_len,
                          const spm_vcf_opts *opts, vc_opts &O)
{
    if (!rname || !sample || (!sites && n)) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !rname ? "rname" : !sample ? "sample" : "sites with n_sites > 0");
        return SPM_E_INVALID;
    }
    if (const char *why = vc_opts_of(opts, O)) {
        SPM_SET_ERR(ctx, "%s: %s", who, why);
        return SPM_E_INVALID;
    }
    const bool bad_rname = !jst_sam_name_ok(rname, strlen(rname));
    if (bad_rname || !vc_sample_ok(sample, strlen(sample))) {
        SPM_SET_ERR(ctx, "%s: %s %s", who, bad_rname ? "rname" : "sample", kVcNameRule);
        return SPM_E_INVALID;
    }
    if (n > 0xFFFFFFFFull || ref_len > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "%s: %s (not supported)", who, n > 0xFFFFFFFFull ? "more than 2^32 - 1 sites" : "ref_len above 2^32 - 1, beyond what a site's pos can name");
        return SPM_E_UNSUPPORTED;
    }
    return SPM_OK;
}

static const char *const kVcDisorder = "sites whose pos does not ascend strictly or reaches ref_len";

// the stages of one call over a device array of sites that has passed vcf_check_args
static int vcf_run(const char *who, spm_ctx *ctx, const spm_pileup_site *d_sites, uint32_t n, const char *rname, const char *sample,
                   uint64_t ref_len, const vc_opts &O, spm_vcf **out)
{
    const clk::time_point t_call = clk::now();
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    dev_scratch keep;
    hip_events<5> ev; // before the calls, behind them, behind the scan; before the write stage, behind it
    SPM_HIP_CHECK(ctx, ev.create());
    const std::string header = vc_header(rname, sample, ref_len);
    vcf_params P;
    P.sites = d_sites;
    P.n = n;
    P.ref_len = ref_len;
    P.O = O;
    P.rname_len = (uint32_t)strlen(rname);
    P.header_bytes = header.size();
    vcf_ptr R(new spm_vcf, spm_hip_vcf_destroy);
    R->ctx = ctx;
    R->n_calls = n;
    unsigned long long none[kVcCnts] = {};
    const unsigned long long *c = none;
    if (n) {
        void *d_tmp = nullptr, *d_rname = nullptr;
        size_t tmp_bytes = 0;
        SPM_HIP_CHECK(ctx, keep.alloc(&P.counts, kVcCnts * 8));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kVcCnts * 8, st));
        SPM_HIP_CHECK(ctx, scan_u32_tmp_bytes(ctx, n, &tmp_bytes));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 1)));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.lens, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.offs, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_rname, P.rname_len));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_rname, rname, P.rname_len, hipMemcpyHostToDevice, st));
        P.rname = static_cast<const char *>(d_rname);
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_calls, (size_t)n * sizeof(spm_variant_call)));
        P.calls = R->d_calls;
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, vc_call_kernel, n, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        SPM_HIP_CHECK(ctx, exclusive_sum_u32(ctx, d_tmp, tmp_bytes, P.lens, P.offs, n));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kVcCnts)); // the one read-back: the refusals and the size of the text
        c = ctx->h_counters;
        if (c[kVcCntBad]) {
            SPM_SET_ERR(ctx, "%s: %llu %s; ref_len %llu; nothing was returned", who, c[kVcCntBad], kVcDisorder, (unsigned long long)ref_len);
            return SPM_E_INVALID;
        }
    } else {
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    }
    const unsigned long long n_variant = c[kVcCntVariant], n_ref = c[kVcCntRef], n_ref_n = c[kVcCntRefN], n_low = c[kVcCntLowQual];
    P.n_text = header.size() + c[kVcCntLineBytes];
    if (P.n_text > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "%s: a text of %llu bytes, 2^32 or more (not supported)", who, (unsigned long long)P.n_text);
        return SPM_E_UNSUPPORTED;
    }
    R->n_bytes = P.n_text;
    SPM_HIP_CHECK(ctx, hipMalloc(&R->d_text, P.n_text));
    P.text = reinterpret_cast<uint8_t *>(R->d_text);
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->d_text, header.data(), header.size(), hipMemcpyHostToDevice, st));
    if (n) {
        hipLaunchKernelGGL(vc_write_kernel, dim3((n + kVcGroup - 1) / kVcGroup), dim3(kVcGroup), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
    SPM_HIP_CHECK(ctx, hipStreamSynchronize(st)); // (the header and the scratch go with this scope)
    spm_vcf_stats &S = R->stats;
    hipEventElapsedTime(&S.ms_call, ev[0], ev[1]);
    hipEventElapsedTime(&S.ms_scan, ev[1], ev[2]);
    hipEventElapsedTime(&S.ms_write, ev[3], ev[4]);
    S.ms_total = S.ms_call + S.ms_scan + S.ms_write;
    S.group_sites = kVcGroup;
    S.n_sites = n;
    S.n_variant = n_variant;
    S.n_ref = n_ref;
    S.n_ref_n = n_ref_n;
    S.n_low_qual = n_low;
    S.n_header_bytes = header.size();
    S.n_text_bytes = P.n_text;
    S.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] pileup sites vcf: %u sites (%llu lines, %llu LowQual, %llu ref/ref, %llu without a call), %llu bytes: "
                        "device %.3f ms (calls %.3f, scan %.3f, write %.3f), %.3f ms in all\n", n, n_variant, n_low, n_ref, n_ref_n,
                (unsigned long long)P.n_text, S.ms_total, S.ms_call, S.ms_scan, S.ms_write, S.ms_host);
    *out = R.release();
    return SPM_OK;
}

} // namespace spm_hip

extern "C" int spm_hip_pileup_sites_vcf_records(spm_ctx *ctx, const void *device_sites, uint64_t n_sites, const char *rname, const char *sample,
                                                uint64_t ref_len, const spm_vcf_opts *opts, spm_vcf **out)
{
    static const char *const who = "spm_hip_pileup_sites_vcf_records";
    if (out)
        *out = nullptr;
    if (!ctx || !out) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !ctx ? "ctx" : "out");
        return SPM_E_INVALID;
    }
    vc_opts O;
    SPM_TRY(vcf_check_args(who, ctx, device_sites, n_sites, rname, sample, ref_len, opts, O));
    return vcf_run(who, ctx, static_cast<const spm_pileup_site *>(device_sites), (uint32_t)n_sites, rname, sample, ref_len, O, out);
}

extern "C" int spm_hip_pileup_sites_vcf(spm_pileup_sites *s, const char *rname, const char *sample, uint64_t ref_len, const spm_vcf_opts *opts,
                                        spm_vcf **out)
{
    static const char *const who = "spm_hip_pileup_sites_vcf";
    if (out)
        *out = nullptr;
    if (!s || !out)
        return SPM_E_INVALID;
    vc_opts O;
    SPM_TRY(vcf_check_args(who, s->ctx, s->d, s->n, rname, sample, ref_len, opts, O));
    return vcf_run(who, s->ctx, s->d, (uint32_t)s->n, rname, sample, ref_len, O, out);
}

extern "C" int spm_hip_vcf_view(spm_vcf *v, const char **text, uint64_t *n_bytes, const spm_variant_call **calls, uint64_t *n_calls)
{
    if (!v)
        return SPM_E_INVALID;
    SPM_TRY(handle_download(v->ctx, v->have_host, view_part{v->d_text, v->n_bytes, v->host_text}, view_part{v->d_calls, v->n_calls, v->host_calls}));
    out_if(text, (const char *)v->host_text.data());
    out_if(n_bytes, v->n_bytes);
    out_if(calls, (const spm_variant_call *)v->host_calls.data());
    out_if(n_calls, v->n_calls);
    return SPM_OK;
}

extern "C" int spm_hip_vcf_device(spm_vcf *v, const void **text, uint64_t *n_bytes, const void **calls, uint64_t *n_calls)
{
    if (!v)
        return SPM_E_INVALID;
    out_if(text, (const void *)v->d_text);
    out_if(n_bytes, v->n_bytes);
    out_if(calls, (const void *)v->d_calls);
    out_if(n_calls, v->n_calls);
    return SPM_OK;
}

extern "C" int spm_hip_vcf_stats(const spm_vcf *v, spm_vcf_stats *out) { return stats_out(v ? &v->stats : nullptr, out); }

extern "C" void spm_hip_vcf_destroy(spm_vcf *v)
{
    if (v)
        handle_destroy(v, {v->d_text, v->d_calls});
}

extern "C" int spm_hip_vcf_header(const char *rname, const char *sample, uint64_t ref_len, char *buf, uint64_t cap, uint64_t *len)
{
    static const char *const who = "spm_hip_vcf_header";
    if (!rname || !sample || !len || (!buf && cap)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL %s", who, !rname ? "rname" : !sample ? "sample" : !len ? "len" : "buf with cap > 0");
        return SPM_E_INVALID;
    }
    vc_opts O;
    SPM_TRY(vcf_check_args(who, nullptr, nullptr, 0, rname, sample, 0, nullptr, O));
    const std::string h = vc_header(rname, sample, ref_len);
    *len = h.size();
    if (h.size() > cap)
        return SPM_E_OVERFLOW;
    memcpy(buf, h.data(), h.size());
    return SPM_OK;
}

extern "C" int spm_hip_pileup_sites_calls_host(const spm_pileup_site *sites, uint64_t n, const spm_vcf_opts *opts, spm_variant_call *calls)
{
    static const char *const who = "spm_hip_pileup_sites_calls_host";
    vc_opts O;
    const char *why = (!sites || !calls) && n ? "NULL sites or calls with n > 0" : vc_opts_of(opts, O);
    if (!why && !vc_sites_in_order(sites, n, ~0ull))
        why = "sites whose pos does not ascend strictly";
    if (why) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %s", who, why);
        return SPM_E_INVALID;
    }
    vc_serial(sites, n, nullptr, 0, O, 0, false, calls, nullptr);
    return SPM_OK;
}

extern "C" int spm_hip_pileup_sites_vcf_host(const spm_pileup_site *sites, uint64_t n, const char *rname, const char *sample, uint64_t ref_len,
                                             const spm_vcf_opts *opts, char *dst, uint64_t cap, uint64_t *len)
{
    static const char *const who = "spm_hip_pileup_sites_vcf_host";
    if (!len || (!dst && cap)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL %s", who, !len ? "len" : "dst with cap > 0");
        return SPM_E_INVALID;
    }
    vc_opts O;
    SPM_TRY(vcf_check_args(who, nullptr, sites, n, rname, sample, ref_len, opts, O));
    if (!vc_sites_in_order(sites, n, ref_len)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %s; ref_len %llu", who, kVcDisorder, (unsigned long long)ref_len);
        return SPM_E_INVALID;
    }
    std::string text = vc_header(rname, sample, ref_len);
    vc_serial(sites, n, rname, (uint32_t)strlen(rname), O, text.size(), true, nullptr, &text);
    *len = text.size();
    if (text.size() > cap) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %llu bytes need more than cap %llu", who, (unsigned long long)text.size(), (unsigned long long)cap);
        return SPM_E_OVERFLOW;
    }
    memcpy(dst, text.data(), text.size());
    return SPM_OK;
}
