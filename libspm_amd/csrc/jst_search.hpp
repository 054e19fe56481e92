// jst_search.hpp -- the pan-genome search (spm_hip_jst_search) and the accessors of its records (scheme in jst.hpp, DESIGN.md
// 4.5).  gfx950.  Unit: jst.hip.  Search = the segmented scan of the context buffer by the ordinary engines +
// jst_fanout_kernel, here, over the walker of jst_fanout.hpp.
#pragma once

#include "internal.hpp"
#include "jst_fanout.hpp"
#include "jst_handles.hpp"
#include "scratch_layout.hpp"

namespace spm_hip
{

struct jst_fan_params
{
    const spm_hit *hits;
    uint64_t n_hits;                         // segment hits, if the host knows their number ...
    const unsigned long long *n_hits_dev;    // ... else where the scan counts them (launched before the host has read it)
    uint64_t hit_cap;                        //     and the capacity of `hits`
    jst_ctx_tables T;
    const int32_t *m; // needle lengths
    uint32_t report_begin;
    spm_jst_hit *out;
    unsigned long long *out_count;
    uint64_t out_cap;
};

// One thread per segment hit: drop it if its last symbol lies in the left context, else report it for every haplotype
// of the context's group, in haplotype coordinates.  Output slots are drawn with one atomic per wave (a per-record
// atomic on the single counter cost 0.6 ms for 10^6 records).
__global__ void jst_fanout_kernel(jst_dev J, jst_fan_params F)
{
    uint64_t n_hits = F.n_hits;
    if (F.n_hits_dev) {
        const unsigned long long n = *F.n_hits_dev;
        n_hits = n < F.hit_cap ? n : F.hit_cap;
    }
    jst_fan_out<spm_hit>(
        J, F.T, n_hits, F.out_count, F.out_cap,
        [&](uint64_t t, spm_hit &hit, jst_fan_item &it) {
            hit = F.hits[t];
            it.probe = F.report_begin ? hit.pos : hit.pos - 1;
            it.last = F.report_begin ? hit.pos + (uint64_t)F.m[hit.pattern] - 1 : hit.pos - 1;
            it.at = hit.pos;
            return true;
        },
        [&](const spm_hit &hit, unsigned long long slot, uint32_t h, uint64_t ctx_lo, uint64_t local) {
            spm_jst_hit o;
            o.pos = ctx_lo + local;
            o.haplotype = h;
            o.pattern = hit.pattern;
            o.score = hit.score;
            o.reserved = 0;
            F.out[slot] = o;
        });
}

} // namespace spm_hip

extern "C" void spm_hip_jst_hits_destroy(spm_jst_hits *h)
{
    if (!h)
        return;
    if (h->seg)
        spm_hip_hits_destroy(h->seg);
    for (hipEvent_t e : h->sel_ev)
        if (e)
            hipEventDestroy(e);
    if (h->d) {
        if (h->ctx && !h->selected && h->ctx->jst_pool.size() < 4)
            h->ctx->jst_pool.push_back({h->d, h->cap});
        else
            hipFree(h->d);
    }
    delete h;
}

// the fan-out of `grid` workgroups (0: none) between the tree's two events
static int jst_fan_launch(spm_jst *J, const spm_hip::jst_fan_params &G, uint64_t grid)
{
    spm_ctx *ctx = J->ctx;
    SPM_HIP_CHECK(ctx, hipEventRecord(J->fan_ev[0], ctx->stream));
    if (grid) {
        hipLaunchKernelGGL(spm_hip::jst_fanout_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, J->dev(), G);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(J->fan_ev[1], ctx->stream));
    return SPM_OK;
}

extern "C" int spm_hip_jst_search(spm_jst *J, const spm_patterns *patterns, const spm_scan_opts *opts_in,
                                  spm_jst_hits **out)
{
    using namespace spm_hip;
    if (!J || !patterns || !out) {
        SPM_SET_ERR(J ? J->ctx : nullptr, "spm_hip_jst_search: invalid argument");
        return SPM_E_INVALID;
    }
    spm_ctx *ctx = J->ctx;
    if (!J->indexed) {
        SPM_SET_ERR(ctx, "spm_hip_jst_search: call spm_hip_jst_index first");
        return SPM_E_INVALID;
    }
    uint64_t need = 0;
    for (uint32_t p = 0; p < patterns->n; ++p)
        need = std::max<uint64_t>(need, spm_hip_patterns_window_size(patterns, p));
    if (need > J->window) {
        SPM_SET_ERR(ctx, "spm_hip_jst_search: needle window %llu exceeds the indexed window %u",
                    (unsigned long long)need, J->window);
        return SPM_E_INVALID;
    }
    if (patterns->algo == SPM_ALGO_MYERS_PREFIX) {
        SPM_SET_ERR(ctx, "spm_hip_jst_search: the prefix matcher has no meaning over haplotype contexts");
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_hits, void (*)(spm_jst_hits *)> R(new spm_jst_hits, spm_hip_jst_hits_destroy);
    R->ctx = ctx;
    spm_scan_opts o{};
    if (opts_in)
        o = *opts_in;
    o.left_context = 0;
    o.pos_offset = 0;
    R->alignable = (o.flags & SPM_SCAN_ALIGNABLE) != 0; // ours alone: the scan never sees the bit
    o.flags &= ~SPM_SCAN_ALIGNABLE;
    R->jst = J;
    R->patterns = patterns;
    R->pat_strands = patterns->strands;
    R->generation = J->generation;
    R->sel_n_hap = J->H;
    R->sel_n_patterns = std::max<uint64_t>(patterns->n, 1);
    R->sel_max_pos = J->max_hap_len;
    const uint64_t out_cap = o.max_hits ? o.max_hits : (1ull << 22);
    if (o.max_hits == 0)
        o.max_hits = 1ull << 22;
    if (J->n_ctx == 0 || patterns->n == 0) {
        *out = R.release();
        return SPM_OK;
    }
    spm_hits *seg = nullptr;
    for (size_t i = 0; i < ctx->jst_pool.size(); ++i)
        if (ctx->jst_pool[i].second == out_cap) {
            R->d = static_cast<spm_jst_hit *>(ctx->jst_pool[i].first);
            ctx->jst_pool.erase(ctx->jst_pool.begin() + (long)i);
            break;
        }
    if (!R->d)
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d, out_cap * sizeof(spm_jst_hit)));
    R->cap = out_cap;
    if (!J->d_fan_count) {
        SPM_HIP_CHECK(ctx, hipMalloc(&J->d_fan_count, 8));
        SPM_HIP_CHECK(ctx, hipEventCreate(&J->fan_ev[0]));
        SPM_HIP_CHECK(ctx, hipEventCreate(&J->fan_ev[1]));
    }
    jst_fan_params F{};
    F.T = J->ctx_tables();
    F.m = patterns->d_m;
    F.report_begin = patterns->is_myers() ? 0 : 1;
    F.out = R->d;
    F.out_cap = out_cap;
    // The fan-out is launched right behind the scan's kernels, before the host has read the scan's counters: it takes the
    // number of segment hits from the device and counts its records into a spare slot of the scan's counter block, so one
    // read-back serves both (a second host round trip per search cost ~35 us of an idle GPU).  If the scan has to go on
    // after that read-back (overflow, fallback), the fan-out is simply run again below.
    const std::function<int(spm_hits *)> fan_hook = [&](spm_hits *h) -> int {
        jst_fan_params G = F;
        G.hits = h->d_hits;
        G.n_hits_dev = h->d_count;
        G.hit_cap = h->cap;
        G.out_count = h->d_count + kCntFanOut;
        const uint64_t expect = std::max<uint64_t>(1u << 16, 2 * J->seg_hit_hint);
        return jst_fan_launch(J, G, std::min<uint64_t>((expect + 255) / 256, (uint64_t)ctx->n_cu * 64));
    };
    // the verification stage skips end positions inside a context's left context (the fan-out would drop them)
    int rc = scan_impl(ctx, J->ctx_text, 0, J->ctx_bytes, patterns, &o, nullptr, nullptr, nullptr, J->n_ctx, &seg,
                       J->d_ctx_off, J->d_ctx_owned, &fan_hook);
    if (rc != SPM_OK)
        return rc;
    std::unique_ptr<spm_hits, void (*)(spm_hits *)> S(seg, spm_hip_hits_destroy);
    const void *d_rec = nullptr;
    uint64_t n_seg_hits = 0;
    rc = spm_hip_hits_device(seg, &d_rec, &n_seg_hits);
    if (rc != SPM_OK)
        return rc;
    spm_scan_stats ss{};
    spm_hip_hits_stats(seg, &ss);
    J->stats.ms_scan = ss.ms_total;
    J->stats.ms_main = ss.ms_main;
    J->stats.ms_verify = ss.ms_verify;
    J->stats.engine_used = ss.engine_used;
    J->stats.main_launches = ss.main_launches;
    J->stats.segment_hits = n_seg_hits;
    J->stats.fell_back = ss.fell_back;
    J->stats.candidates = ss.n_candidates;
    J->stats.bands = ss.n_bands;
    J->seg_hit_hint = std::max<uint64_t>(J->seg_hit_hint, n_seg_hits);
    unsigned long long n_out = 0;
    if (seg->hook_final) {
        n_out = seg->fan_count; // counted by the fan-out that ran behind the scan, read back with the scan's counters
    } else {
        unsigned long long *d_count = J->d_fan_count;
        SPM_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, 8, ctx->stream));
        jst_fan_params G = F;
        G.hits = static_cast<const spm_hit *>(d_rec);
        G.n_hits = n_seg_hits;
        G.out_count = d_count;
        SPM_TRY(jst_fan_launch(J, G, (n_seg_hits + 255) / 256));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_counters + kLandFanOut, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        n_out = ctx->h_counters[kLandFanOut];
    }
    hipEventElapsedTime(&J->stats.ms_fanout, J->fan_ev[0], J->fan_ev[1]);
    if (n_out > out_cap) {
        SPM_SET_ERR(ctx, "journaled-sequence search produced %llu hits but the buffer holds %llu; raise "
                         "spm_scan_opts.max_hits", n_out, (unsigned long long)out_cap);
        return SPM_E_OVERFLOW;
    }
    R->n = n_out;
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst_search: %llu segment hits -> %llu records; scan %.3f ms (main %.3f, verification %.3f), "
                        "fan-out %.3f ms%s\n", (unsigned long long)n_seg_hits, n_out, J->stats.ms_scan, J->stats.ms_main,
                J->stats.ms_verify, J->stats.ms_fanout, J->stats.fell_back ? "; the seed filter fell back" : "");
    if (R->alignable)
        R->seg = S.release(); // kept for spm_hip_jst_hits_align; otherwise back to the context's pool right here
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_hits_view(spm_jst_hits *h, const spm_jst_hit **records, uint64_t *n)
{
    if (!h || !records || !n)
        return SPM_E_INVALID;
    if (!h->sorted) {
        h->host.resize(h->n);
        if (h->n) {
            SPM_HIP_CHECK(h->ctx, hipMemcpyAsync(h->host.data(), h->d, h->n * sizeof(spm_jst_hit),
                                                 hipMemcpyDeviceToHost, h->ctx->stream));
            SPM_HIP_CHECK(h->ctx, hipStreamSynchronize(h->ctx->stream));
        }
        std::sort(h->host.begin(), h->host.end(), [](const spm_jst_hit &a, const spm_jst_hit &b) {
            if (a.haplotype != b.haplotype)
                return a.haplotype < b.haplotype;
            if (a.pos != b.pos)
                return a.pos < b.pos;
            if (a.pattern != b.pattern)
                return a.pattern < b.pattern;
            return a.score < b.score;
        });
        h->sorted = true;
    }
    *records = h->host.data();
    *n = h->n;
    return SPM_OK;
}

extern "C" int spm_hip_jst_hits_device(spm_jst_hits *h, const void **device_records, uint64_t *n)
{
    if (!h || !device_records || !n)
        return SPM_E_INVALID;
    *device_records = h->d;
    *n = h->n;
    return SPM_OK;
}

extern "C" int spm_hip_jst_hits_copy_device(spm_jst_hits *h, void *device_dst, uint64_t cap, uint64_t *n)
{
    if (!h || !n || (cap && !device_dst))
        return SPM_E_INVALID;
    *n = h->n;
    const uint64_t c = std::min(h->n, cap);
    if (c)
        SPM_HIP_CHECK(h->ctx, hipMemcpyAsync(device_dst, h->d, c * sizeof(spm_jst_hit), hipMemcpyDeviceToDevice,
                                             h->ctx->stream));
    return SPM_OK;
}
