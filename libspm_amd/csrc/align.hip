// align.hip -- spm_hip_hits_align: the begin and the CIGAR transcript of every hit of a scan (what seqan2's findBegin adds
// to a Myers finder).  The kernels are in align.hpp; this file prepares the work list, picks the kernel class of every hit
// and returns the records in both orders.
#include "internal.hpp"
#include "align.hpp"

struct spm_alns
{
    spm_ctx *ctx = nullptr;
    spm_aln *d_recs = nullptr;  // device order
    uint32_t *d_ops = nullptr;
    uint64_t n = 0, n_ops = 0;
    std::vector<spm_aln> host; // host order: (pattern, pos)
    std::vector<uint32_t> host_ops;
    spm_align_stats stats{};
};

namespace
{
// words of a stage-B slot: the band row (2d + 1 diagonals at most) and 2 bits per band cell of rows 1..m
inline uint64_t cigar_slot_words(uint32_t m, int32_t d)
{
    const uint64_t w = 2 * (uint64_t)d + 1;
    return w + ((uint64_t)m * w + 15) / 16;
}

// words of a wave-per-hit stage-B slot: the band row, then two 64-bit ballots per 64 diagonals and row
inline uint64_t wave_slot_words(uint32_t m, int32_t d)
{
    const uint64_t w = 2 * (uint64_t)d + 1;
    return w + (uint64_t)m * ((w + 63) / 64) * 4;
}

constexpr uint64_t kLdsSlotWords = 256;          // 64 slots of at most 1 KiB: 64 KiB per workgroup
constexpr uint64_t kWaveLdsWords = 16384;        // a wave-per-hit slot in LDS: at most 64 KiB per (one-wave) workgroup
constexpr size_t kGlobalBatchBytes = 256u << 20; // scratch of one stage-B launch of the global class

// the set's alignment tables, built once (reversed needles' 64-bit match masks; the needle ranks)
int ensure_align_tables(const spm_patterns *ps)
{
    if (ps->d_align || ps->n == 0)
        return SPM_OK;
    spm_ctx *ctx = ps->ctx;
    const uint32_t sigma = ps->sigma;
    std::vector<uint32_t> off(ps->n + 1, 0);
    for (uint32_t p = 0; p < ps->n; ++p)
        off[p + 1] = off[p] + sigma * (((uint32_t)ps->m[p] + 63) / 64);
    std::vector<uint64_t> rpeq((size_t)off[ps->n] + 1, 0);
    for (uint32_t p = 0; p < ps->n; ++p) {
        const uint32_t m = (uint32_t)ps->m[p], nw = (m + 63) / 64;
        const uint8_t *nd = ps->ranks.data() + ps->offsets[p];
        for (uint32_t i = 0; i < m; ++i) { // bit i of the reversed needle = symbol m - 1 - i
            const uint8_t c = nd[m - 1 - i];
            if (c < sigma)
                rpeq[off[p] + (size_t)c * nw + i / 64] |= 1ull << (i % 64);
        }
    }
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_rpeq = al(rpeq.size() * 8), b_off = al(off.size() * 4), b_ranks = al(ps->ranks.size() + 1);
    const size_t b_offs = al(ps->offsets.size() * 4);
    uint8_t *d = nullptr;
    SPM_HIP_CHECK(ctx, hipMalloc(&d, b_rpeq + b_off + b_ranks + b_offs));
    std::vector<uint8_t> img(b_rpeq + b_off + b_ranks + b_offs, 0);
    memcpy(img.data(), rpeq.data(), rpeq.size() * 8);
    memcpy(img.data() + b_rpeq, off.data(), off.size() * 4);
    if (!ps->ranks.empty())
        memcpy(img.data() + b_rpeq + b_off, ps->ranks.data(), ps->ranks.size());
    memcpy(img.data() + b_rpeq + b_off + b_ranks, ps->offsets.data(), ps->offsets.size() * 4);
    const hipError_t e = hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(d);
        SPM_SET_ERR(ctx, "alignment tables: %s", hipGetErrorString(e));
        return SPM_E_HIP;
    }
    ps->d_align = d;
    ps->d_al_rpeq = reinterpret_cast<const uint64_t *>(d);
    ps->d_al_rpeq_off = reinterpret_cast<const uint32_t *>(d + b_rpeq);
    ps->d_al_ranks = d + b_rpeq + b_off;
    ps->d_al_offsets = reinterpret_cast<const uint32_t *>(d + b_rpeq + b_off + b_ranks);
    return SPM_OK;
}

// stable counting sort of [0, n) by key (key < n_keys)
std::vector<uint32_t> counting_order(const std::vector<uint32_t> &key, uint32_t n_keys)
{
    std::vector<uint64_t> start(n_keys + 1, 0);
    for (uint32_t k : key)
        ++start[k + 1];
    for (uint32_t c = 0; c < n_keys; ++c)
        start[c + 1] += start[c];
    std::vector<uint32_t> ord(key.size());
    for (uint32_t i = 0; i < (uint32_t)key.size(); ++i)
        ord[start[key[i]]++] = i;
    return ord;
}
} // namespace

// the needles' ranks on the device for callers outside this unit (jst_project.hpp)
int spm_align_tables(const spm_patterns *ps) { return ensure_align_tables(ps); }

// The Myers path both entry points share (spm_hip_hits_align; spm_hip_jst_hits_align over a search's segment hits): the
// work list, the kernel class of every hit, stage A and stage B.  Record i of W.d_recs belongs to W.hits[i]; records, pool
// and the error counters come back to the host behind one synchronisation.
int align_run(spm_ctx *ctx, const align_work &W, spm_align_stats &stats)
{
    const spm_patterns *ps = W.ps;
    const uint64_t n = W.n;
    const bool begin_only = W.begin_only;
    const spm_hit *dh = W.hits;
    if (n == 0)
        return SPM_OK;
    int rc = ensure_align_tables(ps);
    if (rc != SPM_OK)
        return rc;
    // ---- the work list: stage-A class = words of the needle (1..4 lane per hit, 5: wave per hit) ----
    const spm_text *text = W.text;
    std::vector<spm_hip::aln_item> items(n);
    std::vector<uint32_t> cls_a(n), cls_b(n);
    for (uint64_t i = 0; i < n; ++i) {
        spm_hip::aln_item &it = items[i];
        const uint64_t e = dh[i].pos - W.pos_offset;
        const uint64_t lo = W.lo[i];
        it.e = e;
        it.lo = lo;
        it.pattern = dh[i].pattern;
        it.d = dh[i].score;
        it.m = (uint32_t)ps->m[dh[i].pattern];
        it.cigar_off = begin_only ? 0 : W.cig_off[i];
        it.rec = (uint32_t)i;
        it.pad = 0;
        if (e > text->n || e < lo || it.d < 0 || (uint32_t)it.d > it.m) {
            SPM_SET_ERR(ctx, "%s: hit %llu (end %llu, distance %d) does not fit its scan", W.who,
                        (unsigned long long)i, (unsigned long long)e, it.d);
            return SPM_E_INVALID;
        }
        const uint32_t nw = std::max(1u, (it.m + 63) / 64);
        cls_a[i] = nw <= 4 ? nw - 1 : 4;
    }
    const std::vector<uint32_t> oa = counting_order(cls_a, 5);
    std::vector<spm_hip::aln_item> items_a(n);
    uint64_t cnt_a[5] = {0, 0, 0, 0, 0};
    for (uint64_t s = 0; s < n; ++s) {
        items_a[s] = items[oa[s]];
        ++cnt_a[cls_a[oa[s]]];
    }
    // stage-B classes over items_a indices: one lane per hit with LDS slots of <= 32, 64, 128, 256 words; beyond that one
    // wave per hit (class 4), its slot in LDS up to kWaveLdsWords, else in the context's scratch
    std::vector<uint64_t> need(n);
    for (uint64_t s = 0; s < n; ++s) {
        need[s] = cigar_slot_words(items_a[s].m, items_a[s].d);
        cls_b[s] = need[s] <= 32 ? 0 : need[s] <= 64 ? 1 : need[s] <= 128 ? 2 : need[s] <= kLdsSlotWords ? 3 : 4;
        if (cls_b[s] == 4)
            need[s] = wave_slot_words(items_a[s].m, items_a[s].d);
    }
    std::vector<uint32_t> ob = counting_order(cls_b, 5);
    uint64_t cnt_b[5] = {0, 0, 0, 0, 0};
    for (uint64_t s = 0; s < n; ++s)
        ++cnt_b[cls_b[s]];
    // the wave class by slot size (launches of like slots)
    const uint64_t g0 = n - cnt_b[4];
    std::stable_sort(ob.begin() + g0, ob.end(), [&](uint32_t x, uint32_t y) { return need[x] < need[y]; });
    uint64_t wave_lds = 0;
    while (g0 + wave_lds < n && need[ob[g0 + wave_lds]] <= kWaveLdsWords)
        ++wave_lds;

    dev_scratch tmp;
    spm_hip::aln_item *d_items = nullptr;
    uint32_t *d_ob = nullptr;
    unsigned long long *d_err = nullptr;
    SPM_HIP_CHECK(ctx, tmp.alloc(&d_items, n * sizeof(spm_hip::aln_item)));
    SPM_HIP_CHECK(ctx, tmp.alloc(&d_ob, n * sizeof(uint32_t)));
    SPM_HIP_CHECK(ctx, tmp.alloc(&d_err, 2 * sizeof(unsigned long long)));
    if (W.n_ops)
        SPM_HIP_CHECK(ctx, hipMemsetAsync(W.d_ops, 0, W.n_ops * 4, ctx->stream));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_items, items_a.data(), n * sizeof(spm_hip::aln_item), hipMemcpyHostToDevice, ctx->stream));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_ob, ob.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(d_err, 0, 2 * sizeof(unsigned long long), ctx->stream));
    // a global-class batch may need the context's scratch: grown now, before the timed launches
    if (!begin_only && g0 + wave_lds < n) {
        rc = ensure_scratch(ctx, std::max<size_t>(kGlobalBatchBytes, need[ob[n - 1]] * 4));
        if (rc != SPM_OK)
            return rc;
    }

    spm_hip::align_params P{};
    P.text = text->d;
    P.rpeq = ps->d_al_rpeq;
    P.rpeq_off = ps->d_al_rpeq_off;
    P.ranks = ps->d_al_ranks;
    P.offsets = ps->d_al_offsets;
    P.sigma = ps->sigma;
    P.pos_offset = W.pos_offset;
    P.recs = W.d_recs;
    P.ops = W.d_ops;
    P.err = d_err;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    struct ev_guard
    {
        hipEvent_t *e;
        ~ev_guard()
        {
            for (int i = 0; i < 3; ++i)
                if (e[i])
                    hipEventDestroy(e[i]);
        }
    } eg{ev};
    for (int i = 0; i < 3; ++i)
        SPM_HIP_CHECK(ctx, hipEventCreate(&ev[i]));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], ctx->stream));
    // ---- stage A ----
    uint64_t s0 = 0;
    for (int c = 0; c < 5; ++c) {
        const uint32_t cn = (uint32_t)cnt_a[c];
        if (cn) {
            const spm_hip::aln_item *it = d_items + s0;
            if (c < 4) {
                const dim3 g((cn + 255) / 256), b(256);
                if (c == 0)
                    hipLaunchKernelGGL(spm_hip::align_begin_lane_kernel<1>, g, b, 0, ctx->stream, P, it, cn);
                else if (c == 1)
                    hipLaunchKernelGGL(spm_hip::align_begin_lane_kernel<2>, g, b, 0, ctx->stream, P, it, cn);
                else if (c == 2)
                    hipLaunchKernelGGL(spm_hip::align_begin_lane_kernel<3>, g, b, 0, ctx->stream, P, it, cn);
                else
                    hipLaunchKernelGGL(spm_hip::align_begin_lane_kernel<4>, g, b, 0, ctx->stream, P, it, cn);
            } else {
                hipLaunchKernelGGL(spm_hip::align_begin_wave_kernel, dim3((cn + 3) / 4), dim3(256), 0, ctx->stream, P, it, cn);
            }
            SPM_HIP_CHECK(ctx, hipGetLastError());
        }
        s0 += cnt_a[c];
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], ctx->stream));
    // ---- stage B ----
    if (!begin_only) {
        uint64_t b0 = 0;
        for (int c = 0; c < 4; ++c) {
            const uint32_t cn = (uint32_t)cnt_b[c];
            if (cn) {
                const size_t lds = (size_t)kWave * 4 * (32u << c);
                hipLaunchKernelGGL(spm_hip::align_cigar_kernel, dim3((cn + 63) / 64), dim3(64), lds, ctx->stream, P,
                                   d_items, d_ob + b0, cn);
                SPM_HIP_CHECK(ctx, hipGetLastError());
            }
            b0 += cnt_b[c];
        }
        // the wave class: LDS launches of slots up to the next power of two, then scratch batches within its size
        for (uint64_t s = g0; s < g0 + wave_lds;) {
            uint64_t cap_w = 1024;
            while (cap_w < need[ob[s]])
                cap_w <<= 1;
            cap_w = std::min<uint64_t>(cap_w, kWaveLdsWords);
            uint64_t z = s;
            while (z < g0 + wave_lds && need[ob[z]] <= cap_w)
                ++z;
            const uint32_t cn = (uint32_t)(z - s);
            hipLaunchKernelGGL(spm_hip::align_cigar_wave_kernel<true>, dim3(cn), dim3(64), cap_w * 4, ctx->stream, P, d_items,
                               d_ob + s, cn, nullptr, (uint64_t)0);
            SPM_HIP_CHECK(ctx, hipGetLastError());
            s = z;
        }
        const uint64_t budget_words = ctx->scratch_bytes / 4;
        for (uint64_t s = g0 + wave_lds; s < n;) {
            uint64_t z = s + 1;
            while (z < n && (z + 1 - s) * need[ob[z]] <= budget_words)
                ++z;
            const uint32_t cn = (uint32_t)(z - s);
            hipLaunchKernelGGL(spm_hip::align_cigar_wave_kernel<false>, dim3(cn), dim3(64), 0, ctx->stream, P, d_items,
                               d_ob + s, cn, static_cast<uint32_t *>(ctx->d_scratch), need[ob[z - 1]]);
            SPM_HIP_CHECK(ctx, hipGetLastError());
            s = z;
        }
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], ctx->stream));
    unsigned long long err[2] = {0, 0};
    if (W.h_recs)
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(W.h_recs, W.d_recs, n * sizeof(spm_aln), hipMemcpyDeviceToHost, ctx->stream));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, ctx->stream));
    if (W.n_ops && W.h_ops)
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(W.h_ops, W.d_ops, W.n_ops * 4, hipMemcpyDeviceToHost, ctx->stream));
    SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (err[0] || err[1]) {
        SPM_SET_ERR(ctx, "%s: %llu begins not found, %llu transcripts failed their check (hits that do not "
                         "belong to this text?)", W.who, err[0], err[1]);
        return SPM_E_INVALID;
    }
    hipEventElapsedTime(&stats.ms_total, ev[0], ev[2]);
    hipEventElapsedTime(&stats.ms_begin, ev[0], ev[1]);
    hipEventElapsedTime(&stats.ms_cigar, ev[1], ev[2]);
    stats.begin_lane = (uint32_t)(n - cnt_a[4]);
    stats.begin_wave = (uint32_t)cnt_a[4];
    if (!begin_only) {
        stats.cigar_lane = (uint32_t)(n - cnt_b[4]);
        stats.cigar_wave = (uint32_t)wave_lds;
        stats.cigar_wave_global = (uint32_t)(cnt_b[4] - wave_lds);
    }
    return SPM_OK;
}

extern "C" int spm_hip_hits_align(spm_hits *h, uint32_t flags, spm_alns **out)
{
    if (!h || !out || (flags & ~SPM_ALIGN_BEGIN_ONLY))
        return SPM_E_INVALID;
    spm_ctx *ctx = h->ctx;
    const auto t_call = clk::now();
    const spm_patterns *ps = h->al_patterns;
    if (h->sel_records) {
        SPM_SET_ERR(ctx, "spm_hip_hits_align: a selection of raw records (spm_hip_records_select) carries no text to align against");
        return SPM_E_INVALID;
    }
    if (!ps || !h->al_text) {
        SPM_SET_ERR(ctx, "spm_hip_hits_align: these hits do not come from spm_hip_scan / spm_hip_scan_segments");
        return SPM_E_UNSUPPORTED;
    }
    if (ps->algo == SPM_ALGO_MYERS_PREFIX) {
        SPM_SET_ERR(ctx, "spm_hip_hits_align: hits of a MYERS_PREFIX set cannot be aligned (not supported)");
        return SPM_E_UNSUPPORTED;
    }
    if (h->al_stateful) {
        SPM_SET_ERR(ctx, "spm_hip_hits_align: hits of a stateful scan (state_in != NULL) cannot be aligned (not supported)");
        return SPM_E_UNSUPPORTED;
    }
    if (h->al_device_segs) {
        SPM_SET_ERR(ctx, "spm_hip_hits_align: hits of a journaled-sequence search cannot be aligned (not supported)");
        return SPM_E_UNSUPPORTED;
    }
    const void *d_hits = nullptr;
    uint64_t n = 0;
    int rc = spm_hip_hits_device(h, &d_hits, &n); // (completes a deferred scan; SPM_E_OVERFLOW for an overflowed one)
    if (rc != SPM_OK)
        return rc;
    if (n > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_hits_align: more than 2^32 - 1 hits");
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_alns, void (*)(spm_alns *)> A(new spm_alns, spm_hip_alns_destroy);
    A->ctx = ctx;
    A->n = n;
    const bool begin_only = (flags & SPM_ALIGN_BEGIN_ONLY) != 0;

    // the hits in device order, and the host order (pattern, pos) of spm_hip_hits_view: by pattern (stable), then by pos
    std::vector<spm_hit> dh(n);
    if (n) {
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(dh.data(), d_hits, n * sizeof(spm_hit), hipMemcpyDeviceToHost, ctx->stream));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    std::vector<uint32_t> pat_key(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (dh[i].pattern >= ps->n) {
            SPM_SET_ERR(ctx, "spm_hip_hits_align: hit of pattern %u outside the set", dh[i].pattern);
            return SPM_E_INVALID;
        }
        pat_key[i] = dh[i].pattern;
    }
    std::vector<uint32_t> horder = counting_order(pat_key, std::max(1u, ps->n));
    for (uint64_t a = 0; a < n;) {
        uint64_t z = a;
        while (z < n && dh[horder[z]].pattern == dh[horder[a]].pattern)
            ++z;
        std::sort(horder.begin() + a, horder.begin() + z,
                  [&](uint32_t x, uint32_t y) { return (int64_t)dh[x].pos < (int64_t)dh[y].pos; });
        a = z;
    }
    // CIGAR offsets: exclusive prefix sum of 2 score + 1 in host order (the bound on the runs of a cost-score transcript)
    std::vector<uint32_t> cig_off(n, 0);
    uint64_t total_ops = 0;
    for (uint64_t s = 0; s < n; ++s) {
        const spm_hit &x = dh[horder[s]];
        cig_off[horder[s]] = (uint32_t)total_ops;
        total_ops += ps->is_myers() ? 2 * (uint64_t)std::max(0, x.score) + 1 : 1;
    }
    if (total_ops > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_hits_align: the CIGAR pool would exceed 2^32 words");
        return SPM_E_UNSUPPORTED;
    }
    A->n_ops = begin_only ? 0 : total_ops;
    std::vector<spm_aln> drec(n);

    if (n && !ps->is_myers()) {
        // exact sets: nothing to compute
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t m = (uint32_t)ps->m[dh[i].pattern];
            drec[i] = spm_aln{dh[i].pos, dh[i].pos + m, dh[i].pattern, dh[i].score, begin_only ? 0u : cig_off[i], begin_only ? 0u : 1u};
        }
        if (!begin_only) {
            A->host_ops.resize(total_ops);
            for (uint64_t i = 0; i < n; ++i)
                A->host_ops[cig_off[i]] = ((uint32_t)ps->m[dh[i].pattern] << 4) | SPM_CIGAR_EQ;
        }
        SPM_HIP_CHECK(ctx, hipMalloc(&A->d_recs, n * sizeof(spm_aln)));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(A->d_recs, drec.data(), n * sizeof(spm_aln), hipMemcpyHostToDevice, ctx->stream));
        if (A->n_ops) {
            SPM_HIP_CHECK(ctx, hipMalloc(&A->d_ops, A->n_ops * 4));
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(A->d_ops, A->host_ops.data(), A->n_ops * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    } else if (n) {
        std::vector<uint64_t> lo(n, h->al_lo);
        if (!h->al_segs.empty()) { // the segment holding the hit's last symbol
            const uint64_t *segs = h->al_segs.data();
            const uint64_t n_segs = h->al_segs.size() - 1;
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t e = dh[i].pos - h->al_pos_offset;
                const uint64_t *u = std::upper_bound(segs, segs + n_segs + 1, e ? e - 1 : 0);
                lo[i] = u == segs ? segs[0] : *(u - 1);
            }
        }
        SPM_HIP_CHECK(ctx, hipMalloc(&A->d_recs, n * sizeof(spm_aln)));
        if (A->n_ops)
            SPM_HIP_CHECK(ctx, hipMalloc(&A->d_ops, A->n_ops * 4));
        A->host_ops.resize(A->n_ops);
        align_work W{};
        W.ps = ps;
        W.text = h->al_text;
        W.pos_offset = h->al_pos_offset;
        W.hits = dh.data();
        W.n = n;
        W.lo = lo.data();
        W.cig_off = cig_off.data();
        W.begin_only = begin_only;
        W.d_recs = A->d_recs;
        W.d_ops = A->d_ops;
        W.n_ops = A->n_ops;
        W.h_recs = drec.data();
        W.h_ops = A->host_ops.data();
        W.who = "spm_hip_hits_align";
        rc = align_run(ctx, W, A->stats);
        if (rc != SPM_OK)
            return rc;
    }
    A->host.resize(n);
    for (uint64_t s = 0; s < n; ++s)
        A->host[s] = drec[horder[s]];
    A->stats.n_alns = n;
    A->stats.n_ops = A->n_ops;
    A->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] align %llu hits%s: %.3f ms device (begins %.3f, transcripts %.3f), %.3f ms in all\n",
                (unsigned long long)n, begin_only ? " (begins only)" : "", A->stats.ms_total, A->stats.ms_begin,
                A->stats.ms_cigar, A->stats.ms_host);
    *out = A.release();
    return SPM_OK;
}

extern "C" int spm_hip_alns_view(spm_alns *a, const spm_aln **records, uint64_t *n, const uint32_t **ops, uint64_t *n_ops)
{
    if (!a)
        return SPM_E_INVALID;
    return pool_out(pool_src<spm_aln>{a->host.data(), a->n, a->host_ops.data(), a->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_alns_device(spm_alns *a, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops)
{
    if (!a)
        return SPM_E_INVALID;
    return pool_out(pool_src<void, void, void>{a->d_recs, a->n, a->d_ops, a->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_alns_stats(const spm_alns *a, spm_align_stats *out)
{
    if (!a || !out)
        return SPM_E_INVALID;
    *out = a->stats;
    return SPM_OK;
}

extern "C" void spm_hip_alns_destroy(spm_alns *a)
{
    if (!a)
        return;
    if (a->ctx && (a->d_recs || a->d_ops))
        hipStreamSynchronize(a->ctx->stream);
    hipFree(a->d_recs);
    hipFree(a->d_ops);
    delete a;
}

void spm_warm_align_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::align_begin_lane_kernel<1>);
}
