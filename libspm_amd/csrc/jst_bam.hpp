// jst_bam.hpp -- BAM records in BGZF blocks (spm_hip_jst_ref_loci_bam; contract in spm_hip.h, scheme in DESIGN.md 4.12, the
// composition in jst_bam_core.hpp).  gfx950.  Unit: jst_sam.hip, with jst_sam.hpp, whose front (the host's refusals, the lines
// stage), measured and closed steps, stats kernel and wave sink base it uses; the file around its record stream is bam_file's
// (output_handles.hpp), which enqueues the frame stage of bgzf.hip (internal.hpp).
//   jst_bam_measure_kernel   one lane per record: resolved against its sources with the query length checked, its shape (item
//                            count, bin; what a record cannot hold is counted as a disagreement), its length by the measuring
//                            sink;
//   jst_bam_write_kernel     one wave per record, four records per workgroup, into the uncompressed stream: the 36 fixed bytes
//                            one per lane, name bytes strided, CIGAR one word per lane through wave_cigar_walk (the text sink's
//                            scheme, the items' size counted in words), SEQ two ranks per lane and byte, QUAL a fill or,
//                            with spm_sam_extras, one value per lane; a tag seven lanes, MD (type Z) the text sink's walk
//                            between its three head bytes and a NUL.  Byte stores: a record starts wherever the one before
//                            it ended.  No atomics.
#pragma once

#include "bgzf_core.hpp"
#include "jst_bam_core.hpp"
#include "jst_sam.hpp"

namespace spm_hip
{

struct jst_bam_params
{
    jst_sam_params P;               // text, n_bytes: the record stream
    const uint8_t *codes = nullptr; // [256] rank -> 4-bit code
    uint32_t *shape = nullptr;      // [cap_lines] n_items | bin << 16
    uint64_t ref_len = 0;
};

__global__ __launch_bounds__(256) void jst_bam_measure_kernel(const jst_bam_params B)
{
    const jst_sam_params &P = B.P;
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    const unsigned long long n_lines = P.counts[kSamCntLines]; // (the lines stage is complete: stream order)
    bool bad = false;
    uint64_t n = 0;
    if (i < P.cap_lines) {
        jst_bam_shape H;
        if (i < n_lines) {
            jst_sam_fields F;
            bad = !jst_sam_resolve(P.S, P.lines[i], P.aux[i], F, true) || !jst_bam_shape_of(P.S, F, B.ref_len, H);
            if (!bad) {
                jst_bam_measure M;
                jst_bam_compose(P.S, F, H, B.codes, 0, M);
                n = M.n;
                bad = n > 0x7FFFFFFFull; // (block_size is an int32)
            }
            n = bad ? 0 : n;
        }
        P.len[i] = (uint32_t)n;
        B.shape[i] = H.n_items | H.bin << 16;
    }
    count_flagged(&P.counts[kSamCntBad], bad);
    wave_count_add(&P.counts[kSamCntBytes], (unsigned long long)n);
}

// The wave sink: the composition of one record, over what it shares with the text's (jst_wave_sink_base).
struct jst_bam_wave_sink : jst_wave_sink_base<uint8_t>
{
    __device__ __forceinline__ void fixed(const uint32_t *w)
    {
        if (lane < kBamFixed)
            store(cur + lane, jst_bam_le_byte(w[lane >> 2], lane & 3));
        cur += kBamFixed;
    }
    __device__ __forceinline__ void num(uint64_t v) // at most 20 digits
    {
        const uint32_t len = jst_sam_dec_len(v);
        if (lane < len)
            store(cur + lane, (uint8_t)jst_sam_dec_char(v, len, lane));
        cur += len;
    }
    __device__ __forceinline__ void fill(uint8_t c, uint64_t n)
    {
        for (uint64_t i = lane; i < n; i += kWave)
            store(cur + i, c);
        cur += n;
    }
    __device__ __forceinline__ void cigar(const uint32_t *words, uint32_t n, bool merge)
    {
        const uint64_t begin = cur;
        cur = begin + 4 * wave_cigar_walk(
                              words, n, merge, lane, [](uint64_t, uint32_t) { return 1u; },
                              [&](uint64_t at, uint64_t run, uint32_t word, uint32_t) {
                                  const uint32_t item = jst_bam_item_word(run, word, merge);
                                  for (uint32_t i = 0; i < 4; ++i)
                                      store(begin + 4 * at + i, jst_bam_le_byte(item, i));
                              });
    }
    __device__ __forceinline__ void seq(const uint8_t *ranks, uint32_t m, const uint8_t *codes)
    {
        const uint32_t n = jst_bam_seq_len(m);
        for (uint32_t i = lane; i < n; i += kWave)
            store(cur + i, jst_bam_seq_byte(ranks, m, codes, i));
        cur += n;
    }
    __device__ __forceinline__ void tag(uint32_t head, uint32_t v)
    {
        if (lane < kBamTag)
            store(cur + lane, jst_bam_tag_byte(head, v, lane));
        cur += kBamTag;
    }
    // MD Z, the text sink's string by the same walk, NUL
    __device__ __forceinline__ void md(const uint32_t *words, uint32_t n, const uint8_t *ref, const char *symbols, uint32_t sigma)
    {
        if (lane < 3)
            store(cur + lane, jst_bam_le_byte(jst_bam_tag_head('M', 'D', 'Z'), lane));
        num(md_words(cur + 3, words, n, ref, symbols, sigma));
        fill(0, 1);
    }
};

__global__ __launch_bounds__(256) void jst_bam_write_kernel(const jst_bam_params B)
{
    const jst_sam_params &P = B.P;
    const uint32_t wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const unsigned long long i = blockIdx.x * 4ull + wv;
    if (i >= P.n_lines)
        return; // (whole waves: i is uniform across the wave, and no workgroup barrier follows)
    jst_sam_fields F;
    if (!jst_sam_resolve(P.S, P.lines[i], P.aux[i], F, false))
        return; // (the measure stage resolved this record and counted a failure: the host does not get here)
    const uint32_t len = P.len[i], shape = B.shape[i];
    if (len < 4)
        return;
    jst_bam_shape H;
    H.n_items = shape & 0xFFFFu;
    H.bin = shape >> 16;
    const uint64_t begin = P.off64[i], end = begin + len;
    jst_bam_wave_sink out{{reinterpret_cast<uint8_t *>(P.text), begin, end < P.n_bytes ? end : P.n_bytes, lane}};
    jst_bam_compose(P.S, F, H, B.codes, len - 4, out);
}

} // namespace spm_hip

extern "C" void spm_hip_bam_destroy(spm_bam *b)
{
    if (b)
        spm_hip::handle_destroy(b, {b->d_file, b->d_records, b->d_lines});
}

// the plain header: BAM\1, l_text, the text of spm_hip_sam_header (sorted: of spm_hip_sam_header_sorted), n_ref = 1, l_name, the
// name with its NUL, l_ref
int bam_plain_header(const char *who, spm_ctx *ctx, const char *rname, uint64_t ref_len, bool sorted, std::vector<uint8_t> &h)
{
    const auto text = sorted ? spm_hip_sam_header_sorted : spm_hip_sam_header;
    if (ref_len == 0) {
        SPM_SET_ERR(ctx, "%s: ref_len is 0", who);
        return SPM_E_INVALID;
    }
    if (ref_len > spm_hip::kBamMaxRefLen) {
        SPM_SET_ERR(ctx, "%s: ref_len %llu is above 2^31 - 1, the longest reference a BAM record can name (not supported)", who,
                    (unsigned long long)ref_len);
        return SPM_E_UNSUPPORTED;
    }
    uint64_t n_text = 0;
    int rc = text(rname, ref_len, nullptr, 0, &n_text);
    if (rc != SPM_E_OVERFLOW) {
        if (ctx && rc == SPM_E_INVALID)
            SPM_SET_ERR(ctx, "%s: rname %s", who, kSamNameRule);
        return rc == SPM_OK ? SPM_E_INVALID : rc;
    }
    const uint32_t l_name = (uint32_t)strlen(rname) + 1;
    h.assign(4 + 4 + n_text + 4 + 4 + l_name + 4, 0);
    auto put32 = [&h](size_t at, uint32_t v) {
        for (int i = 0; i < 4; ++i)
            h[at + i] = (uint8_t)(v >> (8 * i));
    };
    memcpy(h.data(), "BAM\1", 4);
    put32(4, (uint32_t)n_text);
    SPM_TRY(text(rname, ref_len, reinterpret_cast<char *>(h.data()) + 8, n_text, &n_text));
    put32(8 + n_text, 1);
    put32(12 + n_text, l_name);
    memcpy(h.data() + 16 + n_text, rname, l_name - 1);
    put32(16 + n_text + l_name, (uint32_t)ref_len);
    return SPM_OK;
}

static int bam_check_block_data(const char *who, spm_ctx *ctx, uint32_t block_data)
{
    if (block_data <= spm_hip::kBgzfBlockData)
        return SPM_OK;
    SPM_SET_ERR(ctx, "%s: block_data %u above 65280", who, block_data);
    return SPM_E_INVALID;
}

static int bam_header_framed(const char *who, bool sorted, const char *rname, uint64_t ref_len, uint32_t block_data, void *buf, uint64_t cap,
                             uint64_t *len)
{
    if (!rname || !len || (!buf && cap)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL %s", who, !rname ? "rname" : !len ? "len" : "buf with cap > 0");
        return SPM_E_INVALID;
    }
    SPM_TRY(bam_check_block_data(who, nullptr, block_data));
    std::vector<uint8_t> plain;
    SPM_TRY(bam_plain_header(who, nullptr, rname, ref_len, sorted, plain));
    const spm_bgzf_opts o{block_data, 0, 0};
    return spm_hip_bgzf_frame_host(plain.data(), plain.size(), &o, buf, cap, len);
}

extern "C" int spm_hip_bam_header(const char *rname, uint64_t ref_len, uint32_t block_data, void *buf, uint64_t cap, uint64_t *len)
{
    return bam_header_framed("spm_hip_bam_header", false, rname, ref_len, block_data, buf, cap, len);
}

extern "C" int spm_hip_bam_header_sorted(const char *rname, uint64_t ref_len, uint32_t block_data, void *buf, uint64_t cap, uint64_t *len)
{
    return bam_header_framed("spm_hip_bam_header_sorted", true, rname, ref_len, block_data, buf, cap, len);
}

static int bam_run(const char *who, spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs, const spm_patterns *ps,
                   const spm_bam_opts *opts, const spm_sam_extras *ex, spm_bam **out)
{
    using namespace spm_hip;
    if (!l || !out)
        return SPM_E_INVALID;
    *out = nullptr;
    spm_ctx *ctx = l->ctx;
    const auto t_call = clk::now();
    if (!opts) {
        SPM_SET_ERR(ctx, "%s: NULL opts", who);
        return SPM_E_INVALID;
    }
    size_t rname_len = 0;
    uint64_t n_named = 0;
    SPM_TRY(sam_check_args(who, ctx, l, r, pr, rs, ps, &opts->sam, rname_len, n_named));
    if (ex)
        SPM_TRY(sam_check_extras(who, ctx, r, ps, ex, &opts->ref_len));
    SPM_TRY(bam_check_block_data(who, ctx, opts->block_data));
    if (opts->reserved) {
        SPM_SET_ERR(ctx, "%s: reserved is %u (must be 0)", who, opts->reserved);
        return SPM_E_INVALID;
    }
    const uint32_t D = bgzf_block_data(opts->block_data);
    bam_file file;
    bam_ptr R(nullptr, spm_hip_bam_destroy);
    SPM_TRY(file.open(who, ctx, opts->sam.rname, opts->ref_len, D, false, R));
    hipStream_t st = ctx->stream;
    const uint32_t n_reads = (uint32_t)r->n;
    sam_front F;
    hip_events<8> &ev = F.ev;
    jst_bam_params B;
    jst_sam_params &P = B.P; // (no reads: no lines and no bytes)
    uint8_t codes[256];
    dev_scratch keep;
    if (n_reads) {
        SPM_TRY(sam_lines_stage(who, ctx, l, r, pr, rs, ps, &opts->sam, ex, rname_len, n_named, F, &R->d_lines));
        P = F.P;
        // ---- measure (its time, ev[1] .. ev[2], takes in the two allocations and the 256-byte upload below) ----
        jst_bam_rank_codes(opts->sam.symbols, ps->sigma, codes);
        uint8_t *d_codes = nullptr;
        SPM_HIP_CHECK(ctx, keep.alloc(&d_codes, 256));
        SPM_HIP_CHECK(ctx, keep.alloc(&B.shape, (size_t)P.cap_lines * 4));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_codes, codes, 256, hipMemcpyHostToDevice, st));
        B.codes = d_codes;
        B.ref_len = opts->ref_len;
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_bam_measure_kernel, P.cap_lines, B));
        SPM_TRY(sam_measured(who, ctx, F, P, ", ref_len or the reference of the extras, or do not fit a BAM record"));
    }
    const uint64_t n_records = P.n_bytes;
    SPM_TRY(bgzf_check_n_blocks(who, ctx, n_records, D, "record bytes"));
    SPM_TRY(file.place(R.get(), P.n_lines, n_records));
    hip_events<2> ev_frame;
    SPM_HIP_CHECK(ctx, ev_frame.create());
    if (n_reads) {
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_records, std::max<uint64_t>(n_records, 1)));
        P.text = reinterpret_cast<char *>(R->d_records);
        // ---- write ----
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
        hipLaunchKernelGGL(jst_bam_write_kernel, dim3((P.n_lines + 3) / 4), dim3(256), 0, st, B);
        SPM_HIP_CHECK(ctx, hipGetLastError());
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
    }
    // ---- frame ----
    SPM_HIP_CHECK(ctx, hipEventRecord(ev_frame[0], st));
    SPM_TRY(file.frame(R.get()));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev_frame[1], st));
    if (n_reads) {
        // ---- stats ----
        SPM_TRY(sam_closed(ctx, F, P, ev_frame[1], R->stats));
        R->stats.n_records = P.n_lines;
    } else {
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st)); // (header and EOF are in place; the file's header goes out of scope)
    }
    hipEventElapsedTime(&R->stats.ms_frame, ev_frame[0], ev_frame[1]);
    R->stats.ms_total = R->stats.ms_lines + R->stats.ms_measure + R->stats.ms_write + R->stats.ms_frame + R->stats.ms_stats;
    R->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst bam: %u reads -> %llu records (%llu reported, %llu of them rescues, %llu secondary, %llu unmapped), "
                        "%llu bytes in %llu blocks, file %llu bytes: device %.3f ms (lines %.3f, measure %.3f, write %.3f, frame %.3f, "
                        "stats %.3f), %.3f ms in all\n", n_reads, (unsigned long long)R->stats.n_records,
                (unsigned long long)R->stats.n_reported, (unsigned long long)R->stats.n_rescue_lines, (unsigned long long)R->stats.n_secondary,
                (unsigned long long)R->stats.n_unmapped, (unsigned long long)n_records, (unsigned long long)R->stats.n_record_blocks,
                (unsigned long long)R->n_file, R->stats.ms_total, R->stats.ms_lines, R->stats.ms_measure, R->stats.ms_write,
                R->stats.ms_frame, R->stats.ms_stats, R->stats.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_ref_loci_bam(spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs,
                                        const spm_patterns *ps, const spm_bam_opts *opts, spm_bam **out)
{
    return bam_run("spm_hip_jst_ref_loci_bam", l, r, pr, rs, ps, opts, nullptr, out);
}

extern "C" int spm_hip_jst_ref_loci_bam_ex(spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs,
                                           const spm_patterns *ps, const spm_bam_opts *opts, const spm_sam_extras *ex, spm_bam **out)
{
    return bam_run("spm_hip_jst_ref_loci_bam_ex", l, r, pr, rs, ps, opts, ex, out);
}

extern "C" int spm_hip_bam_view(spm_bam *b, const void **file, uint64_t *n_file, const void **records, uint64_t *n_record_bytes,
                                const spm_sam_line **lines, uint64_t *n_lines)
{
    using namespace spm_hip;
    if (!b)
        return SPM_E_INVALID;
    SPM_TRY(handle_download(b->ctx, b->have_host, view_part{b->d_file, b->n_file, b->host_file},
                            view_part{b->d_records, b->n_record_bytes, b->host_records}, view_part{b->d_lines, b->n_lines, b->host_lines}));
    out_if(file, b->host_file.data());
    out_if(n_file, b->n_file);
    out_if(records, b->host_records.data());
    out_if(n_record_bytes, b->n_record_bytes);
    out_if(lines, b->host_lines.data());
    out_if(n_lines, b->n_lines);
    return SPM_OK;
}

extern "C" int spm_hip_bam_device(spm_bam *b, const void **file, uint64_t *n_file, const void **records, uint64_t *n_record_bytes,
                                  const void **lines, uint64_t *n_lines)
{
    using namespace spm_hip;
    if (!b)
        return SPM_E_INVALID;
    out_if(file, b->d_file);
    out_if(n_file, b->n_file);
    out_if(records, b->d_records);
    out_if(n_record_bytes, b->n_record_bytes);
    out_if(lines, b->d_lines);
    out_if(n_lines, b->n_lines);
    return SPM_OK;
}

extern "C" int spm_hip_bam_stats(const spm_bam *b, spm_bam_stats *out) { return spm_hip::stats_out(b ? &b->stats : nullptr, out); }
