// output_handles.hpp -- the result handles of the output stage, and what their C accessors do, written once:
//   spm_sam    jst_sam.hpp                          SAM text and its line records
//   spm_bam    jst_bam.hpp, bam_index.hpp (sort),   a BAM file, its record stream and line records; read by bam_index.hpp
//              bam_markdup.hpp (markdup)            (sort, index), bam_markdup.hpp and bgzf.hip (spm_hip_bam_deflate)
//   spm_bgzf   bgzf.hip                             framed or deflated blocks and their offsets; read by bam_index.hpp (index)
//   spm_bai    bam_index.hpp                        the bytes of a BAI index
//   spm_pileup, spm_pileup_sites   bam_pileup.hpp   the eight count planes of a region; the site records compacted from them
//   spm_vcf    pileup_vcf.hpp                       the VCF text of a site array and one call record per site
// Behind them: the lazy download of a handle's host view, the synchronise-and-free of its device buffers, the copy-out of
// optional out-parameters and of a stats struct; the BAM file around a record stream that spm_hip_jst_ref_loci_bam,
// spm_hip_bam_sort and spm_hip_bam_markdup make; the refusal both BGZF calls and the BAM call word alike.  Host code only: no kernel, no C-ABI
// definition.
#pragma once

#include <cstddef>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "bgzf_core.hpp"

struct spm_sam
{
    spm_ctx *ctx = nullptr;
    char *d_text = nullptr;
    spm_sam_line *d_lines = nullptr;
    uint64_t n_bytes = 0, n_lines = 0;
    bool have_host = false; // the views are downloaded when first asked for
    std::vector<char> host_text;
    std::vector<spm_sam_line> host_lines;
    spm_sam_stats stats{};
};
static_assert(sizeof(spm_sam_opts) == 64 && sizeof(spm_sam_line) == 24 && sizeof(spm_sam_stats) == 72, "spm_hip.h states these sizes");

struct spm_bam
{
    spm_ctx *ctx = nullptr;
    uint8_t *d_file = nullptr, *d_records = nullptr;
    spm_sam_line *d_lines = nullptr;
    uint64_t n_file = 0, n_record_bytes = 0, n_lines = 0;
    bool have_host = false; // the views are downloaded when first asked for
    std::vector<uint8_t> host_file, host_records;
    std::vector<spm_sam_line> host_lines;
    std::vector<uint8_t> plain_header; // the header section before its framing: what spm_hip_bam_deflate compresses again
    spm_bam_stats stats{};
    // what spm_hip_bam_sort writes the new header section from, and spm_hip_bam_index the stored blocks' offsets (bam_index.hpp)
    std::string rname;
    uint64_t ref_len = 0;
    uint32_t block_data = 0; // uncompressed bytes of a full block: never 0
    bool sorted = false;     // made by spm_hip_bam_sort, which then filled sort_stats
    spm_bam_sort_stats sort_stats{};
    bool marked = false;     // made by spm_hip_bam_markdup (bam_markdup.hpp), which then filled markdup_stats
    spm_bam_markdup_stats markdup_stats{};
};
static_assert(sizeof(spm_bam_opts) == 80 && sizeof(spm_bam_stats) == 104, "spm_hip.h states these sizes");
static_assert(sizeof(spm_bam_sort_opts) == 8 && sizeof(spm_bam_sort_stats) == 48, "spm_hip.h states these sizes");
static_assert(sizeof(spm_bam_markdup_opts) == 16 && sizeof(spm_bam_markdup_stats) == 88, "spm_hip.h states these sizes");

struct spm_bgzf
{
    spm_ctx *ctx = nullptr;
    uint8_t *d = nullptr;
    uint64_t n = 0;
    bool have_host = false; // the view is downloaded when first asked for
    std::vector<uint8_t> host;
    spm_bgzf_stats stats{};
    // the blocks' file offsets (spm_hip_bgzf_blocks): n_blocks + 1 of them.  A deflated handle has them on the device from the
    // call on (inside d_offsets_alloc); a framed one makes them from the closed form when first asked for
    uint32_t D = spm_hip::kBgzfBlockData;
    void *d_offsets_alloc = nullptr;
    unsigned long long *d_offsets = nullptr;
    bool have_host_offsets = false;
    std::vector<uint64_t> host_offsets;
    spm_bgzf_deflate_stats deflate{};
    uint64_t n_dynamic_blocks = 0; // spm_hip_bgzf_block_types: of the blocks that are not stored, those with a code of their own
};
static_assert(sizeof(spm_bgzf_opts) == 16 && sizeof(spm_bgzf_stats) == 32, "spm_hip.h states these sizes");
static_assert(sizeof(spm_bgzf_deflate_opts) == 16 && sizeof(spm_bgzf_deflate_stats) == 72, "spm_hip.h states these sizes");

struct spm_bai
{
    spm_ctx *ctx = nullptr;
    uint8_t *d = nullptr;
    uint64_t n = 0;
    bool have_host = false; // the view is downloaded when first asked for
    std::vector<uint8_t> host;
    spm_bai_stats stats{};
};
static_assert(sizeof(spm_bai_stats) == 80, "spm_hip.h states this size");

struct spm_pileup
{
    spm_ctx *ctx = nullptr;
    uint32_t *d = nullptr; // [8 * n] plane-major
    uint64_t begin = 0, n = 0;
    bool have_host = false; // the view is downloaded when first asked for
    std::vector<uint32_t> host;
    spm_pileup_stats stats{};
};
struct spm_pileup_sites
{
    spm_ctx *ctx = nullptr;
    spm_pileup_site *d = nullptr; // [n]
    uint64_t n = 0;
    bool have_host = false; // the view is downloaded when first asked for
    std::vector<spm_pileup_site> host;
};
static_assert(sizeof(spm_pileup_opts) == 32 && sizeof(spm_pileup_stats) == 88, "spm_hip.h states these sizes");
static_assert(sizeof(spm_pileup_site) == 32 && sizeof(spm_pileup_site_opts) == 16, "spm_hip.h states these sizes");

struct spm_vcf
{
    spm_ctx *ctx = nullptr;
    char *d_text = nullptr;
    spm_variant_call *d_calls = nullptr;
    uint64_t n_bytes = 0, n_calls = 0;
    bool have_host = false; // the views are downloaded when first asked for
    std::vector<char> host_text;
    std::vector<spm_variant_call> host_calls;
    spm_vcf_stats stats{};
};
static_assert(sizeof(spm_vcf_opts) == 40 && sizeof(spm_variant_call) == 32 && sizeof(spm_vcf_stats) == 80, "spm_hip.h states these sizes");
static_assert(offsetof(spm_variant_call, len) == 12 && offsetof(spm_variant_call, offset) == 16 && offsetof(spm_variant_call, status) == 24 &&
                  offsetof(spm_variant_call, gt) == 26 && offsetof(spm_variant_call, n_alt) == 28 && offsetof(spm_variant_call, alt) == 29,
              "spm_hip.h states this layout");

#pragma GCC visibility push(hidden) // (inline code of the library's own units, not part of its surface)
namespace spm_hip
{

// ---- what the _view, _device, _stats and _destroy entry points of these handles do ----
// one part of a host view: n items at d, downloaded into `host`
template <class T> struct view_part
{
    const T *d;
    uint64_t n;
    std::vector<T> &host;
};
template <class T> view_part(T *, uint64_t, std::vector<T> &) -> view_part<T>;

// The parts downloaded behind the work of the context's stream, the first time a view is asked for; a handle whose parts are
// all empty touches neither device nor stream.
template <class... T> int handle_download(spm_ctx *ctx, bool &have_host, view_part<T>... part)
{
    if (!have_host && ((part.n != 0) || ...)) {
        SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        (part.host.resize(part.n), ...); // (every page touched before the first copy is in flight)
        hipError_t e = hipSuccess;
        auto fetch = [&](auto &p) {
            if (p.n && e == hipSuccess)
                e = hipMemcpyAsync(p.host.data(), p.d, p.n * sizeof(*p.d), hipMemcpyDeviceToHost, ctx->stream);
        };
        (fetch(part), ...);
        SPM_HIP_CHECK(ctx, e);
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    have_host = true;
    return SPM_OK;
}

// h is not null.  Work of the context's stream may still read the buffers.
template <class Handle> void handle_destroy(Handle *h, std::initializer_list<void *> bufs)
{
    bool any = false;
    for (void *p : bufs)
        any = any || p;
    if (h->ctx && any)
        hipStreamSynchronize(h->ctx->stream);
    for (void *p : bufs)
        hipFree(p);
    delete h;
}

template <class P, class V> void out_if(P *out, const V &v)
{
    if (out)
        *out = v;
}

// from: the stats inside the handle, or null where the handle is null or has none of this kind
template <class S> int stats_out(const S *from, S *out)
{
    if (!from || !out)
        return SPM_E_INVALID;
    *out = *from;
    return SPM_OK;
}

// ---- the refusal of a stream that BGZF cannot count the blocks of; what: "bytes", "record bytes" ----
inline int bgzf_check_n_blocks(const char *who, spm_ctx *ctx, uint64_t n, uint32_t D, const char *what)
{
    if (bgzf_n_blocks(n, D) <= kBgzfMaxBlocks)
        return SPM_OK;
    SPM_SET_ERR(ctx, "%s: %llu %s in blocks of %u are more than 2^31 - 2 blocks (not supported)", who, (unsigned long long)n, what, D);
    return SPM_E_UNSUPPORTED;
}

// ---- A BAM file around a record stream, for the two calls that make a spm_bam.  open and place are apart because the BAM
// call learns the size of its stream between them; the sort knows it from the start. ----
using bam_ptr = std::unique_ptr<spm_bam, void (*)(spm_bam *)>;
struct bam_file
{
    std::vector<uint8_t> header; // the framed header section: the upload reads it until the stream has been waited for

    // the header section built (the refusals are bam_plain_header's) and framed serially; R: a new handle that knows its file
    int open(const char *who, spm_ctx *ctx, const char *rname, uint64_t ref_len, uint32_t D, bool sorted, bam_ptr &R)
    {
        std::vector<uint8_t> plain;
        SPM_TRY(bam_plain_header(who, ctx, rname, ref_len, sorted, plain));
        header.resize(bgzf_framed_size(plain.size(), D, false));
        bgzf_frame_serial(plain.data(), plain.size(), D, false, header.data());
        SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        R.reset(new spm_bam);
        R->ctx = ctx;
        R->rname = rname;
        R->ref_len = ref_len;
        R->block_data = D;
        R->sorted = sorted;
        R->plain_header = std::move(plain);
        return SPM_OK;
    }
    // the file allocated for n_lines records of n_records bytes, the header section uploaded
    int place(spm_bam *R, uint64_t n_lines, uint64_t n_records) const
    {
        spm_ctx *ctx = R->ctx;
        R->n_lines = n_lines;
        R->n_record_bytes = n_records;
        R->n_file = header.size() + bgzf_framed_size(n_records, R->block_data, true);
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_file, R->n_file));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->d_file, header.data(), header.size(), hipMemcpyHostToDevice, ctx->stream));
        return SPM_OK;
    }
    // the frame stage enqueued behind whatever writes R->d_records: the record stream behind the header section, then EOF
    int frame(spm_bam *R) const
    {
        spm_ctx *ctx = R->ctx;
        SPM_HIP_CHECK(ctx, bgzf_frame_enqueue(ctx, R->d_records, R->n_record_bytes, R->block_data, true, R->d_file + header.size()));
        R->stats.header_file_bytes = header.size();
        R->stats.n_record_blocks = bgzf_n_blocks(R->n_record_bytes, R->block_data);
        R->stats.n_file_bytes = R->n_file;
        R->stats.n_record_bytes = R->n_record_bytes;
        return SPM_OK;
    }
};

} // namespace spm_hip
#pragma GCC visibility pop
