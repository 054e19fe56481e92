// jst_handles.hpp -- what the stages of the pan-genome pipeline hand to each other: the tree and the result handle of every
// stage, in the order of the pipeline.  Each handle is written by the stage that makes it and read by the stages behind it,
// which live in other translation units (map in jst.hpp):
//   spm_jst            jst.hpp (create), jst_index.hpp (index)            read by every stage that walks the tree
//   spm_jst_alns       jst_hits_align.hpp, jst_locate.hpp                  read by jst_project.hpp
//   spm_jst_ref_alns   jst_project.hpp, jst_normalize.hpp                  read by jst_normalize.hpp, jst_collapse.hpp
//   spm_jst_ref_loci   jst_collapse.hpp                                    read by jst_reads.hpp .. jst_bam.hpp
//   spm_jst_reads      jst_reads.hpp                                       read by jst_pairs.hpp .. jst_bam.hpp
//   spm_jst_pairs      jst_pairs.hpp                                       read by jst_rescue.hpp .. jst_bam.hpp
//   spm_jst_rescues    jst_rescue.hpp                                      read by jst_sam.hpp, jst_bam.hpp
// (spm_jst_hits, which jst_select.hip shares, is common.hpp's.  The handles of the output stage behind these -- spm_sam, spm_bam,
// spm_bgzf, spm_bai -- are output_handles.hpp's.)  Host structs only: no kernel, no C-ABI definition.
#pragma once

#include <string>
#include <vector>

#include "common.hpp"
#include "device_order.hpp"
#include "jst_ctx_tables.hpp"
#include "jst_walk_core.hpp"

// the ctypes binding (libspm_amd/capi.py) mirrors these layouts
static_assert(sizeof(spm_jst_allele) == 24 && sizeof(spm_jst_hit) == 24 && sizeof(spm_jst_stats) == 104, "C ABI layout");
static_assert(sizeof(spm_jst_aln) == 40 && sizeof(spm_jst_align_stats) == 80, "C ABI layout");

struct spm_jst
{
    spm_ctx *ctx = nullptr;
    const spm_text *ref = nullptr;
    std::vector<spm_jst_allele> al;
    std::vector<uint8_t> alt;
    std::vector<uint64_t> cov;
    uint32_t H = 0, cw = 0, max_rlen = 0;
    uint64_t max_hap_len = 0; // reference length plus all inserted symbols: no haplotype position lies beyond it
    // device allele table
    uint64_t *d_pos = nullptr, *d_aoff = nullptr, *d_cov = nullptr;
    uint32_t *d_rlen = nullptr, *d_alen = nullptr;
    uint8_t *d_alt = nullptr;
    // index
    bool indexed = false;
    uint32_t window = 0;
    uint64_t L = 0, n_blocks = 0, jb = 0, je = 0;
    uint64_t *d_alo = nullptr, *d_hap_start = nullptr;
    uint16_t *d_local_id = nullptr;
    uint64_t n_ctx = 0, ctx_bytes = 0;
    uint64_t *d_ctx_off = nullptr, *d_ctx_base = nullptr, *d_byte_base = nullptr;
    uint32_t *d_ctx_block = nullptr, *d_ctx_owned = nullptr;
    spm_text *ctx_text = nullptr;
    spm_jst_stats stats{};
    // (record buffers of the searches are recycled through the context: a 200 MB hipMalloc / hipFree pair per search
    // cost ~0.3 ms)
    unsigned long long *d_fan_count = nullptr;
    uint64_t seg_hit_hint = 0; // most segment hits a search has seen (sizes the grid of the fan-out launched behind the scan)
    hipEvent_t fan_ev[2] = {nullptr, nullptr};
    // alignment of hits (spm_hip_jst_hits_align): every spm_hip_jst_index starts a new generation -- results of earlier
    // searches point into buffers it freed -- and the context tables are fetched to the host once per generation
    uint64_t generation = 0, h_generation = ~0ull;
    std::vector<uint64_t> h_ctx_off;   // [n_ctx + 1]
    std::vector<uint32_t> h_ctx_owned; // [n_ctx]

    spm_hip::jst_dev dev() const
    {
        spm_hip::jst_dev J{};
        J.ref = ref->d;
        J.n_ref = ref->n;
        J.pos = d_pos;
        J.rlen = d_rlen;
        J.alen = d_alen;
        J.aoff = d_aoff;
        J.alt = d_alt;
        J.cov = d_cov;
        J.n_alleles = al.size();
        J.cw = cw;
        J.n_hap = H;
        J.n_groups = (H + spm_hip::kJstGroup - 1) / spm_hip::kJstGroup;
        J.max_rlen = max_rlen;
        J.window = window;
        J.L = L;
        J.n_blocks = n_blocks;
        J.jb = jb;
        J.je = je;
        J.a_lo = d_alo;
        J.hap_start = d_hap_start;
        return J;
    }
    spm_hip::jst_ctx_tables ctx_tables() const
    {
        return spm_hip::jst_ctx_tables{d_ctx_off, n_ctx, d_ctx_block, d_ctx_owned, d_ctx_base, d_local_id};
    }
    // The context tables on the host, for the alignment entry points: enqueued once per index generation.  The caller
    // synchronises the stream and then sets h_generation = generation.
    int fetch_ctx_tables()
    {
        if (h_generation == generation)
            return SPM_OK;
        h_ctx_off.resize(n_ctx + 1);
        h_ctx_owned.resize(n_ctx);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(h_ctx_off.data(), d_ctx_off, (n_ctx + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (n_ctx)
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(h_ctx_owned.data(), d_ctx_owned, n_ctx * 4, hipMemcpyDeviceToHost, ctx->stream));
        return SPM_OK;
    }
    void free_index()
    {
        hipFree(d_alo);
        hipFree(d_hap_start);
        hipFree(d_local_id);
        hipFree(d_ctx_off);
        hipFree(d_ctx_base);
        hipFree(d_byte_base);
        hipFree(d_ctx_block);
        hipFree(d_ctx_owned);
        d_alo = d_hap_start = d_ctx_off = d_ctx_base = d_byte_base = nullptr;
        d_local_id = nullptr;
        d_ctx_block = d_ctx_owned = nullptr;
        if (ctx_text)
            spm_hip_text_destroy(ctx_text);
        ctx_text = nullptr;
        indexed = false;
        ++generation;
    }
};

struct spm_jst_alns
{
    spm_ctx *ctx = nullptr;
    spm_jst_aln *d_recs = nullptr; // arrival order of the fan-out
    uint32_t *d_ops = nullptr;
    uint64_t n = 0, n_ops = 0;
    std::vector<spm_jst_aln> host; // (haplotype, pos, pattern): the order of spm_hip_jst_hits_view
    std::vector<uint32_t> host_ops;
    spm_jst_align_stats stats{};
    // what spm_hip_jst_alns_project needs to know about the call that made these alignments (jst_project.hpp): the tree and
    // its index generation, the needle set, and whether there are transcripts at all
    spm_jst *jst = nullptr;
    const spm_patterns *patterns = nullptr;
    uint64_t generation = 0;
    bool begin_only = false;
};

struct spm_jst_ref_alns
{
    spm_ctx *ctx = nullptr;
    spm_jst_ref_aln *d_recs = nullptr; // record i belongs to record i of the source's device view
    uint32_t *d_ops = nullptr;
    uint64_t n = 0, n_ops = 0;
    std::vector<spm_jst_ref_aln> host; // record i belongs to record i of the source's host view
    std::vector<uint32_t> host_ops;
    spm_jst_project_stats stats{};
    uint32_t n_patterns = 0; // what spm_hip_jst_ref_alns_collapse plans its keys from: the needles of the set ...
    uint64_t n_ref = 0;      // ... and the reference length (the collapse reads neither tree nor set)
    // what spm_hip_jst_ref_alns_normalize reads: the tree (its reference text) and the needle set behind these records --
    // host bookkeeping only; both must be alive during that call, not after it
    spm_jst *jst = nullptr;
    const spm_patterns *patterns = nullptr;
    bool normalized = false; // made by spm_hip_jst_ref_alns_normalize, which then filled norm_stats
    spm_jst_normalize_stats norm_stats{};
};
static_assert(sizeof(spm_jst_ref_aln) == 40 && sizeof(spm_jst_project_stats) == 64, "C ABI layout");
static_assert(sizeof(spm_jst_normalize_stats) == 96, "C ABI layout");

struct spm_jst_ref_loci
{
    spm_ctx *ctx = nullptr;
    spm_jst_ref_locus *d_loci = nullptr;
    uint32_t *d_ops = nullptr, *d_members = nullptr, *d_map = nullptr;
    int32_t *d_member_scores = nullptr;
    uint64_t n = 0, n_ops = 0, n_members = 0, n_alns = 0;
    std::vector<spm_jst_ref_locus> host;
    std::vector<uint32_t> host_ops, host_members, host_map; // host_map[i]: the locus of record i of the source's HOST view
    std::vector<int32_t> host_member_scores;
    spm_jst_collapse_stats stats{};
};
static_assert(sizeof(spm_jst_ref_locus) == 48 && sizeof(spm_jst_collapse_stats) == 80, "C ABI layout");

struct spm_jst_reads : spm_hip::device_records<spm_jst_read, spm_jst_reads_stats>
{
    uint32_t strands = 1; // what the summary was made with, and from how many loci (spm_hip_jst_ref_loci_pairs asks)
    uint64_t n_loci = 0;
};
static_assert(sizeof(spm_jst_read) == 32 && sizeof(spm_jst_reads_stats) == 48, "spm_hip.h states these sizes");

struct spm_jst_pairs : spm_hip::device_records<spm_jst_pair, spm_jst_pairs_stats>
{
};
static_assert(sizeof(spm_jst_pair_opts) == 16 && sizeof(spm_jst_pair) == 32 && sizeof(spm_jst_pairs_stats) == 72,
              "spm_hip.h states these sizes");

struct spm_jst_rescues : spm_hip::device_records<spm_jst_rescue, spm_jst_rescues_stats>
{
    uint32_t *d_ops = nullptr;
    uint64_t n_ops = 0;
    std::vector<uint32_t> host_ops;
};
static_assert(sizeof(spm_jst_rescue_opts) == 20 && sizeof(spm_jst_rescue) == 48 && sizeof(spm_jst_rescues_stats) == 80,
              "spm_hip.h states these sizes");
