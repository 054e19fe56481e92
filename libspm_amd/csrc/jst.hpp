// jst.hpp -- journaled-sequence (pan-genome) search on the device (config C5).
//
// Contract: the hit set equals the union over haplotypes of a linear scan of each materialised haplotype
// (haplotype, position in haplotype coordinates).  The reference holds no traversal code, only the journaled-sequence
// design (specs/journaled_sequence_class_diagram.drawio) and the matcher hooks (matcher/concept.hpp:26-161).
//
// Scheme (everything below runs on the MI355X; the host only launches):
//   1. the reference axis is cut into blocks of L positions; block j owns the haplotype symbols that stem from
//      reference positions [jL, (j+1)L) (an alt symbol belongs to its allele's position);
//   2. hap_start[j][h] = haplotype coordinate of the first symbol block j owns in haplotype h (column-wise prefix sum
//      of the allele length deltas each haplotype carries);
//   3. a context = the symbols a (block, haplotype) pair owns plus window-1 symbols of left context.  Its signature is
//      exact: where the left context starts (reference position, or allele + offset inside an alt), its length, and
//      the bit set of the alleles the haplotype carries over that stretch.  Equal signatures <=> byte-identical
//      contexts, so one workgroup per (block, group of <= 1024 haplotypes) groups them by signature in LDS;
//   4. one representative per group is spelled out into the context buffer (wave-cooperative copies of reference
//      runs and alt runs), the buffer is scanned as independent segments by the ordinary engines, and each hit whose
//      last symbol lies in the owned part is fanned out to the haplotypes of its group.
// By the window property (a hit depends only on the window_size symbols ending at it) this is exact; work on the
// device is proportional to the distinct sequence content, not to haplotypes x length.
// Here: the C-ABI calls of the tree object spm_jst (create, destroy, extract, length, stats) and the variant generator of C5.
// Everything behind the tree is one translation unit per group of stages; every kernel and every C-ABI call is defined in
// exactly one of them, and a stage reads the stages before it through their handles alone (jst_handles.hpp):
//   jst.hip         tree, index, search
//     jst.hpp             this header
//     jst_index.hpp       spm_hip_jst_index: the build kernels and the build as named stages
//     jst_search.hpp      spm_hip_jst_search, jst_fanout_kernel and the accessors of the records
//   jst_align.hip   alignments of hits in haplotype coordinates (both call align.hip's align_run through jst_align_segments)
//     jst_hits_align.hpp  spm_hip_jst_hits_align, jst_aln_fanout_kernel, and what the call shares with jst_locate.hpp
//     jst_locate.hpp      spm_hip_jst_selection_align
//   jst_ref.hip     alignments in reference coordinates (all three begin with the slot stage)
//     transcript_slots.hpp, jst_project.hpp, jst_normalize.hpp, jst_collapse.hpp
//   jst_reads.hip   per-read and per-pair summaries over loci
//     jst_reads.hpp, jst_pairs.hpp, jst_rescue.hpp
//   jst_sam.hip     output (BAM reuses the SAM front and kernels)
//     jst_sam.hpp, jst_bam.hpp
// and under all of them
//   jst_handles.hpp     the tree and every stage's result handle (spm_sam and spm_bam: output_handles.hpp)
//   jst_walk_core.hpp   what a cell owns and what its context spells (steps 1-3 and the spelling of 4), host and device alike
//   jst_ctx_tables.hpp  the context tables of the index as one set
//   jst_fanout.hpp      the walk of step 4's fan-out, shared by the kernel for hits and the kernel for alignments
// (jst_select.hip, the selection of hits, is a unit of its own beside these.)
#pragma once

#include "internal.hpp"
#include "jst_handles.hpp"
#include "synth.hpp"

extern "C" int spm_hip_jst_create(spm_ctx *ctx, const spm_text *reference, const spm_jst_allele *alleles,
                                  uint64_t n_alleles, const uint8_t *alt_pool, uint64_t alt_pool_len,
                                  const uint64_t *coverage, uint32_t n_haplotypes, spm_jst **out)
{
    if (!ctx || !reference || !out || (n_alleles && (!alleles || !coverage)) || n_haplotypes == 0) {
        SPM_SET_ERR(ctx, "spm_hip_jst_create: invalid argument");
        return SPM_E_INVALID;
    }
    if (n_haplotypes > spm_hip::kJstMaxHap) {
        SPM_SET_ERR(ctx, "spm_hip_jst_create: %u haplotypes, at most %u", n_haplotypes, spm_hip::kJstMaxHap);
        return SPM_E_UNSUPPORTED;
    }
    const uint32_t cw = (n_haplotypes + 63) / 64;
    std::unique_ptr<spm_jst> J(new spm_jst);
    J->ctx = ctx;
    J->ref = reference;
    J->max_hap_len = reference->n;
    J->H = n_haplotypes;
    J->cw = cw;
    J->al.assign(alleles, alleles + n_alleles);
    J->cov.assign(coverage, coverage + n_alleles * cw);
    if (alt_pool_len)
        J->alt.assign(alt_pool, alt_pool + alt_pool_len);
    for (uint64_t i = 0; i < n_alleles; ++i) {
        spm_jst_allele &a = J->al[i];
        if (a.pos > reference->n || (i && a.pos < J->al[i - 1].pos) || a.alt_off + a.alt_len > alt_pool_len ||
            a.alt_len >= (1u << 24)) {
            SPM_SET_ERR(ctx, "spm_hip_jst_create: allele %llu is out of order, out of range or too long",
                        (unsigned long long)i);
            return SPM_E_INVALID;
        }
        a.ref_len = (uint32_t)std::min<uint64_t>(a.ref_len, reference->n - a.pos); // clamp to the reference
        J->max_rlen = std::max(J->max_rlen, a.ref_len);
        J->max_hap_len += a.alt_len;
        for (uint32_t x = 0; x < a.alt_len; ++x)
            if (J->alt[a.alt_off + x] >= reference->sigma) {
                SPM_SET_ERR(ctx, "spm_hip_jst_create: allele %llu holds a symbol that is not a rank < sigma",
                            (unsigned long long)i);
                return SPM_E_INVALID;
            }
        if (n_haplotypes & 63)
            J->cov[i * cw + cw - 1] &= (1ull << (n_haplotypes & 63)) - 1;
    }
    // alleles that overlap on the reference must not share a haplotype
    for (uint64_t i = 0; i < n_alleles; ++i) {
        const uint64_t e = J->al[i].pos + J->al[i].ref_len;
        for (uint64_t j = i + 1; j < n_alleles && J->al[j].pos < e; ++j)
            for (uint32_t w = 0; w < cw; ++w)
                if (J->cov[i * cw + w] & J->cov[j * cw + w]) {
                    SPM_SET_ERR(ctx, "spm_hip_jst_create: alleles %llu and %llu overlap on a shared haplotype",
                                (unsigned long long)i, (unsigned long long)j);
                    return SPM_E_UNSUPPORTED;
                }
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t na = std::max<uint64_t>(n_alleles, 1);
    std::vector<uint64_t> pos(na, 0), aoff(na, 0);
    std::vector<uint32_t> rlen(na, 0), alen(na, 0);
    for (uint64_t i = 0; i < n_alleles; ++i) {
        pos[i] = J->al[i].pos;
        aoff[i] = J->al[i].alt_off;
        rlen[i] = J->al[i].ref_len;
        alen[i] = J->al[i].alt_len;
    }
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_pos, na * 8));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_aoff, na * 8));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_rlen, na * 4));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_alen, na * 4));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_cov, na * cw * 8));
    SPM_HIP_CHECK(ctx, hipMalloc(&J->d_alt, std::max<uint64_t>(alt_pool_len, 1) + 64));
    SPM_HIP_CHECK(ctx, hipMemcpy(J->d_pos, pos.data(), na * 8, hipMemcpyHostToDevice));
    SPM_HIP_CHECK(ctx, hipMemcpy(J->d_aoff, aoff.data(), na * 8, hipMemcpyHostToDevice));
    SPM_HIP_CHECK(ctx, hipMemcpy(J->d_rlen, rlen.data(), na * 4, hipMemcpyHostToDevice));
    SPM_HIP_CHECK(ctx, hipMemcpy(J->d_alen, alen.data(), na * 4, hipMemcpyHostToDevice));
    if (n_alleles)
        SPM_HIP_CHECK(ctx, hipMemcpy(J->d_cov, J->cov.data(), n_alleles * cw * 8, hipMemcpyHostToDevice));
    if (alt_pool_len)
        SPM_HIP_CHECK(ctx, hipMemcpy(J->d_alt, J->alt.data(), alt_pool_len, hipMemcpyHostToDevice));
    *out = J.release();
    return SPM_OK;
}

extern "C" void spm_hip_jst_destroy(spm_jst *J)
{
    if (!J)
        return;
    hipSetDevice(J->ctx->device);
    hipStreamSynchronize(J->ctx->stream);
    J->free_index();
    hipFree(J->d_fan_count);
    if (J->fan_ev[0]) {
        hipEventDestroy(J->fan_ev[0]);
        hipEventDestroy(J->fan_ev[1]);
    }
    hipFree(J->d_pos);
    hipFree(J->d_aoff);
    hipFree(J->d_rlen);
    hipFree(J->d_alen);
    hipFree(J->d_cov);
    hipFree(J->d_alt);
    delete J;
}

extern "C" uint64_t spm_hip_jst_haplotype_length(const spm_jst *J, uint32_t h)
{
    if (!J || h >= J->H)
        return 0;
    int64_t len = (int64_t)J->ref->n;
    for (size_t i = 0; i < J->al.size(); ++i)
        if ((J->cov[i * J->cw + (h >> 6)] >> (h & 63)) & 1)
            len += (int64_t)J->al[i].alt_len - (int64_t)J->al[i].ref_len;
    return (uint64_t)len;
}

extern "C" int spm_hip_jst_extract(spm_jst *J, uint32_t h, uint64_t begin, uint64_t n, uint8_t *out)
{
    if (!J || h >= J->H || (n && !out)) {
        SPM_SET_ERR(J ? J->ctx : nullptr, "spm_hip_jst_extract: invalid argument");
        return SPM_E_INVALID;
    }
    spm_ctx *ctx = J->ctx;
    const uint64_t end = begin + n;
    uint64_t r = 0, hp = 0; // reference cursor, haplotype coordinate of reference[r]
    auto ref_piece = [&](uint64_t hp0, uint64_t r0, uint64_t len) -> int { // haplotype [hp0, hp0+len) = reference[r0..]
        const uint64_t lo = std::max(hp0, begin), hi = std::min(hp0 + len, end);
        if (lo < hi)
            return spm_hip_text_download(ctx, J->ref, r0 + (lo - hp0), hi - lo, out + (lo - begin));
        return SPM_OK;
    };
    for (size_t i = 0; i < J->al.size() && hp < end; ++i) {
        if (!((J->cov[i * J->cw + (h >> 6)] >> (h & 63)) & 1))
            continue;
        const spm_jst_allele &a = J->al[i];
        const uint64_t run = a.pos - r;
        int rc = ref_piece(hp, r, run);
        if (rc != SPM_OK)
            return rc;
        hp += run;
        const uint64_t lo = std::max(hp, begin), hi = std::min(hp + a.alt_len, end);
        for (uint64_t x = lo; x < hi; ++x)
            out[x - begin] = J->alt[a.alt_off + (x - hp)];
        hp += a.alt_len;
        r = a.pos + a.ref_len;
    }
    if (hp < end) {
        if (hp + (J->ref->n - r) < end) {
            SPM_SET_ERR(ctx, "spm_hip_jst_extract: range beyond the end of haplotype %u", h);
            return SPM_E_INVALID;
        }
        int rc = ref_piece(hp, r, J->ref->n - r);
        if (rc != SPM_OK)
            return rc;
    }
    return SPM_OK;
}

extern "C" int spm_hip_jst_stats(const spm_jst *J, spm_jst_stats *out)
{
    if (!J || !out)
        return SPM_E_INVALID;
    *out = J->stats;
    return SPM_OK;
}

// Synthetic variants of config C5.  Per 1000-base block b of the reference: one SNP at an offset in
// [0, 900); per 10 000 bases one indel of length 1..50 placed in [900, 950) of one of its 1000-blocks, so no two
// alleles overlap.  Everything derives from mix64(seed_var, global block index), i.e. shards agree on the variants.
extern "C" int spm_hip_jst_synth_variants(uint64_t seed_text, uint64_t seed_var, uint64_t ref_begin, uint64_t n_ref,
                                          uint32_t n_hap, spm_jst_allele *alleles, uint64_t *n_alleles,
                                          uint8_t *alt_pool, uint64_t *alt_pool_len, uint64_t *coverage)
{
    using spm_hip::mix64;
    if (!n_alleles || !alt_pool_len || n_hap == 0 || n_hap > 64 || (ref_begin % 10000) != 0)
        return SPM_E_INVALID;
    const uint64_t hap_mask = n_hap == 64 ? ~0ull : ((1ull << n_hap) - 1);
    uint64_t na = 0, np = 0;
    auto cov_of = [&](uint64_t r) {
        uint64_t c = mix64(r ^ 0xC0FEull) & hap_mask;
        if (c == 0)
            c = 1ull << (r % n_hap);
        return c;
    };
    const uint64_t g0 = ref_begin / 1000;
    for (uint64_t b = 0; b * 1000 < n_ref; ++b) {
        const uint64_t gb = g0 + b;
        {
            const uint64_t r = mix64(seed_var + 2 * gb);
            const uint64_t p = b * 1000 + r % 900;
            if (p < n_ref) {
                if (alleles) {
                    const uint8_t rb = spm_hip::synth_base(seed_text, ref_begin + p);
                    alleles[na] = spm_jst_allele{p, 1, 1, np};
                    alt_pool[np] = (uint8_t)((rb + 1 + (r >> 20) % 3) & 3);
                    coverage[na] = cov_of(r);
                }
                ++na;
                ++np;
            }
        }
        const uint64_t r10 = mix64(seed_var + 2 * (gb / 10) + 1);
        if (gb % 10 == r10 % 10) {
            const uint64_t p = b * 1000 + 900 + (r10 >> 8) % 50;
            const uint32_t len = 1 + (uint32_t)((r10 >> 16) % 50);
            const bool del = (r10 >> 24) & 1;
            if (p + len <= n_ref && p < n_ref) {
                if (alleles) {
                    if (del) {
                        alleles[na] = spm_jst_allele{p, len, 0, np};
                    } else {
                        alleles[na] = spm_jst_allele{p, 0, len, np};
                        for (uint32_t x = 0; x < len; ++x)
                            alt_pool[np + x] = (uint8_t)((mix64(r10 + 0x1234567ull * (x / 32 + 1)) >> (2 * (x & 31))) & 3);
                    }
                    coverage[na] = cov_of(r10 ^ 0x5555ull);
                }
                ++na;
                if (!del)
                    np += len;
            }
        }
    }
    *n_alleles = na;
    *alt_pool_len = np;
    return SPM_OK;
}
