// jst_ctx_tables.hpp -- the context tables of a pan-genome index as one set (scheme in jst.hpp): what spm_jst::ctx_tables()
// (jst_handles.hpp) hands to the kernels behind the index.  A plain struct of pointers, host and device alike.
#pragma once

#include <cstdint>

namespace spm_hip
{

// The context tables of an index (spm_jst::ctx_tables()): written by the build (jst_index.hpp), read by everything behind it.
struct jst_ctx_tables
{
    uint64_t *ctx_off;         // [n_ctx + 1] where context c starts in the context buffer; row n_ctx = its length
    uint64_t n_ctx;
    uint32_t *ctx_block;       // [n_ctx] (block - jb, haplotype group) cell of the context
    uint32_t *ctx_owned;       // [n_ctx] offset of the first owned symbol
    const uint64_t *ctx_base;  // [cells + 1] exclusive scan of the cells' context counts
    const uint16_t *local_id;  // [(je - jb) * n_hap]: context of the haplotype inside its cell | 0x8000 for the representative
};

} // namespace spm_hip
