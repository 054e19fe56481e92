// jst_fanout.hpp -- from what was found in the context buffer of a pan-genome index to one record per haplotype that shares
// the context (scheme in jst.hpp).  gfx950.  The body the two fan-out kernels share (jst_fan_out) and what
// it reads an item as.  The kernels sit with their launches, each in its unit: jst_fanout_kernel (segment hits -> spm_jst_hit,
// behind every search) in jst_search.hpp, jst_aln_fanout_kernel (segment alignments -> spm_jst_aln) in jst_hits_align.hpp.
#pragma once

#include "jst_ctx_tables.hpp"
#include "jst_walk_core.hpp"
#include "wave.hpp"

namespace spm_hip
{

// the context ids of 8 consecutive haplotypes of one block: one 16-byte load when the row allows it
__device__ __forceinline__ void jst_load_ids8(const uint16_t *p, uint32_t n_valid, uint16_t (&v)[8])
{
    if (n_valid >= 8 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i)
            v[i] = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            v[i] = (uint32_t)i < n_valid ? p[i] : kJstNone;
    }
}

// what an item (a segment hit, a segment alignment) says about its place in the context buffer
struct jst_fan_item
{
    uint64_t probe; // a symbol of the item's own context: it finds the context
    uint64_t last;  // the item's last symbol: in the left context -> dropped (the previous block's context reports it)
    uint64_t at;    // the coordinate its records carry, handed to `store` local to the context
    uint64_t span;  // symbols in front of `at` that must not lie left of the context (0 where the item knows none)
};

// The body of both fan-outs: one lane per item t < n_items (an Item: what is read from the input array), grid-stride.
//   bool load(t, Item &, jst_fan_item &)                 reads and validates item t
//   void store(Item, slot, haplotype, ctx_lo, local)     the record of one member haplotype, whose context starts at ctx_lo
// Pass 1 finds the item's context, drops the item if its last symbol is not owned, and counts the haplotypes of the cell
// that share the context; the wave reserves their slots with one atomic; pass 2 stores one record per member, slots beyond
// out_cap counted but not written.  The trip count is wave-uniform and a dead lane asks for 0 slots, so all 64 lanes reach
// the reservation of every round (wave_reserve is wave-collective).
template <class Item, class Load, class Store>
__device__ __forceinline__ void jst_fan_out(const jst_dev &J, const jst_ctx_tables &T, uint64_t n_items,
                                            unsigned long long *out_count, uint64_t out_cap, Load load, Store store)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n_items + stride - 1) / stride;
    for (uint64_t rd = 0; rd < rounds; ++rd) {
        const uint64_t t = rd * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        Item x{}; // (of this round: nothing of an item is carried into the next one)
        jst_fan_item it{};
        bool live = t < n_items && load(t, x, it);
        uint64_t c = 0, local = 0, jr = 0;
        uint32_t id = 0, members = 0, h_lo = 0, h_hi = 0;
        if (live) {
            uint64_t lo = 0, hi = T.n_ctx; // ctx_off[lo] <= probe < ctx_off[hi]
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (T.ctx_off[mid] <= it.probe)
                    lo = mid;
                else
                    hi = mid;
            }
            c = lo;
            const uint64_t off = T.ctx_off[c];
            local = it.at - off;
            live = it.last - off >= T.ctx_owned[c] && local >= it.span;
        }
        if (live) {
            const uint64_t cb = T.ctx_block[c]; // (block, haplotype group) cell of the context
            jr = cb / J.n_groups;
            h_lo = (uint32_t)(cb % J.n_groups) * kJstGroup;
            h_hi = min(J.n_hap, h_lo + kJstGroup);
            id = (uint32_t)(c - T.ctx_base[cb]);
            for (uint32_t h = h_lo; h < h_hi; h += 8) {
                uint16_t v[8];
                jst_load_ids8(T.local_id + jr * J.n_hap + h, h_hi - h, v);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    members += (v[i] != kJstNone && (uint32_t)(v[i] & 0x7FFFu) == id) ? 1u : 0u;
            }
        }
        unsigned long long slot = wave_reserve(out_count, members);
        if (!live || members == 0)
            continue;
        // (eight haplotypes at a time: their start coordinates are loaded together, then the records are stored -- one at a
        // time the compiler has to keep every load behind the previous record's store, a dependent round trip per member)
        const uint64_t j = J.jb + jr;
        for (uint32_t h = h_lo; h < h_hi; h += 8) {
            uint16_t v[8];
            jst_load_ids8(T.local_id + jr * J.n_hap + h, h_hi - h, v);
            bool mem[8];
            uint64_t a[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                mem[i] = v[i] != kJstNone && (uint32_t)(v[i] & 0x7FFFu) == id;
                a[i] = mem[i] ? J.hap_start[j * J.n_hap + h + i] : 0;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!mem[i])
                    continue;
                const uint64_t ctx_lo = a[i] - std::min<uint64_t>(J.window ? J.window - 1 : 0, a[i]);
                if (slot < out_cap)
                    store(x, slot, h + i, ctx_lo, local);
                ++slot;
            }
        }
    }
}

} // namespace spm_hip
