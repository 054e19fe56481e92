// filter_params.hpp -- the parameter blocks of the seed filter's kernels (filter.hpp) and the constants their launches are
// sized with.  No device code: the driver (scan_filter.hip) fills the blocks, the stage units launch with them.
#pragma once

#include "filter.hpp" // the records the blocks point at

namespace spm_hip
{

// The chunk a wave of the streaming kernel is filling lives in LDS behind the level-1 table (kCandRec words per wave:
// {base lo, base hi, used, size, survivors of the current span, span given up, span begin lo, hi}; touched only on the
// rare survivor path and once per span, so nothing stays live across the streaming loop): slots [base + used, base + size)
// are free.
//
// Span budget: a span (the unit of work a wave dequeues) that produces more than `span_budget` survivors -- or meets a
// full survivor buffer -- gives up: it emits nothing more, its text range goes to the overflow list, and the host
// re-scans exactly those ranges with the brute-force kernel (hits deduplicated through the same `seen` set).  Repeat-rich
// megabases then cost their own brute-force time, not a re-run of the whole scan.
constexpr uint32_t kCandLdsSlot = 4; // words after lds_words where the per-wave chunk records start
constexpr uint32_t kCandRec = 8;     // words per wave
constexpr uint32_t kDenseQueueBytes = 1536; // behind the chunk records, dense passes: one dense_queue per wave (filter_dense.hpp)

struct filter_params
{
    const uint8_t *text;
    uint64_t text_alloc;
    uint64_t lo, hi;          // examine windows fully inside [lo, hi)
    uint32_t stride;          // S in {1,2,4,8,16}
    uint32_t bitmap_words;    // power of two, <= 32768 (128 KiB)
    uint32_t n_probes;        // Bloom probes per key
    uint32_t span_chunks;     // chunks per span
    uint32_t span_unit;       // symbols per chunk: 1024 (1-byte text) or 4096 (2-bit shadow)
    uint32_t dynamic;         // how spans leave the queue at counters[kCntSpanHead]: 1 per wave, 2 per workgroup (plan_span)
    uint32_t key_len;         // H: symbols per key (12..16); windows are H symbols, keys 2H bits
    uint32_t key_mask;        // (1 << 2H) - 1
    uint32_t hash_variant;    // 1: Bloom cascade, 2: perfect-hash fingerprints, 3: dense pass, 4: presence bits
    uint32_t lds_words;       // size of the LDS image (bitmap, or fingerprint table + displacement table)
    uint32_t chd_slot_mask;   // fingerprint slots - 1
    uint32_t chd_bucket_shift; // bucket = x >> shift
    uint32_t chd_disp_off;    // byte offset of the displacement table inside the LDS image
    const uint32_t *bitmap;   // [bitmap_words]
    uint32_t span_budget;     // survivors one span may produce before it gives up
    uint32_t pass;            // which sub-batch of the needle set this launch filters for (survivor::pad)
    uint32_t anchor_c, anchor_cm; // anchored passes: a window is looked up iff its leading dimer d = sym0 | sym1 << 2 has
                                  // (d ^ anchor_c) & anchor_cm == 0
    // dense passes (filter_shared.hpp): lds = presence bits; a window is looked up iff its dimer matches one of the n_pat patterns
    uint32_t n_pat, pat_c[kDensePatterns], pat_cm[kDensePatterns];
    uint32_t bucket_shift;
    const uint4 *buckets;     // fingerprint buckets, L2-resident
    survivor *surv;
    unsigned long long *counters; // the scan's counter block (scan_plan.hpp: scan_counter)
    uint64_t surv_cap;
    uint64_t *ovf_spans;      // [ovf_cap][2]: {first text index, symbols} of every span that gave up
    uint64_t ovf_cap;
};

constexpr uint32_t kHitStage = 192; // hit records a wave of verify_kernel collects before it moves them out

// the band kernels, verify_kernel and verify_wave_kernel (filter_verify.hpp)
struct verify_params
{
    const uint8_t *text;
    uint64_t text_alloc; // readable bytes from text
    uint64_t ctx_begin;  // first symbol of the haystack that may be consumed
    uint64_t scan_begin; // owned: last symbol index in [scan_begin, scan_end)
    uint64_t scan_end;
    uint64_t pos_offset;
    const band_rec *bands;
    const unsigned long long *counters; // [band_counter] = entries of the band list
    uint32_t band_counter;              // kCntBandSlots: the list resolve_kernel wrote; kCntBandsSelected / kCntRunHeads: the kept list
    uint32_t preselected;               // 1: the list holds only bands with enough seed hits, their table slots reset
    uint64_t band_cap;
    ulonglong2 *band_tab;               // band table (slots are given back as the bands are consumed), see band_value()
    uint32_t table_mask, band_bits;     // ... its size - 1 and key layout (band_runs_kernel looks neighbours up)
    uint32_t runs;                      // 1: band_runs_kernel has compacted the heads of runs; the list holds heads only
    const uint8_t *surplus; // per needle: seed hits a band needs (seeds - k); nullptr = 1 for every needle
    uint32_t Bw;            // diagonals per band
    uint32_t overlap;       // 1: bands extend k + 1 diagonals into the next one (sets with surplus seeds)
    uint32_t max_m;         // diagonals are counted from max_m before the haystack's first symbol
    const uint32_t *peq32; // the brute table: [group][sigma+1][nw_table][64], needles top-aligned
    uint32_t sigma;        // alphabet size; LDS holds sigma+1 rows per thread (row sigma = no match)
    uint32_t nw_table;     // words per needle in that table
    uint32_t max_k;        // largest k of the set: 2*max_k + 1 end-position slots per candidate
    const int32_t *m;      // per pattern
    const int32_t *k;
    uint32_t report_begin; // 1: exact matchers report begin = end - m
    uint32_t max_span;     // diagonals of a band beyond the first: Bw - 1 (+ max_k + 1 with overlap)
    uint32_t wave_text;    // wave-per-candidate kernel: bytes of LDS per group for the candidate's text window
    unsigned long long *seen; // hash set of (pattern << 40 | end)
    uint32_t seen_mask;
    spm_hit *hits;
    unsigned long long *hit_counter; // counters[kCntHits]
    uint64_t hit_cap;
    unsigned long long *overflow; // counters[kCntVoid]
    const uint64_t *seg_offsets;  // segmented haystacks: n_segments+1 ascending offsets, or nullptr
    uint64_t n_segments;
    const uint32_t *seg_owned;    // optional, per segment: only hits whose last symbol lies at or behind this offset
                                  // are wanted (journaled-sequence contexts: the symbols before it are left context)
};

// resolve_kernel (filter_resolve.hpp says what it does with them)
struct resolve_params
{
    const survivor *surv;
    unsigned long long *counters; // the scan's counter block (scan_plan.hpp: scan_counter)
    uint64_t surv_cap;
    const pass_entry *passes; // key directories, one per pass
    const uint4 *entries;     // {val = needle << 11 | offset, seed signature, range code, key}: a key's entries side by side
    uint32_t key_len;
    uint32_t flank_check;     // 1: dna4 set without surplus seeds: seed signatures are checked against the packed text
    uint32_t pieces_check;    // 1: ... and the piece count (see pieces_visit)
    const uint8_t *text;
    uint64_t text_alloc;            // readable bytes from text
    const uint8_t *needle_ranks;    // the needles' symbols back to back, padded (nullptr: no whole-seed check)
    const uint32_t *needle_offsets; // start of every needle in needle_ranks
    const uint16_t *seed_q;         // seed length of every needle
    const int32_t *m, *k;
    uint64_t hay_begin, hay_end;    // unsegmented scans: the haystack
    const uint64_t *seg_offsets;
    uint64_t n_segments;
    uint32_t Bw, overlap, max_m;
    uint32_t band_bits;             // key = pattern << 43 | segment << band_bits | band
    ulonglong2 *band_tab;           // {key, value} per slot, see band_value()
    uint32_t table_mask;
    band_rec *bands;
    uint64_t band_cap;
    const uint32_t *needle_pk;      // dna4 sets: the needles 2 bits per symbol, 16 symbols per word (pack16's bit order)
    const uint32_t *pk_offsets;     // first word of every needle in needle_pk
    // Exact sets whose needles are their own (single) seed: a pair that passed the whole-seed check IS an occurrence and
    // is reported from here -- no band, no verification launch (C2: Shift-Or |P| = 32).
    uint32_t exact_hits;
    uint32_t report_begin;          // 1: report begin = end - |P| (the exact matchers)
    uint64_t scan_begin, scan_end;  // owned: last symbol index in [scan_begin, scan_end)
    uint64_t pos_offset;
    const uint32_t *seg_owned;
    unsigned long long *seen;
    uint32_t seen_mask;
    spm_hit *hits;
    unsigned long long *hit_counter, *overflow;
    uint64_t hit_cap;
    // The band table is shared by the scans of a context and must be EMPTY when a scan starts (a slot left behind by an
    // earlier scan makes this one take a band for "already listed" and never verify it).  A scan whose band list or table
    // overflows leaves such slots; the host empties the table before the next scan -- unless that scan was launched before
    // the host looked (deferred completion, SPM_SCAN_DEFER).  So the overflow is also recorded HERE, on the device, where it
    // sticks until the host has emptied the table: a scan that finds it set declares itself void.
    uint32_t *table_poison;
};

} // namespace spm_hip
