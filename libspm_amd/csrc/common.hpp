// common.hpp -- internal types of libspm_hip.so (MI355X / gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/spm_hip.h"
#include "scan_plan.hpp"

namespace spm_hip
{

constexpr int kWave = 64; // CDNA wavefront

// a value that is the same in every lane, moved to SGPRs (the compiler cannot prove uniformity of a loaded value)
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
}

struct error_sink
{
    std::string msg;
};

extern thread_local std::string g_init_error;

} // namespace spm_hip

struct hits_block // device buffers + events of one scan result, recycled through the context
{
    spm_hit *d_hits = nullptr;
    unsigned long long *d_count = nullptr; // kCntBlock counters (scan_plan.hpp: scan_counter)
    uint64_t cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // scan begins, main pass begins, ... ends, verification ends
    bool zeroed = false; // the counters were cleared when the block went back to the pool
    unsigned long long *h_c = nullptr; // pinned: where a deferred scan's counters land (allocated on first use, recycled)
    hipEvent_t ev_done = nullptr;
};

struct spm_ctx
{
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_cu = 256;
    std::string err;
    // scratch reused across scans
    void *d_scratch = nullptr;
    size_t scratch_bytes = 0;
    std::vector<hits_block> pool;
    std::vector<std::pair<void *, uint64_t>> jst_pool; // record buffers of journaled-sequence searches (pointer, capacity)
    // band table of the filter engine: empty between scans (see run_filter)
    ulonglong2 *d_band_tab = nullptr; // {key, value} per slot (filter.hpp: band_value)
    uint64_t band_slots = 0;
    bool band_dirty = false;
    uint32_t *d_table_poison = nullptr; // device flag: the table holds slots a scan left behind (filter_params.hpp: resolve_params)
    // pinned staging of needle-set uploads: two halves, so the host fills one while the other travels (patterns.hip)
    uint8_t *h_stage = nullptr;
    size_t stage_half = 0;
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    unsigned long long *h_counters = nullptr; // pinned: the per-scan counter read-back lands here (a pageable target costs
                                              // an extra staging hop on every scan)
};

struct spm_text
{
    spm_ctx *ctx = nullptr;
    uint8_t *d = nullptr;
    uint64_t n = 0;
    uint64_t alloc = 0; // bytes readable from d (>= n)
    uint32_t sigma = 4;
    bool owned = false;
    uint32_t *d_packed = nullptr; // optional 2-bit shadow (spm_hip_text_pack), zero-padded to whole 4096-symbol chunks
    uint64_t packed_words = 0;
};

struct spm_hits : hits_block // (its buffers, counters and events: taken from the context's pool and given back to it)
{
    spm_ctx *ctx = nullptr;
    uint64_t cand_cap = 0; // survivor list capacity of the filter run
    uint64_t band_cap = 0;
    uint64_t n = 0;
    bool counted = false;
    bool hook_final = false;          // the caller's after-launch work (scan_impl) ran on the final hit list ...
    unsigned long long fan_count = 0; // ... and counted this much into kCntFanOut
    bool sorted_host = false;
    std::vector<spm_hit> host;
    spm_scan_stats stats{};
    bool timed = false;
    void *d_aux[2] = {nullptr, nullptr}; // segmented scans: tile table, segment offsets (freed with the hits)
    // deferred completion (SPM_SCAN_DEFER): the counters are on their way to h_c behind ev_done; what the scan was, in case
    // it has to be repeated
    bool pending = false;
    bool c_on_the_way = false;  // ... the copy of the counters into h_c has been enqueued (by the scan, or by the device-side
                                // fused copy, whose kernel writes them itself: one launch less in a C2 step)
    bool d_count_cleared = false; // the fused-copy kernel consumed the device counters and cleared them for the next scan
    const spm_text *d_text = nullptr;
    const struct spm_patterns *d_patterns = nullptr;
    uint64_t d_begin = 0, d_end = 0;
    spm_scan_opts d_opts{};
    // what spm_hip_hits_align needs to know about the scan that made these hits (align.hip)
    const spm_text *al_text = nullptr;
    const struct spm_patterns *al_patterns = nullptr;
    uint64_t al_lo = 0;             // first symbol an alignment may use (whole scans; segmented: the hit's segment start)
    uint64_t al_pos_offset = 0;
    bool al_stateful = false;       // state_in != NULL
    bool al_device_segs = false;    // segment table only on the device (journaled-sequence search)
    std::vector<uint64_t> al_segs;  // segmented scans: the segment table (n_segments + 1 offsets)
    // a result made by spm_hip_hits_select / spm_hip_records_select (select.hip): ev[0..2] time its order and select steps
    bool selected = false;
    bool sel_records = false;       // ... out of a raw record buffer: no alignment context
    bool sel_timed = false;         // sel.ms_* still have to be read off the events
    uint64_t sel_n_patterns = 0, sel_bias = 0, sel_max_rel = 0; // sel_records: what the buffer's range was found to be
    spm_select_stats sel{};
};

struct spm_jst_hits // (jst.hip: searches; jst_select.hip: selections)
{
    spm_ctx *ctx = nullptr;
    spm_jst_hit *d = nullptr;
    uint64_t cap = 0;
    uint64_t n = 0;
    bool sorted = false;
    std::vector<spm_jst_hit> host;
    // searches with SPM_SCAN_ALIGNABLE: what spm_hip_jst_hits_align needs
    bool alignable = false;
    spm_jst *jst = nullptr;
    const struct spm_patterns *patterns = nullptr;
    uint32_t pat_strands = 0; // the set's strands as the search found them (the set may be gone when a selection asks); 0: no set
    uint64_t generation = 0;
    spm_hits *seg = nullptr; // the search's segment hits, owned (nullptr: the search had nothing to scan)
    // what a selection plans its sort key from: set by the search (the tree's bounds), or by the range kernel of
    // spm_hip_jst_records_select, and inherited by every selection of a selection
    uint64_t sel_n_hap = 1, sel_n_patterns = 1, sel_max_pos = 0;
    // a result made by spm_hip_jst_hits_select / spm_hip_jst_records_select: a buffer of exactly n records that is freed, not
    // pooled, and three events that time its order and select steps
    bool selected = false;
    bool sel_timed = false;
    hipEvent_t sel_ev[3] = {nullptr, nullptr, nullptr};
    spm_select_stats sel{};
};

// A deferred scan that had to be repeated: `h` takes over the buffers and the outcome of the repeated scan, which gets
// h's in exchange and is destroyed by the caller.  The only place that knows which members are device resources: the
// hits_block (whose pinned block and event stay where they are) and the per-scan tables in d_aux.
inline void hits_adopt(spm_hits &h, spm_hits &from)
{
    std::swap(static_cast<hits_block &>(h), static_cast<hits_block &>(from));
    std::swap(h.h_c, from.h_c);
    std::swap(h.ev_done, from.ev_done);
    std::swap(h.d_aux, from.d_aux);
    from.d_count_cleared = h.d_count_cleared; // (the flags follow the buffers they describe)
    h.d_count_cleared = false;
    h.n = from.n;
    h.counted = from.counted;
    h.stats = from.stats;
    h.cand_cap = from.cand_cap;
    h.band_cap = from.band_cap;
    h.timed = from.timed;
    h.sorted_host = false;
    h.host.clear();
}

// a step of a scan that reports through its return code, like SPM_HIP_CHECK for HIP calls
#define SPM_TRY(call)                                                                                                  \
    do {                                                                                                               \
        const int _rc = (call);                                                                                        \
        if (_rc != SPM_OK)                                                                                             \
            return _rc;                                                                                                \
    } while (0)

struct pass_entry // key directory of one pass of the seed filter, in L2 (filter_resolve.hpp: resolve_kernel)
{
    const uint4 *ht; // {key, first entry, entries, -}, open addressing; an empty slot has .z == 0
    uint32_t ht_mask;
    uint32_t pad;
};

// scope guard for temporary device buffers: freed on every return path
struct dev_scratch
{
    std::vector<void *> owned;
    template <typename T>
    hipError_t alloc(T **p, size_t bytes)
    {
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), bytes);
        if (e == hipSuccess)
            owned.push_back(*p);
        return e;
    }
    ~dev_scratch()
    {
        for (void *p : owned)
            hipFree(p);
    }
};

#define SPM_SET_ERR(ctx, ...)                                                                                          \
    do {                                                                                                               \
        char _b[512];                                                                                                  \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                                                                         \
        if (ctx)                                                                                                       \
            (ctx)->err = _b;                                                                                           \
        else                                                                                                           \
            spm_hip::g_init_error = _b;                                                                                \
    } while (0)

#define SPM_HIP_CHECK(ctx, call)                                                                                       \
    do {                                                                                                               \
        hipError_t _e = (call);                                                                                        \
        if (_e != hipSuccess) {                                                                                        \
            SPM_SET_ERR(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__);               \
            return SPM_E_HIP;                                                                                          \
        }                                                                                                              \
    } while (0)
