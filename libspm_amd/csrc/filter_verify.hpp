// filter_verify.hpp -- the verification stage of the seed filter (filter.hpp): the passes over the band list (selection, runs
// of adjacent bands, release) and the two verification kernels.  The band kernels are no templates: exactly one translation
// unit (filter_verify.hip) includes this header.
#pragma once

#include "brute.hpp" // myers_lane
#include "filter_params.hpp"
#include "pack.hpp"
#include "wave.hpp"

namespace spm_hip
{

// one key per reported hit in the scan's dedupe set; true if this is the first report of (pattern, end)
__device__ __forceinline__ bool seen_insert(const verify_params &P, uint32_t pat, int64_t e)
{
    return seen_insert_raw(P.seen, P.seen_mask, P.overflow, pat, e);
}

// Sets with surplus seeds (k >= kMergeMinK): most bands hold a single chance match of a short key and are NOT verified.
// This pass keeps the bands that collected enough seed hits -- a dense list, so the wave-per-band verification (one
// ~0.2 ms serial chain per band) gets one band per wave instead of two on some and none on most -- and gives every table
// slot back.
__global__ __launch_bounds__(256) void band_select_kernel(const verify_params P, band_rec *out, unsigned long long *out_count)
{
    unsigned long long n = P.counters[kCntBandSlots];
    if (n > P.band_cap)
        n = P.band_cap;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t i = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool keep = false;
        band_rec c;
        c.val = kBandInvalid;
        if (i < n) {
            c = P.bands[i];
            if (c.val != kBandInvalid) {
                const uint32_t cnt = (uint32_t)band_value(P.band_tab[c.slot].y, true);
                band_release(P.band_tab, c.slot);
                keep = cnt >= (P.surplus ? (uint32_t)P.surplus[c.val >> 11] : 1u);
            }
        }
        const uint64_t m = __ballot(keep);
        if (m != 0) {
            unsigned long long base = 0;
            const int leader = __ffsll((unsigned long long)m) - 1;
            if ((int)lane == leader)
                base = atomicAdd(out_count, (unsigned long long)__popcll(m));
            base = __shfl(base, leader);
            if (keep)
                out[base + __popcll(m & ((1ull << lane) - 1))] = c; // (<= the entries of the input list)
        }
    }
}

// ---- runs of adjacent bands ------------------------------------------------------------------------------------------
// A repeat stretch of the text that a needle (nearly) matches is hit on a hundred diagonals in a row: three, four bands of
// 32, each of which would be verified on its own -- |P| + k columns of cold start each time for 32 + 2k end positions --
// and every one of its hits would go through the dedupe set (a compare-and-swap in a table of a gigabyte: memory-side
// atomics are what the verification of a repeat-rich text runs out of first).  band_runs_kernel (sets without surplus
// seeds, long band lists only) looks every band's neighbours up in the band table BEFORE the verification gives the slots
// back: a band whose predecessor exists is a FOLLOWER (not verified on its own), a band without one -- or at a multiple of
// kRunMax, so that no lane gets more than kRunMax bands (a wave waits for its longest lane: four bands are 237 columns
// against the 141 of one, and already save 58 % of four cold starts) -- is the HEAD of a run and records how many bands
// follow it and the last hit diagonal of the last one.  The heads are compacted into a list of their own; the verification
// runs through the diagonals of a whole run with one cold start.  In band_rec::val (low 11 bits, 0 when the kernel did not run):
constexpr uint32_t kRunAnalysed = 0x400u; // band_runs_kernel has looked at this band
constexpr uint32_t kRunFollower = 0x200u; // ... and found its predecessor: the head of the run covers it
constexpr uint32_t kRunLenShift = 5, kRunLenMask = 0x3u, kRunHiMask = 0x1Fu; // head: followers (0..3), last hit diagonal (0..31)
// head: the band right before / right behind the run exists too (the run was cut at a multiple of kRunMax): only there can
// another verification report the same (needle, end) -- the seeds of one occurrence lie within k diagonals of each other,
// i.e. in one band or in two adjacent ones, and adjacent bands belong to one run unless the cut falls between them.  So a
// head asks the dedupe set only about the end positions within reach of such a side, and reports the rest as they come.
constexpr uint32_t kRunTouchLeft = 0x80u, kRunTouchRight = 0x100u;
constexpr uint32_t kRunMax = 4;

__device__ __forceinline__ uint32_t band_lookup(const verify_params &P, unsigned long long bkey)
{
    uint32_t s2 = (uint32_t)mix64(bkey) & P.table_mask;
    for (uint32_t tries = 0; tries < 8192; ++tries) {
        const unsigned long long o = P.band_tab[s2].x;
        if (o == bkey)
            return s2;
        if (o == kBandEmpty)
            return 0xFFFFFFFFu;
        s2 = (s2 + 1) & P.table_mask;
    }
    return 0xFFFFFFFFu;
}

// One pass over the band list: classify every band (head / follower), write the code into its record, and compact the heads
// into `heads` (a workgroup takes 2048 records at a time and reserves room for its heads with ONE atomic -- a wave-level
// reservation would be 500 000 atomics on one word for a 30 M list).  The verification then runs over `heads` only and
// leaves the table alone; band_release_kernel gives every slot of the original list back afterwards.
__global__ __launch_bounds__(256) void band_runs_kernel(const verify_params P, band_rec *bands, band_rec *heads,
                                                        unsigned long long *head_count)
{
    __shared__ uint32_t wave_tot01[4], wave_tot23[4];
    __shared__ unsigned long long chunk_base;
    unsigned long long n = P.counters[P.band_counter];
    if (n > P.band_cap)
        n = P.band_cap;
    constexpr uint32_t PER = 8;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t c0 = (uint64_t)blockIdx.x * (256 * PER); c0 < n; c0 += (uint64_t)gridDim.x * (256 * PER)) {
        band_rec mine[PER];
        uint32_t head_mask = 0, cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint64_t i = c0 + (uint64_t)j * 256 + tid;
            mine[j].val = kBandInvalid;
            if (i >= n)
                continue;
            band_rec c = bands[i];
            if (c.val == kBandInvalid)
                continue;
            const unsigned long long base = ((unsigned long long)(c.val >> 11) << 43) | ((unsigned long long)c.seg << P.band_bits);
            uint32_t code = kRunAnalysed;
            const bool pred = c.band > 0 && band_lookup(P, base | (unsigned long long)(c.band - 1)) != 0xFFFFFFFFu;
            if (c.band % kRunMax != 0 && pred) {
                code |= kRunFollower;
            } else {
                uint32_t followers = 0, last = c.slot;
                bool cut = true; // the run ends at a multiple of kRunMax (then the band behind it may exist)
                for (uint32_t r = 1; r < kRunMax && (c.band + r) % kRunMax != 0; ++r) {
                    const uint32_t s2 = band_lookup(P, base | (unsigned long long)(c.band + r));
                    if (s2 == 0xFFFFFFFFu) {
                        cut = false;
                        break;
                    }
                    followers = r;
                    last = s2;
                }
                const bool succ = cut && band_lookup(P, base | (unsigned long long)(c.band + followers + 1)) != 0xFFFFFFFFu;
                const unsigned long long v = band_value(P.band_tab[last].y, false);
                const uint32_t hi = v ? (uint32_t)(63 - __clzll((long long)v)) : 0u;
                code |= (followers << kRunLenShift) | (hi & kRunHiMask) | (pred ? kRunTouchLeft : 0u) | (succ ? kRunTouchRight : 0u);
                head_mask |= 1u << j;
                ++cnt;
            }
            c.val = (c.val & ~0x7FFu) | code;
            mine[j] = c;
        }
        // where this thread's heads go: one reservation per chunk, and inside the chunk the heads are laid out BY RUN LENGTH
        // (class = followers, 0..3): the verification takes 64 consecutive heads per wave and runs as long as its longest
        // run -- 231 columns for four bands against 135 for one --, so waves of one class waste nothing.  Four 16-bit counters
        // (<= 2048 heads per chunk) travel in two words through the prefix sums.
        uint32_t c01 = 0, c23 = 0; // this thread's heads per class: classes 0, 1 in c01 (low, high half), 2, 3 in c23
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j)
            if (head_mask & (1u << j)) {
                const uint32_t cls = (mine[j].val >> kRunLenShift) & kRunLenMask;
                const uint32_t one = 1u << (16 * (cls & 1u));
                c01 += cls < 2 ? one : 0u;
                c23 += cls < 2 ? 0u : one;
            }
        uint32_t i01 = c01, i23 = c23; // (flat: the paired prefix; as two wave_prefix_incl it is scheduled differently)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u01 = (uint32_t)__shfl_up((int)i01, o), u23 = (uint32_t)__shfl_up((int)i23, o);
            if (lane >= (uint32_t)o) {
                i01 += u01;
                i23 += u23;
            }
        }
        if (lane == 63) {
            wave_tot01[wave] = i01;
            wave_tot23[wave] = i23;
        }
        __syncthreads();
        uint32_t off01 = 0, off23 = 0, tot01 = 0, tot23 = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            off01 += w < wave ? wave_tot01[w] : 0u;
            off23 += w < wave ? wave_tot23[w] : 0u;
            tot01 += wave_tot01[w];
            tot23 += wave_tot23[w];
        }
        const uint32_t tot[4] = {tot01 & 0xFFFFu, tot01 >> 16, tot23 & 0xFFFFu, tot23 >> 16};
        const uint32_t total = tot[0] + tot[1] + tot[2] + tot[3];
        if (tid == 0)
            chunk_base = total ? atomicAdd(head_count, (unsigned long long)total) : 0ull;
        __syncthreads();
        // class c starts behind the classes before it; inside it: the waves before this one, then the lanes before this one
        const uint32_t mine_before[4] = {(off01 & 0xFFFFu) + ((i01 - c01) & 0xFFFFu), (off01 >> 16) + ((i01 - c01) >> 16),
                                         (off23 & 0xFFFFu) + ((i23 - c23) & 0xFFFFu), (off23 >> 16) + ((i23 - c23) >> 16)};
        uint64_t pos[4];
        pos[0] = chunk_base + mine_before[0];
        pos[1] = chunk_base + tot[0] + mine_before[1];
        pos[2] = chunk_base + tot[0] + tot[1] + mine_before[2];
        pos[3] = chunk_base + tot[0] + tot[1] + tot[2] + mine_before[3];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j)
            if (head_mask & (1u << j)) {
                const uint32_t cls = (mine[j].val >> kRunLenShift) & kRunLenMask;
                // (a select chain instead of pos[cls]: a dynamically indexed array would live in scratch memory)
                const uint64_t at = cls == 0 ? pos[0] : cls == 1 ? pos[1] : cls == 2 ? pos[2] : pos[3];
                heads[at] = mine[j]; // (<= the entries of the input list)
                pos[0] += cls == 0 ? 1u : 0u;
                pos[1] += cls == 1 ? 1u : 0u;
                pos[2] += cls == 2 ? 1u : 0u;
                pos[3] += cls == 3 ? 1u : 0u;
            }
        __syncthreads();
    }
}

// ... and after the verification of the heads: every band of the original list gives its table slot back
__global__ __launch_bounds__(256) void band_release_kernel(const verify_params P, const band_rec *bands, uint32_t counter)
{
    unsigned long long n = P.counters[counter];
    if (n > P.band_cap)
        n = P.band_cap;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const band_rec c = bands[i];
        if (c.val != kBandInvalid)
            band_release(P.band_tab, c.slot);
    }
}

// ---------------------------------------------------------------------------------------------------
// verification: one lane per candidate
// ---------------------------------------------------------------------------------------------------
// What a band record stands for (verification side).  Returns false if the band has too few seed hits, lies outside the
// owned range, or is an unused list slot.  Consumes the band's table slot (the table is empty again after the scan).
struct band_geom
{
    uint32_t pat;
    int64_t m, k;
    int64_t e_lo, e_hi; // exclusive end positions it answers for
    int64_t ws;         // cold start
    int64_t dd_lo, dd_hi; // end positions <= dd_lo or >= dd_hi go through the dedupe set (heads of runs: the rest cannot
                          // be reported by anybody else); everything, unless band_runs_kernel has analysed the band
};

__device__ __forceinline__ bool decode_band(const verify_params &P, const band_rec &c, bool consume, band_geom &g)
{
    if (c.val == kBandInvalid)
        return false;
    g.pat = c.val >> 11;
    unsigned long long v = 1;
    if (!P.preselected) {
        v = band_value(P.band_tab[c.slot].y, P.overlap != 0);
        if (consume)
            band_release(P.band_tab, c.slot);
        if (c.val & kRunFollower)
            return false; // the head of its run verifies this band's diagonals too
        if (P.overlap ? (uint32_t)v < (P.surplus ? (uint32_t)P.surplus[g.pat] : 1u) : v == 0)
            return false;
    }
    g.m = P.m[g.pat];
    g.k = P.k[g.pat];
    int64_t own_b = (int64_t)P.scan_begin, own_e = (int64_t)P.scan_end, hay_b = (int64_t)P.ctx_begin;
    if (P.seg_offsets) { // every segment is a haystack of its own
        const int64_t sb = (int64_t)P.seg_offsets[c.seg], se = (int64_t)P.seg_offsets[c.seg + 1];
        own_b = P.seg_owned ? sb + (int64_t)P.seg_owned[c.seg] : sb;
        own_e = se;
        hay_b = sb;
    }
    // diagonals d .. d + span: needle position 0 <-> text index d.  Bands that do not overlap know which of their
    // diagonals were hit: an isolated seed hit is verified over its own diagonal, a repeat stretch over the whole band
    const int64_t band_base = hay_b - (int64_t)P.max_m + (int64_t)c.band * (int64_t)P.Bw;
    int64_t d = band_base;
    int64_t span = (int64_t)P.Bw - 1 + (P.overlap ? g.k + 1 : 0);
    if (!P.overlap) {
        const int lo = __ffsll((long long)v) - 1;
        int hi = 63 - __clzll((long long)v);
        if (c.val & kRunAnalysed) // the head of a run of adjacent bands: through the last hit diagonal of its last band
            hi = (int)(((c.val >> kRunLenShift) & kRunLenMask) * P.Bw + (c.val & kRunHiMask));
        d += lo;
        span = hi - lo;
    }
    g.e_lo = d + g.m - g.k;
    g.e_hi = d + g.m + g.k + span;
    g.dd_lo = INT64_MAX; // (every end position is <= this: all of them go through the dedupe set)
    g.dd_hi = INT64_MIN;
    if (!P.overlap && (c.val & kRunAnalysed) && !P.seg_offsets) {
        const int64_t next_base = band_base + (int64_t)(((c.val >> kRunLenShift) & kRunLenMask) + 1) * (int64_t)P.Bw;
        // the run before ends on a diagonal < band_base: its end positions reach band_base - 1 + m + k; the run behind
        // starts on a diagonal >= next_base: its end positions begin at next_base + m - k
        g.dd_lo = (c.val & kRunTouchLeft) ? band_base + g.m + g.k : INT64_MIN;
        g.dd_hi = (c.val & kRunTouchRight) ? next_base + g.m - g.k - 1 : INT64_MAX;
    }
    // ownership: last symbol e-1 in [own_b, own_e)
    if (g.e_lo < own_b + 1)
        g.e_lo = own_b + 1;
    if (g.e_hi > own_e)
        g.e_hi = own_e;
    if (g.e_lo > g.e_hi)
        return false;
    // cold start m+k symbols before the first end position (or at the haystack start)
    g.ws = g.e_lo - (g.m + g.k);
    if (g.ws < hay_b)
        g.ws = hay_b;
    return true;
}

// One lane per candidate.  Same recurrence and layout as the brute kernel (32-bit words, v_bitop3, needles
// top-aligned so that the score delta is bit 31 of the top word): the candidate's needle rows are staged from the
// brute table into LDS ([symbol][word][thread], conflict-free whatever the per-lane symbol), only the NWN top words
// that can hold needle rows are processed, and the text window is read in prefetched 16-byte blocks -- the
// per-symbol dependency chain is one LDS round trip.
template <int NWN>
__global__ __launch_bounds__(256) void verify_kernel(const verify_params P)
{
    // [sigma + 1][NWN][blockDim.x] words, then [16][blockDim.x] uint16: the hits of one text block, then per wave kHitStage
    // hit records on their way out
    extern __shared__ uint32_t vlds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t nthr = blockDim.x;
    const uint32_t rows = P.sigma + 1;
    uint16_t *hitbuf = reinterpret_cast<uint16_t *>(vlds + (size_t)rows * NWN * nthr);
    // Hits leave through a per-wave staging area: a repeat-rich text reports tens of millions of them, and one atomic on
    // the hit counter per wave and text block would be a million atomics on one word (~100 per microsecond).  The wave
    // appends to its stage without atomics and moves kHitStage records out at a time: one atomic, coalesced stores.
    spm_hit *stage = reinterpret_cast<spm_hit *>(hitbuf + (size_t)16 * nthr) + (size_t)(tid >> 6) * kHitStage;
    uint32_t n_staged = 0; // (wave-uniform)
    const uint32_t lane = tid & 63;
    auto flush = [&]() {
        if (n_staged == 0)
            return;
        unsigned long long base = 0;
        if (lane == 0)
            base = atomicAdd(P.hit_counter, (unsigned long long)n_staged);
        base = uniform_u64(base);
        for (uint32_t i = lane; i < n_staged; i += 64)
            if (base + i < P.hit_cap)
                P.hits[base + i] = stage[i];
        n_staged = 0;
        queue_sync();
    };
    unsigned long long n_cand = P.counters[P.band_counter];
    if (n_cand > P.band_cap)
        n_cand = P.band_cap; // overflow is handled by the host
    const uint64_t stride = (uint64_t)gridDim.x * nthr;
    uint32_t n_valid = 0;
    // wave-uniform trip count (the emission below is wave-collective); a lane without a band idles through the round
    const uint64_t rounds = (n_cand + stride - 1) / stride;
    for (uint64_t rd = 0; rd < rounds; ++rd) {
        const uint64_t ci = rd * stride + (uint64_t)blockIdx.x * nthr + tid;
        band_geom g;
        g.pat = 0;
        g.m = 1;
        g.k = 0;
        g.e_lo = 0;
        g.e_hi = -1;
        g.ws = 0;
        // (false: an unused list slot, too few seed hits, or nothing owned)
        // (runs: the list holds heads only and band_release_kernel gives the slots back afterwards)
        const bool active = ci < n_cand && decode_band(P, P.bands[ci], P.runs == 0, g);
        if (active)
            ++n_valid;
        const uint32_t pat = g.pat;
        const int64_t m = g.m, k = g.k, e_lo = g.e_lo, e_hi = active ? g.e_hi : g.ws, ws = g.ws;
        // stage this needle's rows: brute table [group][row][word][lane], top NWN words
        const uint32_t *src = P.peq32 + (((size_t)(pat >> 6) * rows) * P.nw_table + (P.nw_table - NWN)) * 64 + (pat & 63);
        if (active)
            for (uint32_t r = 0; r < rows; ++r)
#pragma unroll
                for (int w = 0; w < NWN; ++w)
                    vlds[((size_t)r * NWN + w) * nthr + tid] = src[((size_t)r * P.nw_table + w) * 64];
        myers_lane<NWN, false> L;
        {
            const int32_t off = NWN * 32 - (int32_t)m;
#pragma unroll
            for (int w = 0; w < NWN; ++w) {
                const int32_t lo = off - w * 32;
                L.VP[w] = lo <= 0 ? 0xFFFFFFFFu : (lo >= 32 ? 0u : (0xFFFFFFFFu << lo));
                L.VN[w] = 0;
            }
            L.score = (int32_t)m;
        }
        const int64_t blk0 = ws & ~15ll;
        uint4 nxt = make_uint4(0, 0, 0, 0);
        if (active)
            nxt = load_text16(P.text, (uint64_t)blk0, P.text_alloc);
        // columns in 32-bit terms relative to the cold start: rel = p - ws in [0, n_cols); end positions from rel_lo on
        const uint32_t n_cols = (uint32_t)(e_hi - ws);
        const uint32_t rel_lo = (uint32_t)(e_lo - 1 - ws);
        const uint32_t sigma = P.sigma;
        uint32_t rel0 = (uint32_t)(blk0 - ws); // (wraps below zero for the symbols of the first block before ws)
        // The text goes by in 16-symbol blocks; the wave steps through them together (trip count: its longest lane -- the
        // head of a run of bands has up to 1.7 times the columns of a single band) and emits the hits of a block right
        // behind it, all lanes at once: one CAS per hit that needs the dedupe set, then into the wave's stage.
        const uint32_t my_blocks = active ? (uint32_t)((e_hi - blk0 + 15) >> 4) : 0u;
        uint32_t max_blocks = my_blocks; // (flat: through wave.hpp's wave_max every instantiation is scheduled differently)
        for (int o = 32; o > 0; o >>= 1)
            max_blocks = max(max_blocks, (uint32_t)__shfl_xor((int)max_blocks, o));
        max_blocks = (uint32_t)__builtin_amdgcn_readfirstlane(max_blocks);
        for (uint32_t bi = 0; bi < max_blocks; ++bi, rel0 += 16) {
            const int64_t blk = blk0 + 16 * (int64_t)bi;
            uint32_t hitmask = 0;
            if (bi < my_blocks) {
                const uint4 cur = nxt;
                if (bi + 1 < my_blocks)
                    nxt = load_text16(P.text, (uint64_t)(blk + 16), P.text_alloc);
                const uint32_t words[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t rel = rel0 + (uint32_t)i;
                    if (rel >= n_cols)
                        continue;
                    uint32_t sym = (words[i >> 2] >> (8 * (i & 3))) & 0xFF;
                    sym = sym < sigma ? sym : sigma;
                    L.step_strided(vlds + ((size_t)sym * NWN) * nthr + tid, nthr);
                    if (L.score <= (int32_t)k && rel >= rel_lo) {
                        hitbuf[(size_t)i * nthr + tid] = (uint16_t)(L.score + 1);
                        hitmask |= 1u << i;
                    }
                }
            }
            if (__ballot(hitmask != 0) == 0)
                continue;
            // pass 1: dedupe across the seeds / bands of one occurrence; what stays in `keep` is new
            uint32_t fresh = 0, keep = 0;
            for (uint32_t mm = hitmask; mm != 0; mm &= mm - 1) {
                const uint32_t i = (uint32_t)__ffs(mm) - 1u;
                const int64_t e = blk + (int64_t)i + 1; // (exclusive end of an occurrence ending at symbol blk + i)
                if ((e > g.dd_lo && e < g.dd_hi) || seen_insert(P, pat, e)) {
                    ++fresh;
                    keep |= 1u << i;
                }
            }
            // pass 2: into the wave's stage (every lane behind the lanes before it)
            uint32_t incl = fresh; // (flat: through wave_prefix_incl three instantiations name their scalar registers differently)
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= (uint32_t)o)
                    incl += up;
            }
            const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)incl, 63));
            if (total == 0)
                continue;
            if (n_staged + total > kHitStage)
                flush();
            unsigned long long direct = 0; // more hits in one block than the stage holds: straight to the hit list
            const bool staged = total <= kHitStage;
            if (!staged) {
                if (lane == 0)
                    direct = atomicAdd(P.hit_counter, (unsigned long long)total);
                direct = uniform_u64(direct);
            }
            uint32_t at = n_staged + incl - fresh;
            for (uint32_t mm = keep; mm != 0; mm &= mm - 1) {
                const uint32_t i = (uint32_t)__ffs(mm) - 1u;
                const int64_t e = blk + (int64_t)i + 1;
                spm_hit h;
                h.pos = (P.report_begin ? (uint64_t)(e - m) : (uint64_t)e) + P.pos_offset;
                h.pattern = pat;
                h.score = (int32_t)hitbuf[(size_t)i * nthr + tid] - 1;
                if (staged)
                    stage[at] = h;
                else if (direct + at < P.hit_cap)
                    P.hits[direct + at] = h;
                ++at;
            }
            if (staged)
                n_staged += total;
            queue_sync();
        }
    }
    flush();
    wave_count_add(P.hit_counter + kCntBandsVerified, n_valid); // bands verified
}


// ---- wave-per-candidate verification for long needles ----------------------------------------------------------
// One lane per 32-row block of the needle instead of one lane per candidate: G lanes form a systolic array that runs
// the block-based Myers recurrence (Myers 1999 / Hyyro 2003: every block takes the horizontal delta hin of the block
// above and hands its own hout down).  At step t lane b processes text column t - b; the text symbol and hout travel
// one lane per step through DPP wave_shr:1.  A column of a 1024-row needle costs one step of ~40 instructions
// instead of 32 blocks x 13 on a single lane, so the latency of one verification drops from ~1.5 ms to ~0.1 ms --
// what matters when a scan leaves a few hundred long bands to verify.  Reads the bottom-aligned table of the cut-off
// kernel ([group][row][nw_table][64]); each lane keeps the <= 5 match masks of its block in registers.
// NB: 32-row blocks per lane.  A scan leaves a few thousand long bands; with one block per lane a |P| = 1024 band takes 32
// lanes, a wave holds two bands, and 2 800 bands are 1 400 busy waves on 1 024 SIMDs: the SIMDs that got two of them run
// every step twice, and they set the kernel's duration.  Two blocks per lane (the second takes the first one's hout in the
// same step) put four bands into a wave -- 700 busy waves, at most one per SIMD -- at ~1.7x the instructions of a step.
// Measured on C5 (2 798 bands of |P| = 1024): one block per lane 0.300 ms, two 0.358 -- a step is a chain of dependent
// instructions, and the second block lengthens it -- so only NB = 1 is launched.  (Written out without the NB loops, the
// kernel compiles to the same registers but a schedule that measured 2 % slower.)
template <int G, int NB>
__global__ __launch_bounds__(256) void verify_wave_kernel(const verify_params P, const uint32_t *__restrict__ peq_bot)
{
    // per group of G lanes: [2*max_k + 1 + max_span] uint16 hit slots, then the candidate's text window (wave_text bytes)
    extern __shared__ uint16_t whit[];
    constexpr uint32_t GPW = 64 / G;
    const uint32_t lane = threadIdx.x & 63, gl = lane & (G - 1), gw = lane / G;
    const uint32_t wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint32_t n_slots = 2 * P.max_k + 1 + P.max_span;
    const uint32_t group_bytes = ((n_slots * 2 + 15) & ~15u) + P.wave_text;
    uint8_t *gbase = reinterpret_cast<uint8_t *>(whit) + (size_t)(wave * GPW + gw) * group_bytes;
    uint16_t *hb = reinterpret_cast<uint16_t *>(gbase);
    uint8_t *tw = gbase + ((n_slots * 2 + 15) & ~15u);
    for (uint32_t r = gl; r < n_slots; r += G)
        hb[r] = 0;
    unsigned long long n_cand = P.counters[P.band_counter];
    if (n_cand > P.band_cap)
        n_cand = P.band_cap;
    const uint64_t stride = (uint64_t)gridDim.x * waves * GPW;
    const uint32_t rows = P.sigma + 1;
    uint32_t n_valid = 0;
    for (uint64_t base = ((uint64_t)blockIdx.x * waves + wave) * GPW; base < n_cand; base += stride) {
        const uint64_t ci = base + gw;
        bool active = ci < n_cand;
        uint32_t pat = 0;
        int64_t m = 1, k = 0, e_lo = 0, e_hi = -1, ws = 0;
        band_rec c;
        c.val = kBandInvalid;
        c.slot = 0;
        if (active)
            c = P.bands[ci];
        {
            band_geom g;
            g.pat = 0;
            g.m = 1;
            g.k = 0;
            g.e_lo = 0;
            g.e_hi = -1;
            g.ws = 0;
            active = active && decode_band(P, c, false, g); // every lane of the group reads the band's count ...
            pat = g.pat;
            m = g.m;
            k = g.k;
            e_lo = g.e_lo;
            e_hi = g.e_hi;
            ws = g.ws;
        }
        __builtin_amdgcn_wave_barrier();
        if (gl == 0 && c.val != kBandInvalid && !P.preselected) // ... then one of them gives the table slot back
            band_release(P.band_tab, c.slot);
        if (active && gl == 0)
            ++n_valid;
        const uint32_t nbk = (uint32_t)((m + 31) >> 5);       // blocks of this needle
        const uint32_t nb = (nbk + NB - 1) / NB;              // lanes that hold them
        const uint32_t n_cols = active ? (uint32_t)(e_hi - ws) : 0u;
        const bool mine = active && gl < nb;
        const bool lane_last = gl + 1 == nb;                  // holds the needle's last block, at index j_last
        const uint32_t j_last = (nbk - 1) % NB;
        uint32_t out_bit[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j)
            out_bit[j] = (gl * NB + (uint32_t)j + 1 == nbk) ? (uint32_t)((m - 1) & 31) : 31u; // where block j's hout is read
        // ---- stage the text window [ws, e_hi) into LDS: 16-byte blocks, the group's lanes side by side ----
        const uint32_t skew = (uint32_t)(ws & 15);
        uint32_t beyond4 = 0; // a byte >= 4 somewhere in the window (never in a validated dna4 text)
        if (active) {
            const uint32_t n_bytes = (skew + n_cols + 15) & ~15u;
            for (uint32_t off = gl * 16; off < n_bytes; off += G * 16) {
                const uint4 v = load_text16(P.text, ((uint64_t)ws & ~15ull) + off, P.text_alloc);
                *reinterpret_cast<uint4 *>(tw + off) = v;
                beyond4 |= (v.x | v.y | v.z | v.w) & 0xFCFCFCFCu;
            }
        }
        const bool plain4 = P.sigma == 4 && __ballot(beyond4 != 0) == 0; // (wave-uniform) every symbol selects a match mask
        uint32_t e0[NB], e1[NB], e2[NB], e3[NB], e4[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            e0[j] = e1[j] = e2[j] = e3[j] = e4[j] = 0;
            const uint32_t gb = gl * NB + (uint32_t)j; // (a block beyond the needle matches nothing)
            if (mine && gb < nbk) {
                const uint32_t *src = peq_bot + (((size_t)(pat >> 6) * rows) * P.nw_table + gb) * 64 + (pat & 63);
                const size_t rs = (size_t)P.nw_table * 64;
                e0[j] = src[0];
                e1[j] = src[rs];
                e2[j] = P.sigma > 2 ? src[2 * rs] : 0u;
                e3[j] = P.sigma > 3 ? src[3 * rs] : 0u;
                e4[j] = P.sigma > 4 ? src[4 * rs] : 0u;
            }
        }
        queue_sync();
        uint32_t Pv[NB], Mv[NB], ho = 0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            Pv[j] = 0xFFFFFFFFu;
            Mv[j] = 0;
        }
        int32_t score = (int32_t)m;
        bool any_hit = false;
        const uint32_t first_slot_col = (uint32_t)(e_lo - ws) - 1; // column whose end position is e_lo
        const uint32_t t_end = n_cols + nb - 1;                    // steps until the last block has seen the last column
        // wave-uniform trip count: the longest group decides
        uint32_t t_wave = active ? t_end : 0u;
        // ... and the steps in which EVERY block of every band of the wave has a column of its window: [t_lo, t_hi)
        uint32_t t_lo = active ? nb - 1 : 0u, t_hi = active ? n_cols : 0xFFFFFFFFu;
        // ... and the first step at which a band of the wave can report an end position (its last block reaches the column
        // of e_lo): the steps before it -- three in four for |P| = 1024, k = 64 -- do not look for hits at all
        uint32_t t_hit = active ? first_slot_col + nb - 1 : 0xFFFFFFFFu;
        for (int o = 32; o >= (int)G; o >>= 1) { // (flat: four butterflies in one loop; one after the other they cost 15 instructions less, not the same code)
            t_wave = max(t_wave, (uint32_t)__shfl_xor((int)t_wave, o));
            t_lo = max(t_lo, (uint32_t)__shfl_xor((int)t_lo, o));
            t_hi = min(t_hi, (uint32_t)__shfl_xor((int)t_hi, o));
            t_hit = min(t_hit, (uint32_t)__shfl_xor((int)t_hit, o));
        }
        t_wave = (uint32_t)__builtin_amdgcn_readfirstlane(t_wave);
        t_lo = (uint32_t)__builtin_amdgcn_readfirstlane(t_lo);
        t_hi = (uint32_t)__builtin_amdgcn_readfirstlane(t_hi);
        t_hit = (uint32_t)__builtin_amdgcn_readfirstlane(t_hit);
        t_hi = t_hi > t_wave ? t_wave : t_hi;
        t_lo = t_lo > t_hi ? t_hi : t_lo;
        t_hit = t_hit < t_lo ? t_lo : (t_hit > t_hi ? t_hi : t_hit);
        uint32_t sym_next = mine ? tw[skew] : 0u; // column 0 (clamped reads below keep every index inside the window)
        // One step of one lane's blocks.  CHECKED: the lane may have no column at this step (the pipeline fills and drains,
        // or a shorter band shares the wave).  The steps in between -- nearly all -- run without exec-mask changes and with
        // the match mask picked by bit selects instead of compare / cndmask chains: a band is a serial chain of ~1500
        // steps, so the scan pays for every instruction and every VALU -> SALU hand-over of a step.
        // (unchecked steps: a lane that holds a block reads its own column, any other lane anything inside its group's LDS;
        // only the lane of the last block can meet score <= k_hit)
        const uint8_t *my_text = mine ? tw + skew - gl : tw;
        const int32_t k_hit = (lane_last && mine) ? (int32_t)k : -1;
        const uint32_t n_rel = n_cols - first_slot_col; // end-position slots of this band
        auto step = [&](uint32_t t, auto checked, auto dna4, auto hits) {
            const uint32_t ho_up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ho, 0x138, 0xF, 0xF, false);
            const uint32_t col = t - gl; // wraps for t < gl: then col >= n_cols
            const uint32_t sym = sym_next;
            if constexpr (decltype(checked)::value) { // next column's symbol, one step ahead of its use
                uint32_t nc = col + 1;
                nc = nc < n_cols ? nc : 0u;
                sym_next = tw[skew + nc];
            } else {
                sym_next = my_text[t + 1];
            }
            if (!decltype(checked)::value || (mine && col < n_cols)) {
                uint32_t hin = gl == 0 ? 0u : ho_up;
                uint32_t s0 = 0, s1 = 0;
                if constexpr (decltype(dna4)::value) {
                    s0 = (uint32_t)((int32_t)(sym << 31) >> 31);
                    s1 = (uint32_t)((int32_t)(sym << 30) >> 31);
                }
                int32_t d_last = 0; // op - on of the needle's last block (meaningful on its lane only)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    uint32_t Eq;
                    if constexpr (decltype(dna4)::value) {
                        const uint32_t lo2 = (e1[j] & s0) | (e0[j] & ~s0), hi2 = (e3[j] & s0) | (e2[j] & ~s0);
                        Eq = (hi2 & s1) | (lo2 & ~s1); // (plain4: no symbol beyond 3 in the window)
                    } else {
                        const uint32_t lo2 = (sym & 1u) ? e1[j] : e0[j], hi2 = (sym & 1u) ? e3[j] : e2[j];
                        Eq = (sym & 2u) ? hi2 : lo2;
                        Eq = sym < 4 ? Eq : (sym == 4 ? e4[j] : 0u);
                        Eq = sym < P.sigma ? Eq : 0u;
                    }
                    const uint32_t hp = hin & 1u, hn = hin >> 1;
                    const uint32_t Xv = Eq | Mv[j];
                    Eq |= hn;
                    const uint32_t Xh = (((Eq & Pv[j]) + Pv[j]) ^ Pv[j]) | Eq;
                    uint32_t Ph = Mv[j] | ~(Xh | Pv[j]);
                    uint32_t Mh = Pv[j] & Xh;
                    const uint32_t op = (Ph >> out_bit[j]) & 1u, on = (Mh >> out_bit[j]) & 1u;
                    hin = op | (on << 1); // this block's hout: the next block's hin, in this very step
                    Ph = (Ph << 1) | hp;
                    Mh = (Mh << 1) | hn;
                    Pv[j] = Mh | ~(Xv | Ph);
                    Mv[j] = Ph & Xv;
                    if (NB == 1 || (uint32_t)j == j_last)
                        d_last = (int32_t)op - (int32_t)on;
                }
                ho = hin;
                score += d_last;
                if constexpr (decltype(hits)::value) {
                    const uint32_t rel = col - first_slot_col;
                    if (score <= k_hit && rel < n_rel) {
                        hb[rel] = (uint16_t)(score + 1);
                        any_hit = true;
                    }
                }
            }
        };
        uint32_t t = 0;
        for (; t < t_lo; ++t)
            step(t, std::true_type{}, std::false_type{}, std::true_type{});
        if (plain4) {
            for (; t < t_hit; ++t)
                step(t, std::false_type{}, std::true_type{}, std::false_type{});
            for (; t < t_hi; ++t)
                step(t, std::false_type{}, std::true_type{}, std::true_type{});
        } else {
            for (; t < t_hi; ++t)
                step(t, std::false_type{}, std::false_type{}, std::true_type{});
        }
        for (; t < t_wave; ++t)
            step(t, std::true_type{}, std::false_type{}, std::true_type{});
        // ---- emission: the lanes of a group share its slots; wave-converged appends ----
        queue_sync();
        if (__ballot(any_hit) != 0) {
            // pass 1: every lane of a group takes the slots r = gl, gl + G, ..: dedupe, keep what is new
            const uint32_t nr = active ? (uint32_t)(e_hi - e_lo) + 1 : 0u;
            uint32_t fresh = 0;
            for (uint32_t r = gl; r < nr; r += G) {
                const uint32_t sc1 = hb[r];
                if (sc1) {
                    if (seen_insert(P, pat, e_lo + (int64_t)r))
                        ++fresh;
                    else
                        hb[r] = 0;
                }
            }
            // pass 2: one reservation for the wave, then every lane writes its run
            unsigned long long idx = wave_reserve_hits(P.hit_counter, fresh);
            for (uint32_t r = gl; r < nr; r += G) {
                const uint32_t sc1 = hb[r];
                hb[r] = 0;
                if (sc1) {
                    if (idx < P.hit_cap) {
                        const int64_t e = e_lo + (int64_t)r;
                        spm_hit h;
                        h.pos = (P.report_begin ? (uint64_t)(e - m) : (uint64_t)e) + P.pos_offset;
                        h.pattern = pat;
                        h.score = (int32_t)sc1 - 1;
                        P.hits[idx] = h;
                    }
                    ++idx;
                }
            }
        }
        queue_sync();
    }
    wave_count_add(P.hit_counter + kCntBandsVerified, n_valid); // bands verified
}

} // namespace spm_hip
