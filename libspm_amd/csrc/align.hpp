// align.hpp -- kernels of spm_hip_hits_align (align.hip): the begin and the CIGAR transcript of every Myers hit.
//
// Stage A (begin): a backward GLOBAL Myers bit-vector scan of the reversed needle over text[e-1], text[e-2], ...: the top
// row gets +1 at every column (D[0][j] = j), so after j symbols the bottom-row score is ED(P, text[e-j, e)).  The first j
// whose score equals the hit's distance d gives the largest begin b = e - j (the score is never below d: d is the minimum
// over every begin >= lo).  It stops at lo, and at j = |P| + d at the latest.  Blocks of 64-bit words exchange only their
// horizontal delta (Hyyro's block formulation: a -1 carried into a block is OR-ed into its match mask).
//   * align_begin_lane_kernel<NW>: one lane per hit, NW = ceil(|P|/64) words in registers (|P| <= 256).
//   * align_begin_wave_kernel: one wave per hit, word w on lane w; lane w runs column j at step j + w (a systolic
//     pipeline: the delta out of word w - 1 for column j arrives by a lane shift one step earlier).
// Stage B (transcript): a banded global DP of P against text[b, e).  Every cell of a cost-d path lies on a diagonal
// j - i in [max(-d, n-m-d), min(d, n-m+d)] (n = e - b, m = |P|), at most 2d + 1 of them.
//   * align_cigar_kernel: one lane per hit, the band row (one word per diagonal) and 2-bit traceback directions (16 per
//     word) in an LDS slot of <= 256 words; the 64 slots of a workgroup are interleaved so that its lanes touch
//     consecutive words.
//   * align_cigar_wave_kernel<kLds>: one wave per hit for larger slots (long needles, large d): the diagonals across the
//     lanes, a row as a wave-wide min-scan, the directions as ballots; the slot in LDS (<= 64 KiB) or in a global scratch
//     slice.
#pragma once

#include "common.hpp"

namespace spm_hip
{

// one hit to align (40 bytes); e and lo in text coordinates
struct aln_item
{
    uint64_t e;
    uint64_t lo;
    uint32_t pattern;
    int32_t d;
    uint32_t m;
    uint32_t cigar_off; // first word of the transcript in the ops pool
    uint32_t rec;       // device record index (= device hit index)
    uint32_t pad;
};
static_assert(sizeof(aln_item) == 40, "aln_item layout");
static_assert(sizeof(spm_aln) == 32, "spm_aln is 32 bytes");

struct align_params
{
    const uint8_t *text;
    const uint64_t *rpeq;         // reversed needles' match masks: [sigma][ceil(m/64)] words from rpeq_off[p]
    const uint32_t *rpeq_off;
    const uint8_t *ranks;         // needle ranks, needle p = ranks[offsets[p] ..)
    const uint32_t *offsets;
    uint32_t sigma;
    uint64_t pos_offset;
    spm_aln *recs;                // device order
    uint32_t *ops;
    unsigned long long *err;      // [0] begins not found, [1] transcripts that failed their own check
};

constexpr uint32_t kAlnInf = 0x3FFFFFFFu;

// one 64-bit block of the Myers recurrence, horizontal delta hin (-1, 0, +1) in from above; returns the delta out of its
// last row and leaves the block's pre-shift Ph / Mh (bit r: row r + 1 of the block went up / down by one)
__device__ __forceinline__ int myers_block(uint64_t &pv, uint64_t &mv, uint64_t eq, int hin, uint64_t &ph_pre,
                                           uint64_t &mh_pre)
{
    const uint64_t neg = hin < 0 ? 1ull : 0ull;
    const uint64_t xv = eq | mv;
    eq |= neg;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    ph_pre = ph;
    mh_pre = mh;
    const int hout = (int)(ph >> 63) - (int)(mh >> 63);
    ph = (ph << 1) | (hin > 0 ? 1ull : 0ull);
    mh = (mh << 1) | neg;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}

__device__ __forceinline__ void write_begin(const align_params &P, const aln_item &it, uint64_t b)
{
    spm_aln r;
    r.begin = b + P.pos_offset;
    r.end = it.e + P.pos_offset;
    r.pattern = it.pattern;
    r.score = it.d;
    r.cigar_off = it.cigar_off;
    r.cigar_len = 0;
    P.recs[it.rec] = r;
}

template <int NW>
__global__ __launch_bounds__(256) void align_begin_lane_kernel(align_params P, const aln_item *__restrict__ items, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const aln_item it = items[i];
    const uint32_t m = it.m;
    const int d = it.d;
    const uint64_t jmax = min<uint64_t>((uint64_t)m + (uint64_t)d, it.e - it.lo);
    const uint64_t *eqb = P.rpeq + P.rpeq_off[it.pattern];
    const uint8_t *t = P.text + it.e - 1;
    const uint32_t lb = (m - 1) & 63; // bottom row's bit in the last word
    uint64_t pv[NW], mv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        pv[w] = ~0ull;
        mv[w] = 0;
    }
    int score = (int)m;
    uint64_t j = 0;
    while (score != d && j < jmax) {
        const uint64_t *eq = eqb + (uint32_t)t[-(int64_t)j] * NW;
        int h = 1;
        uint64_t ph, mh;
#pragma unroll
        for (int w = 0; w < NW; ++w)
            h = myers_block(pv[w], mv[w], eq[w], h, ph, mh);
        score += (int)((ph >> lb) & 1) - (int)((mh >> lb) & 1);
        ++j;
    }
    if (score != d) {
        atomicAdd(&P.err[0], 1ull);
        j = 0;
    }
    write_begin(P, it, it.e - j);
}

// one wave per hit (blockDim 256: four hits per workgroup)
__global__ __launch_bounds__(256) void align_begin_wave_kernel(align_params P, const aln_item *__restrict__ items, uint32_t n)
{
    const uint32_t wv = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int lane = (int)(threadIdx.x % kWave);
    if (wv >= n)
        return; // (whole waves: wv is uniform across the wave)
    const aln_item it = items[wv];
    const uint32_t m = it.m;
    const int d = it.d;
    const int nw = (int)((m + 63) / 64);
    const int64_t jmax = (int64_t)min<uint64_t>((uint64_t)m + (uint64_t)d, it.e - it.lo);
    const uint64_t *eqb = P.rpeq + P.rpeq_off[it.pattern];
    const uint8_t *t = P.text + it.e - 1;
    const uint32_t lb = (m - 1) & 63;
    uint64_t pv = ~0ull, mv = 0;
    int score = (int)m;
    int64_t found = score == d ? 0 : -1;
    int hin = 1;
    const int64_t steps = jmax + nw - 1;
    for (int64_t s = 0; found < 0 && s < steps; ++s) {
        const int64_t j = s - lane;
        int hout = 0;
        int64_t mine = -1;
        if (lane < nw && j >= 0 && j < jmax) {
            uint64_t ph, mh;
            const uint64_t eq = eqb[(uint32_t)t[-j] * (uint32_t)nw + (uint32_t)lane];
            hout = myers_block(pv, mv, eq, lane == 0 ? 1 : hin, ph, mh);
            if (lane == nw - 1) {
                score += (int)((ph >> lb) & 1) - (int)((mh >> lb) & 1);
                if (score == d)
                    mine = j + 1;
            }
        }
        hin = __shfl_up(hout, 1, kWave);
        // the bottom lane's verdict, to every lane (at most one lane can have one)
        const unsigned long long hit = __ballot(mine >= 0);
        if (hit) {
            const int src = __ffsll((long long)hit) - 1;
            found = __shfl(mine, src, kWave);
        }
    }
    if (lane == 0) {
        if (found < 0) {
            atomicAdd(&P.err[0], 1ull);
            found = 0;
        }
        write_begin(P, it, it.e - (uint64_t)found);
    }
}

// Walk back from (m, nt) along the stored directions (0 diagonal, 1 insertion, 2 deletion); the runs are written back to
// front into the record's slice, then reversed in place.  A transcript that leaves the band or outgrows 2d + 1 runs
// counts as an error.
template <typename dir_at_t>
__device__ void trace_back(const align_params &P, const aln_item &it, const uint8_t *pat, const uint8_t *txt, int m, int nt,
                           int lo_off, int W, dir_at_t dir_at)
{
    uint32_t *out = P.ops + it.cigar_off;
    const uint32_t cap = 2u * (uint32_t)it.d + 1u;
    uint32_t nrun = 0, cur = 0, len = 0;
    bool bad = false;
    int r = m, j = nt;
    while (r > 0 || j > 0) {
        uint32_t op;
        if (r == 0) {
            op = SPM_CIGAR_DEL;
        } else if (j == 0) {
            op = SPM_CIGAR_INS;
        } else {
            const int t = j - r - lo_off;
            if (t < 0 || t >= W) {
                bad = true;
                break;
            }
            const uint32_t dir = dir_at(r, t);
            const uint32_t p = pat[r - 1];
            op = dir == 1 ? SPM_CIGAR_INS : dir == 2 ? SPM_CIGAR_DEL : (p < P.sigma && txt[j - 1] == p) ? SPM_CIGAR_EQ : SPM_CIGAR_X;
        }
        if (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X) {
            --r;
            --j;
        } else if (op == SPM_CIGAR_INS) {
            --r;
        } else {
            --j;
        }
        if (op == cur) {
            ++len;
        } else {
            if (len) {
                if (nrun >= cap) {
                    bad = true;
                    break;
                }
                out[nrun++] = len << 4 | cur;
            }
            cur = op;
            len = 1;
        }
    }
    if (!bad && len) {
        if (nrun >= cap)
            bad = true;
        else
            out[nrun++] = len << 4 | cur;
    }
    if (bad) {
        atomicAdd(&P.err[1], 1ull);
        return;
    }
    for (uint32_t a = 0, z = nrun ? nrun - 1 : 0; a < z; ++a, --z) {
        const uint32_t x = out[a];
        out[a] = out[z];
        out[z] = x;
    }
    P.recs[it.rec].cigar_len = nrun;
}

// Banded DP + traceback, one lane per hit, the slot in LDS (blockDim 64, slots interleaved with stride 64).
__global__ __launch_bounds__(64) void align_cigar_kernel(align_params P, const aln_item *__restrict__ items,
                                                         const uint32_t *__restrict__ order, uint32_t n)
{
    extern __shared__ uint32_t lds_slots[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const aln_item it = items[order[i]];
    uint32_t *slot = lds_slots + threadIdx.x;
    const uint32_t stride = kWave;
    const int m = (int)it.m, d = it.d;
    const uint64_t b = P.recs[it.rec].begin - P.pos_offset;
    const int nt = (int)(it.e - b);
    const uint8_t *pat = P.ranks + P.offsets[it.pattern];
    const uint8_t *txt = P.text + b;
    const int lo_off = max(-d, nt - m - d), hi_off = min(d, nt - m + d);
    const int W = hi_off - lo_off + 1;
    uint32_t *row = slot;                       // words [0, W)
    uint32_t *dirs = slot + (size_t)W * stride; // words [W, W + ceil(m W / 16))
    for (int t = 0; t < W; ++t) {
        const int j = lo_off + t;
        row[(size_t)t * stride] = (j >= 0 && j <= nt) ? (uint32_t)j : kAlnInf;
    }
    uint32_t acc = 0, nb = 0;
    size_t dw = 0;
    for (int r = 1; r <= m; ++r) {
        const uint32_t p = pat[r - 1];
        const bool p_ok = p < P.sigma;
        uint32_t left = kAlnInf;
        uint32_t up = row[0];
        for (int t = 0; t < W; ++t) {
            const int j = r + lo_off + t;
            const uint32_t old = up;                                   // D[r-1][j-1]
            up = t + 1 < W ? row[(size_t)(t + 1) * stride] : kAlnInf;  // D[r-1][j]
            uint32_t v = kAlnInf, dir = 0;
            if (j >= 0 && j <= nt) {
                v = j >= 1 ? old + ((p_ok && txt[j - 1] == p) ? 0u : 1u) : kAlnInf;
                if (up + 1 < v) {
                    v = up + 1;
                    dir = 1;
                }
                if (left + 1 < v) {
                    v = left + 1;
                    dir = 2;
                }
                v = min(v, kAlnInf);
            }
            row[(size_t)t * stride] = v;
            left = v;
            acc |= dir << (2 * nb);
            if (++nb == 16) {
                dirs[dw * stride] = acc;
                ++dw;
                acc = 0;
                nb = 0;
            }
        }
    }
    if (nb)
        dirs[dw * stride] = acc;
    const int t_end = nt - m - lo_off;
    if (t_end < 0 || t_end >= W || row[(size_t)t_end * stride] != (uint32_t)d) {
        atomicAdd(&P.err[1], 1ull);
        return;
    }
    trace_back(P, it, pat, txt, m, nt, lo_off, W, [&](int r, int t) {
        const size_t idx = (size_t)(r - 1) * W + t;
        return (dirs[(idx / 16) * stride] >> (2 * (idx % 16))) & 3u;
    });
}

// Banded DP + traceback, one wave per hit (long needles: the C5 shape, |P| = 1024, d <= 64 and beyond).  The band's
// diagonals lie across the lanes, 64 per chunk; a row is D[t] = min(x[t], D[t-1] + 1) with x the diagonal / vertical
// candidates, i.e. t + the running minimum of x[t'] - t' -- one wave-wide min-scan per chunk, the minimum so far carried
// from chunk to chunk.  The directions of a chunk are two ballots (bit 0, bit 1 of the 64 cells), four words per chunk
// and row.  The slot (band row W words, then m * nch * 4 direction words) is in LDS (kLds) or at gstore + block * slot_words.
template <bool kLds>
__global__ __launch_bounds__(64) void align_cigar_wave_kernel(align_params P, const aln_item *__restrict__ items,
                                                              const uint32_t *__restrict__ order, uint32_t n,
                                                              uint32_t *__restrict__ gstore, uint64_t slot_words)
{
    extern __shared__ uint32_t lds_slots[];
    if (blockIdx.x >= n)
        return;
    const int lane = (int)threadIdx.x;
    const aln_item it = items[order[blockIdx.x]];
    uint32_t *slot = kLds ? lds_slots : gstore + (size_t)blockIdx.x * slot_words;
    const int m = (int)it.m, d = it.d;
    const uint64_t b = P.recs[it.rec].begin - P.pos_offset;
    const int nt = (int)(it.e - b);
    const uint8_t *pat = P.ranks + P.offsets[it.pattern];
    const uint8_t *txt = P.text + b;
    const int lo_off = max(-d, nt - m - d), hi_off = min(d, nt - m + d);
    const int W = hi_off - lo_off + 1;
    const int nch = (W + kWave - 1) / kWave;
    uint32_t *row = slot;
    uint32_t *dirs = slot + W;
    for (int t = lane; t < W; t += kWave) {
        const int j = lo_off + t;
        row[t] = (j >= 0 && j <= nt) ? (uint32_t)j : kAlnInf;
    }
    __threadfence_block();
    __syncthreads();
    for (int r = 1; r <= m; ++r) {
        const uint32_t p = pat[r - 1];
        const bool p_ok = p < P.sigma;
        int carry = (int)kAlnInf;
        for (int c = 0; c < nch; ++c) {
            const int t = c * kWave + lane;
            const int j = r + lo_off + t;
            const bool in = t < W && j >= 0 && j <= nt;
            uint32_t diag = kAlnInf, upv = kAlnInf;
            if (in) {
                const uint32_t old = row[t];                              // D[r-1][j-1]
                const uint32_t up = t + 1 < W ? row[t + 1] : kAlnInf;   // D[r-1][j]
                if (j >= 1)
                    diag = min(old + ((p_ok && txt[j - 1] == p) ? 0u : 1u), kAlnInf);
                upv = min(up + 1, kAlnInf);
            }
            int key = (int)min(diag, upv) - t;
            for (int o = 1; o < kWave; o <<= 1) {
                const int y = __shfl_up(key, o, kWave);
                if (lane >= o)
                    key = min(key, y);
            }
            key = min(key, carry);
            carry = __shfl(key, kWave - 1, kWave);
            const uint32_t v = in ? min((uint32_t)(key + t), kAlnInf) : kAlnInf;
            const uint32_t dir = !in || diag == v ? 0u : upv == v ? 1u : 2u;
            const unsigned long long b0 = __ballot(dir & 1u), b1 = __ballot(dir >> 1);
            if (t < W)
                row[t] = v;
            if (lane == 0) {
                uint32_t *w = dirs + ((size_t)(r - 1) * nch + c) * 4;
                w[0] = (uint32_t)b0;
                w[1] = (uint32_t)(b0 >> 32);
                w[2] = (uint32_t)b1;
                w[3] = (uint32_t)(b1 >> 32);
            }
        }
        __threadfence_block();
        __syncthreads();
    }
    if (lane != 0)
        return;
    const int t_end = nt - m - lo_off;
    if (t_end < 0 || t_end >= W || row[t_end] != (uint32_t)d) {
        atomicAdd(&P.err[1], 1ull);
        return;
    }
    trace_back(P, it, pat, txt, m, nt, lo_off, W, [&](int r, int t) {
        const uint32_t *w = dirs + ((size_t)(r - 1) * nch + t / kWave) * 4;
        const int bit = t % kWave, h = bit >> 5;
        return ((w[h] >> (bit & 31)) & 1u) | (((w[2 + h] >> (bit & 31)) & 1u) << 1);
    });
}

} // namespace spm_hip
