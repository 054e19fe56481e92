// jst_sam.hpp -- SAM lines and MAPQ (spm_hip_jst_ref_loci_sam; contract in spm_hip.h, scheme in DESIGN.md 4.11, the rule in
// jst_sam_core.hpp).  gfx950.  Unit: jst_sam.hip.  It reads the handles of the loci, reads, pairs and rescues (jst_handles.hpp)
// and makes a spm_sam (output_handles.hpp).
//   jst_sam_first_rescue_kernel   one lane per rescue record: the ordering test against the record before it, and the first
//                                 record of every pair scattered into first_rescue[pair];
//   jst_sam_lines_kernel<kEmit>   one lane per read: the agreement tests, the reported line of the read (both mates of a pair
//                                 derive the pair's plan: it is a function of the records alone) and, first, the number of
//                                 its lines; an exclusive sum later, the same lanes write the line records;
//   jst_sam_measure_kernel        one lane per line: the record resolved against its sources (every index tested), the byte
//                                 length of the line by the measuring sink;
//   jst_sam_write_kernel<kExtras> one wave per line, four lines per workgroup: the same composition into the wave sink --
//                                 byte i of a field goes to lane i, numbers one digit per lane, CIGAR one word per lane with
//                                 a wave prefix sum over the words' text lengths and a segmented sum for the M runs.  Byte
//                                 stores straight to HBM: consecutive lanes store consecutive bytes.  No atomics.  With
//                                 kExtras (spm_sam_extras): QUAL one value per lane, back to front on a
//                                 reverse line, and MD one transcript word per lane (wave_md_walk) -- a segmented sum gives
//                                 every X and D word the matched positions in front of it, two wave prefix sums place its
//                                 text and find its reference letters;
//   jst_sam_stats_kernel          one lane per line: offset and length into the record, the counts by count_flagged.
#pragma once

#include <string>

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_handles.hpp"
#include "jst_sam_core.hpp"
#include "output_handles.hpp"
#include "scratch_layout.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum {
    kSamCntBad = 0,
    kSamCntLines,
    kSamCntBytes,
    kSamCntReported,
    kSamCntSecondary,
    kSamCntUnmapped,
    kSamCntRescue,
    kSamCnts
};

struct jst_sam_params
{
    jst_sam_src S;
    uint32_t *first_rescue = nullptr; // [n_pairs], what S.first_rescue reads
    uint32_t *cnt = nullptr;          // [n_reads] lines of every read
    uint32_t *offs = nullptr;         // [n_reads] their exclusive sum
    spm_sam_line *lines = nullptr;    // [cap_lines]
    jst_sam_aux *aux = nullptr;       // [cap_lines]
    uint32_t *len = nullptr;          // [cap_lines] bytes of every line, 0 beyond the last
    uint64_t *off64 = nullptr;        // [cap_lines] their exclusive sum
    uint32_t cap_lines = 0;           // the host's bound on the number of lines
    uint32_t n_lines = 0;             // write and stats: what the lines stage counted
    char *text = nullptr;
    uint64_t n_bytes = 0;
    unsigned long long *counts = nullptr; // [kSamCnts]
};

__global__ __launch_bounds__(256) void jst_sam_first_rescue_kernel(const jst_sam_params P)
{
    const unsigned long long j = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (j < P.S.n_rescues) {
        const spm_jst_rescue R = P.S.rescues[j];
        bool first = true;
        bad = !jst_sam_rescue_names_pair(R, P.S.n_pairs);
        if (j > 0) {
            const spm_jst_rescue before = P.S.rescues[j - 1];
            bad = bad || !jst_sam_rescues_ordered(before, R);
            first = before.pair != R.pair;
        }
        if (!bad && first)
            P.first_rescue[R.pair] = (uint32_t)j;
    }
    count_flagged(&P.counts[kSamCntBad], bad);
}

template <bool kEmit> __global__ __launch_bounds__(256) void jst_sam_lines_kernel(const jst_sam_params P)
{
    const unsigned long long r = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    uint32_t n = 0;
    if (r < P.S.n_reads) {
        jst_sam_reported own, other;
        int32_t tlen = 0;
        if (P.S.pairs) {
            const jst_sam_pair_plan plan = jst_sam_plan_pair(P.S, (uint32_t)(r / 2));
            bad = !plan.ok;
            own = plan.mate[r & 1];
            other = plan.mate[(r & 1) ^ 1];
            tlen = (r & 1) ? (int32_t)(0u - (uint32_t)plan.tlen) : plan.tlen;
        } else {
            bool ok = true;
            own = jst_sam_plan_single(P.S, (uint32_t)r, ok);
            bad = !ok;
        }
        if (!bad) {
            n = jst_sam_line_count(P.S.reads[r], own, P.S.flags);
            if (kEmit) {
                const uint32_t at = P.offs[r];
                if (at <= P.cap_lines)
                    jst_sam_read_lines(P.S, (uint32_t)r, own, P.S.pairs ? &other : nullptr, tlen, P.lines + at, P.aux + at, P.cap_lines - at);
            }
        }
        if (!kEmit)
            P.cnt[r] = n;
    }
    if (!kEmit) {
        count_flagged(&P.counts[kSamCntBad], bad);
        wave_count_add(&P.counts[kSamCntLines], (unsigned long long)n);
    }
}

__global__ __launch_bounds__(256) void jst_sam_measure_kernel(const jst_sam_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    const unsigned long long n_lines = P.counts[kSamCntLines]; // (the lines stage is complete: stream order)
    bool bad = false;
    uint64_t n = 0;
    if (i < P.cap_lines) {
        if (i < n_lines) {
            jst_sam_fields F;
            bad = !jst_sam_resolve(P.S, P.lines[i], P.aux[i], F, true);
            if (!bad) {
                jst_sam_measure M;
                jst_sam_compose(P.S, F, M);
                n = M.n;
                bad = n > 0xFFFFFFFFull;
            }
            n = bad ? 0 : n;
        }
        P.len[i] = (uint32_t)n;
    }
    count_flagged(&P.counts[kSamCntBad], bad);
    wave_count_add(&P.counts[kSamCntBytes], (unsigned long long)n);
}

// The items of a transcript across a wave, for the sinks that write them (the text's <len><op>, a BAM record's words).  Lane w
// of a pass takes word w.  A word that ends an item -- every word, or with `merge` the last word of a maximal run of = / X
// words -- holds the item's length (a segmented sum over the wave, plus what the pass before left open), asks len_of(run, word)
// for the item's size in the sink's units and gets put(at, run, word, size) with `at` the wave prefix sum of the sizes in
// front of it.  -> the size of all items.  words, n, merge and the return value are wave-uniform.
template <class LenOf, class Put>
__device__ __forceinline__ uint64_t wave_cigar_walk(const uint32_t *words, uint32_t n, bool merge, uint32_t lane, LenOf len_of, Put put)
{
    uint64_t carry = 0, done = 0; // the length of the M run the passes so far left open; the size of the items so far
    bool open = false;
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t w = base + lane;
        const bool live = w < n;
        const uint32_t word = live ? words[w] : 0u;
        const bool has_next = live && w + 1 < n;
        const uint32_t next = has_next ? words[w + 1] : 0u;
        const bool is_m = live && merge && jst_sam_op_is_m(word);
        const bool next_m = has_next && merge && jst_sam_op_is_m(next);
        const int left_m = __shfl_up(is_m ? 1 : 0, 1);
        const bool prev_m = lane == 0 ? open : left_m != 0;
        const bool start = !(is_m && prev_m);
        const uint32_t id = (uint32_t)__popcll(__ballot(start) & (~0ull >> (63 - lane)));
        run_sum<uint64_t> v{live ? (uint64_t)(word >> 4) : 0ull};
        if (lane == 0 && !start)
            v.v += carry;
        wave_run_scan(id, v);
        const bool last = live && !(is_m && next_m);
        const uint32_t len = last ? len_of(v.v, word) : 0u;
        uint32_t incl = len; // (flat: through wave_prefix_incl the two write kernels are scheduled differently)
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if ((int)lane >= o)
                incl += up;
        }
        const uint32_t total = __shfl(incl, 63);
        if (last)
            put(done + (incl - len), v.v, word, len);
        open = __shfl((live && !last) ? 1 : 0, 63) != 0;
        carry = __shfl(v.v, 63);
        done += total;
    }
    return done;
}

// The breaking words (X, D) of a transcript across a wave, for the sinks that write an MD string.  Lane w of a pass takes word
// w.  A breaking word closes a run -- the = and I words since the breaking word before it -- and holds the matched positions of
// that run (a segmented sum over the wave; lane 0's run takes in what the passes so far left open, which is how a count crosses
// a pass border), its first reference position counted from the transcript's (a wave prefix sum over the words' reference
// spans, on top of the passes so far), and gets put(at, c, word, ref_at, len) with len = jst_sam_md_word_len(c, word) and `at`
// the wave prefix sum of the lengths in front of it.  -> the size of all items; `open`: the count behind the last breaking word,
// which the sink prints.  words, n, open and the return value are wave-uniform.
template <class Put> __device__ __forceinline__ uint64_t wave_md_walk(const uint32_t *words, uint32_t n, uint32_t lane, uint64_t &open, Put put)
{
    uint64_t carry = 0, done = 0, ref_done = 0; // the open run's count; the size of the items so far; reference positions so far
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t w = base + lane;
        const uint32_t word = w < n ? words[w] : 0u; // (a word 0 neither breaks nor counts)
        const bool brk = jst_sam_md_breaks(word);
        // lanes of one run share the number of breaking words below them; the breaking word is its run's last lane
        const uint32_t id = (uint32_t)__popcll(__ballot(brk) & ((1ull << lane) - 1ull));
        run_sum<uint64_t> v{(uint64_t)jst_sam_md_matched(word)};
        if (lane == 0)
            v.v += carry;
        wave_run_scan(id, v);
        const uint32_t span = jst_sam_md_ref_span(word);
        uint64_t ref_incl = span;
        const uint64_t len = brk ? jst_sam_md_word_len(v.v, word) : 0ull;
        uint64_t incl = len;
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t up = __shfl_up(incl, o), ref_up = __shfl_up(ref_incl, o);
            if ((int)lane >= o) {
                incl += up;
                ref_incl += ref_up;
            }
        }
        if (brk)
            put(done + (incl - len), v.v, word, ref_done + (ref_incl - span), len);
        const uint64_t last = __shfl(v.v, 63);
        carry = __shfl(brk ? 1 : 0, 63) ? 0ull : last;
        done += __shfl(incl, 63);
        ref_done += __shfl(ref_incl, 63);
    }
    open = carry;
    return done;
}

// What the two wave sinks share: byte i of a field to lane i.  cur is wave-uniform.  No store lands outside [cur at
// construction, end): the line's, or the record's, own bytes.
template <class Byte> struct jst_wave_sink_base
{
    Byte *to;
    uint64_t cur, end;
    uint32_t lane;

    __device__ __forceinline__ void store(uint64_t at, Byte c)
    {
        if (at < end)
            to[at] = c;
    }
    __device__ __forceinline__ void bytes(const char *p, uint64_t n)
    {
        for (uint64_t i = lane; i < n; i += kWave)
            store(cur + i, (Byte)p[i]);
        cur += n;
    }
    __device__ __forceinline__ void qual(const uint8_t *values, uint32_t m, bool reverse, uint8_t add)
    {
        for (uint32_t i = lane; i < jst_sam_qual_len(m); i += kWave)
            store(cur + i, (Byte)jst_sam_qual_byte(values, m, reverse, add, i));
        cur += jst_sam_qual_len(m);
    }
    // the MD string from `begin` on: every lane writes the bytes of its own breaking word (a long D loops).  cur: behind them.
    // -> the count behind the last breaking word, which the sink prints as a number
    __device__ __forceinline__ uint64_t md_words(uint64_t begin, const uint32_t *words, uint32_t n, const uint8_t *ref, const char *symbols,
                                                 uint32_t sigma)
    {
        uint64_t open = 0;
        cur = begin + wave_md_walk(words, n, lane, open, [&](uint64_t at, uint64_t c, uint32_t word, uint64_t ref_at, uint64_t len) {
                  for (uint64_t i = 0; i < len; ++i)
                      store(begin + at + i, (Byte)jst_sam_md_word_char(c, word, ref + ref_at, symbols, sigma, i));
              });
        return open;
    }
};

// The wave sink: the composition of one line.
struct jst_sam_wave_sink : jst_wave_sink_base<char>
{
    __device__ __forceinline__ void text(uint64_t lit, uint32_t n_lit)
    {
        if (lane < n_lit)
            store(cur + lane, (char)(lit >> (8 * lane)));
        cur += n_lit;
    }
    // literal, sign and digits are at most 8 + 1 + 20 characters: one pass of the wave, lane i writes character i
    __device__ __forceinline__ void num(uint64_t lit, uint32_t n_lit, uint64_t v, bool negative)
    {
        const uint32_t head = n_lit + (negative ? 1u : 0u), len = jst_sam_dec_len(v);
        if (lane < n_lit)
            store(cur + lane, (char)(lit >> (8 * lane)));
        else if (lane < head)
            store(cur + lane, '-');
        else if (lane < head + len)
            store(cur + lane, jst_sam_dec_char(v, len, lane - head));
        cur += head + len;
    }
    __device__ __forceinline__ void seq(const uint8_t *ranks, uint32_t m, const char *symbols, uint32_t sigma)
    {
        for (uint32_t i = lane; i < m; i += kWave)
            store(cur + i, jst_sam_seq_char(ranks[i], symbols, sigma));
        cur += m;
    }
    __device__ __forceinline__ void cigar(const uint32_t *words, uint32_t n, bool merge)
    {
        const uint64_t begin = cur;
        cur = begin + wave_cigar_walk(
                          words, n, merge, lane, [](uint64_t run, uint32_t) { return jst_sam_word_len(run); },
                          [&](uint64_t at, uint64_t run, uint32_t word, uint32_t len) {
                              const char op = jst_sam_op_char(word & 15u, merge);
                              for (uint32_t i = 0; i < len; ++i)
                                  store(begin + at + i, jst_sam_word_char(run, op, len, i));
                          });
    }
    __device__ __forceinline__ void md(const uint32_t *words, uint32_t n, const uint8_t *ref, const char *symbols, uint32_t sigma)
    {
        num(0, 0, md_words(cur, words, n, ref, symbols, sigma), false);
    }
};

// kExtras: the call has qualities or a reference (spm_sam_extras); without, the composition leaves both kinds of field out
template <bool kExtras> __global__ __launch_bounds__(256) void jst_sam_write_kernel(const jst_sam_params P)
{
    const uint32_t wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const unsigned long long i = blockIdx.x * 4ull + wv;
    if (i >= P.n_lines)
        return; // (whole waves: i is uniform across the wave, and no workgroup barrier follows)
    jst_sam_fields F;
    if (!jst_sam_resolve(P.S, P.lines[i], P.aux[i], F, false))
        return; // (the measure stage resolved this record and counted a failure: the host does not get here)
    const uint64_t begin = P.off64[i], end = begin + P.len[i];
    jst_sam_wave_sink out{{P.text, begin, end < P.n_bytes ? end : P.n_bytes, lane}};
    jst_sam_compose<kExtras>(P.S, F, out);
}

__global__ __launch_bounds__(256) void jst_sam_stats_kernel(const jst_sam_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    uint32_t kind = ~0u;
    if (i < P.n_lines) {
        kind = P.lines[i].kind;
        P.lines[i].offset = P.off64[i];
        P.lines[i].len = P.len[i];
    }
    count_flagged(&P.counts[kSamCntReported], kind == SPM_SAM_LOCUS || kind == SPM_SAM_RESCUE);
    count_flagged(&P.counts[kSamCntSecondary], kind == SPM_SAM_SECONDARY_LINE);
    count_flagged(&P.counts[kSamCntUnmapped], kind == SPM_SAM_UNMAPPED);
    count_flagged(&P.counts[kSamCntRescue], kind == SPM_SAM_RESCUE);
}

struct sam_cnt_op
{
    const uint32_t *cnt;
    __host__ __device__ uint32_t operator()(uint32_t i) const { return cnt[i]; }
};
struct sam_len_op
{
    const uint32_t *len;
    __host__ __device__ uint64_t operator()(uint32_t i) const { return len[i]; }
};

} // namespace spm_hip

static_assert(sizeof(spm_hip::jst_sam_aux) == 24 && sizeof(spm_sam_extras) == 32, "spm_hip.h states these sizes");

extern "C" void spm_hip_sam_destroy(spm_sam *s)
{
    if (s)
        spm_hip::handle_destroy(s, {s->d_text, s->d_lines});
}

// what a reference name, and a read name, has to be: the tail of each refusal
static const char *const kSamNameRule = "is empty, longer than 254 bytes, \"*\" or holds a byte outside '!' .. '~'";

extern "C" int spm_hip_sam_mapq(const spm_sam_opts *opts, uint32_t n_best, uint32_t n_next)
{
    if (!opts || opts->mapq_defaults > 1)
        return -1;
    return spm_hip::jst_sam_mapq(spm_hip::jst_sam_tables_of(*opts), n_best, n_next);
}

static int sam_header_text(const char *so, const char *rname, uint64_t ref_len, char *buf, uint64_t cap, uint64_t *len)
{
    if (!rname || !len || (!buf && cap))
        return SPM_E_INVALID;
    if (!spm_hip::jst_sam_name_ok(rname, strlen(rname))) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: rname %s", "spm_hip_sam_header", kSamNameRule);
        return SPM_E_INVALID;
    }
    const std::string h = std::string("@HD\tVN:1.6\tSO:") + so + "\n@SQ\tSN:" + rname + "\tLN:" + std::to_string(ref_len) + "\n";
    *len = h.size();
    if (h.size() > cap)
        return SPM_E_OVERFLOW;
    memcpy(buf, h.data(), h.size());
    return SPM_OK;
}

extern "C" int spm_hip_sam_header(const char *rname, uint64_t ref_len, char *buf, uint64_t cap, uint64_t *len)
{
    return sam_header_text("unknown", rname, ref_len, buf, cap, len);
}

extern "C" int spm_hip_sam_header_sorted(const char *rname, uint64_t ref_len, char *buf, uint64_t cap, uint64_t *len)
{
    return sam_header_text("coordinate", rname, ref_len, buf, cap, len);
}

// ---- the front that spm_hip_jst_ref_loci_sam and spm_hip_jst_ref_loci_bam share: what is refused on the host, and the lines
// stage with everything it needs on the device ----
struct sam_front
{
    spm_hip::jst_sam_params P{};
    dev_scratch keep;          // the strings of the opts on the device
    std::vector<uint8_t> img;  // ... and on the host, until the copy has been waited for
    std::vector<uint64_t> q_off; // the qualities' offsets, likewise
    spm_hip::hip_events<8> ev; // [0], [1]: around the lines stage; the rest are the caller's
    uint8_t *d_tmp = nullptr;  // the scans' temporary storage, in the context's scratch behind the arrays of P
    size_t tmp64 = 0;
};

static int sam_check_args(const char *who, spm_ctx *ctx, spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs,
                          const spm_patterns *ps, const spm_sam_opts *opts, size_t &rname_len, uint64_t &n_named)
{
    using namespace spm_hip;
    if (!r || !ps || !opts || !opts->rname || !opts->symbols) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !r ? "reads handle" : !ps ? "patterns" : !opts ? "opts" : !opts->rname ? "rname" : "symbols");
        return SPM_E_INVALID;
    }
    if ((opts->flags & ~(SPM_SAM_CIGAR_M | SPM_SAM_SECONDARY)) || opts->reserved || opts->mapq_defaults > 1) {
        SPM_SET_ERR(ctx, "%s: unknown flag bits 0x%x, reserved %llu (must be 0) or mapq_defaults %u (0 or 1)", who, opts->flags,
                    (unsigned long long)opts->reserved, opts->mapq_defaults);
        return SPM_E_INVALID;
    }
    if (rs && !pr) {
        SPM_SET_ERR(ctx, "%s: rescues without pairs", who);
        return SPM_E_INVALID;
    }
    if (r->ctx != ctx || ps->ctx != ctx || (pr && pr->ctx != ctx) || (rs && rs->ctx != ctx)) {
        SPM_SET_ERR(ctx, "%s: the %s belongs to another context", who,
                    r->ctx != ctx ? "reads handle" : ps->ctx != ctx ? "needle set" : (pr && pr->ctx != ctx) ? "pairs handle" : "rescues handle");
        return SPM_E_INVALID;
    }
    if (r->n_loci != l->n) {
        SPM_SET_ERR(ctx, "%s: the reads handle was made from %llu loci, these are %llu", who, (unsigned long long)r->n_loci,
                    (unsigned long long)l->n);
        return SPM_E_INVALID;
    }
    if (pr && (r->strands != 2 || (r->n & 1) || pr->n != r->n / 2)) {
        SPM_SET_ERR(ctx, "%s: %llu pairs do not belong to %llu reads made with strands == %u (mates need 2)", who, (unsigned long long)pr->n,
                    (unsigned long long)r->n, r->strands);
        return SPM_E_INVALID;
    }
    if (ps->algo == SPM_ALGO_MYERS_PREFIX) {
        SPM_SET_ERR(ctx, "%s: a MYERS_PREFIX needle set has no alignments to print (not supported)", who);
        return SPM_E_UNSUPPORTED;
    }
    if ((uint64_t)ps->n != (uint64_t)r->strands * r->n) {
        SPM_SET_ERR(ctx, "%s: %u needles are not the set of %llu reads on %u strand(s)", who, ps->n, (unsigned long long)r->n, r->strands);
        return SPM_E_INVALID;
    }
    if (strlen(opts->symbols) != ps->sigma) {
        SPM_SET_ERR(ctx, "%s: symbols has %zu characters, the needle set sigma %u", who, strlen(opts->symbols), ps->sigma);
        return SPM_E_INVALID;
    }
    rname_len = strlen(opts->rname);
    if (!jst_sam_name_ok(opts->rname, rname_len)) {
        SPM_SET_ERR(ctx, "%s: rname %s", who, kSamNameRule);
        return SPM_E_INVALID;
    }
    n_named = pr ? pr->n : r->n;
    if (!opts->names != !opts->name_off || (!opts->names && opts->n_names) || (opts->names && opts->n_names != n_named)) {
        SPM_SET_ERR(ctx, "%s: %llu names (names %s, name_off %s) for %llu %s", who, (unsigned long long)opts->n_names,
                    opts->names ? "given" : "NULL", opts->name_off ? "given" : "NULL", (unsigned long long)n_named, pr ? "pairs" : "reads");
        return SPM_E_INVALID;
    }
    if (opts->names) {
        if (opts->name_off[0] != 0) {
            SPM_SET_ERR(ctx, "%s: name_off does not ascend from 0", who);
            return SPM_E_INVALID;
        }
        for (uint64_t i = 0; i < n_named; ++i) {
            if (opts->name_off[i + 1] < opts->name_off[i]) {
                SPM_SET_ERR(ctx, "%s: name_off does not ascend at name %llu", who, (unsigned long long)i);
                return SPM_E_INVALID;
            }
            if (!jst_sam_name_ok(opts->names + opts->name_off[i], opts->name_off[i + 1] - opts->name_off[i])) {
                SPM_SET_ERR(ctx, "%s: name %llu %s", who, (unsigned long long)i, kSamNameRule);
                return SPM_E_INVALID;
            }
        }
    }
    const bool secondary = (opts->flags & SPM_SAM_SECONDARY) != 0;
    if (l->n > 0xFFFFFFFFull || r->n + (secondary ? l->n : 0) > 0xFFFFFFFFull || (rs && rs->n > 0xFFFFFFFFull)) {
        SPM_SET_ERR(ctx, "%s: %llu reads and %llu loci: more than 2^32 - 1 lines", who, (unsigned long long)r->n, (unsigned long long)l->n);
        return SPM_E_UNSUPPORTED;
    }
    return SPM_OK;
}

// What spm_sam_extras adds to the refusals (ex != NULL).  bam_ref_len: the BAM call's ref_len, which the reference has to have.
static int sam_check_extras(const char *who, spm_ctx *ctx, const spm_jst_reads *r, const spm_patterns *ps, const spm_sam_extras *ex,
                            const uint64_t *bam_ref_len)
{
    if ((ex->flags & ~SPM_SAM_MD) || ex->reserved) {
        SPM_SET_ERR(ctx, "%s: extras: unknown flags bits 0x%x or reserved %u (must be 0)", who, ex->flags, ex->reserved);
        return SPM_E_INVALID;
    }
    if (((ex->flags & SPM_SAM_MD) != 0) != (ex->reference != nullptr)) {
        SPM_SET_ERR(ctx, "%s: extras: %s", who, ex->reference ? "a reference without SPM_SAM_MD in flags" : "SPM_SAM_MD in flags without a reference");
        return SPM_E_INVALID;
    }
    if (ex->reference) {
        if (ex->reference->ctx != ctx) {
            SPM_SET_ERR(ctx, "%s: extras: the reference belongs to another context", who);
            return SPM_E_INVALID;
        }
        if (ex->reference->sigma != ps->sigma) {
            SPM_SET_ERR(ctx, "%s: extras: the reference has sigma %u, the needle set sigma %u", who, ex->reference->sigma, ps->sigma);
            return SPM_E_INVALID;
        }
        if (bam_ref_len && ex->reference->n != *bam_ref_len) {
            SPM_SET_ERR(ctx, "%s: extras: the reference has %llu symbols, ref_len is %llu", who, (unsigned long long)ex->reference->n,
                        (unsigned long long)*bam_ref_len);
            return SPM_E_INVALID;
        }
    }
    if ((ex->qual != nullptr) != (ex->n_qual != 0)) {
        SPM_SET_ERR(ctx, "%s: extras: %s", who, ex->qual ? "qual with n_qual 0" : "n_qual without qual");
        return SPM_E_INVALID;
    }
    if (ex->qual) {
        uint64_t sum = 0;
        for (uint64_t i = 0; i < r->n; ++i)
            sum += (uint64_t)ps->m[r->strands * i];
        if (ex->n_qual != sum) {
            SPM_SET_ERR(ctx, "%s: extras: n_qual is %llu, the read lengths add up to %llu", who, (unsigned long long)ex->n_qual,
                        (unsigned long long)sum);
            return SPM_E_INVALID;
        }
        for (uint64_t i = 0; i < ex->n_qual; ++i)
            if (ex->qual[i] > 93) {
                SPM_SET_ERR(ctx, "%s: extras: qual[%llu] is %u, above 93", who, (unsigned long long)i, ex->qual[i]);
                return SPM_E_INVALID;
            }
    }
    return SPM_OK;
}

// n_reads > 0.  *d_lines: the line records, allocated here, the caller's to free.  ex: checked, or NULL
static int sam_lines_stage(const char *who, spm_ctx *ctx, spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs,
                           const spm_patterns *ps, const spm_sam_opts *opts, const spm_sam_extras *ex, size_t rname_len, uint64_t n_named,
                           sam_front &F, spm_sam_line **d_lines)
{
    using namespace spm_hip;
    (void)who;
    const bool secondary = (opts->flags & SPM_SAM_SECONDARY) != 0;
    const uint32_t n_reads = (uint32_t)r->n;
    hipStream_t st = ctx->stream;
    SPM_HIP_CHECK(ctx, F.ev.create());
    SPM_TRY(spm_align_tables(ps)); // the needles' ranks on the device (built once per set)
    jst_sam_params &P = F.P;
    jst_sam_src &S = P.S;
    S.loci = l->d_loci;
    S.n_loci = l->d_loci ? (uint32_t)l->n : 0u;
    S.ops = l->d_ops;
    S.n_ops = l->d_ops ? l->n_ops : 0;
    S.reads = r->d;
    S.n_reads = n_reads;
    S.strands = r->strands;
    S.pairs = pr ? pr->d : nullptr;
    S.n_pairs = pr ? (uint32_t)pr->n : 0u;
    S.rescues = rs ? rs->d : nullptr;
    S.n_rescues = rs && rs->d ? (uint32_t)rs->n : 0u;
    S.rescue_ops = rs ? rs->d_ops : nullptr;
    S.n_rescue_ops = rs && rs->d_ops ? rs->n_ops : 0;
    S.ranks = ps->d_al_ranks;
    S.offsets = ps->d_al_offsets;
    S.m = ps->d_m;
    S.n_needles = ps->n;
    S.sigma = ps->sigma;
    S.rname_len = (uint32_t)rname_len;
    S.tables = jst_sam_tables_of(*opts);
    S.flags = opts->flags;
    P.cap_lines = n_reads + (secondary ? S.n_loci : 0u);
    // ---- the strings of the opts, copied: rname, symbols, names, name_off in one allocation ----
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t names_bytes = opts->names ? (size_t)opts->name_off[n_named] : 0;
    const size_t b_rname = al(rname_len + 1), b_sym = al(ps->sigma + 1), b_off = al(opts->names ? (n_named + 1) * 8 : 0);
    std::vector<uint8_t> &img = F.img;
    img.assign(b_rname + b_sym + b_off + al(names_bytes + 1), 0);
    memcpy(img.data(), opts->rname, rname_len);
    memcpy(img.data() + b_rname, opts->symbols, ps->sigma);
    if (opts->names) {
        memcpy(img.data() + b_rname + b_sym, opts->name_off, (n_named + 1) * 8);
        memcpy(img.data() + b_rname + b_sym + b_off, opts->names, names_bytes);
    }
    dev_scratch &keep = F.keep;
    char *d_img = nullptr;
    SPM_HIP_CHECK(ctx, keep.alloc(&d_img, img.size()));
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_img, img.data(), img.size(), hipMemcpyHostToDevice, st));
    S.rname = d_img;
    S.symbols = d_img + b_rname;
    if (opts->names) {
        S.name_off = reinterpret_cast<const uint64_t *>(d_img + b_rname + b_sym);
        S.names = d_img + b_rname + b_sym + b_off;
    }
    // ---- the extras: the qualities and their offsets copied, the reference where it is resident ----
    if (ex && ex->qual) {
        F.q_off.assign((size_t)n_reads + 1, 0);
        for (uint32_t i = 0; i < n_reads; ++i)
            F.q_off[i + 1] = F.q_off[i] + (uint64_t)ps->m[(size_t)r->strands * i];
        uint64_t *d_q_off = nullptr;
        uint8_t *d_qual = nullptr;
        SPM_HIP_CHECK(ctx, keep.alloc(&d_q_off, F.q_off.size() * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_qual, ex->n_qual));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_q_off, F.q_off.data(), F.q_off.size() * 8, hipMemcpyHostToDevice, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_qual, ex->qual, ex->n_qual, hipMemcpyHostToDevice, st));
        S.q_off = d_q_off;
        S.qual = d_qual;
    }
    if (ex && ex->reference) {
        S.ref = ex->reference->d;
        S.ref_n = ex->reference->n;
    }
    // ---- scratch ----
    size_t tmp32 = 0;
    size_t &tmp64 = F.tmp64;
    SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(sam_cnt_op{nullptr}), n_reads, &tmp32));
    SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint64_t>(ctx, counted<uint64_t>(sam_len_op{nullptr}), P.cap_lines, &tmp64));
    uint8_t *&d_tmp = F.d_tmp;
    scratch_layout L;
    L.take(P.first_rescue, S.n_pairs);
    L.take(P.cnt, n_reads);
    L.take(P.offs, n_reads);
    L.take(P.aux, P.cap_lines);
    L.take(P.len, P.cap_lines);
    L.take(P.off64, P.cap_lines);
    L.take(P.counts, kSamCnts);
    L.take(d_tmp, std::max(tmp32, tmp64));
    SPM_TRY(ensure_scratch(ctx, L.bytes()));
    L.bind(ctx->d_scratch);
    S.first_rescue = rs ? P.first_rescue : nullptr;
    SPM_HIP_CHECK(ctx, hipMalloc(d_lines, (size_t)P.cap_lines * sizeof(spm_sam_line)));
    P.lines = *d_lines;
    // ---- lines ----
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kSamCnts * 8, st));
    SPM_HIP_CHECK(ctx, hipEventRecord(F.ev[0], st));
    if (rs) {
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.first_rescue, 0xFF, (size_t)S.n_pairs * 4, st));
        if (S.n_rescues)
            SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_sam_first_rescue_kernel, S.n_rescues, P));
    }
    SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_sam_lines_kernel<false>, n_reads, P));
    SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp32, counted<uint32_t>(sam_cnt_op{P.cnt}), P.offs, n_reads));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_sam_lines_kernel<true>, n_reads, P));
    SPM_HIP_CHECK(ctx, hipEventRecord(F.ev[1], st));
    return SPM_OK;
}

// Behind the measure launch of either format: the lines' offsets, the one read-back before anything is written, the refusal
// (`clause`: what else a record of this format can disagree with), n_lines and n_bytes.  P: the params the format launches with
static int sam_measured(const char *who, spm_ctx *ctx, sam_front &F, spm_hip::jst_sam_params &P, const char *clause)
{
    using namespace spm_hip;
    SPM_HIP_CHECK(ctx, exclusive_sum(ctx, F.d_tmp, F.tmp64, counted<uint64_t>(sam_len_op{P.len}), P.off64, P.cap_lines));
    SPM_HIP_CHECK(ctx, hipEventRecord(F.ev[2], ctx->stream));
    SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kSamCnts));
    const unsigned long long *c = ctx->h_counters;
    if (c[kSamCntBad] || c[kSamCntLines] > P.cap_lines) {
        SPM_SET_ERR(ctx, "%s: %llu records of the reads, pairs or rescues disagree with each other, these loci, their pools, the "
                         "needle set%s; nothing was written", who, c[kSamCntBad], clause);
        return SPM_E_INVALID;
    }
    P.n_lines = (uint32_t)c[kSamCntLines];
    P.n_bytes = c[kSamCntBytes];
    return SPM_OK;
}

// Behind the last stage that writes (`before`: the event that closed it): the stats kernel, the second read-back, the four
// counts and the four stage times that spm_sam_stats and spm_bam_stats share by name.
template <class Stats> static int sam_closed(spm_ctx *ctx, sam_front &F, const spm_hip::jst_sam_params &P, hipEvent_t before, Stats &S)
{
    using namespace spm_hip;
    SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_sam_stats_kernel, P.n_lines, P));
    SPM_HIP_CHECK(ctx, hipEventRecord(F.ev[5], ctx->stream));
    SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kSamCnts));
    const unsigned long long *c = ctx->h_counters;
    S.n_reported = c[kSamCntReported];
    S.n_secondary = c[kSamCntSecondary];
    S.n_unmapped = c[kSamCntUnmapped];
    S.n_rescue_lines = c[kSamCntRescue];
    hipEventElapsedTime(&S.ms_lines, F.ev[0], F.ev[1]);
    hipEventElapsedTime(&S.ms_measure, F.ev[1], F.ev[2]);
    hipEventElapsedTime(&S.ms_write, F.ev[3], F.ev[4]);
    hipEventElapsedTime(&S.ms_stats, before, F.ev[5]);
    return SPM_OK;
}

static int sam_run(const char *who, spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs, const spm_patterns *ps,
                   const spm_sam_opts *opts, const spm_sam_extras *ex, spm_sam **out)
{
    using namespace spm_hip;
    if (!l || !out)
        return SPM_E_INVALID;
    *out = nullptr;
    spm_ctx *ctx = l->ctx;
    const auto t_call = clk::now();
    size_t rname_len = 0;
    uint64_t n_named = 0;
    SPM_TRY(sam_check_args(who, ctx, l, r, pr, rs, ps, opts, rname_len, n_named));
    if (ex)
        SPM_TRY(sam_check_extras(who, ctx, r, ps, ex, nullptr));
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_sam, void (*)(spm_sam *)> R(new spm_sam, spm_hip_sam_destroy);
    R->ctx = ctx;
    const uint32_t n_reads = (uint32_t)r->n;
    if (n_reads) {
        hipStream_t st = ctx->stream;
        sam_front F;
        SPM_TRY(sam_lines_stage(who, ctx, l, r, pr, rs, ps, opts, ex, rname_len, n_named, F, &R->d_lines));
        jst_sam_params &P = F.P;
        hip_events<8> &ev = F.ev;
        // ---- measure ----
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_sam_measure_kernel, P.cap_lines, P));
        SPM_TRY(sam_measured(who, ctx, F, P, " or the reference of the extras"));
        R->n_lines = P.n_lines;
        R->n_bytes = P.n_bytes;
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_text, std::max<uint64_t>(P.n_bytes, 1)));
        P.text = R->d_text;
        // ---- write ----
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
        if (P.S.qual || P.S.ref)
            hipLaunchKernelGGL(jst_sam_write_kernel<true>, dim3((P.n_lines + 3) / 4), dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL(jst_sam_write_kernel<false>, dim3((P.n_lines + 3) / 4), dim3(256), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
        // ---- stats ----
        SPM_TRY(sam_closed(ctx, F, P, ev[4], R->stats));
        R->stats.n_lines = P.n_lines;
        R->stats.n_bytes = P.n_bytes;
        R->stats.ms_total = R->stats.ms_lines + R->stats.ms_measure + R->stats.ms_write + R->stats.ms_stats;
    }
    R->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst sam: %u reads -> %llu lines (%llu reported, %llu of them rescues, %llu secondary, %llu unmapped), "
                        "%llu bytes: device %.3f ms (lines %.3f, measure %.3f, write %.3f, stats %.3f), %.3f ms in all\n", n_reads,
                (unsigned long long)R->stats.n_lines, (unsigned long long)R->stats.n_reported, (unsigned long long)R->stats.n_rescue_lines,
                (unsigned long long)R->stats.n_secondary, (unsigned long long)R->stats.n_unmapped, (unsigned long long)R->stats.n_bytes,
                R->stats.ms_total, R->stats.ms_lines, R->stats.ms_measure, R->stats.ms_write, R->stats.ms_stats, R->stats.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_ref_loci_sam(spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs,
                                        const spm_patterns *ps, const spm_sam_opts *opts, spm_sam **out)
{
    return sam_run("spm_hip_jst_ref_loci_sam", l, r, pr, rs, ps, opts, nullptr, out);
}

extern "C" int spm_hip_jst_ref_loci_sam_ex(spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, spm_jst_rescues *rs,
                                           const spm_patterns *ps, const spm_sam_opts *opts, const spm_sam_extras *ex, spm_sam **out)
{
    return sam_run("spm_hip_jst_ref_loci_sam_ex", l, r, pr, rs, ps, opts, ex, out);
}

extern "C" int spm_hip_sam_view(spm_sam *s, const char **text, uint64_t *n_bytes, const spm_sam_line **lines, uint64_t *n_lines)
{
    using namespace spm_hip;
    if (!s)
        return SPM_E_INVALID;
    SPM_TRY(handle_download(s->ctx, s->have_host, view_part{s->d_text, s->n_bytes, s->host_text}, view_part{s->d_lines, s->n_lines, s->host_lines}));
    out_if(text, s->host_text.data());
    out_if(n_bytes, s->n_bytes);
    out_if(lines, s->host_lines.data());
    out_if(n_lines, s->n_lines);
    return SPM_OK;
}

extern "C" int spm_hip_sam_device(spm_sam *s, const void **text, uint64_t *n_bytes, const void **lines, uint64_t *n_lines)
{
    using namespace spm_hip;
    if (!s)
        return SPM_E_INVALID;
    out_if(text, s->d_text);
    out_if(n_bytes, s->n_bytes);
    out_if(lines, s->d_lines);
    out_if(n_lines, s->n_lines);
    return SPM_OK;
}

extern "C" int spm_hip_sam_stats(const spm_sam *s, spm_sam_stats *out) { return spm_hip::stats_out(s ? &s->stats : nullptr, out); }
