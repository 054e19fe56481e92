// jst_sam_core.hpp -- the rule of spm_hip_jst_ref_loci_sam (contract in spm_hip.h, scheme in DESIGN.md 4.11).
// Host-compilable (g++, clang++) and device code alike: the kernels of jst_sam.hpp use the MAPQ policy, the agreement
// predicates, the reported lines of a read or a pair, the composition of a line and, per kind of field, ONE function for its
// byte length and ONE for its bytes; the CPU tests instantiate the same functions (tests/cpp/jst_sam_core_cases.cpp).
//
// A line is composed once (jst_sam_compose) and handed, field by field, to a sink: the measuring sink adds up the lengths,
// the serial sink writes the bytes one after the other, the wave sink of jst_sam.hpp gives byte i of a field to lane i.  All
// three call the length and byte functions below and nothing else, so what is measured is what is written.
//
// Two kinds of field come with spm_sam_extras (scheme in DESIGN.md 4.11a): qual, the read's base qualities as sequenced, printed
// back to front on a line whose SEQ is the reverse complement; and md, the MD string of a transcript against the resident
// reference, whose items are the transcript's BREAKING words (X, D), each with the count of matched positions in front of it.
#pragma once

#include "hd.hpp"
#include "jst_rescue_core.hpp"

namespace spm_hip
{

constexpr uint32_t kSamNone = 0xFFFFFFFFu; // no locus, no rescue, no source
constexpr uint32_t kSamMaxName = 254;

// ---- MAPQ ----
struct jst_sam_mapq_tables
{
    uint8_t unique[4], multi[4];
};
// unique: a convention (see spm_hip.h); multi: floor(-10 log10(1 - 1/n)) for n = 2, 3, 4, >= 5
SPM_HD inline jst_sam_mapq_tables jst_sam_default_tables() { return jst_sam_mapq_tables{{60, 40, 30, 20}, {3, 1, 1, 0}}; }
SPM_HD inline jst_sam_mapq_tables jst_sam_tables_of(const spm_sam_opts &o)
{
    if (o.mapq_defaults)
        return jst_sam_default_tables();
    jst_sam_mapq_tables T;
    for (int i = 0; i < 4; ++i) {
        T.unique[i] = o.mapq_unique[i];
        T.multi[i] = o.mapq_multi[i];
    }
    return T;
}
SPM_HD inline uint8_t jst_sam_mapq(const jst_sam_mapq_tables &T, uint32_t n_best, uint32_t n_next)
{
    if (n_best == 0)
        return 0;
    if (n_best == 1)
        return T.unique[n_next < 3u ? n_next : 3u];
    return T.multi[(n_best < 5u ? n_best : 5u) - 2u];
}

// ---- decimal numbers: the digit count, and the character at place i from the left ----
SPM_HD inline uint32_t jst_sam_dec_len(uint64_t v)
{
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}
SPM_HD inline char jst_sam_dec_char(uint64_t v, uint32_t len, uint32_t i) // i < len == jst_sam_dec_len(v)
{
    for (uint32_t j = i + 1; j < len; ++j)
        v /= 10;
    return (char)('0' + v % 10);
}
SPM_HD inline uint64_t jst_sam_int_abs(int32_t v) { return v < 0 ? (uint64_t)(-(int64_t)v) : (uint64_t)v; }
SPM_HD inline uint32_t jst_sam_int_len(int32_t v) { return (v < 0 ? 1u : 0u) + jst_sam_dec_len(jst_sam_int_abs(v)); }
SPM_HD inline char jst_sam_int_char(int32_t v, uint32_t len, uint32_t i)
{
    if (v < 0)
        return i == 0 ? '-' : jst_sam_dec_char(jst_sam_int_abs(v), len - 1, i - 1);
    return jst_sam_dec_char((uint64_t)v, len, i);
}

// ---- SEQ: rank -> letter ----
SPM_HD inline char jst_sam_seq_char(uint8_t rank, const char *symbols, uint32_t sigma) { return rank < sigma ? symbols[rank] : 'N'; }

// ---- CIGAR: one word (or one merged run) as <len><op> ----
SPM_HD inline bool jst_sam_op_is_m(uint32_t word)
{
    const uint32_t op = word & 15u;
    return op == SPM_CIGAR_EQ || op == SPM_CIGAR_X;
}
SPM_HD inline char jst_sam_op_char(uint32_t op, bool as_m)
{
    if (as_m && (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X))
        return 'M';
    return op == SPM_CIGAR_EQ ? '=' : op == SPM_CIGAR_X ? 'X' : op == SPM_CIGAR_INS ? 'I' : op == SPM_CIGAR_DEL ? 'D' : '?';
}
SPM_HD inline uint32_t jst_sam_word_len(uint64_t run_len) { return jst_sam_dec_len(run_len) + 1; }
SPM_HD inline char jst_sam_word_char(uint64_t run_len, char op, uint32_t len, uint32_t i) // i < len == jst_sam_word_len(run_len)
{
    return i + 1 == len ? op : jst_sam_dec_char(run_len, len - 1, i);
}
// query and reference symbols of a transcript
SPM_HD inline void jst_sam_cigar_spans(const uint32_t *words, uint32_t n, uint64_t &query, uint64_t &ref)
{
    query = ref = 0;
    for (uint32_t w = 0; w < n; ++w) {
        const uint32_t op = words[w] & 15u, len = words[w] >> 4;
        query += (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X || op == SPM_CIGAR_INS) ? len : 0u;
        ref += (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X || op == SPM_CIGAR_DEL) ? len : 0u;
    }
}
// Walks the printed items of a transcript: f(run length, op character) per word, or per maximal run of = / X words with
// `merge`.  The serial form of what the wave does with a segmented sum.
template <class F> SPM_HD inline void jst_sam_cigar_items(const uint32_t *words, uint32_t n, bool merge, F &&f)
{
    uint64_t run = 0;
    for (uint32_t w = 0; w < n; ++w) {
        const uint32_t word = words[w];
        if (merge && jst_sam_op_is_m(word)) {
            run += word >> 4;
            if (w + 1 == n || !jst_sam_op_is_m(words[w + 1])) {
                f(run, 'M');
                run = 0;
            }
        } else {
            f((uint64_t)(word >> 4), jst_sam_op_char(word & 15u, false));
        }
    }
}

// ---- QUAL: value i of the read as the line prints it; `reverse`: the line's SEQ is the reverse complement ----
SPM_HD inline uint32_t jst_sam_qual_len(uint32_t m) { return m; }
SPM_HD inline uint8_t jst_sam_qual_byte(const uint8_t *values, uint32_t m, bool reverse, uint8_t add, uint32_t i) // i < m
{
    return (uint8_t)(values[reverse ? m - 1 - i : i] + add);
}

// ---- MD: a breaking word (X, D) behind `c` matched positions, as text ----
//   X of length L: c, then per position the reference letter, "0" between two of them   (5, AC -> 5A0C)
//   D of length L: c, '^', the L reference letters                                      (3, GT -> 3^GT)
// = adds to c, I does nothing, the count behind the last breaking word ends the string.
SPM_HD inline bool jst_sam_md_breaks(uint32_t word)
{
    const uint32_t op = word & 15u;
    return (op == SPM_CIGAR_X || op == SPM_CIGAR_DEL) && (word >> 4) != 0; // (a word of length 0 prints nothing)
}
SPM_HD inline uint32_t jst_sam_md_matched(uint32_t word) { return (word & 15u) == SPM_CIGAR_EQ ? word >> 4 : 0u; }
SPM_HD inline uint32_t jst_sam_md_ref_span(uint32_t word) // reference positions a word consumes
{
    const uint32_t op = word & 15u;
    return (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X || op == SPM_CIGAR_DEL) ? word >> 4 : 0u;
}
SPM_HD inline uint64_t jst_sam_md_word_len(uint64_t c, uint32_t word) // jst_sam_md_breaks(word)
{
    const uint64_t L = word >> 4;
    return jst_sam_dec_len(c) + ((word & 15u) == SPM_CIGAR_X ? 2 * L - 1 : L + 1);
}
// ref: the reference ranks at the word's first position; i < len == jst_sam_md_word_len(c, word)
SPM_HD inline char jst_sam_md_word_char(uint64_t c, uint32_t word, const uint8_t *ref, const char *symbols, uint32_t sigma, uint64_t i)
{
    const uint32_t digits = jst_sam_dec_len(c);
    if (i < digits)
        return jst_sam_dec_char(c, digits, (uint32_t)i);
    const uint64_t j = i - digits;
    if ((word & 15u) == SPM_CIGAR_X)
        return (j & 1u) ? '0' : jst_sam_seq_char(ref[j >> 1], symbols, sigma);
    return j == 0 ? '^' : jst_sam_seq_char(ref[j - 1], symbols, sigma);
}
// Walks the breaking words of a transcript: f(c, word, at) with c the matched positions in front of the word and `at` its first
// reference position, counted from the transcript's.  -> the count behind the last one.  The serial form of what the wave does
// with a segmented sum.
template <class F> SPM_HD inline uint64_t jst_sam_md_items(const uint32_t *words, uint32_t n, F &&f)
{
    uint64_t c = 0, at = 0;
    for (uint32_t w = 0; w < n; ++w) {
        const uint32_t word = words[w];
        if (jst_sam_md_breaks(word)) {
            f(c, word, at);
            c = 0;
        } else {
            c += jst_sam_md_matched(word);
        }
        at += jst_sam_md_ref_span(word);
    }
    return c;
}
// every X column disagrees with the read: ref at the transcript's first reference position, needle at its first query symbol
SPM_HD inline bool jst_sam_md_agrees(const uint32_t *words, uint32_t n, const uint8_t *ref, const uint8_t *needle)
{
    uint64_t r = 0, q = 0;
    bool ok = true;
    for (uint32_t w = 0; w < n; ++w) {
        const uint32_t op = words[w] & 15u, len = words[w] >> 4;
        if (op == SPM_CIGAR_X)
            for (uint32_t i = 0; i < len; ++i)
                ok = ok && ref[r + i] != needle[q + i];
        q += (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X || op == SPM_CIGAR_INS) ? len : 0u;
        r += (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X || op == SPM_CIGAR_DEL) ? len : 0u;
    }
    return ok;
}

// ---- names: SAM's [!-~]{1,254}, and "*" alone means "no name" ----
inline bool jst_sam_name_ok(const char *s, uint64_t len)
{
    if (len == 0 || len > kSamMaxName || (len == 1 && s[0] == '*'))
        return false;
    for (uint64_t i = 0; i < len; ++i)
        if (s[i] < '!' || s[i] > '~')
            return false;
    return true;
}

// ---- what the rule reads ----
struct jst_sam_src
{
    const spm_jst_ref_locus *loci = nullptr;
    uint32_t n_loci = 0;
    const uint32_t *ops = nullptr; // the loci's transcripts
    uint64_t n_ops = 0;
    const spm_jst_read *reads = nullptr;
    uint32_t n_reads = 0, strands = 1;
    const spm_jst_pair *pairs = nullptr; // nullptr: single-end
    uint32_t n_pairs = 0;
    const spm_jst_rescue *rescues = nullptr;
    uint32_t n_rescues = 0;
    const uint32_t *rescue_ops = nullptr;
    uint64_t n_rescue_ops = 0;
    const uint32_t *first_rescue = nullptr; // [n_pairs] the first rescue record of every pair, kSamNone: none
    const uint8_t *ranks = nullptr;         // needle p = ranks[offsets[p] .. offsets[p] + m[p])
    const uint32_t *offsets = nullptr;
    const int32_t *m = nullptr;
    uint32_t n_needles = 0, sigma = 4;
    const char *rname = nullptr, *symbols = nullptr, *names = nullptr;
    const uint64_t *name_off = nullptr;
    uint32_t rname_len = 0;
    jst_sam_mapq_tables tables{};
    uint32_t flags = 0;
    // spm_sam_extras: read r's qualities are qual[q_off[r] .. q_off[r] + m[strands * r]); the reference ranks, set with SPM_SAM_MD
    const uint8_t *qual = nullptr;
    const uint64_t *q_off = nullptr; // [n_reads + 1]
    const uint8_t *ref = nullptr;
    uint64_t ref_n = 0;
};

// what a line carries besides its record: the mate's POS, the signed TLEN, the counts behind the MAPQ
struct jst_sam_aux // 24 bytes
{
    uint64_t mate_pos; // POS of the mate's reported line; 0: it has none
    int32_t tlen;
    uint32_t x0, x1;
    uint32_t pad;
};

// ---- agreement predicates: each before a value is used as an index ----
// the run of `read` lies inside the loci, its head and tail name the read, its primary lies inside it
SPM_HD inline bool jst_sam_read_ok(const spm_jst_ref_locus *loci, uint64_t n, const spm_jst_read &R, uint32_t read, uint32_t strands)
{
    if (R.n_forward > R.n_loci || (uint64_t)R.first_locus + R.n_loci > n)
        return false;
    if (R.n_loci == 0)
        return R.primary == kSamNone;
    const uint32_t lo = R.first_locus, hi = lo + R.n_loci;
    if (loci[lo].pattern / strands != read || loci[hi - 1].pattern / strands != read)
        return false;
    return R.primary >= lo && R.primary < hi;
}
SPM_HD inline bool jst_sam_in_run(const spm_jst_read &R, uint32_t locus) { return locus >= R.first_locus && locus - R.first_locus < R.n_loci; }
// a transcript [off, off + len) lies inside a pool of n words and is not empty
SPM_HD inline bool jst_sam_transcript_ok(uint32_t off, uint32_t len, uint64_t n) { return len >= 1 && (uint64_t)off + len <= n; }
// rescue records j - 1 and j (j >= 1) are ordered by (pair, mate rescued), strictly
SPM_HD inline bool jst_sam_rescues_ordered(const spm_jst_rescue &before, const spm_jst_rescue &R)
{
    const uint64_t a = (uint64_t)before.pair << 1 | ((before.pattern >> 1) & 1u), b = (uint64_t)R.pair << 1 | ((R.pattern >> 1) & 1u);
    return a < b;
}
// a rescue record names a pair inside the pairs and a needle of that pair
SPM_HD inline bool jst_sam_rescue_names_pair(const spm_jst_rescue &R, uint32_t n_pairs) { return R.pair < n_pairs && (R.pattern >> 2) == R.pair; }
// ... and an anchor that is that pair's locus for the OTHER mate, in a pair that is not proper
SPM_HD inline bool jst_sam_rescue_ok(const spm_jst_rescue &R, const spm_jst_pair &P, uint32_t pair, uint32_t n_pairs)
{
    if (!jst_sam_rescue_names_pair(R, n_pairs) || R.pair != pair || R.status > SPM_RESCUE_NOT_CONCORDANT || (P.flag1 & 0x2u))
        return false;
    const uint32_t rescued = (R.pattern >> 1) & 1u;
    const uint32_t anchor = rescued ? P.locus1 : P.locus2;
    return anchor != kSamNone && R.anchor == anchor;
}

// ---- the reported line of a read ----
struct jst_sam_reported
{
    uint32_t source = kSamNone;
    uint32_t x0 = 0, x1 = 0; // the counts behind the MAPQ
    uint64_t pos = 0;        // POS; 0: no line
    uint16_t flag = 0;
    uint8_t mapq = 0, kind = SPM_SAM_UNMAPPED;
    bool reverse = false;
};
struct jst_sam_pair_plan
{
    jst_sam_reported mate[2];
    int32_t tlen = 0; // mate 1's; mate 2's line has its negative
    bool ok = true;
};

SPM_HD inline jst_sam_reported jst_sam_plan_single(const jst_sam_src &S, uint32_t read, bool &ok)
{
    jst_sam_reported O;
    const spm_jst_read R = S.reads[read];
    ok = jst_sam_read_ok(S.loci, S.n_loci, R, read, S.strands);
    O.flag = 0x4;
    if (!ok || R.primary == kSamNone)
        return O;
    const spm_jst_ref_locus L = S.loci[R.primary];
    O.kind = SPM_SAM_LOCUS;
    O.source = R.primary;
    O.reverse = S.strands == 2 && (L.pattern & 1u);
    O.flag = O.reverse ? 0x10 : 0;
    O.x0 = R.n_best;
    O.x1 = R.n_next;
    O.mapq = jst_sam_mapq(S.tables, R.n_best, R.n_next);
    O.pos = L.ref_begin + 1;
    return O;
}

// the flag of the anchor's line beside a used rescue
SPM_HD inline uint16_t jst_sam_anchor_flag(uint16_t pair_flag, uint16_t rescue_flag)
{
    const uint16_t f = (uint16_t)((pair_flag | 0x2u) & ~0x8u & ~0x20u);
    return (uint16_t)(f | ((rescue_flag & 0x10u) ? 0x20u : 0u));
}

// Which of a pair's rescue records is used: candidates c[0 .. n) in record order, index of the RESCUED one with the smallest
// score, on a tie the first; -1: none
SPM_HD inline int jst_sam_choose_rescue(const spm_jst_rescue *c, int n)
{
    int used = -1;
    for (int i = 0; i < n; ++i)
        if (c[i].status == SPM_RESCUE_RESCUED && (used < 0 || c[i].score < c[used].score))
            used = i;
    return used;
}

// The two reported lines of pair p (S.pairs is set, strands == 2).
SPM_HD inline jst_sam_pair_plan jst_sam_plan_pair(const jst_sam_src &S, uint32_t p)
{
    jst_sam_pair_plan O;
    const spm_jst_pair R = S.pairs[p];
    const spm_jst_read M[2] = {S.reads[2 * p], S.reads[2 * p + 1]};
    const uint32_t locus[2] = {R.locus1, R.locus2};
    const uint16_t flag[2] = {R.flag1, R.flag2};
    O.ok = jst_sam_read_ok(S.loci, S.n_loci, M[0], 2 * p, 2) && jst_sam_read_ok(S.loci, S.n_loci, M[1], 2 * p + 1, 2) &&
           jst_rescue_pair_ok(S.loci, S.n_loci, M[0], M[1], R, p, ~0ull);
    for (int x = 0; x < 2 && O.ok; ++x)
        O.ok = locus[x] == kSamNone || jst_sam_in_run(M[x], locus[x]);
    if (!O.ok)
        return O;
    // the rescue records of the pair: at most two, contiguous from first_rescue[p]
    spm_jst_rescue c[2] = {};
    int n_c = 0;
    uint32_t first = kSamNone;
    if (S.rescues && S.first_rescue && (first = S.first_rescue[p]) != kSamNone) {
        for (uint32_t j = first; n_c < 2 && j < S.n_rescues && j - first < 2u && S.rescues[j].pair == p; ++j) {
            c[n_c] = S.rescues[j];
            if (!jst_sam_rescue_ok(c[n_c], R, p, S.n_pairs) ||
                (c[n_c].status == SPM_RESCUE_RESCUED && !jst_sam_transcript_ok(c[n_c].cigar_off, c[n_c].cigar_len, S.n_rescue_ops))) {
                O.ok = false;
                return O;
            }
            ++n_c;
        }
    }
    const int used = jst_sam_choose_rescue(c, n_c);
    const bool proper = (R.flag1 & 0x2u) != 0;
    if (used >= 0) {
        const spm_jst_rescue U = c[used];
        const uint32_t y = (U.pattern >> 1) & 1u, a = y ^ 1u; // the rescued mate, the anchor's
        const spm_jst_ref_locus A = S.loci[U.anchor];          // (U.anchor == locus[a] < n_loci: jst_rescue_pair_ok)
        const uint8_t q = jst_sam_mapq(S.tables, M[a].n_best, M[a].n_next);
        O.mate[y].kind = SPM_SAM_RESCUE;
        O.mate[y].source = first + (uint32_t)used;
        O.mate[y].flag = U.flag;
        O.mate[y].pos = U.ref_begin + 1;
        O.mate[y].reverse = (U.flag & 0x10u) != 0;
        O.mate[a].kind = SPM_SAM_LOCUS;
        O.mate[a].source = U.anchor;
        O.mate[a].flag = jst_sam_anchor_flag(flag[a], U.flag);
        O.mate[a].pos = A.ref_begin + 1;
        O.mate[a].reverse = (A.pattern & 1u) != 0;
        for (int x = 0; x < 2; ++x) {
            O.mate[x].mapq = q;
            O.mate[x].x0 = M[a].n_best;
            O.mate[x].x1 = M[a].n_next;
        }
        O.tlen = U.tlen;
        return O;
    }
    for (int x = 0; x < 2; ++x) {
        O.mate[x].flag = flag[x];
        if (locus[x] == kSamNone)
            continue;
        const spm_jst_ref_locus L = S.loci[locus[x]];
        O.mate[x].kind = SPM_SAM_LOCUS;
        O.mate[x].source = locus[x];
        O.mate[x].pos = L.ref_begin + 1;
        O.mate[x].reverse = (L.pattern & 1u) != 0;
        O.mate[x].x0 = proper ? R.n_best : M[x].n_best;
        O.mate[x].x1 = proper ? R.n_next : M[x].n_next;
        O.mate[x].mapq = jst_sam_mapq(S.tables, O.mate[x].x0, O.mate[x].x1);
    }
    O.tlen = R.tlen;
    return O;
}

// the lines of a read: its reported line and, with SPM_SAM_SECONDARY, every locus of it that is not the reported one
SPM_HD inline uint32_t jst_sam_line_count(const spm_jst_read &R, const jst_sam_reported &own, uint32_t flags)
{
    if (!(flags & SPM_SAM_SECONDARY))
        return 1;
    return 1 + R.n_loci - (own.kind == SPM_SAM_LOCUS ? 1u : 0u);
}

// the flag of a secondary line; paired: mate2 and the mate's reported line
SPM_HD inline uint16_t jst_sam_secondary_flag(bool reverse, bool paired, bool mate2, const jst_sam_reported &other)
{
    uint32_t f = 0x100u | (reverse ? 0x10u : 0u);
    if (paired)
        f |= 0x1u | (mate2 ? 0x80u : 0x40u) | (other.kind == SPM_SAM_UNMAPPED ? 0x8u : (other.reverse ? 0x20u : 0u));
    return (uint16_t)f;
}

// The records of read r's lines, written to lines[0 .. count) and aux[0 .. count): the reported line, then the secondaries
// in locus order.  own / other: the plan (other only in paired mode); tlen: this mate's.
SPM_HD inline void jst_sam_read_lines(const jst_sam_src &S, uint32_t read, const jst_sam_reported &own, const jst_sam_reported *other,
                                      int32_t tlen, spm_sam_line *lines, jst_sam_aux *aux, uint32_t cap)
{
    const uint64_t mate_pos = other ? other->pos : 0;
    uint32_t at = 0;
    spm_sam_line L{};
    L.read = read;
    L.source = own.source;
    L.flag = own.flag;
    L.mapq = own.mapq;
    L.kind = own.kind;
    if (at < cap) {
        lines[at] = L;
        aux[at] = jst_sam_aux{mate_pos, own.kind == SPM_SAM_UNMAPPED ? 0 : tlen, own.x0, own.x1, 0};
    }
    ++at;
    if (!(S.flags & SPM_SAM_SECONDARY))
        return;
    const spm_jst_read R = S.reads[read]; // (tested by the plan)
    for (uint32_t i = R.first_locus; i < R.first_locus + R.n_loci; ++i) {
        if (own.kind == SPM_SAM_LOCUS && i == own.source)
            continue;
        L.source = i;
        L.flag = jst_sam_secondary_flag(S.strands == 2 && (S.loci[i].pattern & 1u), other != nullptr, (read & 1u) != 0,
                                        other ? *other : jst_sam_reported{});
        L.mapq = 255;
        L.kind = SPM_SAM_SECONDARY_LINE;
        if (at < cap) {
            lines[at] = L;
            aux[at] = jst_sam_aux{mate_pos, 0, 0, 0, 0};
        }
        ++at;
    }
}

// ---- a line resolved against its sources: everything the composition prints ----
struct jst_sam_fields
{
    uint64_t name = 0;       // index of the QNAME
    uint64_t pos = 0, pnext = 0;
    const uint32_t *words = nullptr; // nullptr: CIGAR *
    uint32_t n_words = 0;
    const uint8_t *seq = nullptr;    // nullptr: SEQ *
    uint32_t m = 0;
    uint32_t flag = 0, mapq = 0;
    int32_t tlen = 0, nm = 0, xh = 0;
    uint32_t xn = 0, x0 = 0, x1 = 0;
    uint8_t kind = SPM_SAM_UNMAPPED;
    bool rname = false, rnext = false;
    const uint8_t *qual = nullptr; // nullptr: QUAL *
    const uint8_t *md_ref = nullptr; // the reference at pos - 1; nullptr: no MD
    bool qual_reverse = false;
};

// Does the record of a line agree with its sources?  Every index before it is one; fills F when it does.  check_query: walk
// the transcript and compare its query length with the needle's (the measure stage does, once per line).
SPM_HD inline bool jst_sam_resolve(const jst_sam_src &S, const spm_sam_line &L, const jst_sam_aux &A, jst_sam_fields &F,
                                   bool check_query)
{
    F = jst_sam_fields{};
    if (L.read >= S.n_reads || L.kind > SPM_SAM_SECONDARY_LINE)
        return false;
    const bool paired = S.pairs != nullptr, mapped = L.kind != SPM_SAM_UNMAPPED;
    const bool mate_has = paired && !(L.flag & 0x8u) && A.mate_pos != 0;
    F.kind = L.kind;
    F.name = paired ? L.read / 2 : L.read;
    F.flag = L.flag;
    F.mapq = L.mapq;
    F.tlen = A.tlen;
    F.x0 = A.x0;
    F.x1 = A.x1;
    uint32_t pattern = S.strands * L.read; // an unmapped line prints the forward read
    uint64_t ref_end = 0;
    bool reverse = false;
    if (L.kind == SPM_SAM_LOCUS || L.kind == SPM_SAM_SECONDARY_LINE) {
        if (L.source >= S.n_loci)
            return false;
        const spm_jst_ref_locus X = S.loci[L.source];
        if (X.pattern / S.strands != L.read || X.ref_begin > X.ref_end || !jst_sam_transcript_ok(X.cigar_off, X.cigar_len, S.n_ops))
            return false;
        pattern = X.pattern;
        reverse = S.strands == 2 && (X.pattern & 1u);
        ref_end = X.ref_end;
        F.pos = X.ref_begin + 1;
        F.words = S.ops + X.cigar_off;
        F.n_words = X.cigar_len;
        F.nm = X.ref_score;
        F.xh = X.score;
        F.xn = X.n_haplotypes;
    } else if (L.kind == SPM_SAM_RESCUE) {
        if (L.source >= S.n_rescues)
            return false;
        const spm_jst_rescue X = S.rescues[L.source];
        if ((X.pattern >> 1) != L.read || X.ref_begin > X.ref_end || !jst_sam_transcript_ok(X.cigar_off, X.cigar_len, S.n_rescue_ops))
            return false;
        pattern = X.pattern;
        reverse = (X.flag & 0x10u) != 0;
        ref_end = X.ref_end;
        F.pos = X.ref_begin + 1;
        F.words = S.rescue_ops + X.cigar_off;
        F.n_words = X.cigar_len;
        F.nm = X.score;
    }
    if (pattern >= S.n_needles || S.m[pattern] < 0)
        return false;
    F.m = (uint32_t)S.m[pattern];
    if (mapped && S.ref)
        F.md_ref = S.ref + (F.pos - 1);
    if (mapped && check_query) { // the query length of the transcript is the needle's
        uint64_t q, r;
        jst_sam_cigar_spans(F.words, F.n_words, q, r);
        if (q != F.m)
            return false;
        if (S.ref) { // the locus and what the transcript spans lie inside the reference, whose X columns disagree with the read
            if (ref_end > S.ref_n || F.pos - 1 > S.ref_n || r > S.ref_n - (F.pos - 1))
                return false;
            if (!jst_sam_md_agrees(F.words, F.n_words, F.md_ref, S.ranks + S.offsets[pattern]))
                return false;
        }
    }
    if (L.kind != SPM_SAM_SECONDARY_LINE) {
        F.seq = S.ranks + S.offsets[pattern];
        if (S.qual) { // (a read and its reverse complement have one length: what q_off was summed from)
            if (S.m[S.strands * L.read] != S.m[pattern])
                return false;
            F.qual = S.qual + S.q_off[L.read];
            F.qual_reverse = reverse;
        }
    }
    if (!mapped)
        F.pos = mate_has ? A.mate_pos : 0;
    F.rname = mapped || mate_has;
    F.rnext = paired && (mapped || mate_has);
    F.pnext = mate_has ? A.mate_pos : (paired && mapped ? F.pos : 0);
    return true;
}

// up to 8 characters in a uint64, the first in the low byte: the literal pieces of a line
SPM_HD constexpr uint64_t jst_sam_pack(const char *s, int n) { return n == 0 ? 0ull : (uint64_t)(uint8_t)s[0] | jst_sam_pack(s + 1, n - 1) << 8; }
#define SPM_SAM_LIT(s) ::spm_hip::jst_sam_pack(s, (int)sizeof(s) - 1), (uint32_t)(sizeof(s) - 1)

// The composition of a line.  A sink takes
//   num(lit, n_lit, v, negative)   n_lit literal characters, then '-' if negative, then v in decimal
//   text(lit, n_lit)               literal characters
//   bytes(p, n)                    n characters at p
//   seq(ranks, m, symbols, sigma)  m ranks as letters
//   cigar(words, n, merge)
//   qual(values, m, reverse, add)  m values + add, back to front with reverse
//   md(words, n, ref, symbols, sigma)   the MD string; ref: the reference at the transcript's first position
// kExtras = false: a composition that knows neither qual nor md, for a call without spm_sam_extras (the write kernel of such a
// call is then the code it was before the two fields existed).
template <bool kExtras = true, class Sink> SPM_HD inline void jst_sam_compose(const jst_sam_src &S, const jst_sam_fields &F, Sink &out)
{
    if (S.names)
        out.bytes(S.names + S.name_off[F.name], S.name_off[F.name + 1] - S.name_off[F.name]);
    else
        out.num(0, 0, F.name, false);
    out.num(SPM_SAM_LIT("\t"), F.flag, false);
    if (F.rname) {
        out.text(SPM_SAM_LIT("\t"));
        out.bytes(S.rname, S.rname_len);
    } else {
        out.text(SPM_SAM_LIT("\t*"));
    }
    out.num(SPM_SAM_LIT("\t"), F.pos, false);
    out.num(SPM_SAM_LIT("\t"), F.mapq, false);
    if (F.words) {
        out.text(SPM_SAM_LIT("\t"));
        out.cigar(F.words, F.n_words, (S.flags & SPM_SAM_CIGAR_M) != 0);
    } else {
        out.text(SPM_SAM_LIT("\t*"));
    }
    if (F.rnext)
        out.num(SPM_SAM_LIT("\t=\t"), F.pnext, false);
    else
        out.num(SPM_SAM_LIT("\t*\t"), F.pnext, false);
    out.num(SPM_SAM_LIT("\t"), jst_sam_int_abs(F.tlen), F.tlen < 0);
    if (F.seq) {
        out.text(SPM_SAM_LIT("\t"));
        out.seq(F.seq, F.m, S.symbols, S.sigma);
        if (kExtras && F.qual) {
            out.text(SPM_SAM_LIT("\t"));
            out.qual(F.qual, F.m, F.qual_reverse, 33);
        } else {
            out.text(SPM_SAM_LIT("\t*"));
        }
    } else {
        out.text(SPM_SAM_LIT("\t*\t*"));
    }
    if (F.kind != SPM_SAM_UNMAPPED) {
        out.num(SPM_SAM_LIT("\tNM:i:"), jst_sam_int_abs(F.nm), F.nm < 0);
        if (kExtras && F.md_ref) {
            out.text(SPM_SAM_LIT("\tMD:Z:"));
            out.md(F.words, F.n_words, F.md_ref, S.symbols, S.sigma);
        }
        if (F.kind == SPM_SAM_RESCUE) {
            out.text(SPM_SAM_LIT("\tXR:i:1"));
        } else {
            out.num(SPM_SAM_LIT("\tXH:i:"), jst_sam_int_abs(F.xh), F.xh < 0);
            out.num(SPM_SAM_LIT("\tXN:i:"), F.xn, false);
        }
        if (F.kind != SPM_SAM_SECONDARY_LINE) {
            out.num(SPM_SAM_LIT("\tX0:i:"), F.x0, false);
            out.num(SPM_SAM_LIT("\tX1:i:"), F.x1, false);
        }
    }
    out.text(SPM_SAM_LIT("\n"));
}

// the measuring sink: lengths only
struct jst_sam_measure
{
    uint64_t n = 0;
    SPM_HD void num(uint64_t, uint32_t n_lit, uint64_t v, bool negative) { n += n_lit + (negative ? 1u : 0u) + jst_sam_dec_len(v); }
    SPM_HD void text(uint64_t, uint32_t n_lit) { n += n_lit; }
    SPM_HD void bytes(const char *, uint64_t len) { n += len; }
    SPM_HD void seq(const uint8_t *, uint32_t m, const char *, uint32_t) { n += m; }
    SPM_HD void cigar(const uint32_t *words, uint32_t n_words, bool merge)
    {
        uint64_t add = 0;
        jst_sam_cigar_items(words, n_words, merge, [&add](uint64_t run, char) { add += jst_sam_word_len(run); });
        n += add;
    }
    SPM_HD void qual(const uint8_t *, uint32_t m, bool, uint8_t) { n += jst_sam_qual_len(m); }
    SPM_HD void md(const uint32_t *words, uint32_t n_words, const uint8_t *, const char *, uint32_t)
    {
        uint64_t add = 0;
        const uint64_t c = jst_sam_md_items(words, n_words, [&add](uint64_t c, uint32_t word, uint64_t) { add += jst_sam_md_word_len(c, word); });
        n += add + jst_sam_dec_len(c);
    }
};

// the serial sink: the bytes one after the other into [to, to + cap); n counts on beyond cap without writing
struct jst_sam_serial
{
    char *to = nullptr;
    uint64_t cap = 0, n = 0;
    SPM_HD void put(char c)
    {
        if (n < cap)
            to[n] = c;
        ++n;
    }
    SPM_HD void num(uint64_t lit, uint32_t n_lit, uint64_t v, bool negative)
    {
        text(lit, n_lit);
        if (negative)
            put('-');
        const uint32_t len = jst_sam_dec_len(v);
        for (uint32_t i = 0; i < len; ++i)
            put(jst_sam_dec_char(v, len, i));
    }
    SPM_HD void text(uint64_t lit, uint32_t n_lit)
    {
        for (uint32_t i = 0; i < n_lit; ++i)
            put((char)(lit >> (8 * i)));
    }
    SPM_HD void bytes(const char *p, uint64_t len)
    {
        for (uint64_t i = 0; i < len; ++i)
            put(p[i]);
    }
    SPM_HD void seq(const uint8_t *ranks, uint32_t m, const char *symbols, uint32_t sigma)
    {
        for (uint32_t i = 0; i < m; ++i)
            put(jst_sam_seq_char(ranks[i], symbols, sigma));
    }
    SPM_HD void cigar(const uint32_t *words, uint32_t n_words, bool merge)
    {
        jst_sam_cigar_items(words, n_words, merge, [this](uint64_t run, char op) {
            const uint32_t len = jst_sam_word_len(run);
            for (uint32_t i = 0; i < len; ++i)
                put(jst_sam_word_char(run, op, len, i));
        });
    }
    SPM_HD void qual(const uint8_t *values, uint32_t m, bool reverse, uint8_t add)
    {
        for (uint32_t i = 0; i < jst_sam_qual_len(m); ++i)
            put((char)jst_sam_qual_byte(values, m, reverse, add, i));
    }
    SPM_HD void md(const uint32_t *words, uint32_t n_words, const uint8_t *ref, const char *symbols, uint32_t sigma)
    {
        const uint64_t c = jst_sam_md_items(words, n_words, [&](uint64_t c, uint32_t word, uint64_t at) {
            const uint64_t len = jst_sam_md_word_len(c, word);
            for (uint64_t i = 0; i < len; ++i)
                put(jst_sam_md_word_char(c, word, ref + at, symbols, sigma, i));
        });
        num(0, 0, c, false);
    }
};

} // namespace spm_hip
