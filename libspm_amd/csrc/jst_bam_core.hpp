// jst_bam_core.hpp -- the composition of a BAM record (spm_hip_jst_ref_loci_bam; contract in spm_hip.h, scheme in DESIGN.md
// 4.12).  Host-compilable and device code alike, in the manner of jst_sam_core.hpp, whose rule it does not repeat: which
// records exist, their order, FLAG, MAPQ, mate fields and counts are jst_sam_resolve's jst_sam_fields.  Here: the bin, the
// 4-bit code of a letter, what makes a record unwritable, and jst_bam_compose, which hands a record field by field to a sink --
// measuring, serial, or the wave sink of jst_bam.hpp -- through ONE length function and ONE byte function per kind of field.
//
// Tags are 7 bytes each whatever the value (NM, XH, XR: type i; XN, X0, X1: type I, since the counts arrive clamped to
// 0xFFFFFFFF): fixed-width ON PURPOSE, so that a record's length does not depend on its values and lane i of a tag is byte i.
// The one exception is MD (spm_sam_extras), type Z: 4d 44 5a, the string of jst_sam_core.hpp's md, 00.
#pragma once

#include "hd.hpp"
#include "jst_sam_core.hpp"

namespace spm_hip
{

constexpr uint32_t kBamFixed = 36, kBamTag = 7, kBamMaxItems = 65535, kBamMaxRun = (1u << 28) - 1;
constexpr uint64_t kBamMaxRefLen = 0x7FFFFFFFull;

// the standard reg2bin of the SAM specification (section 5.3): the smallest bin that holds [beg, end)
SPM_HD inline uint32_t jst_bam_reg2bin(int32_t beg, int32_t end)
{
    --end;
    if (beg >> 14 == end >> 14)
        return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17)
        return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20)
        return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23)
        return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26)
        return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
// the bin of a record at 0-based pos (-1: none) that spans `span` reference symbols: a span of 0 (unmapped, or a locus inside
// an insertion) counts as 1
SPM_HD inline uint32_t jst_bam_bin(int32_t pos, uint64_t span)
{
    if (pos < 0)
        return 4680;
    const uint64_t end = (uint64_t)pos + (span ? span : 1);
    return jst_bam_reg2bin(pos, (int32_t)(end < 0x7FFFFFFFull ? end : 0x7FFFFFFFull));
}

// the 4-bit code of a letter: its place in =ACMGRSVTWYHKDBN, in either case; anything else is N
SPM_HD inline uint8_t jst_bam_nibble(char c)
{
    const char *const letters = "=ACMGRSVTWYHKDBN";
    const char up = (c >= 'a' && c <= 'z') ? (char)(c - 32) : c;
    for (uint8_t i = 0; i < 16; ++i)
        if (letters[i] == up)
            return i;
    return 15;
}
// codes[rank] for every rank a byte can hold, built once per call
inline void jst_bam_rank_codes(const char *symbols, uint32_t sigma, uint8_t codes[256])
{
    for (uint32_t r = 0; r < 256; ++r)
        codes[r] = r < sigma ? jst_bam_nibble(symbols[r]) : 15;
}

// ---- what makes a record unwritable ----
SPM_HD inline bool jst_bam_items_ok(uint64_t n_items) { return n_items <= kBamMaxItems; }
SPM_HD inline bool jst_bam_run_ok(uint64_t run) { return run >= 1 && run <= kBamMaxRun; }
SPM_HD inline bool jst_bam_end_ok(uint64_t ref_end, uint64_t ref_len) { return ref_end <= ref_len; }

// Walks the items of a transcript as a record holds them: f(run length, a word of the item) per word, or per maximal run of
// = / X words with `merge`.  (jst_sam_cigar_items hands out the op as a character; a record wants the word.)
template <class Fn> SPM_HD inline void jst_bam_cigar_items(const uint32_t *words, uint32_t n, bool merge, Fn &&f)
{
    uint64_t run = 0;
    for (uint32_t w = 0; w < n; ++w) {
        const uint32_t word = words[w];
        if (merge && jst_sam_op_is_m(word)) {
            run += word >> 4;
            if (w + 1 == n || !jst_sam_op_is_m(words[w + 1])) {
                f(run, word);
                run = 0;
            }
        } else {
            f((uint64_t)(word >> 4), word);
        }
    }
}

// what the fixed part needs of the transcript
struct jst_bam_shape
{
    uint32_t n_items = 0; // n_cigar_op
    uint32_t bin = 4680;
};
// -> false: the record cannot be written (an item count above 65535, an item of length 0 or above 2^28 - 1, an end beyond
// the reference)
SPM_HD inline bool jst_bam_shape_of(const jst_sam_src &S, const jst_sam_fields &F, uint64_t ref_len, jst_bam_shape &O)
{
    const bool merge = (S.flags & SPM_SAM_CIGAR_M) != 0;
    uint64_t span = 0, items = 0;
    bool ok = true;
    if (F.words) {
        for (uint32_t w = 0; w < F.n_words; ++w) {
            const uint32_t op = F.words[w] & 15u;
            span += (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X || op == SPM_CIGAR_DEL) ? (F.words[w] >> 4) : 0u;
        }
        jst_bam_cigar_items(F.words, F.n_words, merge, [&](uint64_t run, uint32_t) {
            ++items;
            ok = ok && jst_bam_run_ok(run);
        });
        ok = ok && jst_bam_items_ok(items) && jst_bam_end_ok(F.pos - 1 + span, ref_len); // (F.words: a mapped line, pos >= 1)
    }
    O.n_items = (uint32_t)items;
    O.bin = jst_bam_bin((int32_t)((uint32_t)F.pos - 1u), span);
    return ok;
}

// ---- per kind of field: its length and its byte i ----
SPM_HD inline uint8_t jst_bam_le_byte(uint32_t v, uint32_t i) { return (uint8_t)(v >> (8 * i)); }                 // i < 4
SPM_HD inline uint8_t jst_bam_fixed_byte(const uint32_t *w, uint32_t i) { return jst_bam_le_byte(w[i >> 2], i & 3); } // i < 36
SPM_HD inline uint32_t jst_bam_item_word(uint64_t run, uint32_t word, bool merge) // a printed item as a BAM CIGAR word
{
    return (uint32_t)run << 4 | ((merge && jst_sam_op_is_m(word)) ? 0u : (word & 15u));
}
SPM_HD inline uint32_t jst_bam_seq_len(uint32_t m) { return (m + 1) / 2; }
SPM_HD inline uint8_t jst_bam_seq_byte(const uint8_t *ranks, uint32_t m, const uint8_t *codes, uint32_t i) // i < jst_bam_seq_len(m)
{
    return (uint8_t)(codes[ranks[2 * i]] << 4 | (2 * i + 1 < m ? codes[ranks[2 * i + 1]] : 0));
}
SPM_HD constexpr uint32_t jst_bam_tag_head(char a, char b, char type) { return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)type << 16; }
SPM_HD inline uint8_t jst_bam_tag_byte(uint32_t head, uint32_t v, uint32_t i) { return i < 3 ? jst_bam_le_byte(head, i) : jst_bam_le_byte(v, i - 3); } // i < 7

// the 36 fixed bytes as nine little-endian words: block_size and the eight that follow
SPM_HD inline void jst_bam_fixed(const jst_sam_fields &F, const jst_bam_shape &H, uint32_t block_size, uint32_t l_read_name, uint32_t w[9])
{
    w[0] = block_size;
    w[1] = F.rname ? 0u : ~0u;                              // refID
    w[2] = (uint32_t)F.pos - 1u;                            // pos: POS - 1, POS 0 gives -1
    w[3] = l_read_name | F.mapq << 8 | H.bin << 16;         // l_read_name u8, mapq u8, bin u16
    w[4] = H.n_items | F.flag << 16;                        // n_cigar_op u16, flag u16
    w[5] = F.seq ? F.m : 0u;                                // l_seq
    w[6] = F.rnext ? 0u : ~0u;                              // next_refID
    w[7] = (uint32_t)F.pnext - 1u;                          // next_pos
    w[8] = (uint32_t)F.tlen;
}

// The composition of a record.  A sink takes
//   fixed(w)                   the 36 fixed bytes, nine words
//   bytes(p, n)                n bytes at p
//   num(v)                     v in decimal
//   fill(c, n)                 n bytes c
//   cigar(words, n, merge)     the items as words
//   seq(ranks, m, codes)       m ranks, two per byte
//   tag(head, v)               7 bytes
//   qual(values, m, reverse, add)   as the text's
//   md(words, n, ref, symbols, sigma)   MD Z, the text's string, NUL
// block_size: what the measuring sink found, less 4 (the measuring sink itself does not look at it).
template <class Sink>
SPM_HD inline void jst_bam_compose(const jst_sam_src &S, const jst_sam_fields &F, const jst_bam_shape &H, const uint8_t *codes,
                                   uint32_t block_size, Sink &out)
{
    const uint64_t name_len = S.names ? S.name_off[F.name + 1] - S.name_off[F.name] : jst_sam_dec_len(F.name);
    uint32_t w[9];
    jst_bam_fixed(F, H, block_size, (uint32_t)name_len + 1, w);
    out.fixed(w);
    if (S.names)
        out.bytes(S.names + S.name_off[F.name], name_len);
    else
        out.num(F.name);
    out.fill(0, 1);
    if (F.words)
        out.cigar(F.words, F.n_words, (S.flags & SPM_SAM_CIGAR_M) != 0);
    if (F.seq) {
        out.seq(F.seq, F.m, codes);
        if (F.qual)
            out.qual(F.qual, F.m, F.qual_reverse, 0);
        else
            out.fill(0xff, F.m);
    }
    if (F.kind != SPM_SAM_UNMAPPED) {
        out.tag(jst_bam_tag_head('N', 'M', 'i'), (uint32_t)F.nm);
        if (F.md_ref)
            out.md(F.words, F.n_words, F.md_ref, S.symbols, S.sigma);
        if (F.kind == SPM_SAM_RESCUE) {
            out.tag(jst_bam_tag_head('X', 'R', 'i'), 1);
        } else {
            out.tag(jst_bam_tag_head('X', 'H', 'i'), (uint32_t)F.xh);
            out.tag(jst_bam_tag_head('X', 'N', 'I'), F.xn);
        }
        if (F.kind != SPM_SAM_SECONDARY_LINE) {
            out.tag(jst_bam_tag_head('X', '0', 'I'), F.x0);
            out.tag(jst_bam_tag_head('X', '1', 'I'), F.x1);
        }
    }
}

// the measuring sink: lengths only
struct jst_bam_measure
{
    uint64_t n = 0;
    SPM_HD void fixed(const uint32_t *) { n += kBamFixed; }
    SPM_HD void bytes(const char *, uint64_t len) { n += len; }
    SPM_HD void num(uint64_t v) { n += jst_sam_dec_len(v); }
    SPM_HD void fill(uint8_t, uint64_t len) { n += len; }
    SPM_HD void cigar(const uint32_t *words, uint32_t n_words, bool merge)
    {
        uint64_t add = 0;
        jst_bam_cigar_items(words, n_words, merge, [&add](uint64_t, uint32_t) { add += 4; });
        n += add;
    }
    SPM_HD void seq(const uint8_t *, uint32_t m, const uint8_t *) { n += jst_bam_seq_len(m); }
    SPM_HD void tag(uint32_t, uint32_t) { n += kBamTag; }
    SPM_HD void qual(const uint8_t *, uint32_t m, bool, uint8_t) { n += jst_sam_qual_len(m); }
    SPM_HD void md(const uint32_t *words, uint32_t n_words, const uint8_t *ref, const char *symbols, uint32_t sigma)
    {
        jst_sam_measure M;
        M.md(words, n_words, ref, symbols, sigma);
        n += 3 + M.n + 1;
    }
};

// the serial sink: the bytes one after the other into [to, to + cap); n counts on beyond cap without writing
struct jst_bam_serial
{
    uint8_t *to = nullptr;
    uint64_t cap = 0, n = 0;
    SPM_HD void put(uint8_t c)
    {
        if (n < cap)
            to[n] = c;
        ++n;
    }
    SPM_HD void fixed(const uint32_t *w)
    {
        for (uint32_t i = 0; i < kBamFixed; ++i)
            put(jst_bam_fixed_byte(w, i));
    }
    SPM_HD void bytes(const char *p, uint64_t len)
    {
        for (uint64_t i = 0; i < len; ++i)
            put((uint8_t)p[i]);
    }
    SPM_HD void num(uint64_t v)
    {
        const uint32_t len = jst_sam_dec_len(v);
        for (uint32_t i = 0; i < len; ++i)
            put((uint8_t)jst_sam_dec_char(v, len, i));
    }
    SPM_HD void fill(uint8_t c, uint64_t len)
    {
        for (uint64_t i = 0; i < len; ++i)
            put(c);
    }
    SPM_HD void cigar(const uint32_t *words, uint32_t n_words, bool merge)
    {
        jst_bam_cigar_items(words, n_words, merge, [&](uint64_t run, uint32_t word) {
            const uint32_t item = jst_bam_item_word(run, word, merge);
            for (uint32_t i = 0; i < 4; ++i)
                put(jst_bam_le_byte(item, i));
        });
    }
    SPM_HD void seq(const uint8_t *ranks, uint32_t m, const uint8_t *codes)
    {
        for (uint32_t i = 0; i < jst_bam_seq_len(m); ++i)
            put(jst_bam_seq_byte(ranks, m, codes, i));
    }
    SPM_HD void tag(uint32_t head, uint32_t v)
    {
        for (uint32_t i = 0; i < kBamTag; ++i)
            put(jst_bam_tag_byte(head, v, i));
    }
    SPM_HD void qual(const uint8_t *values, uint32_t m, bool reverse, uint8_t add)
    {
        for (uint32_t i = 0; i < jst_sam_qual_len(m); ++i)
            put(jst_sam_qual_byte(values, m, reverse, add, i));
    }
    SPM_HD void md(const uint32_t *words, uint32_t n_words, const uint8_t *ref, const char *symbols, uint32_t sigma)
    {
        for (uint32_t i = 0; i < 3; ++i)
            put(jst_bam_le_byte(jst_bam_tag_head('M', 'D', 'Z'), i));
        jst_sam_serial T{reinterpret_cast<char *>(to), cap, n};
        T.md(words, n_words, ref, symbols, sigma);
        n = T.n;
        put(0);
    }
};

} // namespace spm_hip
