// libspm/jst/journaled_sequence_tree.hpp -- a reference sequence + variants shared by many haplotypes, and the
// search of a needle set over ALL haplotypes on the MI355X (config C5 of BASELINE.json).
//
// The reference has no traversal code -- only the journaled-sequence design (specs/...class_diagram.drawio) and the
// matcher-side hooks a traverser needs (window_size / capture / restore, matcher/concept.hpp:26-161).  The contract
// taken here is the one SURVEY 8f-2 states: the hit set must equal the union over haplotypes of a linear scan of each
// materialised haplotype, reported as (haplotype, position).
//
// How (GPU-first): the reference axis is cut into blocks; for every haplotype the block's haplotype-local sequence
// plus window_size-1 symbols of left context is a *context*.  Haplotypes that carry the same alleles around a block
// have byte-identical contexts, so contexts are deduplicated and only the UNIQUE ones are laid out back to back and
// scanned -- in one launch -- as independent haystacks (spm_hip_scan_segments).  A hit is owned by the context whose
// block contains its last symbol and is fanned out to every haplotype sharing that context.  By the window property
// (a hit depends only on the window_size symbols ending at it) this is exact.  Work on the device is proportional to
// the distinct sequence content, not to haplotypes x length.
//
// No haplotype is materialised to do this: contexts are cut and deduplicated by *signature* (start point in
// reference/alt space + the alleles the stretch touches) straight from the per-haplotype allele lists, and only one
// representative per signature is spelled out.  Host work is blocks x haplotypes x (alleles per block) plus the unique
// context bytes.
#pragma once

#include <algorithm>
#include <array>
#include <cctype>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <string_view>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include <libspm/hip/context.hpp>
#include <libspm/jst/io.hpp>
#include <libspm/jst/journaled_sequence.hpp>
#include <libspm/matcher/alignment.hpp>
#include <libspm/matcher/hip_pattern_base.hpp>

namespace spm
{
struct jst_hit
{
    std::uint32_t haplotype;
    std::uint64_t position; // what the matcher reports (Myers: exclusive end; exact: begin), haplotype coordinates
    std::uint32_t needle;
    std::int32_t errors;
    bool operator==(jst_hit const &) const noexcept = default;
    auto operator<=>(jst_hit const &) const noexcept = default;
};

// where a hit begins in its haplotype and how it aligns there (journaled_sequence_tree::locate)
struct jst_alignment
{
    std::uint32_t haplotype;
    std::uint32_t needle;
    spm::alignment aln; // begin / end in haplotype coordinates, errors, CIGAR transcript
    bool operator==(jst_alignment const &) const noexcept = default;
};

// the same alignment against the REFERENCE of the tree (journaled_sequence_tree::locate_reference): SAM POS, CIGAR and NM
struct jst_ref_alignment
{
    std::uint32_t haplotype;
    std::uint32_t needle;
    spm::alignment aln;             // reference coordinates, errors = ref_score (X + I + D of the projected transcript)
    std::int32_t haplotype_errors;  // the distance on the haplotype, as locate reports it
    bool operator==(jst_ref_alignment const &) const noexcept = default;
};

// one distinct reference alignment of a needle (journaled_sequence_tree::locate_reference_loci): the alignments of
// locate_reference that agree in needle, reference range and transcript, merged, with the haplotypes that support it
struct jst_ref_locus
{
    std::uint32_t needle;
    spm::alignment aln;             // reference coordinates, errors = ref_score
    std::int32_t haplotype_errors;  // the smallest distance on any supporting haplotype
    std::uint32_t records;          // alignments of locate_reference merged
    std::vector<std::pair<std::uint32_t, std::int32_t>> members; // (haplotype, its smallest distance), ascending haplotype
    bool operator==(jst_ref_locus const &) const noexcept = default;
};

// what a mapper reports per read (journaled_sequence_tree::locate_reads; spm_jst_read in spm_hip.h): where the read's loci
// stand in the loci vector, how many it has on which strand, the primary one -- smallest (haplotype_errors, index) -- and how
// many share the best and the next stratum
struct jst_read
{
    std::uint32_t first_locus, n_loci, n_forward, primary;
    std::int32_t best, best_ref_score;
    std::uint32_t n_best, n_next;
    bool operator==(jst_read const &) const noexcept = default;
};

struct jst_read_loci
{
    std::vector<jst_ref_locus> loci; // of locate_reference_loci_normalized
    std::vector<jst_read> reads;     // one per read, in read order
    bool operator==(jst_read_loci const &) const noexcept = default;
};

// what a mapper reports per pair of mates (journaled_sequence_tree::locate_pairs; spm_jst_pair in spm_hip.h): reads 2p and
// 2p + 1 are the mates of pair p.  The best concordant combination of a forward locus of one mate and a reverse locus of the
// other (FR orientation, min_tlen <= fragment <= max_tlen) by (sum of haplotype_errors, index, index); without one, the
// mates' own primaries
struct jst_pair
{
    std::uint32_t locus1, locus2; // indices into the loci vector; 0xFFFFFFFF: unmapped
    std::int32_t tlen, best;      // SAM TLEN of mate 1 (0: not a proper pair); the error sum (-1: none)
    std::uint32_t n_pairs, n_best, n_next;
    std::uint16_t flag1, flag2;   // SAM FLAG of the two primary lines
    bool operator==(jst_pair const &) const noexcept = default;
};

struct jst_pair_loci
{
    jst_read_loci mapped;         // the loci and the summary of every read
    std::vector<jst_pair> pairs;  // one per pair, in pair order
    bool operator==(jst_pair_loci const &) const noexcept = default;
};

// mate rescue (journaled_sequence_tree::locate_pairs_rescued; spm_jst_rescue in spm_hip.h): one record per job -- a mapped
// mate of a pair without a proper combination, whose partner was searched beside it in the reference with up to k edits --
// ordered by (pair, mate rescued)
struct jst_rescue
{
    std::uint32_t pair, needle, anchor; // the pair, the needle that was aligned, the anchor's index into the loci vector
    alignment aln;                      // against the reference; errors() is the reference distance.  NONE: empty, errors -1
    std::int32_t tlen;                  // SAM TLEN of mate 1; 0 unless RESCUED
    std::uint16_t flag, status;         // SAM FLAG of the rescued mate's line; spm_rescue_status
    bool operator==(jst_rescue const &) const noexcept = default;
};

struct jst_rescued_pair_loci
{
    jst_pair_loci located;              // what locate_pairs returns
    std::vector<jst_rescue> rescues;
    std::vector<std::uint32_t> ops;     // the pool of CIGAR words as the device returned it
    bool operator==(jst_rescued_pair_loci const &) const noexcept = default;
};

// SAM lines (journaled_sequence_tree::map_sam; spm_hip_jst_ref_loci_sam in spm_hip.h): the text, and one record per line
struct jst_sam_line
{
    std::uint64_t offset;               // first byte of the line in the text
    std::uint32_t len, read, source;    // bytes with the \n; the read; locus index, rescue index or 0xFFFFFFFF
    std::uint16_t flag;
    std::uint8_t mapq, kind;            // spm_sam_kind
    bool operator==(jst_sam_line const &) const noexcept = default;
};

struct jst_sam
{
    std::string text;
    std::vector<jst_sam_line> lines;
    bool operator==(jst_sam const &) const noexcept = default;
};

struct jst_sam_options
{
    std::string rname;
    std::string symbols{"ACGT"};
    std::vector<std::string> names;     // one per read (paired: per pair); empty: decimal indices
    bool cigar_m{false}, secondary{false};
    bool default_tables{true};          // false: the two tables below
    std::array<std::uint8_t, 4> mapq_unique{60, 40, 30, 20}, mapq_multi{3, 1, 1, 0};
    // spm_sam_extras: the base qualities, Phred 0 .. 93 as sequenced, one vector per read (empty: none, QUAL "*"); an MD:Z: tag
    // behind NM on every line with a CIGAR, against the tree's reference
    std::vector<std::vector<std::uint8_t>> qualities;
    bool md{false};
};

// what stands between the loci and the lines of map_sam: nothing (single-end), the pairing, the pairing and the mate rescue
struct jst_sam_pairing
{
    bool paired{false};
    std::uint32_t min_tlen{1}, max_tlen{1};
    bool rescue{false};
    std::uint32_t k{0};
};

// one genotyped site of jst_bam::calls: spm_variant_call of spm_hip.h, field for field
struct jst_variant_call
{
    std::uint32_t pos, depth, qual, len;
    std::uint64_t offset;
    std::uint8_t status, gq;
    std::array<std::uint8_t, 2> gt;
    std::uint8_t n_alt;
    std::array<std::uint8_t, 2> alt;
    bool operator==(jst_variant_call const &) const noexcept = default;
};

// A BAM file of a mapping (journaled_sequence_tree::map_bam; spm_hip_jst_ref_loci_bam in spm_hip.h): the complete file (header
// section, record blocks, EOF block), the uncompressed record stream, and one record per BAM record as for map_sam, whose
// offset / len locate it in that stream
struct jst_bam_options
{
    jst_sam_options sam;
    std::uint64_t ref_len{0};           // 1 .. 2^31 - 1
    std::uint32_t block_data{0};        // uncompressed bytes per BGZF block, 0: 65280
    bool deflate{false};                // the blocks compressed (spm_hip_bam_deflate / spm_hip_bgzf_deflate_host), not stored
    bool dynamic{false};                // with deflate only: a block may take a Huffman code of its own (SPM_BGZF_DYNAMIC)
    bool sort{false};                   // the records in coordinate order under SO:coordinate (spm_hip_bam_sort)
    bool index{false};                  // with sort: jst_bam::bai, the .bai of the file (spm_hip_bam_index / spm_hip_bai_build_host)
    bool mark_duplicates{false};        // FLAG 0x400 on duplicate reads and pairs, behind sort and before deflate / index
                                        // (spm_hip_bam_markdup / spm_hip_bam_markdup_host; default min_qual)
    bool pileup{false};                 // with sort: jst_bam::pileup, the per-base counts of the file over the whole reference, behind
                                        // mark_duplicates (spm_hip_bam_pileup / spm_hip_bam_pileup_host; default options)
    bool call_variants{false};          // with pileup: jst_bam::vcf and jst_bam::calls, the sites of that pileup against the tree's
                                        // reference genotyped (spm_hip_pileup_sites, spm_hip_pileup_sites_vcf / the host twins; default
                                        // options, CHROM sam.rname, the sample column `sample`)
    std::string sample{"sample"};
};

struct jst_bam
{
    std::string file, records;
    std::vector<jst_sam_line> lines;
    std::uint64_t header_file_bytes{0}; // where the first record block starts
    std::vector<std::uint64_t> block_offsets; // with jst_bam_options::deflate only: the file offset of every record block, then their end
    std::string bai;                    // with jst_bam_options::index: the bytes of the file's .bai
    std::vector<std::uint32_t> pileup;  // with jst_bam_options::pileup: 8 planes (SPM_PILEUP_A ..) x ref_len counts, plane-major
    std::string vcf;                    // with jst_bam_options::call_variants: the VCF file of the pileup's sites
    std::vector<jst_variant_call> calls; // ... and one call record per site
    bool operator==(jst_bam const &) const noexcept = default;
    // the BGZF virtual file offset of record i
    std::uint64_t virtual_offset(std::size_t i, std::uint32_t block_data = 0) const
    {
        std::uint64_t const D = block_data ? block_data : 65280u, u = lines[i].offset;
        if (!block_offsets.empty())
            return block_offsets[u / D] << 16 | (u % D);
        return (header_file_bytes + (u / D) * (D + 31)) << 16 | (u % D);
    }
};

struct jst_search_stats
{
    std::uint64_t haplotype_symbols{}; // sum of haplotype lengths (what per-haplotype scans would read)
    std::uint64_t context_symbols{};   // symbols actually laid out for the device after deduplication
    std::uint64_t contexts{}, unique_contexts{};
};

class journaled_sequence_tree
{
    std::vector<std::uint8_t> _reference;
    io::vcf_data _variants;

    // the tree resident on the MI355X (reference text + allele table + context index), built on first use
    struct device_tree
    {
        hip::text_ptr reference{};
        spm_jst * tree{};
        bool tried{}, usable{};
        std::size_t window{}, block{};
        ~device_tree()
        {
            if (tree)
                spm_hip_jst_destroy(tree);
        }
    };
    std::shared_ptr<device_tree> _device{std::make_shared<device_tree>()};

public:
    journaled_sequence_tree(std::vector<std::uint8_t> reference, io::vcf_data variants) :
        _reference{std::move(reference)}, _variants{std::move(variants)}
    {}

    std::size_t haplotype_count() const noexcept { return _variants.n_haplotypes; }
    std::vector<std::uint8_t> const & reference() const noexcept { return _reference; }

    // Haplotype h as a journaled sequence over the reference (alleles applied from the right so that reference
    // positions stay valid).  `ref_to_hap`, if given, receives the breakpoints of the monotone coordinate map:
    // reference position p maps to p + shift of the last breakpoint at or before p.
    journaled_sequence<std::uint8_t> haplotype(std::size_t h,
                                               std::vector<std::pair<std::size_t, std::ptrdiff_t>> * ref_to_hap = nullptr) const
    {
        journaled_sequence<std::uint8_t> js{std::span<std::uint8_t const>{_reference}};
        std::vector<io::vcf_allele const *> mine;
        for (auto const & a : _variants.alleles)
            if (a.coverage[h])
                mine.push_back(&a);
        for (auto it = mine.rbegin(); it != mine.rend(); ++it) {
            io::vcf_allele const & a = **it;
            js.replace(js.begin() + static_cast<std::ptrdiff_t>(a.pos),
                       js.begin() + static_cast<std::ptrdiff_t>(std::min(a.pos + a.ref_len, _reference.size())),
                       std::span<std::uint8_t const>{a.alt});
        }
        if (ref_to_hap) {
            ref_to_hap->clear();
            std::ptrdiff_t shift = 0;
            for (io::vcf_allele const * a : mine) {
                std::ptrdiff_t const d = static_cast<std::ptrdiff_t>(a->alt.size()) - static_cast<std::ptrdiff_t>(a->ref_len);
                if (d != 0) {
                    shift += d;
                    ref_to_hap->emplace_back(a->pos + a->ref_len, shift); // positions behind the allele are shifted
                }
            }
        }
        return js;
    }

    // Per-haplotype event table: the alleles it carries, in reference order, with running coordinate shifts.
    // Haplotype symbols are generated by walking the reference: an allele at p emits its alt when the walk reaches p
    // and skips ref_len reference symbols.  Symbol ownership for blocking: an alt symbol belongs to reference
    // position p, a reference symbol to its own position.
    struct hap_events
    {
        std::vector<std::uint32_t> id;       // index into _variants.alleles
        std::vector<std::uint64_t> p, rend;  // allele reference interval [p, rend)
        std::vector<std::uint64_t> hs;       // haplotype position of the first alt symbol
        std::vector<std::int64_t> cs;        // cumulative shift (alt - ref lengths) after this allele
        std::uint64_t length{};
    };

    hap_events events_of(std::size_t h) const
    {
        hap_events E;
        std::int64_t shift = 0;
        std::uint64_t last_end = 0;
        for (std::size_t i = 0; i < _variants.alleles.size(); ++i) {
            io::vcf_allele const & a = _variants.alleles[i];
            if (!a.coverage[h])
                continue;
            std::uint64_t const p = std::max<std::uint64_t>(a.pos, last_end); // overlapping alleles: clip (none in the fixtures)
            std::uint64_t const rend = std::max<std::uint64_t>(p, std::min<std::uint64_t>(a.pos + a.ref_len, _reference.size()));
            E.id.push_back(static_cast<std::uint32_t>(i));
            E.p.push_back(p);
            E.rend.push_back(rend);
            E.hs.push_back(static_cast<std::uint64_t>(static_cast<std::int64_t>(p) + shift));
            shift += static_cast<std::int64_t>(a.alt.size()) - static_cast<std::int64_t>(rend - p);
            E.cs.push_back(shift);
            last_end = rend;
        }
        E.length = static_cast<std::uint64_t>(static_cast<std::int64_t>(_reference.size()) + shift);
        return E;
    }

    // haplotype position of the first symbol owned by reference positions >= r
    static std::uint64_t owned_from(hap_events const & E, std::uint64_t r)
    {
        std::size_t const n = static_cast<std::size_t>(std::lower_bound(E.p.begin(), E.p.end(), r) - E.p.begin());
        if (n == 0)
            return r;
        return static_cast<std::uint64_t>(static_cast<std::int64_t>(std::max(r, E.rend[n - 1])) + E.cs[n - 1]);
    }

    // Append haplotype symbols [lo, hi) to `out`, and the signature of that stretch to `sig` (start point in
    // reference/alt space + the alleles it touches): equal signatures <=> byte-identical stretches.
    void emit_range(hap_events const & E, std::uint64_t lo, std::uint64_t hi, std::vector<std::uint8_t> * out,
                    std::vector<std::uint64_t> & sig) const
    {
        // first allele whose alt ends after lo
        std::size_t i = static_cast<std::size_t>(std::upper_bound(E.hs.begin(), E.hs.end(), lo) - E.hs.begin());
        if (i > 0 && lo < E.hs[i - 1] + _variants.alleles[E.id[i - 1]].alt.size())
            --i; // lo falls inside the alt of allele i-1
        std::uint64_t pos = lo;
        // reference position that haplotype position `pos` reads when it is in a reference run before allele i
        auto ref_of = [&](std::uint64_t hp, std::size_t idx) {
            return static_cast<std::uint64_t>(static_cast<std::int64_t>(hp) - (idx == 0 ? 0 : E.cs[idx - 1]));
        };
        bool first = true;
        while (pos < hi) {
            std::uint64_t const next_hs = i < E.hs.size() ? E.hs[i] : E.length;
            if (pos < next_hs) { // reference run up to the next allele
                std::uint64_t const r0 = ref_of(pos, i);
                std::uint64_t const n = std::min(hi, next_hs) - pos;
                if (first)
                    sig.push_back(r0 << 1); // start inside a reference run
                if (out)
                    out->insert(out->end(), _reference.begin() + static_cast<std::ptrdiff_t>(r0),
                                _reference.begin() + static_cast<std::ptrdiff_t>(r0 + n));
                pos += n;
            } else { // inside / at the alt of allele i
                std::vector<std::uint8_t> const & alt = _variants.alleles[E.id[i]].alt;
                std::uint64_t const off = pos - E.hs[i];
                if (first)
                    sig.push_back((off << 1) | 1); // start inside an alt, at this offset
                sig.push_back(static_cast<std::uint64_t>(E.id[i]) + (1ull << 40));
                if (off < alt.size()) {
                    std::uint64_t const n = std::min<std::uint64_t>(hi - pos, alt.size() - off);
                    if (out)
                        out->insert(out->end(), alt.begin() + static_cast<std::ptrdiff_t>(off),
                                    alt.begin() + static_cast<std::ptrdiff_t>(off + n));
                    pos += n;
                }
                ++i;
                if (pos < hi && i <= E.hs.size()) {
                    // a deletion (or the ref part of a replacement) was skipped: it is part of the signature above
                }
            }
            first = false;
        }
        // alleles that emit nothing but sit at the very end still matter only to later positions: not part of this range
        sig.push_back(hi - lo);
    }

    struct context_index
    {
        struct member
        {
            std::uint32_t haplotype;
            std::uint64_t ctx_lo; // haplotype coordinate of the context's first symbol
        };
        struct context
        {
            std::size_t offset{}, length{}, owned_from{};
            std::vector<member> members;
        };
        std::vector<context> contexts;
        std::vector<std::uint8_t> buffer;
        jst_search_stats stats{};
    };

    // Cut every haplotype into per-block contexts (block = `L` reference positions, plus window-1 symbols of left
    // context) and deduplicate them by signature -- no haplotype is materialised; work is proportional to
    // blocks x haplotypes x (alleles per block) plus the unique context bytes.
    context_index build_contexts(std::size_t window, std::size_t L) const
    {
        context_index X;
        std::size_t const H = haplotype_count();
        std::size_t const n_blocks = (_reference.size() + L - 1) / L;
        struct sig_hash
        {
            std::size_t operator()(std::vector<std::uint64_t> const & v) const noexcept
            {
                std::uint64_t h = 0x9E3779B97F4A7C15ull;
                for (std::uint64_t x : v) {
                    h ^= x + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
                    h *= 0xBF58476D1CE4E5B9ull;
                }
                return static_cast<std::size_t>(h ^ (h >> 31));
            }
        };
        std::unordered_map<std::vector<std::uint64_t>, std::size_t, sig_hash> index;
        std::vector<std::uint64_t> sig;
        for (std::size_t h = 0; h < H; ++h) {
            hap_events const E = events_of(h);
            X.stats.haplotype_symbols += E.length;
            std::uint64_t prev_b = 0;
            for (std::size_t j = 0; j < n_blocks; ++j) {
                std::uint64_t const a = j == 0 ? 0 : prev_b;
                std::uint64_t const b = j + 1 == n_blocks ? E.length : std::max(a, std::min(E.length, owned_from(E, (j + 1) * L)));
                prev_b = b;
                if (b == a)
                    continue;
                std::uint64_t const lo = a >= window - 1 ? a - (window - 1) : 0;
                sig.clear();
                sig.push_back(a - lo); // ownership is part of the identity
                emit_range(E, lo, b, nullptr, sig);
                ++X.stats.contexts;
                auto [it, fresh] = index.try_emplace(sig, X.contexts.size());
                if (fresh) {
                    typename context_index::context c;
                    c.offset = X.buffer.size();
                    c.length = static_cast<std::size_t>(b - lo);
                    c.owned_from = static_cast<std::size_t>(a - lo);
                    std::vector<std::uint64_t> ignore;
                    emit_range(E, lo, b, &X.buffer, ignore);
                    X.contexts.push_back(std::move(c));
                }
                X.contexts[it->second].members.push_back({static_cast<std::uint32_t>(h), lo});
            }
        }
        X.stats.unique_contexts = X.contexts.size();
        X.stats.context_symbols = X.buffer.size();
        return X;
    }

    // Search a compiled needle set over every haplotype.  `window` = max spm::window_size of the set, `needle_len`
    // = per-needle lengths (exact matchers report the begin position, so the last symbol is begin + |P| - 1).
    // The contexts are cut, deduplicated and spelled out on the device (spm_hip_jst_*, include/spm_hip.h); trees the
    // device path does not take (alleles overlapping on a shared haplotype, > 65 535 haplotypes) go through
    // search_host, which builds the same contexts on the host.  Both return the same hits.
    std::vector<jst_hit> search(spm_patterns * needles, std::size_t window, std::vector<std::uint32_t> const & needle_len,
                                bool reports_begin, std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return search_device(needles, window, block, stats);
        return search_host(needles, window, needle_len, reports_begin, block, stats);
    }

    // The same search with a selection of the hits (spm_hip_jst_hits_select): one hit per locus of every haplotype -- the locus
    // is (haplotype, needle) --, with `strata` only the hits within that many errors of the best one of their (haplotype,
    // needle), with `across` of their needle on all haplotypes.  Restricted to one haplotype these are the hits
    // batch_matcher's operator()(haystack, callback, selection) fires on that haplotype spelled out.  The order is search's.
    // Trees the device path does not take go through search_host and select_host; both routes return the same vector.
    std::vector<jst_hit> search(spm_patterns * needles, std::size_t window, std::vector<std::uint32_t> const & needle_len,
                                bool reports_begin, hip::hit_selection const & selection, std::size_t block = 0,
                                jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return search_device(needles, window, selection, block, stats);
        return select_host(search_host(needles, window, needle_len, reports_begin, block, stats), needles, needle_len,
                           reports_begin, selection);
    }

    std::vector<jst_hit> search_device(spm_patterns * needles, std::size_t window, hip::hit_selection const & selection,
                                       std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        spm_ctx * ctx = hip::default_context();
        spm_jst_hits * hh = device_search(needles, window, block, 0, stats);
        spm_select_opts o{};
        o.flags = hip::select_flags(selection, true);
        o.window = selection.window.value_or(SPM_SELECT_WINDOW_K);
        o.strata = selection.strata.value_or(0u);
        spm_jst_hits * sel = nullptr;
        if (spm_hip_jst_hits_select(hh, &o, &sel) != SPM_OK)
            hip::fatal("spm_hip_jst_hits_select", ctx);
        spm_hip_jst_hits_destroy(hh); // (the selection has a buffer of its own)
        spm_jst_hit const * rec = nullptr;
        std::uint64_t n = 0;
        if (spm_hip_jst_hits_view(sel, &rec, &n) != SPM_OK)
            hip::fatal("spm_hip_jst_hits_view", ctx);
        std::vector<jst_hit> out;
        out.reserve(n);
        for (std::uint64_t i = 0; i < n; ++i)
            out.push_back({rec[i].haplotype, rec[i].pos, rec[i].pattern, rec[i].score});
        spm_hip_jst_hits_destroy(sel);
        std::sort(out.begin(), out.end());
        return out;
    }

    // The rule of spm_hip_jst_hits_select written out on the host, for the hits of search_host.
    static std::vector<jst_hit> select_host(std::vector<jst_hit> hits, spm_patterns * needles,
                                            std::vector<std::uint32_t> const & needle_len, bool reports_begin,
                                            hip::hit_selection const & selection)
    {
        if (selection.across && !selection.strata)
            hip::fatal("journaled_sequence_tree::search (hit_selection::across needs strata)", hip::default_context());
        if (selection.strands && !selection.strata)
            hip::fatal("journaled_sequence_tree::search (hit_selection::strands needs strata)", hip::default_context());
        std::uint32_t const shift = selection.strands ? 1u : 0u; // the minimum's unit: the needle, or the read = needle >> 1
        std::sort(hits.begin(), hits.end(), [](jst_hit const & a, jst_hit const & b) {
            return std::tuple{a.haplotype, a.needle, a.position} < std::tuple{b.haplotype, b.needle, b.position};
        });
        auto const same = [&](std::size_t i, std::size_t j) {
            return hits[i].haplotype == hits[j].haplotype && hits[i].needle == hits[j].needle;
        };
        auto const same_unit = [&](std::size_t i, std::size_t j) {
            return hits[i].haplotype == hits[j].haplotype && hits[i].needle >> shift == hits[j].needle >> shift;
        };
        std::vector<std::int64_t> best(selection.across ? needle_len.size() : hits.size(), INT64_MAX); // per unit / group head
        std::vector<std::size_t> slot(hits.size());
        for (std::size_t i = 0; i < hits.size(); ++i) {
            slot[i] = selection.across ? hits[i].needle >> shift : i && same_unit(i, i - 1) ? slot[i - 1] : i;
            best[slot[i]] = std::min<std::int64_t>(best[slot[i]], hits[i].errors);
        }
        std::vector<jst_hit> out;
        for (std::size_t i = 0; i < hits.size(); ++i) {
            std::uint32_t const p = hits[i].needle;
            // the needle's own k: what its window exceeds its length by (exact matchers: 0)
            std::uint64_t const w = !selection.loci     ? 0
                                    : selection.window ? *selection.window
                                    : reports_begin    ? 0
                                                       : spm_hip_patterns_window_size(needles, p) - needle_len[p];
            bool keep = true;
            for (std::size_t j = i; keep && j-- > 0 && same(i, j) && hits[i].position - hits[j].position <= w;)
                keep = hits[j].errors > hits[i].errors; // to the left: a tie is better
            for (std::size_t j = i + 1; keep && j < hits.size() && same(i, j) && hits[j].position - hits[i].position <= w; ++j)
                keep = hits[j].errors >= hits[i].errors;
            if (keep && selection.strata)
                keep = hits[i].errors <= best[slot[i]] + static_cast<std::int64_t>(*selection.strata);
            if (keep)
                out.push_back(hits[i]);
        }
        std::sort(out.begin(), out.end());
        return out;
    }

    // true once the tree is resident on the device (first call uploads it)
    bool device_ready() const
    {
        device_tree & D = *_device;
        if (D.tried)
            return D.usable;
        D.tried = true;
        spm_ctx * ctx = hip::default_context();
        std::size_t const H = haplotype_count(), cw = (H + 63) / 64;
        std::vector<spm_jst_allele> al;
        std::vector<std::uint8_t> pool;
        std::vector<std::uint64_t> cov;
        al.reserve(_variants.alleles.size());
        cov.reserve(_variants.alleles.size() * cw);
        for (io::vcf_allele const & a : _variants.alleles) {
            al.push_back({a.pos, static_cast<std::uint32_t>(a.ref_len), static_cast<std::uint32_t>(a.alt.size()), pool.size()});
            pool.insert(pool.end(), a.alt.begin(), a.alt.end());
            for (std::size_t w = 0; w < cw; ++w) {
                std::uint64_t bits = 0;
                for (std::size_t h = w * 64; h < std::min(H, (w + 1) * 64); ++h)
                    bits |= static_cast<std::uint64_t>(a.coverage[h] != 0) << (h & 63);
                cov.push_back(bits);
            }
        }
        std::uint32_t sigma = 4;
        for (std::uint8_t c : _reference)
            sigma = std::max<std::uint32_t>(sigma, c + 1u);
        for (std::uint8_t c : pool)
            sigma = std::max<std::uint32_t>(sigma, c + 1u);
        spm_text * t = nullptr;
        if (H == 0 || spm_hip_text_upload(ctx, _reference.data(), _reference.size(), sigma, &t) != SPM_OK)
            return false;
        D.reference = hip::text_ptr{t};
        int const rc = spm_hip_jst_create(ctx, t, al.data(), al.size(), pool.data(), pool.size(), cov.data(),
                                          static_cast<std::uint32_t>(H), &D.tree);
        if (rc == SPM_E_HIP)
            hip::fatal("spm_hip_jst_create", ctx);
        D.usable = rc == SPM_OK;
        return D.usable;
    }

    // search + begin and transcript of every hit: what batch_matcher::locate returns on each materialised haplotype, sorted
    // like search's hits.  One alignment per segment hit is computed and shared by the haplotypes of its context
    // (spm_hip_jst_hits_align); trees the device path does not take go through locate_host.  Both return the same vector.
    std::vector<jst_alignment> locate(spm_patterns * needles, std::size_t window, std::vector<std::uint32_t> const & needle_len,
                                      bool reports_begin, std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_device(needles, window, reports_begin, block, stats);
        return locate_host(needles, window, needle_len, reports_begin, block, stats);
    }

    // locate of the SELECTED hits only: begin and transcript of the loci search(..., selection) keeps, in its order.  Device
    // route: search, select, then spm_hip_jst_selection_align, which locates the kept records in the index and aligns their
    // distinct segment hits once.  Trees the device path does not take: locate_host, filtered to the records select_host keeps,
    // matched by (haplotype, needle, position, errors).  Both routes return the same vector.
    std::vector<jst_alignment> locate(spm_patterns * needles, std::size_t window, std::vector<std::uint32_t> const & needle_len,
                                      bool reports_begin, hip::hit_selection const & selection, std::size_t block = 0,
                                      jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_device(needles, window, reports_begin, selection, block, stats);
        return locate_selected_host(needles, window, needle_len, reports_begin, selection, block, stats);
    }

    std::vector<jst_alignment> locate_selected_host(spm_patterns * needles, std::size_t window,
                                                    std::vector<std::uint32_t> const & needle_len, bool reports_begin,
                                                    hip::hit_selection const & selection, std::size_t block = 0,
                                                    jst_search_stats * stats = nullptr) const
    {
        std::vector<jst_alignment> all = locate_host(needles, window, needle_len, reports_begin, block, stats);
        std::vector<jst_hit> hits;
        hits.reserve(all.size());
        auto const as_hit = [reports_begin](jst_alignment const & x) {
            return jst_hit{x.haplotype, reports_begin ? x.aln.begin_position() : x.aln.end_position(), x.needle,
                           static_cast<std::int32_t>(x.aln.errors())};
        };
        for (jst_alignment const & x : all)
            hits.push_back(as_hit(x));
        std::vector<jst_hit> const kept = select_host(std::move(hits), needles, needle_len, reports_begin, selection); // sorted
        std::erase_if(all, [&](jst_alignment const & x) { return !std::binary_search(kept.begin(), kept.end(), as_hit(x)); });
        return all;
    }

    std::vector<jst_alignment> locate_device(spm_patterns * needles, std::size_t window, bool reports_begin,
                                             hip::hit_selection const & selection, std::size_t block = 0,
                                             jst_search_stats * stats = nullptr) const
    {
        return alignments_of(device_alns(needles, window, selection, block, stats).get(), reports_begin);
    }

    std::vector<jst_alignment> locate_device(spm_patterns * needles, std::size_t window, bool reports_begin,
                                             std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        return alignments_of(device_alns(needles, window, block, stats).get(), reports_begin);
    }

    // ---- locate in REFERENCE coordinates: every alignment of locate projected through the alleles its haplotype carries
    // (the contract of spm_hip_jst_alns_project in spm_hip.h), in locate's order.  needle_ranks: the needles' symbols -- an X of
    // the haplotype transcript may be an = against the reference, which only the symbols tell.  Device route: locate_device
    // followed by the projection, once per shared transcript.  Trees the device path does not take: the result of locate_host,
    // projected on the host through the journal (project_host, a route of its own: it looks every haplotype position up in
    // the event table instead of walking a cursor).  Both return the same vector.
    std::vector<jst_ref_alignment> locate_reference(spm_patterns * needles, std::size_t window,
                                                    std::vector<std::vector<std::uint8_t>> const & needle_ranks, bool reports_begin,
                                                    std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_device(needles, window, reports_begin, block, stats);
        return locate_reference_host(needles, window, needle_ranks, reports_begin, block, stats);
    }

    std::vector<jst_ref_alignment> locate_reference(spm_patterns * needles, std::size_t window,
                                                    std::vector<std::vector<std::uint8_t>> const & needle_ranks, bool reports_begin,
                                                    hip::hit_selection const & selection, std::size_t block = 0,
                                                    jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_device(needles, window, reports_begin, selection, block, stats);
        return locate_reference_host(needles, window, needle_ranks, reports_begin, selection, block, stats);
    }

    std::vector<jst_ref_alignment> locate_reference_device(spm_patterns * needles, std::size_t window, bool reports_begin,
                                                           std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        return projections_of(device_alns(needles, window, block, stats).get(), reports_begin);
    }

    std::vector<jst_ref_alignment> locate_reference_device(spm_patterns * needles, std::size_t window, bool reports_begin,
                                                           hip::hit_selection const & selection, std::size_t block = 0,
                                                           jst_search_stats * stats = nullptr) const
    {
        return projections_of(device_alns(needles, window, selection, block, stats).get(), reports_begin);
    }

    std::vector<jst_ref_alignment> locate_reference_host(spm_patterns * needles, std::size_t window,
                                                         std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                         bool reports_begin, std::size_t block = 0,
                                                         jst_search_stats * stats = nullptr) const
    {
        return project_host(locate_host(needles, window, lengths_of(needle_ranks), reports_begin, block, stats), needle_ranks);
    }

    std::vector<jst_ref_alignment> locate_reference_host(spm_patterns * needles, std::size_t window,
                                                         std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                         bool reports_begin, hip::hit_selection const & selection,
                                                         std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        return project_host(locate_selected_host(needles, window, lengths_of(needle_ranks), reports_begin, selection, block, stats),
                            needle_ranks);
    }

    // ---- one record per distinct reference alignment: locate_reference collapsed by the contract of
    // spm_hip_jst_ref_alns_collapse in spm_hip.h -- loci in (needle, begin, end, errors, CIGAR length, CIGAR words) order.
    // Device route: locate on the device, projection, collapse.  Trees the device path does not take, and the second opinion of
    // the tests: locate_reference_host, sorted and folded on the host (collapse_host).  Both return the same vector.
    std::vector<jst_ref_locus> locate_reference_loci(spm_patterns * needles, std::size_t window,
                                                     std::vector<std::vector<std::uint8_t>> const & needle_ranks, bool reports_begin,
                                                     std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_loci_device(needles, window, block, stats);
        return locate_reference_loci_host(needles, window, needle_ranks, reports_begin, block, stats);
    }

    std::vector<jst_ref_locus> locate_reference_loci(spm_patterns * needles, std::size_t window,
                                                     std::vector<std::vector<std::uint8_t>> const & needle_ranks, bool reports_begin,
                                                     hip::hit_selection const & selection, std::size_t block = 0,
                                                     jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_loci_device(needles, window, selection, block, stats);
        return locate_reference_loci_host(needles, window, needle_ranks, reports_begin, selection, block, stats);
    }

    std::vector<jst_ref_locus> locate_reference_loci_device(spm_patterns * needles, std::size_t window, std::size_t block = 0,
                                                            jst_search_stats * stats = nullptr) const
    {
        return loci_of(device_alns(needles, window, block, stats).get());
    }

    std::vector<jst_ref_locus> locate_reference_loci_device(spm_patterns * needles, std::size_t window,
                                                            hip::hit_selection const & selection, std::size_t block = 0,
                                                            jst_search_stats * stats = nullptr) const
    {
        return loci_of(device_alns(needles, window, selection, block, stats).get());
    }

    std::vector<jst_ref_locus> locate_reference_loci_host(spm_patterns * needles, std::size_t window,
                                                          std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                          bool reports_begin, std::size_t block = 0,
                                                          jst_search_stats * stats = nullptr) const
    {
        return collapse_host(locate_reference_host(needles, window, needle_ranks, reports_begin, block, stats));
    }

    std::vector<jst_ref_locus> locate_reference_loci_host(spm_patterns * needles, std::size_t window,
                                                          std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                          bool reports_begin, hip::hit_selection const & selection,
                                                          std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        return collapse_host(locate_reference_host(needles, window, needle_ranks, reports_begin, selection, block, stats));
    }

    // ---- locate_reference and locate_reference_loci with every indel at its leftmost equivalent place (the contract of
    // spm_hip_jst_ref_alns_normalize in spm_hip.h): haplotypes that differ only in WHICH copy of a repeat an indel touches say
    // the same about the reference, and collapse to one locus.  Device route: locate + projection + normalisation (+ collapse).
    // Trees the device path does not take, and the second opinion of the tests: locate_reference_host through normalize_host,
    // the rule in column form, a route of its own.  Both return the same vector.
    std::vector<jst_ref_alignment> locate_reference_normalized(spm_patterns * needles, std::size_t window,
                                                               std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                               bool reports_begin, std::size_t block = 0,
                                                               jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_normalized_device(needles, window, reports_begin, block, stats);
        return locate_reference_normalized_host(needles, window, needle_ranks, reports_begin, block, stats);
    }

    std::vector<jst_ref_alignment> locate_reference_normalized(spm_patterns * needles, std::size_t window,
                                                               std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                               bool reports_begin, hip::hit_selection const & selection,
                                                               std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_normalized_device(needles, window, reports_begin, selection, block, stats);
        return locate_reference_normalized_host(needles, window, needle_ranks, reports_begin, selection, block, stats);
    }

    std::vector<jst_ref_alignment> locate_reference_normalized_device(spm_patterns * needles, std::size_t window,
                                                                      bool reports_begin, std::size_t block = 0,
                                                                      jst_search_stats * stats = nullptr) const
    {
        return projections_of(device_alns(needles, window, block, stats).get(), reports_begin, true);
    }

    std::vector<jst_ref_alignment> locate_reference_normalized_device(spm_patterns * needles, std::size_t window,
                                                                      bool reports_begin, hip::hit_selection const & selection,
                                                                      std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        return projections_of(device_alns(needles, window, selection, block, stats).get(), reports_begin, true);
    }

    std::vector<jst_ref_alignment> locate_reference_normalized_host(spm_patterns * needles, std::size_t window,
                                                                    std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                                    bool reports_begin, std::size_t block = 0,
                                                                    jst_search_stats * stats = nullptr) const
    {
        return normalize_host(locate_reference_host(needles, window, needle_ranks, reports_begin, block, stats), needle_ranks,
                              _reference);
    }

    std::vector<jst_ref_alignment> locate_reference_normalized_host(spm_patterns * needles, std::size_t window,
                                                                    std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                                    bool reports_begin, hip::hit_selection const & selection,
                                                                    std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        return normalize_host(locate_reference_host(needles, window, needle_ranks, reports_begin, selection, block, stats),
                              needle_ranks, _reference);
    }

    std::vector<jst_ref_locus> locate_reference_loci_normalized(spm_patterns * needles, std::size_t window,
                                                                std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                                bool reports_begin, std::size_t block = 0,
                                                                jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_loci_normalized_device(needles, window, block, stats);
        return locate_reference_loci_normalized_host(needles, window, needle_ranks, reports_begin, block, stats);
    }

    std::vector<jst_ref_locus> locate_reference_loci_normalized(spm_patterns * needles, std::size_t window,
                                                                std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                                bool reports_begin, hip::hit_selection const & selection,
                                                                std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reference_loci_normalized_device(needles, window, selection, block, stats);
        return locate_reference_loci_normalized_host(needles, window, needle_ranks, reports_begin, selection, block, stats);
    }

    std::vector<jst_ref_locus> locate_reference_loci_normalized_device(spm_patterns * needles, std::size_t window,
                                                                       std::size_t block = 0,
                                                                       jst_search_stats * stats = nullptr) const
    {
        return loci_of(device_alns(needles, window, block, stats).get(), true);
    }

    std::vector<jst_ref_locus> locate_reference_loci_normalized_device(spm_patterns * needles, std::size_t window,
                                                                       hip::hit_selection const & selection, std::size_t block = 0,
                                                                       jst_search_stats * stats = nullptr) const
    {
        return loci_of(device_alns(needles, window, selection, block, stats).get(), true);
    }

    std::vector<jst_ref_locus> locate_reference_loci_normalized_host(spm_patterns * needles, std::size_t window,
                                                                     std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                                     bool reports_begin, std::size_t block = 0,
                                                                     jst_search_stats * stats = nullptr) const
    {
        return collapse_host(locate_reference_normalized_host(needles, window, needle_ranks, reports_begin, block, stats));
    }

    std::vector<jst_ref_locus> locate_reference_loci_normalized_host(spm_patterns * needles, std::size_t window,
                                                                     std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                                     bool reports_begin, hip::hit_selection const & selection,
                                                                     std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        return collapse_host(locate_reference_normalized_host(needles, window, needle_ranks, reports_begin, selection, block, stats));
    }

    // ---- the normalised loci of a selection and, per read, their summary (the contract of spm_hip_jst_ref_loci_reads in
    // spm_hip.h).  strands: 2 for needles compiled with both_strands (read = needle >> 1), else 1.  Device route: the
    // normalised-loci chain plus spm_hip_jst_ref_loci_reads.  Host route: the host loci and a plain loop.  Both return the same.
    jst_read_loci locate_reads(spm_patterns * needles, std::size_t window, std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                               bool reports_begin, std::uint32_t strands, std::uint32_t n_reads,
                               hip::hit_selection const & selection, std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_reads_device(needles, window, strands, n_reads, selection, block, stats);
        return locate_reads_host(needles, window, needle_ranks, reports_begin, strands, n_reads, selection, block, stats);
    }

    jst_read_loci locate_reads_device(spm_patterns * needles, std::size_t window, std::uint32_t strands, std::uint32_t n_reads,
                                      hip::hit_selection const & selection, std::size_t block = 0,
                                      jst_search_stats * stats = nullptr) const
    {
        jst_read_loci out;
        out.loci = loci_of(device_alns(needles, window, selection, block, stats).get(), true, strands, n_reads, &out.reads);
        return out;
    }

    jst_read_loci locate_reads_host(spm_patterns * needles, std::size_t window,
                                    std::vector<std::vector<std::uint8_t>> const & needle_ranks, bool reports_begin,
                                    std::uint32_t strands, std::uint32_t n_reads, hip::hit_selection const & selection,
                                    std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        jst_read_loci out;
        out.loci = locate_reference_loci_normalized_host(needles, window, needle_ranks, reports_begin, selection, block, stats);
        out.reads = reads_host(out.loci, strands, n_reads);
        return out;
    }

    // the summary as a plain loop over loci in their order (needle first: the loci of a read are contiguous)
    static std::vector<jst_read> reads_host(std::vector<jst_ref_locus> const & loci, std::uint32_t strands, std::uint32_t n_reads)
    {
        if (strands != 1 && strands != 2)
            hip::fatal("journaled_sequence_tree::locate_reads (strands is 1 or 2)", hip::default_context());
        std::vector<jst_read> out;
        std::size_t i = 0;
        for (std::uint32_t r = 0; r < n_reads; ++r) {
            jst_read R{static_cast<std::uint32_t>(i), 0, 0, 0xFFFFFFFFu, -1, -1, 0, 0};
            std::size_t const lo = i;
            for (; i < loci.size() && loci[i].needle / strands == r; ++i) {
                R.n_loci += 1;
                R.n_forward += loci[i].needle % strands == 0;
                if (R.primary == 0xFFFFFFFFu || loci[i].haplotype_errors < R.best) {
                    R.primary = static_cast<std::uint32_t>(i);
                    R.best = loci[i].haplotype_errors;
                    R.best_ref_score = loci[i].aln.errors();
                }
            }
            for (std::size_t j = lo; j < i; ++j) {
                R.n_best += loci[j].haplotype_errors == R.best;
                R.n_next += static_cast<std::int64_t>(loci[j].haplotype_errors) == static_cast<std::int64_t>(R.best) + 1;
            }
            out.push_back(R);
        }
        if (i != loci.size())
            hip::fatal("journaled_sequence_tree::locate_reads (a locus names a needle outside the reads)", hip::default_context());
        return out;
    }

    // ---- the mates of paired-end reads (the contract of spm_hip_jst_ref_loci_pairs in spm_hip.h): needles compiled with
    // both_strands from n_reads reads, n_reads even, reads 2p and 2p + 1 the mates of pair p.  Device route: the chain of
    // locate_reads plus spm_hip_jst_ref_loci_pairs.  Host route: the host loci, the host summary and a plain loop over all
    // combinations.  Both return the same.
    jst_pair_loci locate_pairs(spm_patterns * needles, std::size_t window, std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                               bool reports_begin, std::uint32_t n_reads, std::uint32_t min_tlen, std::uint32_t max_tlen,
                               hip::hit_selection const & selection, std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return locate_pairs_device(needles, window, n_reads, min_tlen, max_tlen, selection, block, stats);
        return locate_pairs_host(needles, window, needle_ranks, reports_begin, n_reads, min_tlen, max_tlen, selection, block, stats);
    }

    jst_pair_loci locate_pairs_device(spm_patterns * needles, std::size_t window, std::uint32_t n_reads, std::uint32_t min_tlen,
                                      std::uint32_t max_tlen, hip::hit_selection const & selection, std::size_t block = 0,
                                      jst_search_stats * stats = nullptr) const
    {
        jst_pair_loci out;
        spm_jst_pair_opts const opts{min_tlen, max_tlen, 0, 0};
        out.mapped.loci = loci_of(device_alns(needles, window, selection, block, stats).get(), true, 2, n_reads, &out.mapped.reads,
                                  &opts, &out.pairs);
        return out;
    }

    // ---- locate_pairs plus mate rescue (the contract of spm_hip_jst_pairs_rescue in spm_hip.h): every pair without a proper
    // combination gets one job per mapped mate, searched in the tree's reference with up to k edits.  Device route only: the
    // search and the alignment are the device's (there is no second traceback on the host).
    jst_rescued_pair_loci locate_pairs_rescued(spm_patterns * needles, std::size_t window, std::uint32_t n_reads,
                                               std::uint32_t min_tlen, std::uint32_t max_tlen, std::uint32_t k,
                                               hip::hit_selection const & selection, std::size_t block = 0,
                                               jst_search_stats * stats = nullptr) const
    {
        if (!device_ready())
            hip::fatal("journaled_sequence_tree::locate_pairs_rescued (tree not representable on the device)", hip::default_context());
        jst_rescued_pair_loci out;
        spm_jst_pair_opts const opts{min_tlen, max_tlen, 0, 0};
        rescue_request const rescue{spm_jst_rescue_opts{min_tlen, max_tlen, k, 0, 0}, _device->reference.get(), needles, &out.rescues,
                                    &out.ops};
        out.located.mapped.loci = loci_of(device_alns(needles, window, selection, block, stats).get(), true, 2, n_reads,
                                          &out.located.mapped.reads, &opts, &out.located.pairs, &rescue);
        return out;
    }

    // ---- the SAM lines of a mapping (the contract of spm_hip_jst_ref_loci_sam in spm_hip.h), behind locate_reads, locate_pairs
    // or locate_pairs_rescued as `pairing` says.  Device route: the same chain plus spm_hip_jst_ref_loci_sam.  Host route: the
    // host structs those calls return and a plain std::string formatter (sam_host).  Both return the same.
    jst_sam map_sam(spm_patterns * needles, std::size_t window, std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                    bool reports_begin, std::uint32_t strands, std::uint32_t n_reads, jst_sam_pairing const & pairing,
                    jst_sam_options const & options, hip::hit_selection const & selection, std::size_t block = 0,
                    jst_search_stats * stats = nullptr) const
    {
        if (device_ready())
            return map_sam_device(needles, window, strands, n_reads, pairing, options, selection, block, stats);
        return map_sam_host(needles, window, needle_ranks, reports_begin, strands, n_reads, pairing, options, selection, block, stats);
    }

    jst_sam map_sam_device(spm_patterns * needles, std::size_t window, std::uint32_t strands, std::uint32_t n_reads,
                           jst_sam_pairing const & pairing, jst_sam_options const & options, hip::hit_selection const & selection,
                           std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (!device_ready())
            hip::fatal("journaled_sequence_tree::map_sam_device (tree not representable on the device)", hip::default_context());
        jst_sam out;
        std::vector<jst_read> reads;
        std::vector<jst_pair> pairs;
        std::vector<jst_rescue> rescues;
        std::vector<std::uint32_t> rescue_ops;
        spm_jst_pair_opts const opts{pairing.min_tlen, pairing.max_tlen, 0, 0};
        rescue_request const rescue{spm_jst_rescue_opts{pairing.min_tlen, pairing.max_tlen, pairing.k, 0, 0}, _device->reference.get(),
                                    needles, &rescues, &rescue_ops};
        sam_request const sam{&options, needles, &out, nullptr, nullptr, _device->reference.get()};
        loci_of(device_alns(needles, window, selection, block, stats).get(), true, pairing.paired ? 2 : strands, n_reads, &reads,
                pairing.paired ? &opts : nullptr, pairing.paired ? &pairs : nullptr,
                pairing.paired && pairing.rescue ? &rescue : nullptr, &sam);
        return out;
    }

    jst_sam map_sam_host(spm_patterns * needles, std::size_t window, std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                         bool reports_begin, std::uint32_t strands, std::uint32_t n_reads, jst_sam_pairing const & pairing,
                         jst_sam_options const & options, hip::hit_selection const & selection, std::size_t block = 0,
                         jst_search_stats * stats = nullptr) const
    {
        if (pairing.paired && pairing.rescue) { // (the rescue search itself has one route: the device's)
            jst_rescued_pair_loci const R = locate_pairs_rescued(needles, window, n_reads, pairing.min_tlen, pairing.max_tlen, pairing.k,
                                                                 selection, block, stats);
            return sam_host(R.located.mapped, &R.located.pairs, &R.rescues, needle_ranks, 2, options, &_reference);
        }
        if (pairing.paired) {
            jst_pair_loci const P = locate_pairs(needles, window, needle_ranks, reports_begin, n_reads, pairing.min_tlen, pairing.max_tlen,
                                                 selection, block, stats);
            return sam_host(P.mapped, &P.pairs, nullptr, needle_ranks, 2, options, &_reference);
        }
        return sam_host(locate_reads(needles, window, needle_ranks, reports_begin, strands, n_reads, selection, block, stats), nullptr,
                        nullptr, needle_ranks, strands, options, &_reference);
    }

    // ---- the same mapping as a BAM file (the contract of spm_hip_jst_ref_loci_bam in spm_hip.h).  Device route: the chain plus
    // that call.  Host route: map_sam_host's lines, each converted to a record from its TEXT FIELDS (bam_of_sam, a plain
    // SAM-to-BAM converter that shares no code with the device's composition), framed by spm_hip_bgzf_frame_host.  Both return
    // the same bytes.
    jst_bam map_bam(spm_patterns * needles, std::size_t window, std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                    bool reports_begin, std::uint32_t strands, std::uint32_t n_reads, jst_sam_pairing const & pairing,
                    jst_bam_options const & options, hip::hit_selection const & selection, std::size_t block = 0,
                    jst_search_stats * stats = nullptr) const
    {
        if (options.index && !options.sort)
            hip::fatal("journaled_sequence_tree::map_bam (index without sort: an index needs a coordinate-sorted file)", hip::default_context());
        if (options.pileup && !options.sort)
            hip::fatal("journaled_sequence_tree::map_bam (pileup without sort: a pileup needs a coordinate-sorted file)", hip::default_context());
        if (options.call_variants && !options.pileup)
            hip::fatal("journaled_sequence_tree::map_bam (call_variants without pileup: the calls are made from a pileup's sites)", hip::default_context());
        if (device_ready())
            return map_bam_device(needles, window, strands, n_reads, pairing, options, selection, block, stats);
        return map_bam_host(needles, window, needle_ranks, reports_begin, strands, n_reads, pairing, options, selection, block, stats);
    }

    jst_bam map_bam_device(spm_patterns * needles, std::size_t window, std::uint32_t strands, std::uint32_t n_reads,
                           jst_sam_pairing const & pairing, jst_bam_options const & options, hip::hit_selection const & selection,
                           std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        if (!device_ready())
            hip::fatal("journaled_sequence_tree::map_bam_device (tree not representable on the device)", hip::default_context());
        if (options.index && !options.sort)
            hip::fatal("journaled_sequence_tree::map_bam (index without sort: an index needs a coordinate-sorted file)", hip::default_context());
        if (options.pileup && !options.sort)
            hip::fatal("journaled_sequence_tree::map_bam (pileup without sort: a pileup needs a coordinate-sorted file)", hip::default_context());
        if (options.call_variants && !options.pileup)
            hip::fatal("journaled_sequence_tree::map_bam (call_variants without pileup: the calls are made from a pileup's sites)", hip::default_context());
        jst_bam out;
        std::vector<jst_read> reads;
        std::vector<jst_pair> pairs;
        std::vector<jst_rescue> rescues;
        std::vector<std::uint32_t> rescue_ops;
        spm_jst_pair_opts const opts{pairing.min_tlen, pairing.max_tlen, 0, 0};
        rescue_request const rescue{spm_jst_rescue_opts{pairing.min_tlen, pairing.max_tlen, pairing.k, 0, 0}, _device->reference.get(),
                                    needles, &rescues, &rescue_ops};
        sam_request const bam{&options.sam, needles, nullptr, &options, &out, _device->reference.get()};
        loci_of(device_alns(needles, window, selection, block, stats).get(), true, pairing.paired ? 2 : strands, n_reads, &reads,
                pairing.paired ? &opts : nullptr, pairing.paired ? &pairs : nullptr,
                pairing.paired && pairing.rescue ? &rescue : nullptr, &bam);
        return out;
    }

    jst_bam map_bam_host(spm_patterns * needles, std::size_t window, std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                         bool reports_begin, std::uint32_t strands, std::uint32_t n_reads, jst_sam_pairing const & pairing,
                         jst_bam_options const & options, hip::hit_selection const & selection, std::size_t block = 0,
                         jst_search_stats * stats = nullptr) const
    {
        return bam_of_sam(map_sam_host(needles, window, needle_ranks, reports_begin, strands, n_reads, pairing, options.sam, selection,
                                       block, stats),
                          options, &_reference);
    }

    // SAM lines to a BAM file, from the text alone and the SAM specification (section 4.2): every field parsed back out of its
    // line.  Tags are written as the contract of spm_hip.h types them: NM XH XR int32, XN X0 X1 uint32, a Z tag (MD) as its
    // string and a NUL.  QUAL "*" is absent (ff), any other is its values.
    // reference: the tree's reference ranks, read with jst_bam_options::call_variants alone.
    static jst_bam bam_of_sam(jst_sam const & sam, jst_bam_options const & o, std::vector<std::uint8_t> const * reference = nullptr)
    {
        spm_ctx const * const ctx = nullptr; // (no device is needed: the host-only calls leave their message without a context)
        auto const put = [](std::string & to, std::uint64_t v, int bytes) {
            for (int i = 0; i < bytes; ++i)
                to.push_back(static_cast<char>((v >> (8 * i)) & 0xFF));
        };
        auto const reg2bin = [](std::int64_t beg, std::int64_t end) -> std::uint32_t {
            --end;
            int const shifts[5] = {14, 17, 20, 23, 26};
            std::uint32_t const firsts[5] = {4681, 585, 73, 9, 1};
            for (int i = 0; i < 5; ++i)
                if ((beg >> shifts[i]) == (end >> shifts[i]))
                    return static_cast<std::uint32_t>(firsts[i] + (beg >> shifts[i]));
            return 0;
        };
        std::string const seq_letters = "=ACMGRSVTWYHKDBN", cigar_ops = "MIDNSHP=X";
        if (o.index && !o.sort)
            hip::fatal("journaled_sequence_tree::map_bam (index without sort: an index needs a coordinate-sorted file)", ctx);
        if (o.pileup && !o.sort)
            hip::fatal("journaled_sequence_tree::map_bam (pileup without sort: a pileup needs a coordinate-sorted file)", ctx);
        if (o.call_variants && !o.pileup)
            hip::fatal("journaled_sequence_tree::map_bam (call_variants without pileup: the calls are made from a pileup's sites)", ctx);
        jst_bam out;
        // the records in read order, and what coordinate order looks at: without a position or not, POS, the reverse strand
        struct converted
        {
            std::string bytes; // block_size and all
            jst_sam_line line;
            bool unplaced;
            std::int64_t pos;
            bool reverse;
        };
        std::vector<converted> recs;
        for (std::size_t i = 0; i < sam.lines.size(); ++i) {
            std::string const line = sam.text.substr(sam.lines[i].offset, sam.lines[i].len - 1); // (without the \n)
            std::vector<std::string> f;
            for (std::size_t at = 0;;) {
                std::size_t const tab = line.find('\t', at);
                f.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
                if (tab == std::string::npos)
                    break;
                at = tab + 1;
            }
            if (f.size() < 11)
                hip::fatal("journaled_sequence_tree::map_bam (a SAM line of fewer than 11 fields)", ctx);
            std::int64_t const pos = std::stoll(f[3]) - 1, pnext = std::stoll(f[7]) - 1;
            std::string cigar;
            std::uint64_t span = 0, n_items = 0;
            if (f[5] != "*")
                for (std::size_t at = 0; at < f[5].size();) {
                    std::size_t used = 0;
                    std::uint64_t const n = std::stoull(f[5].substr(at), &used);
                    std::size_t const op = cigar_ops.find(f[5][at + used]);
                    if (op == std::string::npos)
                        hip::fatal("journaled_sequence_tree::map_bam (an unknown CIGAR operation)", ctx);
                    put(cigar, n << 4 | op, 4);
                    span += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? n : 0;
                    ++n_items;
                    at += used + 1;
                }
            std::string seq;
            std::uint32_t const l_seq = f[9] == "*" ? 0u : static_cast<std::uint32_t>(f[9].size());
            for (std::uint32_t j = 0; j < l_seq; j += 2) {
                auto const code = [&](char c) {
                    std::size_t const at = seq_letters.find(static_cast<char>(std::toupper(static_cast<unsigned char>(c))));
                    return at == std::string::npos ? 15u : static_cast<unsigned>(at);
                };
                seq.push_back(static_cast<char>(code(f[9][j]) << 4 | (j + 1 < l_seq ? code(f[9][j + 1]) : 0u)));
            }
            std::string rec;
            put(rec, f[2] == "*" ? 0xFFFFFFFFu : 0u, 4);
            put(rec, static_cast<std::uint32_t>(pos), 4);
            put(rec, f[0].size() + 1, 1);
            put(rec, std::stoul(f[4]), 1);
            put(rec, pos < 0 ? 4680u : reg2bin(pos, pos + static_cast<std::int64_t>(std::max<std::uint64_t>(span, 1))), 2);
            put(rec, n_items, 2);
            put(rec, std::stoul(f[1]), 2);
            put(rec, l_seq, 4);
            put(rec, f[6] == "*" ? 0xFFFFFFFFu : 0u, 4); // ("=" is the one reference)
            put(rec, static_cast<std::uint32_t>(pnext), 4);
            put(rec, static_cast<std::uint32_t>(std::stoll(f[8])), 4);
            rec += f[0];
            rec.push_back('\0');
            rec += cigar;
            rec += seq;
            if (f[10] == "*") {
                rec.append(l_seq, static_cast<char>(0xFF));
            } else {
                if (f[10].size() != l_seq)
                    hip::fatal("journaled_sequence_tree::map_bam (QUAL and SEQ of different lengths)", ctx);
                for (char const c : f[10])
                    rec.push_back(static_cast<char>(c - 33));
            }
            for (std::size_t t = 11; t < f.size(); ++t) {
                std::string const tag = f[t].substr(0, 2);
                if (f[t].size() >= 5 && f[t][3] == 'Z') {
                    rec += tag + "Z" + f[t].substr(5);
                    rec.push_back('\0');
                    continue;
                }
                bool const is_signed = tag == "NM" || tag == "XH" || tag == "XR";
                rec += tag;
                rec.push_back(is_signed ? 'i' : 'I');
                put(rec, is_signed ? static_cast<std::uint32_t>(std::stoll(f[t].substr(5))) : static_cast<std::uint32_t>(std::stoull(f[t].substr(5))), 4);
            }
            converted c{{}, {0, static_cast<std::uint32_t>(rec.size() + 4), sam.lines[i].read, sam.lines[i].source, sam.lines[i].flag,
                             sam.lines[i].mapq, sam.lines[i].kind},
                        f[2] == "*", pos, (std::stoul(f[1]) & 0x10u) != 0};
            put(c.bytes, rec.size(), 4);
            c.bytes += rec;
            recs.push_back(std::move(c));
        }
        // coordinate order: the records of the reference first, by position, forward before reverse; ties stay in read order
        if (o.sort)
            std::stable_sort(recs.begin(), recs.end(), [](converted const & a, converted const & b) {
                if (a.unplaced != b.unplaced)
                    return b.unplaced;
                if (a.pos != b.pos)
                    return a.pos < b.pos;
                return !a.reverse && b.reverse;
            });
        for (converted & c : recs) {
            c.line.offset = out.records.size();
            out.lines.push_back(c.line);
            out.records += c.bytes;
        }
        if (o.mark_duplicates) { // the serial builder over the records just written: one bit of byte 19 per record, and the line's flag
            std::vector<spm_sam_line> lines;
            for (jst_sam_line const & l : out.lines)
                lines.push_back(spm_sam_line{l.offset, l.len, l.read, l.source, l.flag, l.mapq, l.kind});
            std::vector<std::uint8_t> dup(lines.size(), 0);
            if (spm_hip_bam_markdup_host(out.records.data(), out.records.size(), lines.data(), lines.size(), o.ref_len, nullptr, dup.data()) != SPM_OK)
                hip::fatal("spm_hip_bam_markdup_host", ctx);
            for (std::size_t i = 0; i < dup.size(); ++i) {
                char & high = out.records[out.lines[i].offset + 19];
                high = static_cast<char>((static_cast<std::uint8_t>(high) & ~0x4u) | (dup[i] ? 0x4u : 0u));
                out.lines[i].flag = static_cast<std::uint16_t>((out.lines[i].flag & ~0x400u) | (dup[i] ? 0x400u : 0u));
            }
        }
        if (o.pileup) { // the serial builder over the records just written, marks and all
            std::vector<spm_sam_line> lines;
            for (jst_sam_line const & l : out.lines)
                lines.push_back(spm_sam_line{l.offset, l.len, l.read, l.source, l.flag, l.mapq, l.kind});
            out.pileup.assign(SPM_PILEUP_PLANES * o.ref_len, 0);
            if (spm_hip_bam_pileup_host(out.records.data(), out.records.size(), lines.data(), lines.size(), o.ref_len, nullptr,
                                        out.pileup.data()) != SPM_OK)
                hip::fatal("spm_hip_bam_pileup_host", ctx);
        }
        if (o.call_variants) { // the host twins over the counts just made: sites, then calls and text
            if (reference == nullptr || reference->size() < o.ref_len)
                hip::fatal("journaled_sequence_tree::map_bam (call_variants: no reference of ref_len ranks)", ctx);
            std::uint64_t n_sites = 0, n_text = 0;
            int const sized = spm_hip_pileup_sites_host(out.pileup.data(), 0, o.ref_len, reference->data(), reference->size(), nullptr, nullptr,
                                                        0, &n_sites); // (how many: SPM_E_OVERFLOW unless there is none)
            std::vector<spm_pileup_site> sites(n_sites);
            if ((sized != SPM_OK && sized != SPM_E_OVERFLOW) ||
                spm_hip_pileup_sites_host(out.pileup.data(), 0, o.ref_len, reference->data(), reference->size(), nullptr, sites.data(),
                                          sites.size(), &n_sites) != SPM_OK)
                hip::fatal("spm_hip_pileup_sites_host", ctx);
            std::vector<spm_variant_call> calls(n_sites);
            if (spm_hip_pileup_sites_calls_host(sites.data(), n_sites, nullptr, calls.data()) != SPM_OK)
                hip::fatal("spm_hip_pileup_sites_calls_host", ctx);
            if (spm_hip_pileup_sites_vcf_host(sites.data(), n_sites, o.sam.rname.c_str(), o.sample.c_str(), o.ref_len, nullptr, nullptr, 0,
                                              &n_text) != SPM_E_OVERFLOW)
                hip::fatal("spm_hip_pileup_sites_vcf_host", ctx);
            out.vcf.assign(n_text, '\0');
            if (spm_hip_pileup_sites_vcf_host(sites.data(), n_sites, o.sam.rname.c_str(), o.sample.c_str(), o.ref_len, nullptr, out.vcf.data(),
                                              n_text, &n_text) != SPM_OK)
                hip::fatal("spm_hip_pileup_sites_vcf_host", ctx);
            // the host twin of the calls knows no text: offset and len are those of the lines, in site order behind the header
            std::uint64_t header = 0;
            if (spm_hip_vcf_header(o.sam.rname.c_str(), o.sample.c_str(), o.ref_len, nullptr, 0, &header) != SPM_E_OVERFLOW)
                hip::fatal("spm_hip_vcf_header", ctx);
            std::uint64_t at = header;
            for (spm_variant_call & c : calls) {
                std::uint64_t const end = c.status == SPM_CALL_VARIANT ? out.vcf.find('\n', at) + 1 : at;
                c.offset = at;
                c.len = static_cast<std::uint32_t>(end - at);
                at = end;
            }
            calls_of(calls.data(), calls.size(), out.calls);
        }
        // the header: BAM\1, l_text, the SAM header, one reference; framed on its own, then the records and the EOF block
        std::uint64_t n_text = 0;
        auto const header_text = o.sort ? spm_hip_sam_header_sorted : spm_hip_sam_header;
        if (header_text(o.sam.rname.c_str(), o.ref_len, nullptr, 0, &n_text) != SPM_E_OVERFLOW || o.ref_len == 0 ||
            o.ref_len > 0x7FFFFFFFull)
            hip::fatal("journaled_sequence_tree::map_bam (rname or ref_len)", ctx);
        std::string text(n_text, '\0'), plain = std::string("BAM\1", 4);
        if (header_text(o.sam.rname.c_str(), o.ref_len, text.data(), n_text, &n_text) != SPM_OK)
            hip::fatal("spm_hip_sam_header", ctx);
        put(plain, n_text, 4);
        plain += text;
        put(plain, 1, 4);
        put(plain, o.sam.rname.size() + 1, 4);
        plain += o.sam.rname;
        plain.push_back('\0');
        put(plain, o.ref_len, 4);
        auto const frame = [&](std::string const & data, bool eof) {
            spm_bgzf_opts const z{o.block_data, eof ? SPM_BGZF_EOF : 0u, 0};
            spm_bgzf_deflate_opts const dz{o.block_data, (eof ? SPM_BGZF_EOF : 0u) | (o.dynamic ? SPM_BGZF_DYNAMIC : 0u), 1, 0};
            std::uint64_t need = 0;
            int rc = o.deflate ? spm_hip_bgzf_deflate_bound(data.size(), &dz, &need)
                               : spm_hip_bgzf_frame_host(data.data(), data.size(), &z, nullptr, 0, &need);
            std::string framed(need, '\0');
            if (o.deflate && rc == SPM_OK)
                rc = spm_hip_bgzf_deflate_host(data.data(), data.size(), &dz, framed.data(), need, &need);
            else if (rc == SPM_E_OVERFLOW)
                rc = spm_hip_bgzf_frame_host(data.data(), data.size(), &z, framed.data(), need, &need);
            if (rc != SPM_OK)
                hip::fatal(o.deflate ? "spm_hip_bgzf_deflate_host" : "spm_hip_bgzf_frame_host", ctx);
            framed.resize(need);
            return framed;
        };
        out.file = frame(plain, false);
        out.header_file_bytes = out.file.size();
        out.file += frame(out.records, true);
        if (o.deflate) { // the record blocks, found by their BSIZE fields
            std::uint64_t at = out.header_file_bytes;
            for (std::uint64_t const end = out.file.size() - 28; at < end;
                 at += (static_cast<std::uint8_t>(out.file[at + 16]) | static_cast<std::uint64_t>(static_cast<std::uint8_t>(out.file[at + 17])) << 8) + 1)
                out.block_offsets.push_back(at);
            out.block_offsets.push_back(at);
        }
        if (o.index) { // over the block offsets of the file just written: found above, or the closed form of stored blocks
            std::uint64_t const D = o.block_data ? o.block_data : 65280u, n_blocks = (out.records.size() + D - 1) / D;
            std::vector<std::uint64_t> offsets = out.block_offsets;
            if (!o.deflate) {
                for (std::uint64_t b = 0; b < n_blocks; ++b)
                    offsets.push_back(out.header_file_bytes + b * (D + 31));
                offsets.push_back(out.header_file_bytes + out.records.size() + 31 * n_blocks);
            }
            std::vector<spm_sam_line> lines;
            for (jst_sam_line const & l : out.lines)
                lines.push_back(spm_sam_line{l.offset, l.len, l.read, l.source, l.flag, l.mapq, l.kind});
            std::uint64_t need = 0;
            if (spm_hip_bai_build_host(out.records.data(), out.records.size(), lines.data(), lines.size(), offsets.data(), n_blocks,
                                       o.block_data, nullptr, 0, &need) != SPM_E_OVERFLOW)
                hip::fatal("spm_hip_bai_build_host", ctx);
            out.bai.assign(need, '\0');
            if (spm_hip_bai_build_host(out.records.data(), out.records.size(), lines.data(), lines.size(), offsets.data(), n_blocks,
                                       o.block_data, out.bai.data(), need, &need) != SPM_OK)
                hip::fatal("spm_hip_bai_build_host", ctx);
        }
        return out;
    }

    // The rule of spm_hip.h as a plain formatter over the host structs: which line a read reports, MAPQ from the tables, the
    // mate fields, the secondary lines, every field with std::to_string.  reference: the ranks that jst_sam_options::md reads.
    static jst_sam sam_host(jst_read_loci const & mapped, std::vector<jst_pair> const * pairs, std::vector<jst_rescue> const * rescues,
                            std::vector<std::vector<std::uint8_t>> const & needle_ranks, std::uint32_t strands,
                            jst_sam_options const & o, std::vector<std::uint8_t> const * reference = nullptr)
    {
        constexpr std::uint32_t none = 0xFFFFFFFFu;
        std::vector<jst_ref_locus> const & loci = mapped.loci;
        std::size_t const n_reads = mapped.reads.size();
        bool const paired = pairs != nullptr;
        if ((paired && (strands != 2 || pairs->size() * 2 != n_reads)) || (rescues != nullptr && !paired) ||
            needle_ranks.size() != static_cast<std::size_t>(strands) * n_reads ||
            (!o.names.empty() && o.names.size() != (paired ? pairs->size() : n_reads)))
            hip::fatal("journaled_sequence_tree::map_sam (pairs, rescues, needles or names do not belong to these reads)",
                       hip::default_context());
        if ((!o.qualities.empty() && o.qualities.size() != n_reads) || (o.md && reference == nullptr))
            hip::fatal("journaled_sequence_tree::map_sam (one vector of qualities per read; md needs the reference)", hip::default_context());
        for (std::size_t r = 0; r < o.qualities.size(); ++r)
            if (o.qualities[r].size() != needle_ranks[strands * r].size() ||
                std::any_of(o.qualities[r].begin(), o.qualities[r].end(), [](std::uint8_t q) { return q > 93; }))
                hip::fatal("journaled_sequence_tree::map_sam (a read's qualities: one per symbol, 0 .. 93)", hip::default_context());
        // QUAL of read r: the values + 33, back to front beside a reverse-complemented SEQ
        auto const qual_text = [&](std::size_t r, bool reverse) {
            if (o.qualities.empty())
                return std::string("*");
            std::string text;
            for (std::uint8_t const q : o.qualities[r])
                text += static_cast<char>(q + 33);
            if (reverse)
                std::reverse(text.begin(), text.end());
            return text;
        };
        // MD of a transcript whose first reference position is `begin`: the count of matched positions, broken by every
        // mismatched position (its reference letter) and every deletion (^ and its letters); an insertion breaks nothing
        auto const md_tag = [&](std::vector<std::uint32_t> const & words, std::uint64_t begin) {
            if (!o.md)
                return std::string();
            std::string text = "\tMD:Z:";
            std::uint64_t matched = 0, at = begin;
            auto const letter = [&](std::uint64_t p) {
                if (p >= reference->size())
                    hip::fatal("journaled_sequence_tree::map_sam (an alignment beyond the reference)", hip::default_context());
                return (*reference)[p] < o.symbols.size() ? o.symbols[(*reference)[p]] : 'N';
            };
            for (std::uint32_t const w : words) {
                std::uint32_t const op = w & 15u, n = w >> 4;
                if (op == SPM_CIGAR_EQ)
                    matched += n;
                for (std::uint32_t i = 0; op == SPM_CIGAR_X && i < n; ++i) {
                    text += std::to_string(matched) + letter(at + i);
                    matched = 0;
                }
                if (op == SPM_CIGAR_DEL && n) {
                    text += std::to_string(matched) + "^";
                    for (std::uint32_t i = 0; i < n; ++i)
                        text += letter(at + i);
                    matched = 0;
                }
                at += op == SPM_CIGAR_INS ? 0u : n;
            }
            return text + std::to_string(matched);
        };
        std::array<std::uint8_t, 4> const unique = o.default_tables ? std::array<std::uint8_t, 4>{60, 40, 30, 20} : o.mapq_unique;
        std::array<std::uint8_t, 4> const multi = o.default_tables ? std::array<std::uint8_t, 4>{3, 1, 1, 0} : o.mapq_multi;
        auto const mapq = [&](std::uint32_t n_best, std::uint32_t n_next) -> std::uint8_t {
            if (n_best == 0)
                return 0;
            return n_best == 1 ? unique[std::min<std::uint32_t>(n_next, 3)] : multi[std::min<std::uint32_t>(n_best, 5) - 2];
        };
        auto const cigar_text = [&](std::vector<std::uint32_t> const & words) {
            std::string text;
            std::uint64_t run = 0;
            for (std::size_t w = 0; w < words.size(); ++w) {
                std::uint32_t const op = words[w] & 15u;
                bool const is_m = o.cigar_m && (op == SPM_CIGAR_EQ || op == SPM_CIGAR_X);
                run += words[w] >> 4;
                if (is_m && w + 1 < words.size() && ((words[w + 1] & 15u) == SPM_CIGAR_EQ || (words[w + 1] & 15u) == SPM_CIGAR_X))
                    continue;
                text += std::to_string(run);
                text += is_m ? 'M' : op == SPM_CIGAR_EQ ? '=' : op == SPM_CIGAR_X ? 'X' : op == SPM_CIGAR_INS ? 'I' : 'D';
                run = 0;
            }
            return text;
        };
        auto const seq_text = [&](std::uint32_t needle) {
            std::string text;
            for (std::uint8_t const r : needle_ranks[needle])
                text += r < o.symbols.size() ? o.symbols[r] : 'N';
            return text;
        };
        struct reported
        {
            std::uint8_t kind{SPM_SAM_UNMAPPED}, mapq{0};
            std::uint32_t source{0xFFFFFFFFu}, x0{0}, x1{0};
            std::uint16_t flag{0};
            std::uint64_t pos{0};
            bool reverse{false};
            std::int32_t tlen{0};
        };
        std::vector<reported> rep(n_reads);
        auto const of_locus = [&](std::uint32_t i, std::uint16_t flag, std::uint32_t n_best, std::uint32_t n_next) {
            reported R;
            R.kind = SPM_SAM_LOCUS;
            R.source = i;
            R.flag = flag;
            R.x0 = n_best;
            R.x1 = n_next;
            R.mapq = mapq(n_best, n_next);
            R.pos = loci[i].aln.begin_position() + 1;
            R.reverse = strands == 2 && (loci[i].needle & 1u);
            return R;
        };
        if (!paired) {
            for (std::size_t r = 0; r < n_reads; ++r) {
                jst_read const & M = mapped.reads[r];
                rep[r].flag = 0x4;
                if (M.primary != none)
                    rep[r] = of_locus(M.primary, strands == 2 && (loci[M.primary].needle & 1u) ? 0x10 : 0, M.n_best, M.n_next);
            }
        } else {
            std::vector<std::size_t> used(pairs->size(), static_cast<std::size_t>(-1));
            for (std::size_t j = 0; rescues != nullptr && j < rescues->size(); ++j) {
                jst_rescue const & U = (*rescues)[j];
                if (U.status != SPM_RESCUE_RESCUED)
                    continue;
                std::size_t & u = used[U.pair];
                if (u == static_cast<std::size_t>(-1) || U.aln.errors() < (*rescues)[u].aln.errors())
                    u = j;
            }
            for (std::size_t p = 0; p < pairs->size(); ++p) {
                jst_pair const & P = (*pairs)[p];
                std::uint32_t const locus[2] = {P.locus1, P.locus2};
                std::uint16_t const flag[2] = {P.flag1, P.flag2};
                std::int32_t tlen = P.tlen;
                if (used[p] != static_cast<std::size_t>(-1)) {
                    jst_rescue const & U = (*rescues)[used[p]];
                    std::size_t const y = (U.needle >> 1) & 1u, a = y ^ 1u;
                    jst_read const & A = mapped.reads[2 * p + a];
                    reported & Y = rep[2 * p + y];
                    Y.kind = SPM_SAM_RESCUE;
                    Y.source = static_cast<std::uint32_t>(used[p]);
                    Y.flag = U.flag;
                    Y.pos = U.aln.begin_position() + 1;
                    Y.reverse = (U.flag & 0x10) != 0;
                    Y.x0 = A.n_best;
                    Y.x1 = A.n_next;
                    Y.mapq = mapq(A.n_best, A.n_next);
                    auto const fixed = static_cast<std::uint16_t>(((flag[a] | 0x2) & ~0x28) | (Y.reverse ? 0x20 : 0));
                    rep[2 * p + a] = of_locus(U.anchor, fixed, A.n_best, A.n_next);
                    tlen = U.tlen;
                } else {
                    bool const proper = (P.flag1 & 0x2) != 0;
                    for (std::size_t x = 0; x < 2; ++x) {
                        jst_read const & M = mapped.reads[2 * p + x];
                        rep[2 * p + x].flag = flag[x];
                        if (locus[x] != none)
                            rep[2 * p + x] = of_locus(locus[x], flag[x], proper ? P.n_best : M.n_best, proper ? P.n_next : M.n_next);
                    }
                }
                rep[2 * p].tlen = rep[2 * p].kind == SPM_SAM_UNMAPPED ? 0 : tlen;
                rep[2 * p + 1].tlen = rep[2 * p + 1].kind == SPM_SAM_UNMAPPED ? 0 : -tlen;
            }
        }
        jst_sam out;
        auto const emit = [&](std::size_t r, std::uint8_t kind, std::uint32_t source, std::uint16_t flag, std::uint8_t q,
                              reported const & own, std::int32_t tlen) {
            reported const * other = paired ? &rep[r ^ 1u] : nullptr;
            std::uint64_t const mate_pos = other != nullptr && other->kind != SPM_SAM_UNMAPPED ? other->pos : 0;
            bool const is_mapped = kind != SPM_SAM_UNMAPPED;
            std::uint64_t pos = mate_pos;
            std::string cigar = "*", seq, tags, qual = "*";
            if (kind == SPM_SAM_LOCUS || kind == SPM_SAM_SECONDARY_LINE) {
                jst_ref_locus const & X = loci[source];
                pos = X.aln.begin_position() + 1;
                cigar = cigar_text(X.aln.cigar());
                seq = kind == SPM_SAM_LOCUS ? seq_text(X.needle) : "*";
                if (kind == SPM_SAM_LOCUS)
                    qual = qual_text(r, strands == 2 && (X.needle & 1u));
                tags = "\tNM:i:" + std::to_string(X.aln.errors()) + md_tag(X.aln.cigar(), X.aln.begin_position()) + "\tXH:i:" +
                       std::to_string(X.haplotype_errors) + "\tXN:i:" + std::to_string(X.members.size());
            } else if (kind == SPM_SAM_RESCUE) {
                jst_rescue const & X = (*rescues)[source];
                pos = X.aln.begin_position() + 1;
                cigar = cigar_text(X.aln.cigar());
                seq = seq_text(X.needle);
                qual = qual_text(r, (X.flag & 0x10) != 0);
                tags = "\tNM:i:" + std::to_string(X.aln.errors()) + md_tag(X.aln.cigar(), X.aln.begin_position()) + "\tXR:i:1";
            } else {
                seq = seq_text(static_cast<std::uint32_t>(strands * r));
                qual = qual_text(r, false);
            }
            if (kind == SPM_SAM_LOCUS || kind == SPM_SAM_RESCUE)
                tags += "\tX0:i:" + std::to_string(own.x0) + "\tX1:i:" + std::to_string(own.x1);
            std::size_t const name = paired ? r / 2 : r;
            std::string line = o.names.empty() ? std::to_string(name) : o.names[name];
            line += "\t" + std::to_string(flag) + "\t" + (is_mapped || mate_pos ? o.rname : std::string("*")) + "\t" + std::to_string(pos) +
                    "\t" + std::to_string(q) + "\t" + cigar + "\t";
            if (!paired || (!is_mapped && !mate_pos))
                line += "*\t0";
            else
                line += "=\t" + std::to_string(mate_pos ? mate_pos : pos);
            line += "\t" + std::to_string(tlen) + "\t" + seq + "\t" + qual + tags + "\n";
            out.lines.push_back({out.text.size(), static_cast<std::uint32_t>(line.size()), static_cast<std::uint32_t>(r), source, flag, q,
                                 kind});
            out.text += line;
        };
        for (std::size_t r = 0; r < n_reads; ++r) {
            reported const & own = rep[r];
            emit(r, own.kind, own.source, own.flag, own.mapq, own, own.tlen);
            if (!o.secondary)
                continue;
            jst_read const & M = mapped.reads[r];
            for (std::uint32_t i = M.first_locus; i < M.first_locus + M.n_loci; ++i) {
                if (own.kind == SPM_SAM_LOCUS && i == own.source)
                    continue;
                std::uint32_t flag = 0x100u | (strands == 2 && (loci[i].needle & 1u) ? 0x10u : 0u);
                if (paired) {
                    reported const & other = rep[r ^ 1u];
                    flag |= 0x1u | (r & 1u ? 0x80u : 0x40u) | (other.kind == SPM_SAM_UNMAPPED ? 0x8u : other.reverse ? 0x20u : 0u);
                }
                emit(r, SPM_SAM_SECONDARY_LINE, i, static_cast<std::uint16_t>(flag), 255, own, 0);
            }
        }
        return out;
    }

    jst_pair_loci locate_pairs_host(spm_patterns * needles, std::size_t window,
                                    std::vector<std::vector<std::uint8_t>> const & needle_ranks, bool reports_begin,
                                    std::uint32_t n_reads, std::uint32_t min_tlen, std::uint32_t max_tlen,
                                    hip::hit_selection const & selection, std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        jst_pair_loci out;
        out.mapped = locate_reads_host(needles, window, needle_ranks, reports_begin, 2, n_reads, selection, block, stats);
        out.pairs = pairs_host(out.mapped, min_tlen, max_tlen);
        return out;
    }

    // the rule as a plain loop: per pair, every forward locus of one mate against every reverse locus of the other
    static std::vector<jst_pair> pairs_host(jst_read_loci const & mapped, std::uint32_t min_tlen, std::uint32_t max_tlen)
    {
        if (min_tlen < 1 || min_tlen > max_tlen || max_tlen > 0x7FFFFFFFu || mapped.reads.size() % 2 != 0)
            hip::fatal("journaled_sequence_tree::locate_pairs (1 <= min_tlen <= max_tlen <= 2^31 - 1, an even number of reads)",
                       hip::default_context());
        std::vector<jst_ref_locus> const & loci = mapped.loci;
        auto const clamp = [](std::uint64_t x) { return static_cast<std::uint32_t>(std::min<std::uint64_t>(x, 0xFFFFFFFFu)); };
        std::vector<jst_pair> out;
        for (std::size_t p = 0; p < mapped.reads.size() / 2; ++p) {
            jst_read const mate[2] = {mapped.reads[2 * p], mapped.reads[2 * p + 1]};
            std::int64_t best = -1;
            std::uint32_t best_a = 0, best_b = 0;
            std::uint64_t n_pairs = 0, n_best = 0, n_next = 0;
            for (int pass = 0; pass < 2; ++pass) // the minimum, then the counts against it
                for (int m = 0; m < 2; ++m) {
                    jst_read const &F = mate[m], &V = mate[m ^ 1];
                    for (std::uint32_t a = F.first_locus; a < F.first_locus + F.n_forward; ++a)
                        for (std::uint32_t b = V.first_locus + V.n_forward; b < V.first_locus + V.n_loci; ++b) {
                            alignment const &A = loci[a].aln, &B = loci[b].aln;
                            if (A.begin_position() > B.begin_position() || A.end_position() > B.end_position())
                                continue;
                            std::size_t const t = B.end_position() - A.begin_position();
                            if (t < min_tlen || t > max_tlen)
                                continue;
                            std::int64_t const sum = static_cast<std::int64_t>(loci[a].haplotype_errors) + loci[b].haplotype_errors;
                            if (pass == 0) { // (a ascends, then b: the first of equal sums stays)
                                if (best < 0 || sum < best) {
                                    best = sum;
                                    best_a = a;
                                    best_b = b;
                                }
                            } else {
                                n_pairs += 1;
                                n_best += sum == best;
                                n_next += sum == best + 1;
                            }
                        }
                }
            bool const proper = best >= 0;
            jst_pair P{mate[0].primary, mate[1].primary, 0, -1, 0, 0, 0, 0, 0};
            if (proper) {
                bool const mate1_forward = (loci[best_a].needle & 2u) == 0;
                auto const t = static_cast<std::int32_t>(loci[best_b].aln.end_position() - loci[best_a].aln.begin_position());
                P = {mate1_forward ? best_a : best_b, mate1_forward ? best_b : best_a, mate1_forward ? t : -t,
                     static_cast<std::int32_t>(best), clamp(n_pairs), clamp(n_best), clamp(n_next), 0, 0};
            }
            bool const un1 = P.locus1 == 0xFFFFFFFFu, un2 = P.locus2 == 0xFFFFFFFFu;
            bool const rev1 = !un1 && (loci[P.locus1].needle & 1u), rev2 = !un2 && (loci[P.locus2].needle & 1u);
            auto const flag = [&](bool second, bool self_un, bool other_un, bool self_rev, bool other_rev) {
                return static_cast<std::uint16_t>(0x1u | (proper ? 0x2u : 0u) | (self_un ? 0x4u : 0u) | (other_un ? 0x8u : 0u) |
                                                  (self_rev ? 0x10u : 0u) | (other_rev ? 0x20u : 0u) | (second ? 0x80u : 0x40u));
            };
            P.flag1 = flag(false, un1, un2, rev1, rev2);
            P.flag2 = flag(true, un2, un1, rev2, rev1);
            out.push_back(P);
        }
        return out;
    }

    // The normalisation on the host, in column form: one op per column, a gap run moved one step at a time by the rule of
    // spm_hip.h.  i and r -- the needle symbols and reference positions the columns before the run consume -- are counted
    // anew for every step.
    template <typename reference_t>
    static std::vector<jst_ref_alignment> normalize_host(std::vector<jst_ref_alignment> alns,
                                                         std::vector<std::vector<std::uint8_t>> const & needle_ranks,
                                                         reference_t const & reference)
    {
        for (jst_ref_alignment & a : alns) {
            std::vector<std::uint8_t> const & P = needle_ranks[a.needle];
            std::vector<std::uint32_t> col;
            for (std::uint32_t const w : a.aln.cigar())
                col.insert(col.end(), w >> 4, w & 15u);
            std::size_t const n = col.size();
            for (std::size_t at = 0; at < n;) {
                std::uint32_t const op = col[at];
                if (op != SPM_CIGAR_INS && op != SPM_CIGAR_DEL) {
                    ++at;
                    continue;
                }
                std::size_t c = at, L = 0;
                while (c + L < n && col[c + L] == op)
                    ++L;
                while (c >= 2 && col[c - 1] == SPM_CIGAR_EQ) {
                    std::size_t i = 0, r = a.aln.begin_position();
                    for (std::size_t k = 0; k < c; ++k) {
                        i += col[k] != SPM_CIGAR_DEL;
                        r += col[k] != SPM_CIGAR_INS;
                    }
                    if (op == SPM_CIGAR_INS ? P[i - 1] != P[i + L - 1] : !(reference[r - 1] == reference[r + L - 1]))
                        break;
                    col[c - 1] = op;
                    col[c - 1 + L] = SPM_CIGAR_EQ;
                    for (--c; c >= 1 && col[c - 1] == op; --c) // a run of the same op on the left: one run from now on
                        ++L;
                }
                at = c + L;
            }
            std::vector<std::uint32_t> words;
            for (std::size_t lo = 0; lo < n;) {
                std::size_t hi = lo;
                while (hi < n && col[hi] == col[lo])
                    ++hi;
                words.push_back(static_cast<std::uint32_t>((hi - lo) << 4) | col[lo]);
                lo = hi;
            }
            a.aln = alignment{a.aln.begin_position(), a.aln.end_position(), a.aln.errors(), words.data(), words.size()};
        }
        return alns;
    }

    // The collapse on the host: sort by content, fold equal neighbours, then sort and fold the members of every locus.
    static std::vector<jst_ref_locus> collapse_host(std::vector<jst_ref_alignment> alns)
    {
        auto key = [](jst_ref_alignment const & x) {
            return std::tuple{x.needle, x.aln.begin_position(), x.aln.end_position(), x.aln.errors(), x.aln.cigar().size()};
        };
        auto less = [&](jst_ref_alignment const & a, jst_ref_alignment const & b) {
            return key(a) != key(b) ? key(a) < key(b) : a.aln.cigar() < b.aln.cigar(); // (equal sizes: word by word)
        };
        std::sort(alns.begin(), alns.end(), less);
        std::vector<jst_ref_locus> out;
        for (jst_ref_alignment const & x : alns) {
            if (out.empty() || out.back().needle != x.needle || !(out.back().aln == x.aln))
                out.push_back({x.needle, x.aln, x.haplotype_errors, 0u, {}});
            jst_ref_locus & l = out.back();
            l.haplotype_errors = std::min(l.haplotype_errors, x.haplotype_errors);
            ++l.records;
            l.members.emplace_back(x.haplotype, x.haplotype_errors);
        }
        for (jst_ref_locus & l : out) {
            std::sort(l.members.begin(), l.members.end()); // (haplotype, errors): the smallest distance of a haplotype comes first
            l.members.erase(std::unique(l.members.begin(), l.members.end(),
                                        [](auto const & a, auto const & b) { return a.first == b.first; }),
                            l.members.end());
        }
        return out;
    }

    // The projection on the host.  Haplotype position x is looked up in the event table of its haplotype: inside the alt of
    // allele (p, rend, alt) at offset k it is paired with p + k while k < rend - p and inserted with anchor p + min(rend - p,
    // |alt|) beyond; in a reference run it is paired with x minus the shift of the alleles before it.
    std::vector<jst_ref_alignment> project_host(std::vector<jst_alignment> const & alns,
                                                std::vector<std::vector<std::uint8_t>> const & needle_ranks) const
    {
        std::vector<jst_ref_alignment> out;
        out.reserve(alns.size());
        std::uint32_t cached = ~0u;
        hap_events E;
        for (jst_alignment const & a : alns) {
            if (a.haplotype != cached) { // (locate's order is haplotype-major)
                E = events_of(a.haplotype);
                cached = a.haplotype;
            }
            std::vector<std::uint8_t> const & P = needle_ranks[a.needle];
            std::vector<std::uint32_t> words;
            auto put = [&words](std::uint32_t op, std::uint64_t n) {
                if (n == 0)
                    return;
                if (!words.empty() && (words.back() & 15u) == op)
                    words.back() += static_cast<std::uint32_t>(n << 4);
                else
                    words.push_back(static_cast<std::uint32_t>(n << 4) | op);
            };
            std::uint64_t x = a.aln.begin_position(), first = 0, prev = 0, cost = 0;
            std::size_t i = 0;
            bool have = false;
            auto where = [&](std::uint64_t hx, bool & paired) { // the reference position or the anchor of haplotype symbol hx
                std::size_t const n = static_cast<std::size_t>(std::upper_bound(E.hs.begin(), E.hs.end(), hx) - E.hs.begin());
                paired = true;
                if (n == 0)
                    return hx;
                std::uint64_t const al = _variants.alleles[E.id[n - 1]].alt.size(), rl = E.rend[n - 1] - E.p[n - 1];
                std::uint64_t const k = hx - E.hs[n - 1];
                if (k >= al)
                    return static_cast<std::uint64_t>(static_cast<std::int64_t>(hx) - E.cs[n - 1]);
                paired = k < rl;
                return E.p[n - 1] + (paired ? k : std::min(rl, al));
            };
            bool paired = true;
            std::uint64_t const anchor = x < E.length ? where(x, paired) : _reference.size();
            for (std::uint32_t const w : a.aln.cigar())
                for (std::uint32_t c = 0; c < (w >> 4); ++c) {
                    std::uint32_t const op = w & 15u;
                    if (op == SPM_CIGAR_INS) {
                        put(SPM_CIGAR_INS, 1);
                        ++cost, ++i;
                        continue;
                    }
                    std::uint64_t const rho = where(x++, paired);
                    if (paired) {
                        if (have) {
                            put(SPM_CIGAR_DEL, rho - prev - 1);
                            cost += rho - prev - 1;
                        } else {
                            first = rho;
                        }
                        have = true;
                        prev = rho;
                        if (op == SPM_CIGAR_DEL) {
                            put(SPM_CIGAR_DEL, 1);
                            ++cost;
                        } else {
                            bool const eq = P[i++] == _reference[rho];
                            put(eq ? SPM_CIGAR_EQ : SPM_CIGAR_X, 1);
                            cost += eq ? 0 : 1;
                        }
                    } else if (op != SPM_CIGAR_DEL) {
                        put(SPM_CIGAR_INS, 1);
                        ++cost, ++i;
                    }
                }
            out.push_back({a.haplotype, a.needle,
                           alignment{static_cast<std::size_t>(have ? first : anchor), static_cast<std::size_t>(have ? prev + 1 : anchor),
                                     static_cast<int>(cost), words.data(), words.size()},
                           static_cast<std::int32_t>(a.aln.errors())});
        }
        return out;
    }

    std::vector<jst_hit> search_device(spm_patterns * needles, std::size_t window, std::size_t block = 0,
                                       jst_search_stats * stats = nullptr) const
    {
        spm_ctx * ctx = hip::default_context();
        spm_jst_hits * hh = device_search(needles, window, block, 0, stats);
        spm_jst_hit const * rec = nullptr;
        std::uint64_t n = 0;
        if (spm_hip_jst_hits_view(hh, &rec, &n) != SPM_OK)
            hip::fatal("spm_hip_jst_hits_view", ctx);
        std::vector<jst_hit> out;
        out.reserve(n);
        for (std::uint64_t i = 0; i < n; ++i)
            out.push_back({rec[i].haplotype, rec[i].pos, rec[i].pattern, rec[i].score});
        spm_hip_jst_hits_destroy(hh);
        std::sort(out.begin(), out.end());
        return out;
    }

    // the order of search's hits: (haplotype, position, needle, errors), position = begin (exact) / end (Myers)
    static void sort_alignments(std::vector<jst_alignment> & v, bool reports_begin)
    {
        auto key = [reports_begin](jst_alignment const & x) {
            return std::tuple{x.haplotype, reports_begin ? x.aln.begin_position() : x.aln.end_position(), x.needle,
                              x.aln.errors()};
        };
        std::sort(v.begin(), v.end(), [&](jst_alignment const & a, jst_alignment const & b) { return key(a) < key(b); });
    }

private:
    static std::vector<std::uint32_t> lengths_of(std::vector<std::vector<std::uint8_t>> const & needle_ranks)
    {
        std::vector<std::uint32_t> len;
        for (auto const & nd : needle_ranks)
            len.push_back(static_cast<std::uint32_t>(nd.size()));
        return len;
    }

    // the device alignments of a search: of every hit (the search is made alignable) ...
    hip::jst_alns_ptr device_alns(spm_patterns * needles, std::size_t window, std::size_t block, jst_search_stats * stats) const
    {
        spm_ctx * ctx = hip::default_context();
        spm_jst_hits * hh = device_search(needles, window, block, SPM_SCAN_ALIGNABLE, stats);
        spm_jst_alns * a = nullptr;
        if (spm_hip_jst_hits_align(hh, 0, &a) != SPM_OK)
            hip::fatal("spm_hip_jst_hits_align", ctx);
        spm_hip_jst_hits_destroy(hh);
        return hip::jst_alns_ptr{a};
    }

    // ... and of the hits a selection keeps
    hip::jst_alns_ptr device_alns(spm_patterns * needles, std::size_t window, hip::hit_selection const & selection,
                                  std::size_t block, jst_search_stats * stats) const
    {
        spm_ctx * ctx = hip::default_context();
        spm_jst_hits * hh = device_search(needles, window, block, 0, stats); // (need not be alignable)
        spm_select_opts o{};
        o.flags = hip::select_flags(selection, true);
        o.window = selection.window.value_or(SPM_SELECT_WINDOW_K);
        o.strata = selection.strata.value_or(0u);
        spm_jst_hits * sel = nullptr;
        if (spm_hip_jst_hits_select(hh, &o, &sel) != SPM_OK)
            hip::fatal("spm_hip_jst_hits_select", ctx);
        spm_hip_jst_hits_destroy(hh); // (the selection stays alignable without its source)
        spm_jst_alns * a = nullptr;
        if (spm_hip_jst_selection_align(sel, 0, &a) != SPM_OK)
            hip::fatal("spm_hip_jst_selection_align", ctx);
        spm_hip_jst_hits_destroy(sel);
        return hip::jst_alns_ptr{a};
    }

    static std::vector<jst_alignment> alignments_of(spm_jst_alns * a, bool reports_begin)
    {
        spm_jst_aln const * rec = nullptr;
        std::uint32_t const * ops = nullptr;
        std::uint64_t n = 0, n_ops = 0;
        if (spm_hip_jst_alns_view(a, &rec, &n, &ops, &n_ops) != SPM_OK)
            hip::fatal("spm_hip_jst_alns_view", hip::default_context());
        std::vector<jst_alignment> out;
        out.reserve(n);
        for (std::uint64_t i = 0; i < n; ++i)
            out.push_back({rec[i].haplotype, rec[i].pattern,
                           alignment{static_cast<std::size_t>(rec[i].begin), static_cast<std::size_t>(rec[i].end), rec[i].score,
                                     ops + rec[i].cigar_off, rec[i].cigar_len}});
        sort_alignments(out, reports_begin);
        return out;
    }

    // the projection of device alignments, left-normalised if asked for (record i still belongs to record i of the source);
    // the caller owns the result
    static spm_jst_ref_alns * projected(spm_jst_alns * a, bool normalized)
    {
        spm_ctx * ctx = hip::default_context();
        spm_jst_ref_alns * r = nullptr;
        if (spm_hip_jst_alns_project(a, 0, &r) != SPM_OK)
            hip::fatal("spm_hip_jst_alns_project", ctx);
        if (!normalized)
            return r;
        spm_jst_ref_alns * z = nullptr;
        int const rc = spm_hip_jst_ref_alns_normalize(r, 0, &z);
        spm_hip_jst_ref_alns_destroy(r); // (the result stays valid without its source)
        if (rc != SPM_OK)
            hip::fatal("spm_hip_jst_ref_alns_normalize", ctx);
        return z;
    }

    // the projection of device alignments, in the order alignments_of gives the alignments themselves: record i of the
    // projection's host view belongs to record i of the source's
    static std::vector<jst_ref_alignment> projections_of(spm_jst_alns * a, bool reports_begin, bool normalized = false)
    {
        spm_ctx * ctx = hip::default_context();
        spm_jst_ref_alns * r = projected(a, normalized);
        std::unique_ptr<spm_jst_ref_alns, decltype(&spm_hip_jst_ref_alns_destroy)> owner{r, &spm_hip_jst_ref_alns_destroy};
        spm_jst_aln const * src = nullptr;
        spm_jst_ref_aln const * rec = nullptr;
        std::uint32_t const * ops = nullptr;
        std::uint64_t n = 0, n_src = 0, n_ops = 0;
        if (spm_hip_jst_alns_view(a, &src, &n_src, nullptr, nullptr) != SPM_OK ||
            spm_hip_jst_ref_alns_view(r, &rec, &n, &ops, &n_ops) != SPM_OK || n != n_src)
            hip::fatal("spm_hip_jst_ref_alns_view", ctx);
        std::vector<std::uint64_t> order(n);
        for (std::uint64_t i = 0; i < n; ++i)
            order[i] = i;
        auto key = [&](std::uint64_t i) {
            return std::tuple{src[i].haplotype, reports_begin ? src[i].begin : src[i].end, src[i].pattern, src[i].score};
        };
        std::sort(order.begin(), order.end(), [&](std::uint64_t x, std::uint64_t y) { return key(x) < key(y); });
        std::vector<jst_ref_alignment> out;
        out.reserve(n);
        for (std::uint64_t const i : order)
            out.push_back({rec[i].haplotype, rec[i].pattern,
                           alignment{static_cast<std::size_t>(rec[i].ref_begin), static_cast<std::size_t>(rec[i].ref_end),
                                     rec[i].ref_score, ops + rec[i].cigar_off, rec[i].cigar_len},
                           rec[i].score});
        return out;
    }

    // what loci_of needs for the mate rescue behind the pairs: the bounds and k, the reference, the needles, where the answer goes
    struct rescue_request
    {
        spm_jst_rescue_opts opts;
        spm_text const * reference;
        spm_patterns const * needles;
        std::vector<jst_rescue> * rescues;
        std::vector<std::uint32_t> * ops;
    };

    // what loci_of needs for the SAM lines behind everything else it was asked for: the options, the needles, where the answer goes
    static void calls_of(spm_variant_call const * calls, std::uint64_t n, std::vector<jst_variant_call> & out)
    {
        out.clear();
        for (std::uint64_t i = 0; i < n; ++i) {
            spm_variant_call const & c = calls[i];
            out.push_back(jst_variant_call{c.pos, c.depth, c.qual, c.len, c.offset, c.status, c.gq, {c.gt[0], c.gt[1]}, c.n_alt, {c.alt[0], c.alt[1]}});
        }
    }

    struct sam_request
    {
        jst_sam_options const * options;
        spm_patterns const * needles;
        jst_sam * out;
        jst_bam_options const * bam_options = nullptr; // map_bam: the BAM call instead, into bam_out
        jst_bam * bam_out = nullptr;
        spm_text const * reference = nullptr; // the resident reference ranks: what jst_sam_options::md reads
    };

    // spm_hip_jst_ref_loci_sam over the handles loci_of holds (pr, rs: nullptr where there are none), and its host view
    static void sam_of(spm_jst_ref_loci * l, spm_jst_reads * rd, spm_jst_pairs * pr, spm_jst_rescues * rs, sam_request const & req)
    {
        spm_ctx * ctx = hip::default_context();
        jst_sam_options const & o = *req.options;
        std::string blob;
        std::vector<std::uint64_t> off{0};
        for (std::string const & name : o.names) {
            blob += name;
            off.push_back(blob.size());
        }
        spm_sam_opts opts{};
        opts.rname = o.rname.c_str();
        opts.symbols = o.symbols.c_str();
        if (!o.names.empty()) {
            opts.names = blob.data();
            opts.name_off = off.data();
            opts.n_names = o.names.size();
        }
        std::copy(o.mapq_unique.begin(), o.mapq_unique.end(), opts.mapq_unique);
        std::copy(o.mapq_multi.begin(), o.mapq_multi.end(), opts.mapq_multi);
        opts.mapq_defaults = o.default_tables ? 1 : 0;
        opts.flags = (o.cigar_m ? SPM_SAM_CIGAR_M : 0u) | (o.secondary ? SPM_SAM_SECONDARY : 0u);
        std::vector<std::uint8_t> qual; // the qualities back to back in read order
        for (std::vector<std::uint8_t> const & q : o.qualities)
            qual.insert(qual.end(), q.begin(), q.end());
        spm_sam_extras extras{};
        extras.qual = qual.empty() ? nullptr : qual.data();
        extras.n_qual = qual.size();
        extras.reference = o.md ? req.reference : nullptr;
        extras.flags = o.md ? SPM_SAM_MD : 0u;
        if (req.bam_out != nullptr) {
            spm_bam_opts const bopts{opts, req.bam_options->ref_len, req.bam_options->block_data, 0};
            spm_bam * b = nullptr;
            if (spm_hip_jst_ref_loci_bam_ex(l, rd, pr, rs, req.needles, &bopts, &extras, &b) != SPM_OK)
                hip::fatal("spm_hip_jst_ref_loci_bam_ex", ctx);
            std::unique_ptr<spm_bam, decltype(&spm_hip_bam_destroy)> owner{b, &spm_hip_bam_destroy};
            if (req.bam_options->sort) { // the handle in coordinate order takes the place of the one in read order
                spm_bam * sorted = nullptr;
                if (spm_hip_bam_sort(b, nullptr, &sorted) != SPM_OK)
                    hip::fatal("spm_hip_bam_sort", ctx);
                owner.reset(sorted);
                b = sorted;
            }
            if (req.bam_options->mark_duplicates) { // ... and the marked handle the place of that one
                spm_bam * marked = nullptr;
                if (spm_hip_bam_markdup(b, nullptr, &marked) != SPM_OK)
                    hip::fatal("spm_hip_bam_markdup", ctx);
                owner.reset(marked);
                b = marked;
            }
            req.bam_out->pileup.clear();
            if (req.bam_options->pileup) { // the counts of the handle as it stands: sorted, and marked where that was asked for
                spm_pileup * p = nullptr;
                if (spm_hip_bam_pileup(b, nullptr, &p) != SPM_OK)
                    hip::fatal("spm_hip_bam_pileup", ctx);
                std::unique_ptr<spm_pileup, decltype(&spm_hip_pileup_destroy)> pileup_owner{p, &spm_hip_pileup_destroy};
                std::uint32_t const * counts = nullptr;
                std::uint64_t n = 0;
                if (spm_hip_pileup_view(p, &counts, &n) != SPM_OK)
                    hip::fatal("spm_hip_pileup_view", ctx);
                req.bam_out->pileup.assign(counts, counts + SPM_PILEUP_PLANES * n);
                req.bam_out->vcf.clear();
                req.bam_out->calls.clear();
                if (req.bam_options->call_variants) { // the sites of these counts against the resident reference, genotyped on the device
                    spm_pileup_sites * sites = nullptr;
                    if (spm_hip_pileup_sites(p, req.reference, nullptr, &sites) != SPM_OK)
                        hip::fatal("spm_hip_pileup_sites", ctx);
                    std::unique_ptr<spm_pileup_sites, decltype(&spm_hip_pileup_sites_destroy)> sites_owner{sites, &spm_hip_pileup_sites_destroy};
                    spm_vcf * v = nullptr;
                    if (spm_hip_pileup_sites_vcf(sites, o.rname.c_str(), req.bam_options->sample.c_str(), req.bam_options->ref_len, nullptr, &v) != SPM_OK)
                        hip::fatal("spm_hip_pileup_sites_vcf", ctx);
                    std::unique_ptr<spm_vcf, decltype(&spm_hip_vcf_destroy)> vcf_owner{v, &spm_hip_vcf_destroy};
                    char const * text = nullptr;
                    spm_variant_call const * calls = nullptr;
                    std::uint64_t n_bytes = 0, n_calls = 0;
                    if (spm_hip_vcf_view(v, &text, &n_bytes, &calls, &n_calls) != SPM_OK)
                        hip::fatal("spm_hip_vcf_view", ctx);
                    req.bam_out->vcf.assign(text, n_bytes);
                    calls_of(calls, n_calls, req.bam_out->calls);
                }
            }
            spm_bgzf * index_of = nullptr; // the deflated file, where the index is the deflated file's
            auto const index = [&] {
                req.bam_out->bai.clear();
                if (!req.bam_options->index)
                    return;
                spm_bai * bai = nullptr;
                if (spm_hip_bam_index(b, index_of, &bai) != SPM_OK)
                    hip::fatal("spm_hip_bam_index", ctx);
                std::unique_ptr<spm_bai, decltype(&spm_hip_bai_destroy)> bai_owner{bai, &spm_hip_bai_destroy};
                void const * bytes = nullptr;
                std::uint64_t n = 0;
                if (spm_hip_bai_view(bai, &bytes, &n) != SPM_OK)
                    hip::fatal("spm_hip_bai_view", ctx);
                req.bam_out->bai.assign(static_cast<char const *>(bytes), n);
            };
            void const * file = nullptr;
            void const * records = nullptr;
            spm_sam_line const * lines = nullptr;
            std::uint64_t n_file = 0, n_records = 0, n_lines = 0;
            spm_bam_stats st{};
            if (spm_hip_bam_view(b, &file, &n_file, &records, &n_records, &lines, &n_lines) != SPM_OK || spm_hip_bam_stats(b, &st) != SPM_OK)
                hip::fatal("spm_hip_bam_view", ctx);
            req.bam_out->file.assign(static_cast<char const *>(file), n_file);
            req.bam_out->records.assign(static_cast<char const *>(records), n_records);
            req.bam_out->header_file_bytes = st.header_file_bytes;
            req.bam_out->block_offsets.clear();
            if (req.bam_options->deflate) {
                spm_bgzf_deflate_opts const dz{req.bam_options->block_data, SPM_BGZF_EOF | (req.bam_options->dynamic ? SPM_BGZF_DYNAMIC : 0u), 1, 0};
                spm_bgzf * z = nullptr;
                if (spm_hip_bam_deflate(b, &dz, &z) != SPM_OK)
                    hip::fatal("spm_hip_bam_deflate", ctx);
                std::unique_ptr<spm_bgzf, decltype(&spm_hip_bgzf_destroy)> deflated{z, &spm_hip_bgzf_destroy};
                std::uint64_t const * offsets = nullptr;
                std::uint64_t n_blocks = 0;
                spm_bgzf_deflate_stats ds{};
                if (spm_hip_bgzf_view(z, &file, &n_file) != SPM_OK || spm_hip_bgzf_blocks(z, &offsets, &n_blocks) != SPM_OK ||
                    spm_hip_bgzf_deflate_stats(z, &ds) != SPM_OK)
                    hip::fatal("spm_hip_bgzf_view", ctx);
                req.bam_out->file.assign(static_cast<char const *>(file), n_file);
                req.bam_out->header_file_bytes = ds.n_prefix_bytes;
                req.bam_out->block_offsets.assign(offsets, offsets + n_blocks + 1);
                index_of = z;
                index();
            } else {
                index();
            }
            req.bam_out->lines.clear();
            for (std::uint64_t i = 0; i < n_lines; ++i)
                req.bam_out->lines.push_back({lines[i].offset, lines[i].len, lines[i].read, lines[i].source, lines[i].flag,
                                              lines[i].mapq, lines[i].kind});
            return;
        }
        spm_sam * s = nullptr;
        if (spm_hip_jst_ref_loci_sam_ex(l, rd, pr, rs, req.needles, &opts, &extras, &s) != SPM_OK)
            hip::fatal("spm_hip_jst_ref_loci_sam_ex", ctx);
        std::unique_ptr<spm_sam, decltype(&spm_hip_sam_destroy)> owner{s, &spm_hip_sam_destroy};
        char const * text = nullptr;
        spm_sam_line const * lines = nullptr;
        std::uint64_t n_bytes = 0, n_lines = 0;
        if (spm_hip_sam_view(s, &text, &n_bytes, &lines, &n_lines) != SPM_OK)
            hip::fatal("spm_hip_sam_view", ctx);
        req.out->text.assign(text, text + n_bytes);
        req.out->lines.clear();
        for (std::uint64_t i = 0; i < n_lines; ++i)
            req.out->lines.push_back({lines[i].offset, lines[i].len, lines[i].read, lines[i].source, lines[i].flag, lines[i].mapq,
                                      lines[i].kind});
    }

    // the loci of device alignments: projection, collapse, the host view as it comes (it is in locus order)
    // ... and, where asked for, the summary of n_reads reads over them (spm_hip_jst_ref_loci_reads) and the pairs of their
    // mates (spm_hip_jst_ref_loci_pairs)
    static std::vector<jst_ref_locus> loci_of(spm_jst_alns * a, bool normalized = false, std::uint32_t strands = 1,
                                              std::uint32_t n_reads = 0, std::vector<jst_read> * reads = nullptr,
                                              spm_jst_pair_opts const * pair_opts = nullptr, std::vector<jst_pair> * pairs = nullptr,
                                              rescue_request const * rescue = nullptr, sam_request const * sam = nullptr)
    {
        spm_ctx * ctx = hip::default_context();
        spm_jst_ref_alns * r = projected(a, normalized);
        spm_jst_ref_loci * l = nullptr;
        int const rc = spm_hip_jst_ref_alns_collapse(r, 0, &l);
        spm_hip_jst_ref_alns_destroy(r); // (the loci stay valid without their source)
        if (rc != SPM_OK)
            hip::fatal("spm_hip_jst_ref_alns_collapse", ctx);
        std::unique_ptr<spm_jst_ref_loci, decltype(&spm_hip_jst_ref_loci_destroy)> owner{l, &spm_hip_jst_ref_loci_destroy};
        spm_jst_ref_locus const * rec = nullptr;
        std::uint32_t const *ops = nullptr, *members = nullptr;
        std::int32_t const * scores = nullptr;
        std::uint64_t n = 0, n_ops = 0, n_members = 0;
        if (spm_hip_jst_ref_loci_view(l, &rec, &n, &ops, &n_ops, &members, &scores, &n_members) != SPM_OK)
            hip::fatal("spm_hip_jst_ref_loci_view", ctx);
        std::vector<jst_ref_locus> out;
        out.reserve(n);
        for (std::uint64_t i = 0; i < n; ++i) {
            jst_ref_locus x{rec[i].pattern,
                            alignment{static_cast<std::size_t>(rec[i].ref_begin), static_cast<std::size_t>(rec[i].ref_end),
                                      rec[i].ref_score, ops + rec[i].cigar_off, rec[i].cigar_len},
                            rec[i].score, rec[i].n_records, {}};
            for (std::uint32_t m = 0; m < rec[i].n_haplotypes; ++m)
                x.members.emplace_back(members[rec[i].member_off + m], scores[rec[i].member_off + m]);
            out.push_back(std::move(x));
        }
        if (reads != nullptr) {
            spm_jst_reads * rd = nullptr;
            if (spm_hip_jst_ref_loci_reads(l, strands, n_reads, 0, &rd) != SPM_OK)
                hip::fatal("spm_hip_jst_ref_loci_reads", ctx);
            std::unique_ptr<spm_jst_reads, decltype(&spm_hip_jst_reads_destroy)> rd_owner{rd, &spm_hip_jst_reads_destroy};
            spm_jst_read const * rr = nullptr;
            std::uint64_t nr = 0;
            if (spm_hip_jst_reads_view(rd, &rr, &nr) != SPM_OK)
                hip::fatal("spm_hip_jst_reads_view", ctx);
            reads->clear();
            for (std::uint64_t i = 0; i < nr; ++i)
                reads->push_back({rr[i].first_locus, rr[i].n_loci, rr[i].n_forward, rr[i].primary, rr[i].best,
                                  rr[i].best_ref_score, rr[i].n_best, rr[i].n_next});
            if (pairs != nullptr) {
                spm_jst_pairs * pr = nullptr;
                if (spm_hip_jst_ref_loci_pairs(l, rd, pair_opts, &pr) != SPM_OK)
                    hip::fatal("spm_hip_jst_ref_loci_pairs", ctx);
                std::unique_ptr<spm_jst_pairs, decltype(&spm_hip_jst_pairs_destroy)> pr_owner{pr, &spm_hip_jst_pairs_destroy};
                spm_jst_pair const * pp = nullptr;
                std::uint64_t np = 0;
                if (spm_hip_jst_pairs_view(pr, &pp, &np) != SPM_OK)
                    hip::fatal("spm_hip_jst_pairs_view", ctx);
                pairs->clear();
                for (std::uint64_t i = 0; i < np; ++i)
                    pairs->push_back({pp[i].locus1, pp[i].locus2, pp[i].tlen, pp[i].best, pp[i].n_pairs, pp[i].n_best, pp[i].n_next,
                                      pp[i].flag1, pp[i].flag2});
                if (rescue != nullptr) {
                    spm_jst_rescues * rs = nullptr;
                    if (spm_hip_jst_pairs_rescue(l, rd, pr, rescue->reference, rescue->needles, &rescue->opts, &rs) != SPM_OK)
                        hip::fatal("spm_hip_jst_pairs_rescue", ctx);
                    std::unique_ptr<spm_jst_rescues, decltype(&spm_hip_jst_rescues_destroy)> rs_owner{rs, &spm_hip_jst_rescues_destroy};
                    spm_jst_rescue const * rr2 = nullptr;
                    std::uint32_t const * rops = nullptr;
                    std::uint64_t n_rescues = 0, n_rops = 0;
                    if (spm_hip_jst_rescues_view(rs, &rr2, &n_rescues, &rops, &n_rops) != SPM_OK)
                        hip::fatal("spm_hip_jst_rescues_view", ctx);
                    rescue->rescues->clear();
                    rescue->ops->assign(rops, rops + n_rops);
                    for (std::uint64_t i = 0; i < n_rescues; ++i)
                        rescue->rescues->push_back({rr2[i].pair, rr2[i].pattern, rr2[i].anchor,
                                                    alignment{static_cast<std::size_t>(rr2[i].ref_begin),
                                                              static_cast<std::size_t>(rr2[i].ref_end), rr2[i].score,
                                                              rops + rr2[i].cigar_off, rr2[i].cigar_len},
                                                    rr2[i].tlen, rr2[i].flag, rr2[i].status});
                    if (sam != nullptr)
                        sam_of(l, rd, pr, rs, *sam);
                } else if (sam != nullptr) {
                    sam_of(l, rd, pr, nullptr, *sam);
                }
            } else if (sam != nullptr) {
                sam_of(l, rd, nullptr, nullptr, *sam);
            }
        }
        return out;
    }

    // index (once per (window, block)) and search on the device; the caller owns the result
    spm_jst_hits * device_search(spm_patterns * needles, std::size_t window, std::size_t block, std::uint32_t flags,
                                 jst_search_stats * stats) const
    {
        spm_ctx * ctx = hip::default_context();
        if (!device_ready())
            hip::fatal("journaled_sequence_tree::search_device (tree not representable on the device)", ctx);
        device_tree & D = *_device;
        window = std::max<std::size_t>(window, 1);
        if (D.window != window || D.block != block) { // index once per (window, block)
            if (spm_hip_jst_index(D.tree, static_cast<std::uint32_t>(window), static_cast<std::uint32_t>(block), 0, 0) != SPM_OK)
                hip::fatal("spm_hip_jst_index", ctx);
            D.window = window;
            D.block = block;
        }
        spm_jst_stats st{};
        spm_hip_jst_stats(D.tree, &st);
        spm_scan_opts opts{};
        opts.max_hits = std::max<std::uint64_t>(1u << 22, 8 * st.context_symbols / window);
        opts.flags = flags;
        spm_jst_hits * hh = nullptr;
        for (int attempt = 0;; ++attempt) { // (a hit buffer that proves too small is doubled, not fatal)
            int const rc = spm_hip_jst_search(D.tree, needles, &opts, &hh);
            if (rc == SPM_OK)
                break;
            if (rc != SPM_E_OVERFLOW || attempt >= 12)
                hip::fatal("spm_hip_jst_search", ctx);
            opts.max_hits *= 2;
        }
        if (stats) {
            stats->haplotype_symbols = st.haplotype_symbols;
            stats->context_symbols = st.context_symbols;
            stats->contexts = st.contexts;
            stats->unique_contexts = st.unique_contexts;
        }
        return hh;
    }

public:

    // The same search with the contexts built on the host (any allele table) and uploaded.
    std::vector<jst_hit> search_host(spm_patterns * needles, std::size_t window, std::vector<std::uint32_t> const & needle_len,
                                     bool reports_begin, std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        spm_ctx * ctx = hip::default_context();
        std::size_t const L = block ? block : std::max<std::size_t>(256, 4 * window);
        context_index const X = build_contexts(window, L);
        auto const & contexts = X.contexts;
        auto const & buffer = X.buffer;
        using member = typename context_index::member;
        using context = typename context_index::context;
        if (stats)
            *stats = X.stats;
        std::vector<jst_hit> out;
        if (contexts.empty())
            return out;

        std::vector<std::uint64_t> seg(contexts.size() + 1);
        for (std::size_t i = 0; i < contexts.size(); ++i)
            seg[i] = contexts[i].offset;
        seg.back() = buffer.size();
        spm_text * t = nullptr;
        if (spm_hip_text_upload(ctx, buffer.data(), buffer.size(), 4, &t) != SPM_OK)
            hip::fatal("spm_hip_text_upload", ctx);
        hip::text_ptr text{t};
        spm_scan_opts opts{};
        opts.max_hits = std::max<std::uint64_t>(1u << 20, 4 * buffer.size() / std::max<std::size_t>(window, 1));
        spm_hit const * rec = nullptr;
        std::uint64_t n = 0;
        hip::hits_ptr hits = hip::scan_all_hits(
            ctx, opts,
            [&](spm_scan_opts const & o, spm_hits ** h) {
                return spm_hip_scan_segments(ctx, text.get(), seg.data(), contexts.size(), needles, &o, h);
            },
            rec, n, "spm_hip_scan_segments");
        for (std::uint64_t i = 0; i < n; ++i) {
            // context of this hit
            std::size_t const c =
                static_cast<std::size_t>(std::upper_bound(seg.begin(), seg.end(), rec[i].pos - (reports_begin ? 0 : 1)) -
                                         seg.begin()) - 1;
            context const & cx = contexts[c];
            std::uint64_t const local = rec[i].pos - cx.offset;
            std::uint64_t const last = reports_begin ? local + needle_len[rec[i].pattern] - 1 : local - 1;
            if (last < cx.owned_from)
                continue; // ends in the left context: owned by the previous block's context
            for (member const & m : cx.members)
                out.push_back({m.haplotype, m.ctx_lo + local, rec[i].pattern, rec[i].score});
        }
        std::sort(out.begin(), out.end());
        return out;
    }

    // locate with the contexts built on the host: the segment hits of spm_hip_scan_segments are aligned as they are
    // (spm_hip_hits_align, lo = the start of the hit's context) and begin / transcript are fanned out exactly as the hits.
    std::vector<jst_alignment> locate_host(spm_patterns * needles, std::size_t window, std::vector<std::uint32_t> const & needle_len,
                                           bool reports_begin, std::size_t block = 0, jst_search_stats * stats = nullptr) const
    {
        spm_ctx * ctx = hip::default_context();
        std::size_t const L = block ? block : std::max<std::size_t>(256, 4 * window);
        context_index const X = build_contexts(window, L);
        auto const & contexts = X.contexts;
        auto const & buffer = X.buffer;
        using member = typename context_index::member;
        using context = typename context_index::context;
        if (stats)
            *stats = X.stats;
        std::vector<jst_alignment> out;
        if (contexts.empty())
            return out;
        std::vector<std::uint64_t> seg(contexts.size() + 1);
        for (std::size_t i = 0; i < contexts.size(); ++i)
            seg[i] = contexts[i].offset;
        seg.back() = buffer.size();
        spm_text * t = nullptr;
        if (spm_hip_text_upload(ctx, buffer.data(), buffer.size(), 4, &t) != SPM_OK)
            hip::fatal("spm_hip_text_upload", ctx);
        hip::text_ptr text{t};
        spm_scan_opts opts{};
        opts.max_hits = std::max<std::uint64_t>(1u << 20, 4 * buffer.size() / std::max<std::size_t>(window, 1));
        spm_hit const * rec = nullptr;
        std::uint64_t n = 0;
        hip::hits_ptr hits = hip::scan_all_hits(
            ctx, opts,
            [&](spm_scan_opts const & o, spm_hits ** h) {
                return spm_hip_scan_segments(ctx, text.get(), seg.data(), contexts.size(), needles, &o, h);
            },
            rec, n, "spm_hip_scan_segments");
        spm_aln const * al = nullptr;
        std::uint32_t const * ops = nullptr;
        hip::alns_ptr alns = hip::align_hits(ctx, hits.get(), al, n, ops);
        for (std::uint64_t i = 0; i < n; ++i) {
            std::uint64_t const last = reports_begin ? al[i].begin + needle_len[al[i].pattern] - 1 : al[i].end - 1;
            std::size_t const c = static_cast<std::size_t>(std::upper_bound(seg.begin(), seg.end(), last) - seg.begin()) - 1;
            context const & cx = contexts[c];
            if (last - cx.offset < cx.owned_from)
                continue; // ends in the left context: owned by the previous block's context
            for (member const & m : cx.members) {
                std::size_t const b = static_cast<std::size_t>(m.ctx_lo + (al[i].begin - cx.offset));
                std::size_t const e = static_cast<std::size_t>(m.ctx_lo + (al[i].end - cx.offset));
                out.push_back({m.haplotype, al[i].pattern, alignment{b, e, al[i].score, ops + al[i].cigar_off, al[i].cigar_len}});
            }
        }
        sort_alignments(out, reports_begin);
        return out;
    }
};
} // namespace spm
