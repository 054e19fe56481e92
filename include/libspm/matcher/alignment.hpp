// libspm/matcher/alignment.hpp -- where a hit begins and how it aligns: the `locate` side of the matchers.
//
// The reference's finder knows the begin of a Myers hit once seqan2's findBegin has run; the finder handed out by
// operator() here reports end - |P| instead (right only for hits without indels).  locate(haystack, callback) scans, runs
// spm_hip_hits_align on the hits, and hands the callback a finder whose begin_position() is the true begin (the largest
// begin at the hit's distance) together with an spm::alignment: begin, end, errors and the CIGAR transcript (needle =
// query, haystack = reference; ops = SPM_CIGAR_*).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include <libspm/hip/context.hpp>

namespace spm
{
class alignment
{
    std::size_t _begin{}, _end{};
    int _errors{};
    std::vector<std::uint32_t> _cigar{};

public:
    alignment() = default;
    alignment(std::size_t b, std::size_t e, int errors, std::uint32_t const * ops, std::size_t n_ops) :
        _begin{b}, _end{e}, _errors{errors}, _cigar(ops, ops + n_ops)
    {}
    std::size_t begin_position() const noexcept { return _begin; }
    std::size_t end_position() const noexcept { return _end; }
    int errors() const noexcept { return _errors; }
    bool operator==(alignment const &) const noexcept = default;
    // BAM-style words len << 4 | op
    std::vector<std::uint32_t> const & cigar() const noexcept { return _cigar; }
    // the same as a SAM string, e.g. "41=1X12=1I45="
    std::string cigar_string() const
    {
        std::string s;
        for (std::uint32_t const w : _cigar) {
            s += std::to_string(w >> 4);
            switch (w & 15u) {
            case SPM_CIGAR_INS: s += 'I'; break;
            case SPM_CIGAR_DEL: s += 'D'; break;
            case SPM_CIGAR_EQ: s += '='; break;
            default: s += 'X'; break;
            }
        }
        return s;
    }
};

namespace hip
{
struct alns_deleter
{
    void operator()(spm_alns * a) const noexcept { spm_hip_alns_destroy(a); }
};
using alns_ptr = std::unique_ptr<spm_alns, alns_deleter>;
struct jst_alns_deleter
{
    void operator()(spm_jst_alns * a) const noexcept { spm_hip_jst_alns_destroy(a); }
};
using jst_alns_ptr = std::unique_ptr<spm_jst_alns, jst_alns_deleter>;

// the alignments of a completed scan, host order (= the order of spm_hip_hits_view); failures are fatal like every other
// call of the mirror
inline alns_ptr align_hits(spm_ctx * ctx, spm_hits * hits, spm_aln const *& rec, std::uint64_t & n, std::uint32_t const *& ops) noexcept
{
    spm_alns * a = nullptr;
    if (spm_hip_hits_align(hits, 0, &a) != SPM_OK)
        fatal("spm_hip_hits_align", ctx);
    alns_ptr out{a};
    std::uint64_t n_ops = 0;
    if (spm_hip_alns_view(a, &rec, &n, &ops, &n_ops) != SPM_OK)
        fatal("spm_hip_alns_view", ctx);
    return out;
}
} // namespace hip
} // namespace spm
