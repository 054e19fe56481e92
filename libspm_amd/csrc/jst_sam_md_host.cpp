// jst_sam_md_host.cpp -- spm_hip_sam_md (contract in spm_hip.h): the MD string of one transcript by the serial sink of
// jst_sam_core.hpp.  PURE HOST C++17 (no HIP, no device): what the tests and the host route of the C++ mirror compare the
// device's strings with.
#include <cstdint>
#include <cstring>

#include "../../include/spm_hip.h"
#include "jst_sam_core.hpp"

extern "C" int spm_hip_sam_md(const uint32_t *words, uint32_t n_words, const uint8_t *ref_ranks, uint64_t ref_len, uint64_t ref_begin,
                              const char *symbols, char *buf, uint64_t cap, uint64_t *len)
{
    using namespace spm_hip;
    if ((!words && n_words) || !ref_ranks || !symbols || !len || (!buf && cap))
        return SPM_E_INVALID;
    uint64_t query = 0, ref = 0;
    jst_sam_cigar_spans(words, n_words, query, ref);
    if (ref_begin > ref_len || ref > ref_len - ref_begin)
        return SPM_E_INVALID;
    const uint32_t sigma = (uint32_t)strlen(symbols);
    jst_sam_measure M;
    M.md(words, n_words, ref_ranks + ref_begin, symbols, sigma);
    *len = M.n;
    if (M.n > cap)
        return SPM_E_OVERFLOW;
    jst_sam_serial T{buf, cap, 0};
    T.md(words, n_words, ref_ranks + ref_begin, symbols, sigma);
    return SPM_OK;
}
