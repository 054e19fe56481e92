// jst_normalize_core.hpp -- left-normalisation of the gap runs of a projected transcript (contract in spm_hip.h under
// spm_hip_jst_ref_alns_normalize, scheme in DESIGN.md 4.6c).  Host-compilable (g++, clang++) and device code alike: the
// normalise kernel of jst_normalize.hpp instantiates jst_normalize_walk with a slice of its scratch buffer, the CPU tests
// instantiate the same template with a vector (tests/cpp/jst_normalize_core_cases.cpp).
//
// The rule is stated in columns; the walk works on words.  The columns settled so far are a STACK of merged words: a gap run
// that steps left takes = columns off the top, a run that meets a run of its own op takes that run off the top and goes on as
// one, and when no step is allowed the run and the = columns it passed are pushed back.  A word store answers
//   cap()      words it holds
//   get(k)     word k (k below the height of the stack, which is never above cap())
//   put(k, w)  writes word k (k < cap())
#pragma once

#include "hd.hpp"

namespace spm_hip
{

constexpr uint32_t kNormIns = 1, kNormDel = 2, kNormEq = 7, kNormX = 8; // SPM_CIGAR_INS / DEL / EQ / X
constexpr uint64_t kNormMaxRun = 0x0FFFFFFFull;                         // a word holds 28 bits of length

struct jst_norm_result
{
    uint64_t n_words = 0;  // words of the normalised transcript
    uint64_t n_steps = 0;  // steps left, summed over the runs
    uint64_t n_joined = 0; // joins of two runs
    uint64_t n_pinned = 0; // stops that only the first-column rule caused (a run that joins another may stop twice)
};

// the settled columns: merged words, as the projection's sink merges them (a run above 2^28 - 1 columns is full words and
// then the rest)
template <class Store>
struct jst_norm_stack
{
    Store &S;
    uint64_t n = 0;    // words
    uint64_t cols = 0; // columns
    bool ok = true;    // false: the store was full
    SPM_HD explicit jst_norm_stack(Store &s) : S(s) {}
    SPM_HD void push(uint32_t op, uint64_t len)
    {
        cols += len;
        if (len && n) {
            const uint32_t w = S.get(n - 1);
            if ((w & 15u) == op) {
                const uint64_t have = w >> 4;
                const uint64_t t = len < kNormMaxRun - have ? len : kNormMaxRun - have;
                S.put(n - 1, (uint32_t)((have + t) << 4) | op);
                len -= t;
            }
        }
        while (len) {
            if (n >= S.cap()) {
                ok = false;
                return;
            }
            const uint64_t t = len < kNormMaxRun ? len : kNormMaxRun;
            S.put(n++, (uint32_t)(t << 4) | op);
            len -= t;
        }
    }
    // takes the run of `op` off the top: its columns (0: the top is of another op, or there is none)
    SPM_HD uint64_t pop_run(uint32_t op)
    {
        uint64_t len = 0;
        while (n && (S.get(n - 1) & 15u) == op) {
            len += S.get(n - 1) >> 4;
            --n;
        }
        cols -= len;
        return len;
    }
    SPM_HD uint32_t top_op() const { return n ? S.get(n - 1) & 15u : 0u; }
};

// words[0, n_words) of `needle` (m ranks) against ref[ref_begin, ref_end), left-normalised into S.  false: the input is not
// what the contract promises (an unknown op, a word of no columns, words that consume more or less than the needle and the
// range, a range outside the reference, a store too small); R and the store are then not to be used.  Every needle and
// reference index read lies inside what the words before it were checked to consume.
template <class Store>
SPM_HD inline bool jst_normalize_walk(const uint32_t *words, uint32_t n_words, const uint8_t *needle, uint32_t m,
                                      const uint8_t *ref, uint64_t n_ref, uint64_t ref_begin, uint64_t ref_end, Store &S,
                                      jst_norm_result &R)
{
    if (ref_begin > ref_end || ref_end > n_ref)
        return false;
    jst_norm_stack<Store> K(S);
    uint64_t i = 0, r = ref_begin; // needle symbols and reference positions the words read so far consume
    uint32_t w = 0;
    while (w < n_words) {
        const uint32_t op = words[w] & 15u;
        uint64_t len = words[w] >> 4;
        ++w;
        if (len == 0)
            return false;
        if (op == kNormEq || op == kNormX) {
            if (len > m - i || len > ref_end - r)
                return false;
            i += len;
            r += len;
            K.push(op, len);
            continue;
        }
        if (op != kNormIns && op != kNormDel)
            return false;
        const bool ins = op == kNormIns;
        for (; w < n_words && (words[w] & 15u) == op; ++w) { // adjacent words of one op are one run
            if ((words[w] >> 4) == 0)
                return false;
            len += words[w] >> 4;
        }
        if (ins ? len > m - i : len > ref_end - r)
            return false;
        // the run is columns [K.cols, K.cols + L); the columns before it consume needle[0, ci) and ref[ref_begin, cr)
        uint64_t L = len, ci = i, cr = r, passed = 0;
        bool pinned = false;
        while (true) {
            const uint64_t E = K.pop_run(kNormEq); // the = columns on the run's left; K.cols is now the first of them
            const uint64_t lim = K.cols == 0 && E ? E - 1 : E; // column 0 never moves
            uint64_t s = 0;
            while (s < lim && (ins ? needle[ci - 1 - s] == needle[ci + L - 1 - s] : ref[cr - 1 - s] == ref[cr + L - 1 - s]))
                ++s;
            if (s == lim && lim < E)
                pinned = ins ? needle[ci - 1 - s] == needle[ci + L - 1 - s] : ref[cr - 1 - s] == ref[cr + L - 1 - s];
            ci -= s;
            cr -= s;
            passed += s;
            R.n_steps += s;
            K.push(kNormEq, E - s);
            if (E == 0 || s < E || K.top_op() != op)
                break;
            const uint64_t L2 = K.pop_run(op); // the new left neighbour is a run of the same op: one run from now on
            L += L2;
            if (ins)
                ci -= L2;
            else
                cr -= L2;
            ++R.n_joined;
        }
        K.push(op, L);
        K.push(kNormEq, passed);
        R.n_pinned += pinned ? 1u : 0u;
        if (ins)
            i += len;
        else
            r += len;
    }
    R.n_words = K.n;
    return K.ok && i == m && r == ref_end;
}

} // namespace spm_hip
