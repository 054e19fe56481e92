// scratch_layout.hpp -- how a call carves its arrays out of the context's one scratch buffer (plain C++17, no HIP: the
// drivers and tests/cpp/scratch_layout_cases.cpp both compile it).  Every slice begins on a 256-byte boundary, in the order
// of the takes; a take of zero bytes is legal, costs nothing and shares its offset with the take after it.
// A driver states every array once -- take(pointer, count): the pointer's own type is the element type -- asks the context
// for bytes(), and bind(base) then points every pointer at its slice.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace spm_hip
{

struct scratch_layout
{
    static constexpr size_t kAlign = 256;

    // the offset of a new slice of `n_bytes`
    size_t take(size_t n_bytes)
    {
        const size_t at = end_;
        end_ += (n_bytes + (kAlign - 1)) & ~(kAlign - 1);
        return at;
    }
    // a new slice of `n` elements for `p` to point at (its offset is returned); p must stay where it is until bind()
    template <class T> size_t take(T *&p, size_t n)
    {
        const size_t at = take(n * sizeof(T));
        bound_.push_back({&p, at, [](void *pp, void *to) { *static_cast<T **>(pp) = static_cast<T *>(to); }});
        return at;
    }
    // what the buffer has to hold: the (aligned) end of the last slice
    size_t bytes() const { return end_; }
    // every pointer of a typed take: base + its offset
    void bind(void *base) const
    {
        for (const bound &b : bound_)
            b.set(b.pp, static_cast<uint8_t *>(base) + b.off);
    }

    template <class T> static T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off); }

  private:
    struct bound
    {
        void *pp; // the T * to set, which set() knows the type of
        size_t off;
        void (*set)(void *pp, void *to);
    };
    size_t end_ = 0;
    std::vector<bound> bound_;
};

} // namespace spm_hip
