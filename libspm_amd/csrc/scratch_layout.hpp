// scratch_layout.hpp -- how a call carves its arrays out of the context's one scratch buffer (plain C++17, no HIP: the
// drivers and tests/cpp/scratch_layout_cases.cpp both compile it).  Every slice begins on a 256-byte boundary, in the order
// of the takes; a take of zero bytes is legal, costs nothing and shares its offset with the take after it.
#pragma once

#include <cstddef>
#include <cstdint>

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
    // what the buffer has to hold: the (aligned) end of the last slice
    size_t bytes() const { return end_; }

    template <class T> static T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off); }

  private:
    size_t end_ = 0;
};

} // namespace spm_hip
