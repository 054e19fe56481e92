// filter_dense.hip -- the kernels of the seed filter's dense pass (filter_dense.hpp) and which of them streams which pass.
// filter_stream.hip launches them, with the geometry of every streaming pass.
#include "filter_launch.hpp"
#include "filter_dense.hpp"

filter_kernel select_dense_kernel(const filter_index &F, bool km)
{
    if (F.dense) { // the dense pass: anchors = a union of n_pat dimer patterns
        switch (F.n_pat) {
        case 0:
        case 1: return seed_filter_dense_kernel<4, 1>;
        case 2: return seed_filter_dense_kernel<4, 2>;
        case 3: return seed_filter_dense_kernel<4, 3>;
        default: return nullptr;
        }
    }
    if (F.hash_variant == 4) { // presence bits + L2 buckets as level 1 of a sparse dna4 pass
        if (F.stride == 1)
            return km ? seed_filter_dense_kernel<4, 1, 1, true> : seed_filter_dense_kernel<4, 1, 1, false>;
        if (F.stride == 2)
            return km ? seed_filter_dense_kernel<4, 1, 2, true> : seed_filter_dense_kernel<4, 1, 2, false>;
    }
    return nullptr;
}

void warm_dense_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)seed_filter_dense_kernel<4, 1>);
}
