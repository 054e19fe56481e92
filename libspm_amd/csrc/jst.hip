// jst.hip -- journaled-sequence (pan-genome) search, config C5: the tree, its index and the search.  What is done with the
// hits is in the units behind it (map in jst.hpp).
// MI355X only; no CPU scan path exists in this library: if HIP fails the call fails.
#include "jst.hpp"
#include "jst_index.hpp"
#include "jst_search.hpp"

void spm_warm_jst_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::jst_fanout_kernel);
}
