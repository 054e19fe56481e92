// jst_reads.hip -- what the loci say about every read and every read pair: the read summary, the pairing of mates, the
// rescue of a missing mate.
#include "jst_reads.hpp"
#include "jst_pairs.hpp"
#include "jst_rescue.hpp"

void spm_warm_jst_reads_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::jst_reads_min_kernel);
}
