// bam_index.hip -- a BAM handle in coordinate order, and the BAI index of a sorted one.
#include "bam_index.hpp"

void spm_warm_bam_index_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::bam_gather_kernel);
}
