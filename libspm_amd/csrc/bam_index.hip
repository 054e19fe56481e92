// bam_index.hip -- a BAM handle in coordinate order, the BAI index of a sorted one, and its duplicates marked.
#include "bam_index.hpp"
#include "bam_markdup.hpp"

void spm_warm_bam_index_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::bam_gather_kernel);
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::md_ends_kernel);
}
