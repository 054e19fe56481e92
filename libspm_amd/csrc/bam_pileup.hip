// bam_pileup.hip -- the per-base pileup of a coordinate-sorted BAM handle, and the variant sites of a pileup.
#include "bam_pileup.hpp"

void spm_warm_bam_pileup_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::pu_tiles_kernel);
}
