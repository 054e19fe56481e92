// jst_sam.hip -- mapped reads written out on the device: SAM lines with MAPQ, and the same lines as BAM records in BGZF blocks.
#include "jst_sam.hpp"
#include "jst_bam.hpp"

void spm_warm_jst_sam_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::jst_sam_measure_kernel);
}
