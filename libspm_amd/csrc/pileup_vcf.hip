// pileup_vcf.hip -- genotype calls for pileup sites and the VCF text of the variant ones.
#include "pileup_vcf.hpp"

void spm_warm_pileup_vcf_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::vc_write_kernel);
}
