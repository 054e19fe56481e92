// jst_align.hip -- begins and alignments of pan-genome hits in haplotype coordinates: of a search's own hits and of the
// records a selection kept.  Both find the distinct segment hits, align them once (align.hip) and hand every haplotype
// its record.
#include "jst_hits_align.hpp"
#include "jst_locate.hpp"

void spm_warm_jst_align_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::jst_aln_fanout_kernel);
}
