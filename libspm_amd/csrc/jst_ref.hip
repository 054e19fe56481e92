// jst_ref.hip -- pan-genome alignments in reference coordinates: projected, left-normalised, collapsed to loci.  All three
// work once per distinct transcript slot (transcript_slots.hpp) and gather.
#include "jst_project.hpp"
#include "jst_normalize.hpp"
#include "jst_collapse.hpp"

void spm_warm_jst_ref_kernels()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)spm_hip::slot_compact_kernel);
}
