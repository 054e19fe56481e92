"""libspm_amd -- MI355X-native online pattern matching behind libspm's matcher API.

Only what the hot path needs lives here: csrc/ (HIP kernels + the C ABI of include/spm_hip.h), the ctypes binding
(capi), a thin object layer (engine) and the multi-GPU hit gather (dist).  The C++ mirror of the reference's
header-only API is in include/libspm/.
"""
from . import capi  # noqa: F401
from .capi import (ALGO_HORSPOOL, ALGO_MYERS, ALGO_MYERS_PREFIX, ALGO_SHIFTOR, ENGINE_AUTO, ENGINE_BRUTE,  # noqa: F401
                   ENGINE_FILTER, SCAN_ALIGNABLE, SCAN_DEFER, SCAN_IGNORE_PACKED, ALIGN_BEGIN_ONLY, SELECT_ACROSS, SELECT_BEST, SELECT_LOCI, SELECT_STRANDS, SELECT_WINDOW_K,
                   SpmError)
from .engine import (ALLELE_DTYPE, ALN_DTYPE, HIT_DTYPE, Alignments, bai_build_host, Bam, bam_header, bam_markdup_host, bam_markdup_opts, bam_pileup_host, PILEUP_PLANES, PILEUP_SITE_DTYPE, pileup_opts, pileup_site_opts, pileup_sites_host, pileup_sites_calls_host, pileup_sites_vcf_host, VARIANT_CALL_DTYPE, vcf_header, vcf_opts, Bgzf, bgzf_deflate_host, bgzf_deflate_opts, bgzf_frame_host, bgzf_opts, JST_ALN_DTYPE, JST_HIT_DTYPE, JST_REF_ALN_DTYPE, JST_REF_LOCUS_DTYPE, JST_PAIR_DTYPE, JST_READ_DTYPE, JST_RESCUE_DTYPE, SAM_LINE_DTYPE, Context, Hits, Jst, JstAlignments, JstHits, JstPairs, JstReads, JstRescues, JstRefAlignments, JstRefLoci, PatternSet, Sam, sam_extras, sam_header, sam_mapq, sam_md, sam_opts, Text, scan, scan_segments, select_jst_records, select_records,
                     synth_variants,  # noqa: F401
                     synth_pattern, synth_repeat_pattern, synth_repeat_text)
