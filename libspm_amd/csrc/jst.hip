// jst.hip -- journaled-sequence (pan-genome) search, config C5.
// MI355X only; no CPU scan path exists in this library: if HIP fails the call fails.
#include "internal.hpp"
#include "synth.hpp"
#include "jst.hpp"
#include "jst_locate.hpp"
#include "transcript_slots.hpp"
#include "jst_project.hpp"
#include "jst_normalize.hpp"
#include "jst_collapse.hpp"
#include "jst_reads.hpp"
#include "jst_pairs.hpp"
#include "jst_rescue.hpp"
