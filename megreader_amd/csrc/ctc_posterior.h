// The CTC posterior as mr_lexicon_transcribe, mr_ctc_beam_search and mr_ctc_align read it (include/megreader_hip.h): one
// definition of lp[t, c], so that the three give the same bits for the same input.
#pragma once
#include "common.h"

namespace mr {

// The log of a probability as the header defines it: taken in f64 and rounded once, the f32 nearest to log y whichever library
// computes it -- so a caller who passes such logs gets the same bits.  (logf is within 1 ulp, not the nearest.)  0 gives -inf.
__device__ __forceinline__ float ctc_log_prob(float y) { return (float)log((double)y); }

// lp of one value as it was read: the value itself with log_probs, else its log
__device__ __forceinline__ float ctc_lp(float y, bool log_probs) { return log_probs ? y : ctc_log_prob(y); }

}  // namespace mr
