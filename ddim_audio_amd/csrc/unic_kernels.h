// Launch wrapper of the multistep update with the folded UniC corrector (unic_kernels.hip; ddim_audio_amd/solver.py with
// corrector=True).  Same rules as step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

// coefficient rows of the corrector's table: (t, s1, s2, s3, c2, c1, w1', w2', w3) fp32, indexed by the device step counter
constexpr int kUnicStride = 9;

// DPM-Solver++ multistep update with a third history term, in place on xt; x0 <- this step's x0 prediction, hist <- the previous
// one, hist2 <- the one before (both nullable: a term whose buffer is missing is neither applied nor kept; hist2 needs hist).
// hipErrorInvalidValue for n not a positive multiple of 4 or hist2 without hist.
hipError_t unic_multistep_update_launch(float* xt, const float* et, float* x0, float* hist, float* hist2, const float* coef,
                                        const int* step, long long n, hipStream_t s);

}  // namespace ddimx
