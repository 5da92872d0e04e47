// Launch wrapper of the multistep ODE-solver update (solver_kernels.hip).  Same rules as step_kernels.h: enqueue on the given stream,
// never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

// coefficient rows of the multistep sampler: (t, s1, s2, s3, c2, c1, w1, w2) fp32, indexed by the device step counter
constexpr int kSolverStride = 8;

// DPM-Solver++ multistep update in place on xt; x0 <- this step's x0 prediction, hist <- the previous one (hist nullable: no
// second history term is applied or kept then)
hipError_t multistep_update_launch(float* xt, const float* et, float* x0, float* hist, const float* coef, const int* step,
                                   long long n, hipStream_t s);

}  // namespace ddimx
