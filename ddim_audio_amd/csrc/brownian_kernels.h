// Launch wrappers of the Brownian-path kernels (brownian_kernels.hip; BrownianStream in ddim_audio_amd/noise.py and solver.py).  Same
// rules as step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "solver_kernels.h"
#include "step_math.h"

namespace ddimx {

constexpr int kBrownianMaxDepth = 16;                                // DDIMXB_MAX_DEPTH
constexpr int kBrownianRecords = kBrownianMaxDepth + 1;              // records of one descent, at most
constexpr int kBrownianStride = 4 + 2 * kBrownianRecords * 4;        // DDIMXB_PLAN_STRIDE: words of one plan row
enum { kBrownianPath = 0, kBrownianIncrement = 1 };                  // DDIMXB_PATH, DDIMXB_INCREMENT

// sde_multistep_update_launch with z the increment of plan row step[0] (kBrownianStride words, include/ddimx_brownian.h) for
// (group of four, first_sample + b) under the key of seed.  The same grid, block and refusals.
hipError_t brownian_multistep_update_launch(float* xt, const float* et, float* x0, float* hist, const float* coef, const int* plan,
                                            const int* step, int B, long long per_sample, unsigned long long seed, unsigned first_sample,
                                            hipStream_t s);
// out [B][per_sample] <- the value of the descent to j of the one row at plan_row (kBrownianPath) or its z (kBrownianIncrement);
// hipErrorInvalidValue for another kind, too.
hipError_t brownian_path_fill_launch(float* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample,
                                     const int* plan_row, int kind, hipStream_t s);

}  // namespace ddimx
