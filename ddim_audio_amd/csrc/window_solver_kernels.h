// Launch wrappers of the windowed multistep solver's kernels (window_solver_kernels.hip; ddim_audio_amd.windowed_solver_steps).
// Same rules as step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "solver_kernels.h"
#include "window_kernels.h"

namespace ddimx {

// beps[n][c][l][:] = the blend of window_blend4 over the windows that cover canvas row l: the canvas-shaped noise prediction the
// fused kernel below forms in registers, written out for the callers that need it whole (the threshold's quantile, the Brownian
// update).  hipErrorInvalidValue unless window_shape_ok, K = ceil(T / H) <= kWindowMaxCover and wt given for K > 1.
hipError_t window_blend_launch(const float* eps, float* beps, const int* jfirst, const int* cnt, const float* wt, int N, int W, int C,
                               int L, int T, int H, int F, hipStream_t s);

// One multistep update (update4_core, step_math.h) of the canvas on row step[0] of the solver's table (kSolverStride floats) from
// the blended noise prediction of the window batch; x0 <- this step's prediction, hist <- the previous one (hist nullable).  A row
// with c1 != 0 adds c1 z: noise[i] when noise (canvas-shaped) is given, else the normal of noise.h for the counter (group of
// four inside the canvas sample, first_sample + n, draw_base + step[0], tag 0) under the key of seed.  hipErrorInvalidValue as
// above and for first_sample + N > 2^32.
hipError_t window_multistep_update_launch(float* x, const float* eps, const float* noise, float* x0, float* hist, const int* jfirst,
                                          const int* cnt, const float* wt, const float* coef, const int* step, int N, int W, int C, int L,
                                          int T, int H, int F, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                                          hipStream_t s);

}  // namespace ddimx
