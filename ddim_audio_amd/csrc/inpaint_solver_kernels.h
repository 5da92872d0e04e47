// Launch wrapper of the multistep inpainting update (inpaint_solver_kernels.hip).  Same rules as step_kernels.h: enqueue on the
// given stream, never allocate or synchronise.  The residual pass of a guided step is inpaint_residual_launch (inpaint_kernels.h)
// with kInpaintSolverStride.
#pragma once
#include "inpaint_kernels.h"

namespace ddimx {

// xt <- the step (include/ddimx_inpaint_solver.h has the operation order), h1 <- the guided prediction, h2 <- the one h1 held;
// flags: 1 = replace, 2 = guided (x0 read, not computed); noise null: z drawn in the kernel from (seed, first_sample, draw_base)
hipError_t inpaint_multistep_update_launch(float* xt, const float* et, const float* noise, float* x0, float* h1, float* h2,
                                           const float* y, const float* m, const float* dx, const float* partials, const float* coef,
                                           const int* step, int B, long long per_sample, int flags, unsigned long long seed,
                                           unsigned first_sample, unsigned draw_base, hipStream_t s);

}  // namespace ddimx
