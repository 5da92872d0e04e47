// DPM-Solver++ multistep sampler (ddim_audio_amd/solver.py; Lu et al. 2022, data-prediction form): the element-wise arithmetic
// of one step, orders 1-3.
//
// The update is update4 (step_math.h) on row step[0] of the solver's table (kSolverStride floats: t, s1, s2, s3, c2, c1 = 0, w1, w2
// -- schedule.dpm_coefficients), so one captured step replays for every iteration and the order of an iteration lives in the
// table.  No noise term.  A history term is applied iff its weight is non-zero (and, for w2, hist is given); the previous
// prediction is read iff a term or hist needs it, so a row with w1 = w2 = 0 gives ddim_update_kernel's bits whatever the history
// buffers hold.  One pass, float4, grid-stride, ddim_update_kernel's launch shape; no atomics and no dependence on the batch.
#include "solver_kernels.h"
#include "step_math.h"

namespace ddimx {

__global__ void __launch_bounds__(256) multistep_update_kernel(float* __restrict__ xt, const float* __restrict__ et,
                                                               float* __restrict__ x0, float* __restrict__ hist,
                                                               const float* __restrict__ coef, const int* __restrict__ step,
                                                               long long n4) {
    const StepRow r = load_row(coef + (size_t)step[0] * kSolverStride, true);
    const bool use1 = r.w1 != 0.f, use2 = r.w2 != 0.f && hist != nullptr;
    const bool load1 = use1 || use2 || hist != nullptr;
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
        update4(xt, et, x0, hist, (size_t)i, r, load1, use1, use2, false, z);
}

hipError_t multistep_update_launch(float* xt, const float* et, float* x0, float* hist, const float* coef, const int* step,
                                   long long n, hipStream_t s) {
    if (n <= 0 || n % 4) return hipErrorInvalidValue;
    const long long n4 = n / 4;
    const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(multistep_update_kernel, dim3(blocks), dim3(256), 0, s, xt, et, x0, hist, coef, step, n4);
    return hipGetLastError();
}

}  // namespace ddimx
