// DPM-Solver++ multistep sampler with the UniC corrector (ddim_audio_amd/solver.py with corrector=True; UniPC, Zhao et al. 2023):
// the element-wise arithmetic of one step, orders 1-3.
//
// Predictor and corrector are both linear in the sample and in the x0 predictions, so "correct with this step's prediction, then
// predict from the corrected sample" is the solver's update with other history weights and one more history term
// (schedule.unic_coefficients): no second sample buffer, no second pass.  The update is update4h (step_math.h) on row step[0] of
// the corrector's table (kUnicStride floats: t, s1, s2, s3, c2, c1 = 0, w1', w2', w3), so one captured step replays for every
// iteration and the order of an iteration lives in the table.  No noise term.  The flags are multistep_update_kernel's, and one
// more of the same kind: a history term is applied iff its weight is non-zero and its buffer is given (hist for w2, hist2 for
// w3), and a buffer is read iff a term or the shift into the next buffer needs it, so a row with w3 = 0 and no hist2 gives
// multistep_update_kernel's bits and a row with w1 = w2 = w3 = 0 ddim_update_kernel's, whatever the history buffers hold.  One
// pass, float4, grid-stride, multistep_update_kernel's launch shape; no atomics and no dependence on the batch.
#include "unic_kernels.h"
#include "step_math.h"

namespace ddimx {

__global__ void __launch_bounds__(256) unic_multistep_update_kernel(float* __restrict__ xt, const float* __restrict__ et,
                                                                    float* __restrict__ x0, float* __restrict__ hist,
                                                                    float* __restrict__ hist2, const float* __restrict__ coef,
                                                                    const int* __restrict__ step, long long n4) {
    const StepRow r = load_row3(coef + (size_t)step[0] * kUnicStride);
    const bool use1 = r.w1 != 0.f, use2 = r.w2 != 0.f && hist != nullptr, use3 = r.w3 != 0.f && hist2 != nullptr;
    const bool load1 = use1 || use2 || hist != nullptr;
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
        update4h(xt, et, x0, hist, hist2, (size_t)i, r, load1, use1, use2, use3, false, z);
}

hipError_t unic_multistep_update_launch(float* xt, const float* et, float* x0, float* hist, float* hist2, const float* coef,
                                        const int* step, long long n, hipStream_t s) {
    if (n <= 0 || n % 4 || (hist2 && !hist)) return hipErrorInvalidValue;
    const long long n4 = n / 4;
    const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(unic_multistep_update_kernel, dim3(blocks), dim3(256), 0, s, xt, et, x0, hist, hist2, coef, step, n4);
    return hipGetLastError();
}

}  // namespace ddimx
