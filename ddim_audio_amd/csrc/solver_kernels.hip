// DPM-Solver++ multistep sampler (ddim_audio_amd/solver.py; Lu et al. 2022, data-prediction form): the element-wise arithmetic
// of one step, orders 1-3.
//
// The scalars come from the coefficient row of the device step counter (kSolverStride floats: t, s1 = sqrt(1-at), s2 = sqrt(at),
// s3 = sqrt(at_next), c2, c1 = 0, w1, w2 -- schedule.dpm_coefficients), so one captured step replays for every iteration and the
// order of an iteration lives in the table.  With m1 = x0[i] (the previous iteration's prediction, still in the buffer) and
// m2 = hist[i] (the one before), per element and in this order:
//   m0 = (x - s1 e) / s2                       ddim_x0    (step_math.h)
//   u  = s3 m0 + c2 e                          ddim_next
//   u  = u + w1 (m0 - m1)     if w1 != 0       fmaf(w1, __fsub_rn(m0, m1), u)
//   u  = u + w2 (m1 - m2)     if w2 != 0       fmaf(w2, __fsub_rn(m1, m2), u)
//   xt <- u, x0 <- m0, hist <- m1 (when hist is given)
// The two conditions are uniform (the row's scalars): a row with w1 = w2 = 0 gives ddim_update_kernel's bits whatever the history
// buffers hold -- the first iteration finds them uninitialised, and their values never enter u.  One pass, float4, grid-stride,
// ddim_update_kernel's launch shape; no atomics and no dependence on the batch.
#include "solver_kernels.h"
#include "step_math.h"

namespace ddimx {

__global__ void __launch_bounds__(256) multistep_update_kernel(float* __restrict__ xt, const float* __restrict__ et,
                                                               float* __restrict__ x0, float* __restrict__ hist,
                                                               const float* __restrict__ coef, const int* __restrict__ step,
                                                               long long n4) {
    const float* c = coef + (size_t)step[0] * kSolverStride;
    const float s1 = c[1], s2 = c[2], s3 = c[3], c2 = c[4], w1 = c[6], w2 = c[7];
    const bool use1 = w1 != 0.f, use2 = w2 != 0.f && hist != nullptr;
    const bool load1 = use1 || use2 || hist != nullptr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 x = ((const float4*)xt)[i];
        const float4 e = ((const float4*)et)[i];
        const float xs[4] = {x.x, x.y, x.z, x.w}, es[4] = {e.x, e.y, e.z, e.w};
        float m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
        if (load1) { const float4 v = ((const float4*)x0)[i]; m1[0] = v.x; m1[1] = v.y; m1[2] = v.z; m1[3] = v.w; }
        if (use2) { const float4 v = ((const float4*)hist)[i]; m2[0] = v.x; m2[1] = v.y; m2[2] = v.z; m2[3] = v.w; }
        float p0[4], out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m0 = ddim_x0(xs[j], es[j], s1, s2);
            float u = ddim_next(m0, es[j], s3, c2);
            if (use1) u = fmaf(w1, __fsub_rn(m0, m1[j]), u);
            if (use2) u = fmaf(w2, __fsub_rn(m1[j], m2[j]), u);
            p0[j] = m0;
            out[j] = u;
        }
        if (hist) ((float4*)hist)[i] = make_float4(m1[0], m1[1], m1[2], m1[3]);
        ((float4*)x0)[i] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        ((float4*)xt)[i] = make_float4(out[0], out[1], out[2], out[3]);
    }
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
