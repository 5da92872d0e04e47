// SDE-DPM-Solver++ multistep sampler (ddim_audio_amd/solver.py with tau > 0; Lu et al. 2022, appendix -- "DPM++ 2M SDE" / "3M SDE"):
// the element-wise arithmetic of one step, orders 1-3, with the noise of the step added in the same pass.
//
// The scalars come from the coefficient row of the device step counter (kSolverStride floats: t, s1, s2, s3, c2, c1, w1, w2 --
// schedule.dpm_coefficients(tau=)), so one captured step replays for every iteration; the order of an iteration and whether it
// adds noise live in the table.  With m1 = x0[i] and m2 = hist[i] on entry, per element and in this order -- the operations and
// the order pool_update_kernel documents:
//   m0 = (x - s1 e) / s2                       ddim_x0    (step_math.h)
//   u  = s3 m0 + c2 e                          ddim_next
//   u  = u + w1 (m0 - m1)     if w1 != 0       fmaf(w1, __fsub_rn(m0, m1), u)
//   u  = u + w2 (m1 - m2)     if w2 != 0       fmaf(w2, __fsub_rn(m1, m2), u)     (and hist is given)
//   u  = u + c1 z             if c1 != 0       fmaf(z, c1, u)
//   xt <- u, x0 <- m0, hist <- m1 (when hist is given)
// so a row with c1 = 0 gives multistep_update_kernel's bits and a row with w1 = w2 = 0 ddim_update_kernel's on the same noise.
// z is noise[i] when the caller hands a buffer (a host generator, a noise_fn); otherwise it is the normal of noise.h for the counter
// (group of four, first_sample + b, draw_base + step[0], tag 0) under the key of seed: element for element what noise_fill_kernel
// writes for that sample and draw, formed here from the same two functions, so there is no noise buffer and no fill launch.  All
// conditions are uniform over a block (the row's scalars and the pointers).  The grid is (blocks per sample, B) like
// noise_fill_kernel's; every block walks its sample's float4s grid-stride.  No atomics, no LDS, vector stores only; a sample's
// result depends on (seed, its global index) and on nothing else of the batch.
#include "sde_kernels.h"
#include "noise.h"

namespace ddimx {

constexpr unsigned kSdeTagStep = 0u;  // noise.py TAG_STEP: the noise a sampler step adds

__global__ void __launch_bounds__(kSampleThreads) sde_multistep_update_kernel(float* __restrict__ xt, const float* __restrict__ et,
                                                                              const float* __restrict__ noise, float* __restrict__ x0,
                                                                              float* __restrict__ hist, const float* __restrict__ coef,
                                                                              const int* __restrict__ step, long long n4, unsigned k0,
                                                                              unsigned k1, unsigned first_sample, unsigned draw_base) {
    const int pos = step[0];
    const float* c = coef + (size_t)pos * kSolverStride;
    const float s1 = c[1], s2 = c[2], s3 = c[3], c2 = c[4], c1 = c[5], w1 = c[6], w2 = c[7];
    const bool use1 = w1 != 0.f, use2 = w2 != 0.f && hist != nullptr, add_z = c1 != 0.f;
    const bool load1 = use1 || use2 || hist != nullptr, load_z = add_z && noise != nullptr, draw_z = add_z && noise == nullptr;
    const unsigned sample = first_sample + blockIdx.y, draw = draw_base + (unsigned)pos;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kSampleThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kSampleThreads) {
        const size_t at = base + (size_t)i;
        const float4 x = ((const float4*)xt)[at];
        const float4 e = ((const float4*)et)[at];
        const float xs[4] = {x.x, x.y, x.z, x.w}, es[4] = {e.x, e.y, e.z, e.w};
        float m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        if (load1) { const float4 v = ((const float4*)x0)[at]; m1[0] = v.x; m1[1] = v.y; m1[2] = v.z; m1[3] = v.w; }
        if (use2) { const float4 v = ((const float4*)hist)[at]; m2[0] = v.x; m2[1] = v.y; m2[2] = v.z; m2[3] = v.w; }
        if (load_z) { const float4 v = ((const float4*)noise)[at]; z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w; }
        if (draw_z) {
            unsigned w[4] = {(unsigned)i, sample, draw, kSdeTagStep};
            philox4x32_10(w, k0, k1);
            noise_pair(w[0], w[1], z[0], z[1]);
            noise_pair(w[2], w[3], z[2], z[3]);
        }
        float p0[4], out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m0 = ddim_x0(xs[j], es[j], s1, s2);
            float u = ddim_next(m0, es[j], s3, c2);
            if (use1) u = fmaf(w1, __fsub_rn(m0, m1[j]), u);
            if (use2) u = fmaf(w2, __fsub_rn(m1[j], m2[j]), u);
            if (add_z) u = fmaf(z[j], c1, u);
            p0[j] = m0;
            out[j] = u;
        }
        if (hist) ((float4*)hist)[at] = make_float4(m1[0], m1[1], m1[2], m1[3]);
        ((float4*)x0)[at] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        ((float4*)xt)[at] = make_float4(out[0], out[1], out[2], out[3]);
    }
}

hipError_t sde_multistep_update_launch(float* xt, const float* et, const float* noise, float* x0, float* hist, const float* coef,
                                       const int* step, int B, long long per_sample, unsigned long long seed, unsigned first_sample,
                                       unsigned draw_base, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    const long long n4 = per_sample / 4;
    if (n4 > (1LL << 32) || (unsigned long long)first_sample + (unsigned long long)B > (1ULL << 32)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kSampleThreads);
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    hipLaunchKernelGGL(sde_multistep_update_kernel, grid, block, 0, s, xt, et, noise, x0, hist, coef, step, n4, k0, k1, first_sample,
                       draw_base);
    return hipGetLastError();
}

}  // namespace ddimx
