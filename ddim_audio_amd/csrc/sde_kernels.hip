// SDE-DPM-Solver++ multistep sampler (ddim_audio_amd/solver.py with tau > 0; Lu et al. 2022, appendix -- "DPM++ 2M SDE" / "3M SDE"):
// the element-wise arithmetic of one step, orders 1-3, with the noise of the step added in the same pass.
//
// The update is update4 (step_math.h) on row step[0] of the solver's table (kSolverStride floats -- schedule.dpm_coefficients(tau=)),
// so one captured step replays for every iteration; the order of an iteration and whether it adds noise live in the table.  The
// history flags are multistep_update_kernel's; the noise term is added iff c1 != 0, so a row with c1 = 0 gives that kernel's bits
// and a row with w1 = w2 = 0 ddim_update_kernel's on the same noise.  z is noise[i] when the caller hands a buffer (a host
// generator, a noise_fn); otherwise it is noise_normals4 (noise.h) for the counter (group of four, first_sample + b,
// draw_base + step[0], tag 0) under the key of seed -- what noise_fill_kernel writes for that sample and draw -- so there is no
// noise buffer and no fill launch.  The grid is (blocks per sample, B) like noise_fill_kernel's; every block walks its sample's
// float4s grid-stride.  No atomics, no LDS, vector stores only; a sample's result depends on (seed, its global index) and on
// nothing else of the batch.
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
    const StepRow r = load_row(coef + (size_t)pos * kSolverStride, true);
    const bool use1 = r.w1 != 0.f, use2 = r.w2 != 0.f && hist != nullptr, add_z = r.c1 != 0.f;
    const bool load1 = use1 || use2 || hist != nullptr, load_z = add_z && noise != nullptr, draw_z = add_z && noise == nullptr;
    const unsigned sample = first_sample + blockIdx.y, draw = draw_base + (unsigned)pos;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kSampleThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kSampleThreads) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (load_z) load4(noise, base + (size_t)i, z);
        if (draw_z) noise_normals4((unsigned)i, sample, draw, kSdeTagStep, k0, k1, z);
        update4(xt, et, x0, hist, base + (size_t)i, r, load1, use1, use2, add_z, z);
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

// The sampling step of a consistency model (consistency.py; Song et al. 2023, multistep consistency sampling): the data prediction
// m = f(xt, t) from the network's raw output, then the re-noising to the next level, a_next m + c1 z, in the same pass.  Row
// step[0] of the table (kCmStride floats, schedule.consistency_coefficients) is (t, p, q, a_next, 0, c1, 0, 0); z and the grid are
// sde_multistep_update_kernel's, so with no buffer the draw is what noise_fill_kernel writes.  The last row has a_next = 1 and
// c1 = 0: xt = x0.
__global__ void __launch_bounds__(kSampleThreads) cm_update_kernel(float* __restrict__ xt, const float* __restrict__ out,
                                                                   const float* __restrict__ noise, float* __restrict__ x0,
                                                                   const float* __restrict__ coef, const int* __restrict__ step,
                                                                   long long n4, unsigned k0, unsigned k1, unsigned first_sample,
                                                                   unsigned draw_base) {
    const int pos = step[0];
    const float* c = coef + (size_t)pos * kCmStride;
    const float p = c[1], q = c[2], an = c[3], c1 = c[5];
    const bool add_z = c1 != 0.f, load_z = add_z && noise != nullptr, draw_z = add_z && noise == nullptr;
    const unsigned sample = first_sample + blockIdx.y, draw = draw_base + (unsigned)pos;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kSampleThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kSampleThreads) {
        float z[4] = {0.f, 0.f, 0.f, 0.f}, x[4], o[4], m[4];
        if (load_z) load4(noise, base + (size_t)i, z);
        if (draw_z) noise_normals4((unsigned)i, sample, draw, kSdeTagStep, k0, k1, z);
        load4(xt, base + (size_t)i, x);
        load4(out, base + (size_t)i, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = consistency_f(x[j], o[j], p, q);
            const float u = __fmul_rn(an, m[j]);
            x[j] = add_z ? fmaf(z[j], c1, u) : u;
        }
        store4(x0, base + (size_t)i, m);
        store4(xt, base + (size_t)i, x);
    }
}

hipError_t cm_update_launch(float* xt, const float* out, const float* noise, float* x0, const float* coef, const int* step, int B,
                            long long per_sample, unsigned long long seed, unsigned first_sample, unsigned draw_base, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    const long long n4 = per_sample / 4;
    if (n4 > (1LL << 32) || (unsigned long long)first_sample + (unsigned long long)B > (1ULL << 32)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kSampleThreads);
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    hipLaunchKernelGGL(cm_update_kernel, grid, block, 0, s, xt, out, noise, x0, coef, step, n4, k0, k1, first_sample, draw_base);
    return hipGetLastError();
}

}  // namespace ddimx
