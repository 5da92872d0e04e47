// Windowed multistep sampling (ddim_audio_amd.windowed_solver_steps): DPM-Solver++ orders 1-3, deterministic or stochastic, on
// one long canvas [N][C][L][F] whose noise prediction is the blend of the overlapping windows' (window_kernels.hip).  The
// multistep update is affine in eps plus canvas-shaped history, so it composes with the blend exactly as the DDIM update does.
//
//   window_multistep_update_kernel   the fused path: per float4 of the canvas, window_blend4 (window_kernels.h) forms the blended
//                                    eps in registers and update4_core (step_math.h) applies row step[0] of the solver's table
//                                    to it, with x0 / hist the canvas-shaped history -- the blend of window_update_kernel followed
//                                    by the arithmetic of sde_multistep_update_kernel, in one pass over the canvas.
//   window_blend_kernel              writes the blended eps alone, canvas-shaped, for the two callers that need it whole before
//                                    any element is updated: the x0 threshold (a quantile over the canvas sample) and the
//                                    Brownian update (its own z source); the existing update kernels then run on the canvas.
//
// Both are HBM-bound and element-wise.  The grid is (blocks per sample, N) like window_update_kernel's: every block belongs to one
// canvas sample and walks its float4s grid-stride, so a canvas sample's result does not depend on its batch.  No atomics, no LDS,
// vector stores only.  The flags of the fused kernel are sde_multistep_update_kernel's, run-time and uniform over the block;
// every load -- the blend's fixed clamped set, x, m1 / m2 / z where their flag holds -- is issued before the first store.
#include "window_solver_kernels.h"
#include "noise.h"

namespace ddimx {

constexpr unsigned kWindowTagStep = 0u;  // noise.py TAG_STEP: the noise a sampler step adds

template <int K>
__global__ void __launch_bounds__(kWindowThreads) window_blend_kernel(const float4* __restrict__ eps, float4* __restrict__ beps,
                                                                      const int* __restrict__ jfirst, const int* __restrict__ cnt,
                                                                      const float* __restrict__ wt, unsigned n4, int W, int L, int T, int H, int F4) {
    const WindowGeom g{n4, W, L, T, H, F4};
    const size_t xbase = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kWindowThreads + threadIdx.x; i < n4; i += gridDim.x * kWindowThreads) {
        float eb[4];
        window_blend4<K>(eps, jfirst, cnt, wt, g, blockIdx.y, i, eb);
        beps[xbase + i] = make_float4(eb[0], eb[1], eb[2], eb[3]);
    }
}

template <int K>
__global__ void __launch_bounds__(kWindowThreads) window_multistep_update_kernel(
    float* __restrict__ x, const float4* __restrict__ eps, const float* __restrict__ noise, float* __restrict__ x0, float* __restrict__ hist,
    const int* __restrict__ jfirst, const int* __restrict__ cnt, const float* __restrict__ wt, const float* __restrict__ coef,
    const int* __restrict__ step, unsigned n4, int W, int L, int T, int H, int F4,
    unsigned k0, unsigned k1, unsigned first_sample, unsigned draw_base) {
    const WindowGeom g{n4, W, L, T, H, F4};
    const int pos = step[0];
    const StepRow r = load_row(coef + (size_t)pos * kSolverStride, true);
    const bool use1 = r.w1 != 0.f, use2 = r.w2 != 0.f && hist != nullptr, add_z = r.c1 != 0.f;
    const bool load1 = use1 || use2 || hist != nullptr, load_z = add_z && noise != nullptr, draw_z = add_z && noise == nullptr;
    const unsigned sample = first_sample + blockIdx.y, draw = draw_base + (unsigned)pos;
    const size_t xbase = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kWindowThreads + threadIdx.x; i < n4; i += gridDim.x * kWindowThreads) {
        const size_t at = xbase + i;
        float e[4], xs[4], m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f}, m0[4];
        window_blend4<K>(eps, jfirst, cnt, wt, g, blockIdx.y, i, e);
        load4(x, at, xs);
        if (load1) load4(x0, at, m1);
        if (use2) load4(hist, at, m2);
        if (load_z) load4(noise, at, z);
        if (draw_z) noise_normals4(i, sample, draw, kWindowTagStep, k0, k1, z);
        update4_core(xs, e, m1, m2, m0, r, use1, use2, add_z, z);
        if (hist) store4(hist, at, m1);
        store4(x0, at, m0);
        store4(x, at, xs);
    }
}

hipError_t window_blend_launch(const float* eps, float* beps, const int* jfirst, const int* cnt, const float* wt, int N, int W, int C,
                               int L, int T, int H, int F, hipStream_t s) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(N, (long long)C * L * F), N);
    const unsigned n4 = (unsigned)((long long)C * L * (F / 4));
    const bool ok = dispatch_cover(K, [&](auto k) {
        hipLaunchKernelGGL((window_blend_kernel<decltype(k)::value>), grid, dim3(kWindowThreads), 0, s, (const float4*)eps, (float4*)beps,
                           jfirst, cnt, wt, n4, W, L, T, H, F / 4);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t window_multistep_update_launch(float* x, const float* eps, const float* noise, float* x0, float* hist, const int* jfirst,
                                          const int* cnt, const float* wt, const float* coef, const int* step, int N, int W, int C, int L,
                                          int T, int H, int F, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                                          hipStream_t s) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K || (unsigned long long)first_sample + (unsigned long long)N > (1ULL << 32)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(N, (long long)C * L * F), N);
    const unsigned n4 = (unsigned)((long long)C * L * (F / 4));
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    const bool ok = dispatch_cover(K, [&](auto k) {
        hipLaunchKernelGGL((window_multistep_update_kernel<decltype(k)::value>), grid, dim3(kWindowThreads), 0, s, x, (const float4*)eps,
                           noise, x0, hist, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4, k0, k1, first_sample, draw_base);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace ddimx
