// Windowed inpainting (ddim_audio_amd.windowed_inpaint_steps): masked DDIM inpainting with reconstruction guidance on one long
// canvas [N][C][L][F] that the network sees through overlapping windows of its own length T (window_kernels.hip).  The guidance
// gradient has to cross the adjoint of gather and blend; the two element-wise passes that frame the forward and the data-only
// backward of a guided step do that:
//
//   window_inpaint_residual_kernel   blends the window batch's eps per canvas row (window_blend4), forms x0 and the masked residual
//                                    r = m (x0 - y) on the canvas, one fp32 partial of sum r^2 per (canvas sample, block) -- the norm
//                                    belongs to the canvas sample -- and SCATTERS the backward's seed: the canvas seed k1 m r of row l
//                                    goes to every window that covers l, times the window's blend weight (the adjoint of the blend).
//                                    A window row is one canvas row and that row is covered by that window, so every element of the
//                                    seed batch is written exactly once and nothing is zeroed first.
//   window_inpaint_update_kernel     inpaint_update_kernel on the canvas.  Guided: reads the blended eps and x0 the residual wrote and
//                                    GATHERS the backward's result -- the sum of d_win over the covering windows in ascending window
//                                    order (window_overlap_add4: the adjoint of the gather).  Not guided: blends eps itself, so a
//                                    replacement-only step is gather, forward and this one launch, like windowed_steps'.
//   window_inpaint_multistep_kernel  inpaint_multistep_update_kernel (inpaint_solver_kernels.hip) on the canvas, for
//                                    windowed_inpaint_solver_steps: the same two sources of eps, x0 and d as the kernel above, the
//                                    13-column row, canvas-shaped history h1 / h2 and z handed or drawn for (group of four within
//                                    the canvas sample, first_sample + n, draw_base + step[0], tag 0).  The residual pass of its
//                                    guided step is window_inpaint_residual_kernel on the wider row (the launch takes the stride).
//
// Both are HBM-bound.  The grid is (blocks per canvas sample, N) with inpaint_residual_kernel's block count: every block belongs to
// one canvas sample and walks its float4s grid-stride, the partials are reduced in inpaint_update_kernel's fixed order, so a canvas
// sample's result does not depend on its batch and one window (L = T) is inpaint_steps bit for bit.  No atomics, no LDS beyond
// block_sum, vector stores only.  The step's arithmetic is inpaint_kernels.h's -- the same calls inpaint_kernels.hip makes; only
// where eps, x0 and d come from differs -- and the locator, cover loads and blend window_kernels.h's.  The K-way gather and
// scatter are row-contiguous: F = 256 puts one canvas row on one wave, whose K window rows are K contiguous 1 KiB pieces.
#include "window_inpaint_kernels.h"
#include "noise.h"

namespace ddimx {

constexpr unsigned kWindowInpaintTagStep = 0u;  // noise.py TAG_STEP: the noise a sampler step adds

template <int K>
__global__ void __launch_bounds__(kInpaintThreads) window_inpaint_residual_kernel(
    const float* __restrict__ x, const float4* __restrict__ eps, const float* __restrict__ y, const float* __restrict__ m,
    float* __restrict__ x0, float* __restrict__ beps, float4* __restrict__ seed, float* __restrict__ partials,
    const int* __restrict__ jfirst, const int* __restrict__ cnt, const float* __restrict__ wt, const float* __restrict__ coef,
    const int* __restrict__ step, unsigned n4, int W, int L, int T, int H, int F4, int stride) {
    const WindowGeom g{n4, W, L, T, H, F4};
    __shared__ float red[kInpaintThreads / 64];
    const InpaintRow c = load_inpaint_row(coef, step, stride);
    const size_t xbase = (size_t)blockIdx.y * n4;
    float acc = 0.f;
    for (unsigned i = blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += gridDim.x * kInpaintThreads) {
        const size_t at = xbase + i;
        const WindowRow r = window_row(g, jfirst, cnt, blockIdx.y, i);
        float w[K], eb[4], xs[4], ys[4], ms[4], p0[4], sd[4];
        window_blend4<K>(eps, wt, g, r, w, eb);
        load4(x, at, xs);
        load4(y, at, ys);
        load4(m, at, ms);
        inpaint_residual4(xs, eb, ys, ms, c, p0, sd, acc);  // on the blended eps
        store4(x0, at, p0);
        store4(beps, at, eb);
        // the adjoint of the blend: window j0 + k takes wt[k][l] times the canvas seed at its row l - (j0 + k) H; one covering window
        // takes the seed itself.  The stores stay inside the batch whatever the plan holds.
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = r.j0 + k, tau = (int)r.l - j * g.H;
            if (k < r.n && j >= 0 && j < g.W && tau >= 0 && tau < g.T) {
                float4 o;
                o.x = r.n == 1 ? sd[0] : __fmul_rn(w[k], sd[0]);
                o.y = r.n == 1 ? sd[1] : __fmul_rn(w[k], sd[1]);
                o.z = r.n == 1 ? sd[2] : __fmul_rn(w[k], sd[2]);
                o.w = r.n == 1 ? sd[3] : __fmul_rn(w[k], sd[3]);
                *r.at(seed, j, tau) = o;
            }
        }
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

template <int K, bool GUIDED, bool REPLACE>
__global__ void __launch_bounds__(kInpaintThreads) window_inpaint_update_kernel(
    float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ noise, float* __restrict__ x0,
    const float* __restrict__ y, const float* __restrict__ m, const float4* __restrict__ dwin, const float* __restrict__ partials,
    int nparts, const int* __restrict__ jfirst, const int* __restrict__ cnt, const float* __restrict__ wt,
    const float* __restrict__ coef, const int* __restrict__ step, unsigned n4, int W, int L, int T, int H, int F4) {
    const WindowGeom g{n4, W, L, T, H, F4};
    __shared__ float red[kInpaintThreads / 64];
    const InpaintRow c = load_inpaint_row(coef, step);
    const float w = GUIDED ? inpaint_weight(partials + (size_t)blockIdx.y * nparts, nparts, c.zeta, red) : 0.f;
    const size_t xbase = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += gridDim.x * kInpaintThreads) {
        const size_t at = xbase + i;
        float es[4], p0[4], gs[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f};
        float ys[4] = {0.f, 0.f, 0.f, 0.f}, ms[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
        if (GUIDED) {
            load4(eps, at, es);  // the blended eps and x0 the residual kernel wrote
            load4(x0, at, p0);
            if (w != 0.f) window_overlap_add4<K>(dwin, wt, g, window_row(g, jfirst, cnt, blockIdx.y, i), gs);
        } else {
            float xs[4];
            window_blend4<K>((const float4*)eps, jfirst, cnt, wt, g, blockIdx.y, i, es);
            load4(x, at, xs);
#pragma unroll
            for (int q = 0; q < 4; ++q) p0[q] = ddim_x0(xs[q], es[q], c.s1, c.s2);
        }
        if (noise) load4(noise, at, nz);
        if (GUIDED || REPLACE) {
            load4(y, at, ys);
            load4(m, at, ms);
        }
        inpaint_update4<GUIDED, REPLACE>(p0, es, ys, ms, gs, nz, noise != nullptr, w, c, out);
        if (!GUIDED) store4(x0, at, p0);
        store4(x, at, out);
    }
}

template <int K, bool GUIDED, bool REPLACE>
__global__ void __launch_bounds__(kInpaintThreads) window_inpaint_multistep_kernel(
    float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ noise, float* __restrict__ x0, float* __restrict__ h1,
    float* __restrict__ h2, const float* __restrict__ y, const float* __restrict__ m, const float4* __restrict__ dwin,
    const float* __restrict__ partials, int nparts, const int* __restrict__ jfirst, const int* __restrict__ cnt,
    const float* __restrict__ wt, const float* __restrict__ coef, const int* __restrict__ step, unsigned n4, int W, int L, int T, int H,
    int F4, unsigned k0, unsigned k1, unsigned first_sample, unsigned draw_base) {
    const WindowGeom g{n4, W, L, T, H, F4};
    __shared__ float red[kInpaintThreads / 64];
    const int pos = step[0];
    const InpaintSolverRow c = load_inpaint_solver_row(coef, pos);
    const float w = GUIDED ? inpaint_weight(partials + (size_t)blockIdx.y * nparts, nparts, c.r.zeta, red) : 0.f;
    const bool fold = GUIDED && w != 0.f;
    const bool use1 = c.w1 != 0.f, use2 = c.w2 != 0.f && h2 != nullptr, load1 = use1 || use2, add_z = c.r.c1 != 0.f;
    const bool load_z = add_z && noise != nullptr, draw_z = add_z && noise == nullptr;
    const unsigned sample = first_sample + blockIdx.y, draw = draw_base + (unsigned)pos;
    const size_t xbase = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += gridDim.x * kInpaintThreads) {
        const size_t at = xbase + i;
        float xs[4] = {0.f, 0.f, 0.f, 0.f}, es[4], p0[4], gs[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        float ys[4] = {0.f, 0.f, 0.f, 0.f}, ms[4] = {0.f, 0.f, 0.f, 0.f}, m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
        float mt[4], out[4];
        if (!GUIDED || REPLACE) load4(x, at, xs);
        if (GUIDED) {
            load4(eps, at, es);  // the blended eps and m0 the residual kernel wrote
            load4(x0, at, p0);
            if (fold) window_overlap_add4<K>(dwin, wt, g, window_row(g, jfirst, cnt, blockIdx.y, i), gs);
        } else {
            window_blend4<K>((const float4*)eps, jfirst, cnt, wt, g, blockIdx.y, i, es);
#pragma unroll
            for (int q = 0; q < 4; ++q) p0[q] = ddim_x0(xs[q], es[q], c.r.s1, c.r.s2);
            store4(x0, at, p0);
        }
        if (load_z) load4(noise, at, z);
        if (draw_z) noise_normals4(i, sample, draw, kWindowInpaintTagStep, k0, k1, z);
        if (GUIDED || REPLACE) {
            load4(y, at, ys);
            load4(m, at, ms);
        }
        if (load1) load4(h1, at, m1);
        if (use2) load4(h2, at, m2);
        inpaint_multistep4<GUIDED, REPLACE>(xs, es, p0, ys, ms, gs, z, m1, m2, w, use1, use2, add_z, c, mt, out);
        if (h2 && load1) store4(h2, at, m1);
        store4(h1, at, mt);
        store4(x, at, out);
    }
}

hipError_t window_inpaint_residual_launch(const float* x, const float* eps, const float* y, const float* m, float* x0, float* beps,
                                          float* seed, float* partials, const int* jfirst, const int* cnt, const float* wt,
                                          const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, hipStream_t s,
                                          int stride) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K) return hipErrorInvalidValue;
    const dim3 grid(window_inpaint_blocks(N, (long long)C * L * F), N);
    const unsigned n4 = (unsigned)((long long)C * L * (F / 4));
    const bool ok = dispatch_cover(K, [&](auto k) {
        hipLaunchKernelGGL((window_inpaint_residual_kernel<decltype(k)::value>), grid, dim3(kInpaintThreads), 0, s, x, (const float4*)eps, y,
                           m, x0, beps, (float4*)seed, partials, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4, stride);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t window_inpaint_update_launch(float* x, const float* eps, const float* noise, float* x0, const float* y, const float* m,
                                        const float* dwin, const float* partials, const int* jfirst, const int* cnt, const float* wt,
                                        const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, int flags,
                                        hipStream_t s) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K || (flags & ~3)) return hipErrorInvalidValue;
    if ((flags & 3) && (!y || !m)) return hipErrorInvalidValue;
    if ((flags & 2) && (!dwin || !partials)) return hipErrorInvalidValue;
    const dim3 grid(window_inpaint_blocks(N, (long long)C * L * F), N);
    const unsigned n4 = (unsigned)((long long)C * L * (F / 4));
    const bool ok = dispatch_cover(K, [&](auto k) {
        dispatch_inpaint_flags(flags, [&](auto guided, auto replace) {
            hipLaunchKernelGGL((window_inpaint_update_kernel<decltype(k)::value, decltype(guided)::value, decltype(replace)::value>), grid,
                               dim3(kInpaintThreads), 0, s, x, eps, noise, x0, y, m, (const float4*)dwin, partials, (int)grid.x, jfirst, cnt,
                               wt, coef, step, n4, W, L, T, H, F / 4);
        });
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t window_inpaint_multistep_launch(float* x, const float* eps, const float* noise, float* x0, float* h1, float* h2, const float* y,
                                           const float* m, const float* dwin, const float* partials, const int* jfirst, const int* cnt,
                                           const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H,
                                           int F, int flags, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                                           hipStream_t s) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K || (flags & ~3) || !h1) return hipErrorInvalidValue;
    if ((flags & 3) && (!y || !m)) return hipErrorInvalidValue;
    if ((flags & 2) && (!dwin || !partials)) return hipErrorInvalidValue;
    if ((unsigned long long)first_sample + (unsigned long long)N > (1ULL << 32)) return hipErrorInvalidValue;
    const dim3 grid(window_inpaint_blocks(N, (long long)C * L * F), N);
    const unsigned n4 = (unsigned)((long long)C * L * (F / 4));
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    const bool ok = dispatch_cover(K, [&](auto k) {
        dispatch_inpaint_flags(flags, [&](auto guided, auto replace) {
            hipLaunchKernelGGL((window_inpaint_multistep_kernel<decltype(k)::value, decltype(guided)::value, decltype(replace)::value>), grid,
                               dim3(kInpaintThreads), 0, s, x, eps, noise, x0, h1, h2, y, m, (const float4*)dwin, partials, (int)grid.x,
                               jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4, k0, k1, first_sample, draw_base);
        });
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace ddimx
