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
//
// Both are HBM-bound.  The grid is (blocks per canvas sample, N) with inpaint_residual_kernel's block count: every block belongs to
// one canvas sample and walks its float4s grid-stride, the partials are reduced in inpaint_update_kernel's fixed order, so a canvas
// sample's result does not depend on its batch and one window (L = T) is inpaint_steps bit for bit.  No atomics, no LDS beyond
// block_sum, vector stores only.  Every scalar operation is step_math.h's, the blend window_kernels.h's.  The K-way gather and
// scatter are row-contiguous: F = 256 puts one canvas row on one wave, whose K window rows are K contiguous 1 KiB pieces.
#include "window_inpaint_kernels.h"

namespace ddimx {

template <int K>
__global__ void __launch_bounds__(kInpaintThreads) window_inpaint_residual_kernel(
    const float* __restrict__ x, const float4* __restrict__ eps, const float* __restrict__ y, const float* __restrict__ m,
    float* __restrict__ x0, float* __restrict__ beps, float4* __restrict__ seed, float* __restrict__ partials,
    const int* __restrict__ jfirst, const int* __restrict__ cnt, const float* __restrict__ wt, const float* __restrict__ coef,
    const int* __restrict__ step, unsigned n4, int W, int L, int T, int H, int F4) {
    __shared__ float red[kInpaintThreads / 64];
    const float* c = coef + (size_t)step[0] * kInpaintStride;
    const float s1 = c[1], s2 = c[2], k1 = c[6];
    const unsigned chan4 = (unsigned)L * (unsigned)F4;  // float4s of one channel of a canvas sample
    const unsigned C = n4 / chan4;
    const size_t win4 = (size_t)T * (size_t)F4;         // ... and of one channel of a window
    const size_t sbase = (size_t)blockIdx.y * (size_t)W * C * win4;  // window 0 of this canvas sample
    const size_t xbase = (size_t)blockIdx.y * n4;
    float acc = 0.f;
    for (unsigned i = blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += gridDim.x * kInpaintThreads) {
        const size_t at = xbase + i;
        float eb[4], xs[4], ys[4], ms[4], p0[4], sd[4];
        window_blend4<K>(eps, jfirst, cnt, wt, blockIdx.y, i, n4, W, L, T, H, F4, eb);
        load4(x, at, xs);
        load4(y, at, ys);
        load4(m, at, ms);
        const unsigned ch = i / chan4, rem = i - ch * chan4;
        const unsigned l = rem / (unsigned)F4, f = rem - l * (unsigned)F4;
        const int n = cnt[l], j0 = jfirst[l];
        float w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = K > 1 ? wt[(size_t)k * (size_t)L + l] : 1.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = ddim_x0(xs[q], eb[q], s1, s2);  // on the blended eps
            const float r = inpaint_residual(v, ys[q], ms[q]);
            acc = fmaf(r, r, acc);
            p0[q] = v;
            sd[q] = inpaint_seed(r, ms[q], k1);
        }
        store4(x0, at, p0);
        store4(beps, at, eb);
        // the adjoint of the blend: window j0 + k takes wt[k][l] times the canvas seed at its row l - (j0 + k) H; one covering window
        // takes the seed itself.  The stores stay inside the batch whatever the plan holds.
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = j0 + k, tau = (int)l - j * H;
            if (k < n && j >= 0 && j < W && tau >= 0 && tau < T) {
                float4 o;
                o.x = n == 1 ? sd[0] : __fmul_rn(w[k], sd[0]);
                o.y = n == 1 ? sd[1] : __fmul_rn(w[k], sd[1]);
                o.z = n == 1 ? sd[2] : __fmul_rn(w[k], sd[2]);
                o.w = n == 1 ? sd[3] : __fmul_rn(w[k], sd[3]);
                seed[sbase + ((size_t)j * C + ch) * win4 + (size_t)tau * (size_t)F4 + f] = o;
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
    __shared__ float red[kInpaintThreads / 64];
    const float* c = coef + (size_t)step[0] * kInpaintStride;
    const float s1 = c[1], s2 = c[2], s3 = c[3], c2 = c[4], c1 = c[5], k2 = c[7], zeta = c[8];
    float w = 0.f;  // zeta / sqrt(L_n); 0 = no guidance term (L_n = 0 or zeta = 0)
    if (GUIDED) {
        // the canvas sample's partials, in inpaint_update_kernel's order: thread i adds partials i, i + 256, ..., then the block sum
        const float* ps = partials + (size_t)blockIdx.y * nparts;
        float v = 0.f;
        for (int p = threadIdx.x; p < nparts; p += kInpaintThreads) v += ps[p];
        const float Ln = block_sum(v, red);
        if (Ln > 0.f && zeta != 0.f) w = (float)((double)zeta / sqrt((double)Ln));  // in double, rounded once to fp32
    }
    const size_t xbase = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += gridDim.x * kInpaintThreads) {
        const size_t at = xbase + i;
        float es[4], p0[4], gs[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f};
        float ys[4] = {0.f, 0.f, 0.f, 0.f}, ms[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
        if (GUIDED) {
            load4(eps, at, es);  // the blended eps and x0 the residual kernel wrote
            load4(x0, at, p0);
            if (w != 0.f) window_overlap_add4<K>(dwin, jfirst, cnt, blockIdx.y, i, n4, W, L, T, H, F4, gs);
        } else {
            float xs[4];
            window_blend4<K>((const float4*)eps, jfirst, cnt, wt, blockIdx.y, i, n4, W, L, T, H, F4, es);
            load4(x, at, xs);
#pragma unroll
            for (int q = 0; q < 4; ++q) p0[q] = ddim_x0(xs[q], es[q], s1, s2);
        }
        if (noise) load4(noise, at, nz);
        if (GUIDED || REPLACE) {
            load4(y, at, ys);
            load4(m, at, ms);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float u = ddim_next(p0[q], es[q], s3, c2);
            if (noise) u = fmaf(nz[q], c1, u);
            // g = d L_n / d x = k2 m^2 (x0 - y) + the overlap-added data-only backward of the weighted seeds
            if (GUIDED && w != 0.f) u = inpaint_guide(u, p0[q], ys[q], ms[q], gs[q], k2, w);
            if (REPLACE) {
                // the known content taken along the same DDIM path; exactly u where m = 0, exactly kv where m = 1
                float kv = ddim_next(ys[q], es[q], s3, c2);
                if (noise) kv = fmaf(nz[q], c1, kv);
                u = inpaint_replace(u, kv, ms[q]);
            }
            out[q] = u;
        }
        if (!GUIDED) store4(x0, at, p0);
        store4(x, at, out);
    }
}

hipError_t window_inpaint_residual_launch(const float* x, const float* eps, const float* y, const float* m, float* x0, float* beps,
                                          float* seed, float* partials, const int* jfirst, const int* cnt, const float* wt,
                                          const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, hipStream_t s) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K) return hipErrorInvalidValue;
    const long long per = (long long)C * L * F;
    const dim3 grid(window_inpaint_blocks(N, per), N);
    const unsigned n4 = (unsigned)(per / 4);
#define DDIMX_WINDOW_CASE(k)                                                                                                        \
    case k:                                                                                                                         \
        hipLaunchKernelGGL((window_inpaint_residual_kernel<k>), grid, dim3(kInpaintThreads), 0, s, x, (const float4*)eps, y, m, x0, beps, \
                           (float4*)seed, partials, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4);                            \
        break;
    switch (K) {
        DDIMX_WINDOW_CASE(1) DDIMX_WINDOW_CASE(2) DDIMX_WINDOW_CASE(3) DDIMX_WINDOW_CASE(4)
        DDIMX_WINDOW_CASE(5) DDIMX_WINDOW_CASE(6) DDIMX_WINDOW_CASE(7) DDIMX_WINDOW_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef DDIMX_WINDOW_CASE
    return hipGetLastError();
}

template <int K>
static void window_inpaint_update_k(int flags, dim3 grid, hipStream_t s, float* x, const float* eps, const float* noise, float* x0,
                                    const float* y, const float* m, const float* dwin, const float* partials, const int* jfirst,
                                    const int* cnt, const float* wt, const float* coef, const int* step, unsigned n4, int W, int L, int T,
                                    int H, int F4) {
#define DDIMX_FLAGS_CASE(v, g, r)                                                                                                      \
    case v:                                                                                                                            \
        hipLaunchKernelGGL((window_inpaint_update_kernel<K, g, r>), grid, dim3(kInpaintThreads), 0, s, x, eps, noise, x0, y, m,          \
                           (const float4*)dwin, partials, (int)grid.x, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F4);                \
        break;
    switch (flags) {
        DDIMX_FLAGS_CASE(0, false, false) DDIMX_FLAGS_CASE(1, false, true) DDIMX_FLAGS_CASE(2, true, false)
        default: hipLaunchKernelGGL((window_inpaint_update_kernel<K, true, true>), grid, dim3(kInpaintThreads), 0, s, x, eps, noise, x0, y, m,
                                    (const float4*)dwin, partials, (int)grid.x, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F4);
    }
#undef DDIMX_FLAGS_CASE
}

hipError_t window_inpaint_update_launch(float* x, const float* eps, const float* noise, float* x0, const float* y, const float* m,
                                        const float* dwin, const float* partials, const int* jfirst, const int* cnt, const float* wt,
                                        const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, int flags,
                                        hipStream_t s) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K || (flags & ~3)) return hipErrorInvalidValue;
    if ((flags & 3) && (!y || !m)) return hipErrorInvalidValue;
    if ((flags & 2) && (!dwin || !partials)) return hipErrorInvalidValue;
    const long long per = (long long)C * L * F;
    const dim3 grid(window_inpaint_blocks(N, per), N);
    const unsigned n4 = (unsigned)(per / 4);
#define DDIMX_WINDOW_CASE(k) \
    case k: window_inpaint_update_k<k>(flags, grid, s, x, eps, noise, x0, y, m, dwin, partials, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4); break;
    switch (K) {
        DDIMX_WINDOW_CASE(1) DDIMX_WINDOW_CASE(2) DDIMX_WINDOW_CASE(3) DDIMX_WINDOW_CASE(4)
        DDIMX_WINDOW_CASE(5) DDIMX_WINDOW_CASE(6) DDIMX_WINDOW_CASE(7) DDIMX_WINDOW_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef DDIMX_WINDOW_CASE
    return hipGetLastError();
}

}  // namespace ddimx
