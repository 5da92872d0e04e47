// Launch wrappers of the windowed inpainting kernels (window_inpaint_kernels.hip; ddim_audio_amd.windowed_inpaint_steps): the
// arithmetic of inpaint_kernels.hip on the canvas of window_kernels.hip.  Same rules as step_kernels.h: enqueue on the given stream,
// never allocate or synchronise.
#pragma once
#include "inpaint_kernels.h"
#include "window_kernels.h"

namespace ddimx {

// blocks per canvas sample of both kernels (= partials per canvas sample): inpaint_residual_kernel's count for a sample of
// C L F elements, so one window (L = T) sums its norm in that kernel's order
inline int window_inpaint_blocks(int N, long long per_sample) { return sample_blocks(N, per_sample, kInpaintMaxBlocks); }

// The adjoint of window_blend4's gather without its weights: the sum over the windows that cover the row's float4 of their float4
// at the row's place in the window (window_load_cover, whose weights go unused), in ascending window order, ((d[j0] + d[j1]) +
// d[j2]) ..., each sum rounded once; one covering window: its value itself.
template <int K>
__device__ __forceinline__ void window_overlap_add4(const float4* __restrict__ d, const float* __restrict__ wt, WindowGeom g, WindowRow r,
                                                    float out[4]) {
    float4 v[K];
    float w[K];
    window_load_cover<K>(d, wt, g, r, v, w);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float acc = lane4(v[0], q);
#pragma unroll
        for (int k = 1; k < K; ++k) acc = k < r.n ? __fadd_rn(acc, lane4(v[k], q)) : acc;
        out[q] = acc;
    }
}

// Guided steps, one pass over the canvas [N][C][L][F] (coefficient row of inpaint_residual_kernel at step[0]; plan of
// window_update_launch): beps = the blend of the window batch's eps (window_blend4), x0 = (x - s1 beps) / s2, r = m (x0 - y),
// partials[n][blk] = the block's sum of r^2 (window_inpaint_blocks per canvas sample), and the seed of the window batch's data-only
// backward: with s = k1 (m r) at canvas row l, window j = jfirst[l] + k (k < cnt[l]) receives wt[k][l] s at its row l - j H, s
// itself where cnt[l] == 1.  Every element of seed [N W][C][T][F] is written exactly once.  stride: kInpaintStride, or
// kInpaintSolverStride for the multistep sampler's table (the same kernel on the wider row, rho where zeta sits).
hipError_t window_inpaint_residual_launch(const float* x, const float* eps, const float* y, const float* m, float* x0, float* beps,
                                          float* seed, float* partials, const int* jfirst, const int* cnt, const float* wt,
                                          const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, hipStream_t s,
                                          int stride = kInpaintStride);

// The update of inpaint_update_launch on the canvas, in place on x; flags: 1 = replace, 2 = guided.  Not guided: eps is the window
// batch's, blended here (x0 computed and written).  Guided: eps is the canvas-shaped beps and x0 is read, both the residual's, and
// d_x of inpaint_update_kernel is window_overlap_add4 of the window batch's d_win.
hipError_t window_inpaint_update_launch(float* x, const float* eps, const float* noise, float* x0, const float* y, const float* m,
                                        const float* dwin, const float* partials, const int* jfirst, const int* cnt, const float* wt,
                                        const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, int flags,
                                        hipStream_t s);

// The update of inpaint_multistep_update_launch (inpaint_solver_kernels.h) on the canvas, in place on x, rows of
// kInpaintSolverStride floats; include/ddimx_window_inpaint_solver.h has the operation order.  eps, x0 and d come from where
// window_inpaint_update_launch takes them; h1 (the guided prediction of the iteration before) and h2 (nullable: the one before
// that) are canvas-shaped; noise null: z drawn in the kernel from (seed, first_sample + n, draw_base + step[0]).
hipError_t window_inpaint_multistep_launch(float* x, const float* eps, const float* noise, float* x0, float* h1, float* h2, const float* y,
                                           const float* m, const float* dwin, const float* partials, const int* jfirst, const int* cnt,
                                           const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H,
                                           int F, int flags, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                                           hipStream_t s);

}  // namespace ddimx
