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

// The adjoint of window_blend4's gather without its weights: the sum over the windows that cover float4 `i` of canvas sample
// `sample` of their float4 at the row's place in the window, in ascending window order, ((d[j0] + d[j1]) + d[j2]) ..., each sum
// rounded once; one covering window: its value itself.  The loads follow window_blend4's rule: K of them from indices clamped into
// the batch, issued unconditionally, what a row does not use (k >= cnt) dropped by a select.
template <int K>
__device__ __forceinline__ void window_overlap_add4(const float4* __restrict__ d, const int* __restrict__ jfirst, const int* __restrict__ cnt,
                                                    unsigned sample, unsigned i, unsigned n4, int W, int L, int T, int H, int F4, float g[4]) {
    const unsigned chan4 = (unsigned)L * (unsigned)F4;
    const unsigned C = n4 / chan4;
    const size_t win4 = (size_t)T * (size_t)F4;
    const size_t dbase = (size_t)sample * (size_t)W * C * win4;
    const unsigned ch = i / chan4, rem = i - ch * chan4;
    const unsigned l = rem / (unsigned)F4, f = rem - l * (unsigned)F4;
    const int n = cnt[l];
    int j0 = jfirst[l];
    j0 = j0 < 0 ? 0 : (j0 > W - 1 ? W - 1 : j0);
    float4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = j0 + k > W - 1 ? W - 1 : j0 + k;
        int tau = (int)l - j * H;
        tau = tau < 0 ? 0 : (tau > T - 1 ? T - 1 : tau);
        v[k] = d[dbase + ((size_t)j * C + ch) * win4 + (size_t)tau * (size_t)F4 + f];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float acc = q == 0 ? v[0].x : q == 1 ? v[0].y : q == 2 ? v[0].z : v[0].w;
#pragma unroll
        for (int k = 1; k < K; ++k) {
            const float dk = q == 0 ? v[k].x : q == 1 ? v[k].y : q == 2 ? v[k].z : v[k].w;
            acc = k < n ? __fadd_rn(acc, dk) : acc;
        }
        g[q] = acc;
    }
}

// Guided steps, one pass over the canvas [N][C][L][F] (coefficient row of inpaint_residual_kernel at step[0]; plan of
// window_update_launch): beps = the blend of the window batch's eps (window_blend4), x0 = (x - s1 beps) / s2, r = m (x0 - y),
// partials[n][blk] = the block's sum of r^2 (window_inpaint_blocks per canvas sample), and the seed of the window batch's data-only
// backward: with s = k1 (m r) at canvas row l, window j = jfirst[l] + k (k < cnt[l]) receives wt[k][l] s at its row l - j H, s
// itself where cnt[l] == 1.  Every element of seed [N W][C][T][F] is written exactly once.
hipError_t window_inpaint_residual_launch(const float* x, const float* eps, const float* y, const float* m, float* x0, float* beps,
                                          float* seed, float* partials, const int* jfirst, const int* cnt, const float* wt,
                                          const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, hipStream_t s);

// The update of inpaint_update_launch on the canvas, in place on x; flags: 1 = replace, 2 = guided.  Not guided: eps is the window
// batch's, blended here (x0 computed and written).  Guided: eps is the canvas-shaped beps and x0 is read, both the residual's, and
// d_x of inpaint_update_kernel is window_overlap_add4 of the window batch's d_win.
hipError_t window_inpaint_update_launch(float* x, const float* eps, const float* noise, float* x0, const float* y, const float* m,
                                        const float* dwin, const float* partials, const int* jfirst, const int* cnt, const float* wt,
                                        const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, int flags,
                                        hipStream_t s);

}  // namespace ddimx
