// Launch wrappers of the windowed long-form sampler kernels (window_kernels.hip; ddim_audio_amd/window.py).  Same rules as
// step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"

namespace ddimx {

constexpr int kWindowThreads = kSampleThreads;  // the grid of either kernel: (sample_blocks, samples)
constexpr int kWindowMaxCover = 8;  // K = ceil(T / H), the most windows that cover one canvas row: the update's unrolled loads

// The geometry both launches share: canvas [N][C][L][F], window batch [N W][C][T][F], window j of canvas sample n = batch sample
// n W + j = canvas rows [j H, j H + T).  True when 1 <= N, W, C; N W <= 65535; F a positive multiple of 4; 1 <= H <= T;
// L = T + (W - 1) H; and one sample of either tensor has fewer than 2^31 float4s (the kernels index inside a sample in 32 bits).
inline bool window_shape_ok(int N, int W, int C, int L, int T, int H, int F) {
    if (N < 1 || W < 1 || C < 1 || T < 1 || H < 1 || H > T || F < 4 || F % 4) return false;
    if ((long long)N * W > 65535) return false;
    if ((long long)L != (long long)T + (long long)(W - 1) * H) return false;
    return (long long)C * L * (F / 4) < (1LL << 31);
}

// K = ceil(T / H), the windows that cover a canvas row, of a geometry that passes window_shape_ok with K <= kWindowMaxCover and, for
// overlapping windows, their weights; else 0
inline int window_cover_ok(const float* wt, int N, int W, int C, int L, int T, int H, int F) {
    if (!window_shape_ok(N, W, C, L, T, H, F)) return 0;
    const int K = (T + H - 1) / H;
    return (K > kWindowMaxCover || (K > 1 && !wt)) ? 0 : K;
}

// The blended noise prediction of float4 `i` of canvas sample `sample` -- the only copy of the blend (window_update_kernel here,
// window_blend_kernel and window_multistep_update_kernel in window_solver_kernels.hip).  Row l of channel ch is covered by the
// windows jfirst[l] .. jfirst[l] + cnt[l] - 1; the loads are a fixed set -- K pieces of eps, K weights, the two plan entries --
// issued unconditionally from indices clamped into the batch (inside for k < cnt by the plan's construction, any valid address
// beyond), and what a row does not use (k >= cnt) is dropped by a select.  One covering window: its eps itself, no multiply;
// otherwise fmaf(wt[c-1], eps[c-1], ... fmaf(wt[1], eps[1], wt[0] * eps[0])), every operation rounded once.
template <int K>
__device__ __forceinline__ void window_blend4(const float4* __restrict__ eps, const int* __restrict__ jfirst, const int* __restrict__ cnt,
                                              const float* __restrict__ wt, unsigned sample, unsigned i, unsigned n4, int W, int L, int T,
                                              int H, int F4, float eb[4]) {
    const unsigned chan4 = (unsigned)L * (unsigned)F4;  // float4s of one channel of a canvas sample
    const unsigned C = n4 / chan4;
    const size_t win4 = (size_t)T * (size_t)F4;         // ... and of one channel of a window
    const size_t ebase = (size_t)sample * (size_t)W * C * win4;  // window 0 of this canvas sample
    const unsigned ch = i / chan4, rem = i - ch * chan4;
    const unsigned l = rem / (unsigned)F4, f = rem - l * (unsigned)F4;
    const int n = cnt[l];
    int j0 = jfirst[l];
    j0 = j0 < 0 ? 0 : (j0 > W - 1 ? W - 1 : j0);
    float4 e[K];
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = j0 + k > W - 1 ? W - 1 : j0 + k;
        int tau = (int)l - j * H;
        tau = tau < 0 ? 0 : (tau > T - 1 ? T - 1 : tau);
        e[k] = eps[ebase + ((size_t)j * C + ch) * win4 + (size_t)tau * (size_t)F4 + f];
        w[k] = K > 1 ? wt[(size_t)k * (size_t)L + l] : 1.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float es[K];
#pragma unroll
        for (int k = 0; k < K; ++k) es[k] = q == 0 ? e[k].x : q == 1 ? e[k].y : q == 2 ? e[k].z : e[k].w;
        eb[q] = es[0];
        if (K > 1) {
            float acc = __fmul_rn(w[0], es[0]);
#pragma unroll
            for (int k = 1; k < K; ++k) acc = k < n ? fmaf(w[k], es[k], acc) : acc;
            eb[q] = n == 1 ? es[0] : acc;
        }
    }
}

// win[n W + j][c][tau][:] = canvas[n][c][j H + tau][:], in 16-byte pieces
hipError_t window_gather_launch(const float* canvas, float* win, int N, int W, int C, int L, int T, int H, int F, hipStream_t s);

// One DDIM update of the canvas from the window batch's noise predictions (coefficient row of ddim_update_kernel at step[0]).
// Per canvas row l the plan gives the first covering window jfirst[l], the number of covering windows cnt[l] (1 .. K) and their
// normalised weights wt[k][l] (k = 0 .. cnt - 1 in ascending window order; [K][L] fp32, unused for K = 1):
//   e  = eps of window jfirst                                         if cnt == 1  (a select: no multiply)
//   e  = fmaf(wt[c-1], eps[jfirst+c-1], ... fmaf(wt[1], eps[jfirst+1], wt[0] * eps[jfirst]))   otherwise
//   x0 = (x - s1 e) / s2,  x = s3 x0 + c2 e (+ c1 noise; noise nullable, canvas-shaped), rounded as ddim_update_kernel rounds them.
// K = ceil(T / H) must be <= kWindowMaxCover.
hipError_t window_update_launch(float* x, const float* eps, const float* noise, float* x0, const int* jfirst, const int* cnt,
                                const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F,
                                hipStream_t s);

}  // namespace ddimx
