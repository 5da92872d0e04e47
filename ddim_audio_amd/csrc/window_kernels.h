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
