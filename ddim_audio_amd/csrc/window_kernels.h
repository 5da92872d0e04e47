// Launch wrappers of the windowed long-form sampler kernels (window_kernels.hip; ddim_audio_amd/window.py), and what every kernel
// on the canvas shares (window_, window_solver_ and window_inpaint_kernels.hip): the geometry checks, the dispatch on the cover
// count, the row locator, the cover loads and the blend.  Same rules as step_kernels.h: enqueue on the given stream, never allocate
// or synchronise.
#pragma once
#include <type_traits>
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

// The integers every canvas kernel takes, gathered for the helpers below: n4 = float4s of one canvas sample (C L F / 4), F4 = F / 4
struct WindowGeom { unsigned n4; int W, L, T, H, F4; };

// fn(std::integral_constant<int, K>{}) for the cover count K = 1 .. kWindowMaxCover -- the only dispatch on it: every K-templated
// kernel is launched from a generic lambda as kernel<decltype(k)::value, ...>; false (nothing called) for any other K
template <class Fn>
bool dispatch_cover(int K, Fn&& fn) {
    static_assert(kWindowMaxCover == 8, "one case per cover count");
    switch (K) {
        case 1: fn(std::integral_constant<int, 1>{}); return true;
        case 2: fn(std::integral_constant<int, 2>{}); return true;
        case 3: fn(std::integral_constant<int, 3>{}); return true;
        case 4: fn(std::integral_constant<int, 4>{}); return true;
        case 5: fn(std::integral_constant<int, 5>{}); return true;
        case 6: fn(std::integral_constant<int, 6>{}); return true;
        case 7: fn(std::integral_constant<int, 7>{}); return true;
        case 8: fn(std::integral_constant<int, 8>{}); return true;
        default: return false;
    }
}

// Where float4 `i` of canvas sample `sample` lies -- the only copy of this arithmetic: channel ch, canvas row l, float4 f of the row,
// and the plan's entries of the row as the plan holds them: the windows j0 = jfirst[l] .. j0 + n - 1, n = cnt[l], cover it.
// at(p, j, tau): the float4 of row tau of window j of this sample at the same (ch, f), in the [N W][C][T][F] batch p.  Both structs
// are a few registers and travel by value.
struct WindowRow {
    unsigned ch, l, f, C;
    size_t win4, first;  // float4s of one channel of a window; the batch sample of window 0 of this canvas sample (n W)
    int F4, n, j0;
    template <class T4>
    __device__ __forceinline__ T4* at(T4* p, int j, int tau) const {
        const size_t base = first * C * win4;  // window 0 of this canvas sample
        return &p[base + ((size_t)j * C + ch) * win4 + (size_t)tau * (size_t)F4 + f];
    }
};
__device__ __forceinline__ WindowRow window_row(WindowGeom g, const int* __restrict__ jfirst, const int* __restrict__ cnt,
                                                unsigned sample, unsigned i) {
    const unsigned chan4 = (unsigned)g.L * (unsigned)g.F4;  // float4s of one channel of a canvas sample
    const unsigned C = g.n4 / chan4;
    const size_t win4 = (size_t)g.T * (size_t)g.F4;
    const size_t first = (size_t)sample * (size_t)g.W;
    const unsigned ch = i / chan4, rem = i - ch * chan4;
    const unsigned l = rem / (unsigned)g.F4, f = rem - l * (unsigned)g.F4;
    return {ch, l, f, C, win4, first, g.F4, cnt[l], jfirst[l]};
}
// v[k] = the row's float4 in window j0 + k of the batch p and w[k] = the window's normalised weight wt[k][l] there (1 where windows
// do not overlap: K = 1 does not read wt), k = 0 .. K - 1.  The loads are a fixed set issued unconditionally from indices clamped
// into the batch (inside for k < n by the plan's construction, any valid address beyond): no load waits for another one's value
// beyond the two plan entries the addresses are formed from, and what a row does not use (k >= n) is dropped by the caller's select.
// A caller that reads no weight (window_overlap_add4) passes wt all the same: a load whose value goes unused is not emitted.
template <int K>
__device__ __forceinline__ void window_load_cover(const float4* __restrict__ p, const float* __restrict__ wt, WindowGeom g,
                                                  WindowRow r, float4 v[K], float w[K]) {
    const int j0 = r.j0 < 0 ? 0 : (r.j0 > g.W - 1 ? g.W - 1 : r.j0);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = j0 + k > g.W - 1 ? g.W - 1 : j0 + k;
        int tau = (int)r.l - j * g.H;
        tau = tau < 0 ? 0 : (tau > g.T - 1 ? g.T - 1 : tau);
        v[k] = *r.at(p, j, tau);
        w[k] = K > 1 ? wt[(size_t)k * (size_t)g.L + r.l] : 1.f;
    }
}
__device__ __forceinline__ float lane4(const float4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }

// The blended noise prediction of the row's float4 -- the only copy of the blend, whichever kernel forms it -- and the weights it
// was formed with.  One covering window: its eps itself, no multiply; otherwise fmaf(wt[c-1], eps[c-1], ... fmaf(wt[1], eps[1],
// wt[0] * eps[0])), every operation rounded once.
template <int K>
__device__ __forceinline__ void window_blend4(const float4* __restrict__ eps, const float* __restrict__ wt, WindowGeom g,
                                              WindowRow r, float w[K], float eb[4]) {
    float4 e[K];
    window_load_cover<K>(eps, wt, g, r, e, w);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        eb[q] = lane4(e[0], q);
        if (K > 1) {
            float acc = __fmul_rn(w[0], lane4(e[0], q));
#pragma unroll
            for (int k = 1; k < K; ++k) acc = k < r.n ? fmaf(w[k], lane4(e[k], q), acc) : acc;
            eb[q] = r.n == 1 ? lane4(e[0], q) : acc;
        }
    }
}
// ... for a kernel that needs the row and its weights for nothing else
template <int K>
__device__ __forceinline__ void window_blend4(const float4* __restrict__ eps, const int* __restrict__ jfirst, const int* __restrict__ cnt,
                                              const float* __restrict__ wt, WindowGeom g, unsigned sample, unsigned i, float eb[4]) {
    float w[K];
    window_blend4<K>(eps, wt, g, window_row(g, jfirst, cnt, sample, i), w, eb);
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
