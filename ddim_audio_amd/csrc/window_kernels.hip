// Windowed long-form sampling (ddim_audio_amd/window.py): one long canvas [N][C][L][F] is denoised through overlapping windows of
// the network's own length T.  Two element-wise kernels frame the forward of a step:
//
//   window_gather_kernel   canvas -> window batch [N W][C][T][F]: window j of canvas sample n (batch sample n W + j) is the canvas
//                          rows [j H, j H + T).  A row is F floats (F % 4 == 0), so every row offset is 16-byte aligned for any
//                          hop H and the copy runs in float4s.
//   window_update_kernel   blends the noise predictions of the (at most K = ceil(T / H)) windows that cover a canvas row with
//                          the row's normalised weights -- a partition of unity -- and applies the DDIM update (step_math.h)
//                          to the canvas, in place.
//
// Both read nothing that depends on N: the grid is (blocks per sample, samples) like inpaint_update_kernel's / noise_fill_kernel's,
// every block belongs to one sample (blockIdx.y) and walks its float4s grid-stride, so one canvas still fills the chip and the
// result of a canvas sample is the same whatever batch it runs in.  No atomics, no LDS.  The update's loads are a fixed set per
// iteration -- x, K pieces of eps, K weights, the two plan entries, the noise -- issued unconditionally from clamped indices
// before the first store; what a row does not use (k >= cnt) is dropped by a select, so no load waits for another one's value
// beyond the two plan entries the addresses are formed from (window_blend4, window_kernels.h: the blend's only copy).  F = 256 puts one canvas row on exactly one wave: the plan entries
// and weights are one broadcast line per wave.
#include "window_kernels.h"

namespace ddimx {

__global__ void __launch_bounds__(kWindowThreads) window_gather_kernel(const float4* __restrict__ canvas, float4* __restrict__ win,
                                                                       unsigned n4, int W, int L, int T, int H, int F4) {
    const unsigned chan4 = (unsigned)T * (unsigned)F4;  // float4s of one channel of a window
    const unsigned C = n4 / chan4;
    const unsigned n = blockIdx.y / (unsigned)W, j = blockIdx.y - n * (unsigned)W;
    const size_t src = ((size_t)n * C * (size_t)L + (size_t)j * (size_t)H) * (size_t)F4;  // row j H of channel 0 of canvas sample n
    const size_t dst = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kWindowThreads + threadIdx.x; i < n4; i += gridDim.x * kWindowThreads) {
        const unsigned ch = i / chan4, rem = i - ch * chan4;  // rem = tau F4 + f: the window's rows are consecutive canvas rows
        win[dst + i] = canvas[src + (size_t)ch * (size_t)L * (size_t)F4 + rem];
    }
}

template <int K, bool NOISE>
__global__ void __launch_bounds__(kWindowThreads) window_update_kernel(
    float4* __restrict__ x, const float4* __restrict__ eps, const float4* __restrict__ noise, float4* __restrict__ x0,
    const int* __restrict__ jfirst, const int* __restrict__ cnt, const float* __restrict__ wt, const float* __restrict__ coef,
    const int* __restrict__ step, unsigned n4, int W, int L, int T, int H, int F4) {
    const float* c = coef + (size_t)step[0] * 6;
    const float s1 = c[1], s2 = c[2], s3 = c[3], c2 = c[4], c1 = c[5];
    const size_t xbase = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kWindowThreads + threadIdx.x; i < n4; i += gridDim.x * kWindowThreads) {
        float eb[4];
        window_blend4<K>(eps, jfirst, cnt, wt, blockIdx.y, i, n4, W, L, T, H, F4, eb);
        const float4 x4 = x[xbase + i];
        float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (NOISE) z4 = noise[xbase + i];
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, nz[4] = {z4.x, z4.y, z4.z, z4.w};
        float p0[4], out[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = ddim_x0(xs[q], eb[q], s1, s2);  // on the blended eps
            float u = ddim_next(v, eb[q], s3, c2);
            if (NOISE) u = fmaf(nz[q], c1, u);
            p0[q] = v;
            out[q] = u;
        }
        x0[xbase + i] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        x[xbase + i] = make_float4(out[0], out[1], out[2], out[3]);
    }
}

hipError_t window_gather_launch(const float* canvas, float* win, int N, int W, int C, int L, int T, int H, int F, hipStream_t s) {
    if (!window_shape_ok(N, W, C, L, T, H, F)) return hipErrorInvalidValue;
    const long long per = (long long)C * T * F;
    hipLaunchKernelGGL(window_gather_kernel, dim3(sample_blocks(N * W, per), N * W), dim3(kWindowThreads), 0, s, (const float4*)canvas,
                       (float4*)win, (unsigned)(per / 4), W, L, T, H, F / 4);
    return hipGetLastError();
}

template <int K>
static void window_update_k(bool has_noise, dim3 grid, hipStream_t s, float* x, const float* eps, const float* noise, float* x0,
                            const int* jfirst, const int* cnt, const float* wt, const float* coef, const int* step, unsigned n4, int W,
                            int L, int T, int H, int F4) {
    if (has_noise)
        hipLaunchKernelGGL((window_update_kernel<K, true>), grid, dim3(kWindowThreads), 0, s, (float4*)x, (const float4*)eps,
                           (const float4*)noise, (float4*)x0, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F4);
    else
        hipLaunchKernelGGL((window_update_kernel<K, false>), grid, dim3(kWindowThreads), 0, s, (float4*)x, (const float4*)eps,
                           (const float4*)noise, (float4*)x0, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F4);
}

hipError_t window_update_launch(float* x, const float* eps, const float* noise, float* x0, const int* jfirst, const int* cnt,
                                const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F,
                                hipStream_t s) {
    if (!window_shape_ok(N, W, C, L, T, H, F)) return hipErrorInvalidValue;
    const int K = (T + H - 1) / H;
    if (K > kWindowMaxCover || (K > 1 && !wt)) return hipErrorInvalidValue;
    const long long per = (long long)C * L * F;
    const dim3 grid(sample_blocks(N, per), N);
    const unsigned n4 = (unsigned)(per / 4);
    const bool z = noise != nullptr;
#define DDIMX_WINDOW_CASE(k) \
    case k: window_update_k<k>(z, grid, s, x, eps, noise, x0, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4); break;
    switch (K) {
        DDIMX_WINDOW_CASE(1) DDIMX_WINDOW_CASE(2) DDIMX_WINDOW_CASE(3) DDIMX_WINDOW_CASE(4)
        DDIMX_WINDOW_CASE(5) DDIMX_WINDOW_CASE(6) DDIMX_WINDOW_CASE(7) DDIMX_WINDOW_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef DDIMX_WINDOW_CASE
    return hipGetLastError();
}

}  // namespace ddimx
