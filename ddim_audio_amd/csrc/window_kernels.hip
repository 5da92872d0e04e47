// Windowed long-form sampling (ddim_audio_amd/window.py): one long canvas [N][C][L][F] is denoised through overlapping windows of
// the network's own length T.  Two element-wise kernels frame the forward of a step:
//
//   window_gather_kernel   canvas -> window batch [N W][C][T][F]: window j of canvas sample n (batch sample n W + j) is the canvas
//                          rows [j H, j H + T).  A row is F floats (F % 4 == 0), so every row offset is 16-byte aligned for any
//                          hop H and the copy runs in float4s.
//   window_update_kernel   blends the noise predictions of the (at most K = ceil(T / H)) windows that cover a canvas row with
//                          the row's normalised weights -- a partition of unity -- (window_blend4) and applies the DDIM update
//                          to the canvas, in place: update4_core (step_math.h) on a DDIM row, no history term.
//
// Both read nothing that depends on N: the grid is (blocks per sample, samples) like inpaint_update_kernel's / noise_fill_kernel's,
// every block belongs to one sample (blockIdx.y) and walks its float4s grid-stride, so one canvas still fills the chip and the
// result of a canvas sample is the same whatever batch it runs in.  No atomics, no LDS.  The update's loads are a fixed set per
// iteration -- x, K pieces of eps, K weights, the two plan entries, the noise -- issued unconditionally from clamped indices
// before the first store; what a row does not use (k >= cnt) is dropped by a select, so no load waits for another one's value
// beyond the two plan entries the addresses are formed from.  The row locator, the cover loads, the blend and the dispatch on K
// are window_kernels.h's, shared with every other canvas kernel.  F = 256 puts one canvas row on exactly one wave: the plan
// entries and weights are one broadcast line per wave.
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
    const WindowGeom g{n4, W, L, T, H, F4};
    const StepRow r = load_row(coef + (size_t)step[0] * 6, false);
    const size_t xbase = (size_t)blockIdx.y * n4;
    for (unsigned i = blockIdx.x * kWindowThreads + threadIdx.x; i < n4; i += gridDim.x * kWindowThreads) {
        const size_t at = xbase + i;
        float e[4], xs[4], z[4] = {0.f, 0.f, 0.f, 0.f}, m0[4];
        window_blend4<K>(eps, jfirst, cnt, wt, g, blockIdx.y, i, e);
        load4((const float*)x, at, xs);
        if (NOISE) load4((const float*)noise, at, z);
        update4_core(xs, e, z, z, m0, r, false, false, NOISE, z);  // the DDIM update: no history term reads m1 / m2
        store4((float*)x0, at, m0);
        store4((float*)x, at, xs);
    }
}

hipError_t window_gather_launch(const float* canvas, float* win, int N, int W, int C, int L, int T, int H, int F, hipStream_t s) {
    if (!window_shape_ok(N, W, C, L, T, H, F)) return hipErrorInvalidValue;
    const long long per = (long long)C * T * F;
    hipLaunchKernelGGL(window_gather_kernel, dim3(sample_blocks(N * W, per), N * W), dim3(kWindowThreads), 0, s, (const float4*)canvas,
                       (float4*)win, (unsigned)(per / 4), W, L, T, H, F / 4);
    return hipGetLastError();
}

hipError_t window_update_launch(float* x, const float* eps, const float* noise, float* x0, const int* jfirst, const int* cnt,
                                const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F,
                                hipStream_t s) {
    const int K = window_cover_ok(wt, N, W, C, L, T, H, F);
    if (!K) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(N, (long long)C * L * F), N);
    const unsigned n4 = (unsigned)((long long)C * L * (F / 4));
    const bool ok = dispatch_cover(K, [&](auto k) {
        if (noise)
            hipLaunchKernelGGL((window_update_kernel<decltype(k)::value, true>), grid, dim3(kWindowThreads), 0, s, (float4*)x, (const float4*)eps,
                               (const float4*)noise, (float4*)x0, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4);
        else
            hipLaunchKernelGGL((window_update_kernel<decltype(k)::value, false>), grid, dim3(kWindowThreads), 0, s, (float4*)x, (const float4*)eps,
                               (const float4*)noise, (float4*)x0, jfirst, cnt, wt, coef, step, n4, W, L, T, H, F / 4);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace ddimx
