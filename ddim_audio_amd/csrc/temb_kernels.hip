// Timestep-embedding MLP (models/diffusion.py:110-120): tiny dense layers forward and backward, and the gather of the
// precomputed embedding table.  gfx950 only.
#include "temb_kernels.h"

namespace ddimx {

// =====================================================================================================
// small dense layer: one wave per output feature, all batch rows at once (weight-bandwidth bound)
// =====================================================================================================
__global__ void __launch_bounds__(256) linear_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx,
                                                          const float* __restrict__ W, const float* __restrict__ bias,
                                                          float* __restrict__ y, int B, int N, int K, int act, int in_silu) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* wr = W + (size_t)n * K;
    for (int b0 = 0; b0 < B; b0 += 8) {
        float acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.f;
        for (int k = lane * 4; k < K; k += 256) {
            const float4 wv = *(const float4*)(wr + k);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if (b0 + r < B) {
                    const size_t row = idx ? (size_t)idx[b0 + r] : (size_t)(b0 + r);
                    float4 xv = *(const float4*)(x + row * K + k);
                    if (in_silu) { xv.x = silu_f(xv.x); xv.y = silu_f(xv.y); xv.z = silu_f(xv.z); xv.w = silu_f(xv.w); }
                    acc[r] = fmaf(xv.x, wv.x, acc[r]); acc[r] = fmaf(xv.y, wv.y, acc[r]);
                    acc[r] = fmaf(xv.z, wv.z, acc[r]); acc[r] = fmaf(xv.w, wv.w, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float t = wave_sum(acc[r]);
            if (lane == 0 && b0 + r < B) {
                const float v = t + bias[n];
                y[(size_t)(b0 + r) * N + n] = act ? silu_f(v) : v;
            }
        }
    }
}

hipError_t linear_rows_launch(const float* x, const int64_t* idx, const float* W, const float* bias, float* y, int B,
                              int N, int K, int act_silu, hipStream_t s, int in_silu) {
    if (K % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(linear_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, s, x, idx, W, bias, y, B, N, K, act_silu, in_silu);
    return hipGetLastError();
}

// rows of a precomputed [n_timesteps][E] timestep-embedding table: out[b] = table[t[b]]  (eval mode: the MLP of
// models/diffusion.py:110-120 is a pure function of t, and all rows of a sampling step share one t)
__global__ void __launch_bounds__(256) temb_gather_kernel(const float* __restrict__ table, const int64_t* __restrict__ t,
                                                          float* __restrict__ out, int E) {
    const int b = blockIdx.y;
    const float4* src = (const float4*)(table + (size_t)t[b] * E);
    float4* dst = (float4*)(out + (size_t)b * E);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < E / 4; i += gridDim.x * 256) dst[i] = src[i];
}
hipError_t temb_gather_launch(const float* table, const int64_t* t, float* out, int B, int E, hipStream_t s) {
    if (E % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(temb_gather_kernel, dim3((E / 4 + 255) / 256, B), dim3(256), 0, s, table, t, out, E);
    return hipGetLastError();
}

// =====================================================================================================
// timestep-embedding MLP backward (models/diffusion.py:110-120): tiny dense layers, batch rows <= a few dozen
// =====================================================================================================
// dW[n][k] = sum_b dy[b][n] * f(x[row(b)][k]),  db[n] = sum_b dy[b][n];  f = SiLU when x_silu (x holds pre-activations)
__global__ void __launch_bounds__(256) linear_bwd_w_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const int64_t* __restrict__ idx, float* __restrict__ dW,
                                                           float* __restrict__ db, int B, int N, int K, int x_silu) {
    const int n = blockIdx.y;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) {
            const size_t row = idx ? (size_t)idx[b] : (size_t)b;
            float xv = x[row * K + k];
            if (x_silu) xv = silu_f(xv);
            acc = fmaf(dy[(size_t)b * N + n], xv, acc);
        }
        dW[(size_t)n * K + k] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float t = 0.f;
        for (int b = 0; b < B; ++b) t += dy[(size_t)b * N + n];
        db[n] = t;
    }
}
// dx[b][k] = (sum_n dy[b][n] W[n][k]) * SiLU'(xpre[b][k]); block = 16 k x 16 n-lanes
__global__ void __launch_bounds__(256) linear_bwd_x_kernel(const float* __restrict__ dy, const float* __restrict__ W,
                                                           const float* __restrict__ xpre, float* __restrict__ dx, int N, int K) {
    __shared__ float red[16][17];
    const int kl = threadIdx.x & 15, nl = threadIdx.x >> 4;
    const int b = blockIdx.y, k = blockIdx.x * 16 + kl;
    float acc = 0.f;
    if (k < K)
        for (int n = nl; n < N; n += 16) acc = fmaf(dy[(size_t)b * N + n], W[(size_t)n * K + k], acc);
    red[nl][kl] = acc;
    __syncthreads();
    if (nl == 0 && k < K) {
        acc = 0.f;
        for (int j = 0; j < 16; ++j) acc += red[j][kl];
        dx[(size_t)b * K + k] = acc * dsilu_f(xpre[(size_t)b * K + k]);
    }
}
hipError_t linear_bwd_w_launch(const float* dy, const float* x, const int64_t* idx, float* dW, float* db, int B, int N, int K,
                               int x_silu, hipStream_t s) {
    hipLaunchKernelGGL(linear_bwd_w_kernel, dim3((K + 255) / 256, N), dim3(256), 0, s, dy, x, idx, dW, db, B, N, K, x_silu);
    return hipGetLastError();
}
hipError_t linear_bwd_x_launch(const float* dy, const float* W, const float* xpre, float* dx, int B, int N, int K, hipStream_t s) {
    hipLaunchKernelGGL(linear_bwd_x_kernel, dim3((K + 15) / 16, B), dim3(256), 0, s, dy, W, xpre, dx, N, K);
    return hipGetLastError();
}

}  // namespace ddimx
