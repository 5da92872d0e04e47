// Row-wise and element-wise kernels of the FNet bottleneck: LayerNorm (inference and training forward, backward), dropout,
// gelu_new, transpose and the cast to fp32 (models/diffusion.py:123-167 + transformers modeling_fnet.py:138-279).  gfx950 only.
#include "fnet_pointwise.h"
#include "gn_kernels.h"

namespace ddimx {

// =====================================================================================================
// LayerNorm over rows (two-pass in registers: mean, then centred variance)
// =====================================================================================================
template <typename TX>
__global__ void __launch_bounds__(256) layernorm_kernel(const TX* __restrict__ x, const float* __restrict__ add,
                                                        int add_rows, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        float* __restrict__ y, int N, int chunk_rows) {
    __shared__ float red[4];
    __shared__ float bc;
    const int m = blockIdx.x, tid = threadIdx.x;
    const TX* xr = x + (size_t)m * N;
    const float* ar = add ? add + (size_t)(m % add_rows) * N : nullptr;
    // every load of the row -- x, the addend, gamma, beta -- is issued before the first use, unconditionally (clamped index,
    // dropped by select): the kernel is a chain of load round trips and barriers, a load under `if (n < N)` is waited for at once
    float v[8], gam[8], bet[8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n0 = tid + i * 256, n = n0 < N ? n0 : N - 1;
        const float xv = to_f<TX>(xr[n]), av = (ar ? ar : gamma)[n];  // (no addend: gamma is read in its place and dropped)
        v[i] = xv + (ar ? av : 0.f);
        gam[i] = gamma[n];
        bet[i] = beta[n];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        if (n >= N) v[i] = 0.f;
        s += v[i];
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) bc = (red[0] + red[1] + red[2] + red[3]) / (float)N;
    __syncthreads();
    const float mean = bc;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        if (n < N) { const float d = v[i] - mean; q = fmaf(d, d, q); }
    }
    q = wave_sum(q);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    if (tid == 0) bc = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)N + eps);
    __syncthreads();
    const float rstd = bc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        if (n < N) {
            // chunk_rows > 0: chunk-major output for fnet_dense_kernel, [sample = m / chunk_rows][n / 4][32 rows][4] (fnet_dense.hip)
            const size_t o = chunk_rows > 0 ? (size_t)(m / chunk_rows) * 32 * N + ((size_t)(n / 4) * 32 + m % chunk_rows) * 4 + n % 4
                                            : (size_t)m * N + n;
            y[o] = (v[i] - mean) * rstd * gam[i] + bet[i];
        }
    }
}

hipError_t layernorm_launch(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma,
                            const float* beta, float eps, float* y, int M, int N, hipStream_t s, int chunk_rows) {
    if (N > 2048 || chunk_rows > 32 || (chunk_rows > 0 && (N % 4 || M % chunk_rows))) return hipErrorInvalidValue;
    dispatch_dtype(x_dtype, [&](auto t) {
        using TX = typename decltype(t)::type;
        hipLaunchKernelGGL(layernorm_kernel<TX>, dim3(M), dim3(256), 0, s, (const TX*)x, add, add_rows, gamma, beta, eps, y, N, chunk_rows);
    });
    return hipGetLastError();
}

// =====================================================================================================
// FNet bottleneck, training (models/diffusion.py:123-167 + transformers modeling_fnet.py:138-279)
// =====================================================================================================
// Dropout masks are a pure function of (seed, stream, element index) so the backward regenerates them instead of
// storing them.  (The reference draws them from torch's global RNG; only the distribution can be matched.)
__device__ __forceinline__ float dropout_keep(unsigned long long seed, unsigned stream, unsigned long long e, unsigned thresh,
                                              float inv_keep) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)stream + 1) + e * 0xD1342543DE82EF95ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 32) >= thresh ? inv_keep : 0.f;
}
static inline unsigned drop_thresh(float p) { return p <= 0.f ? 0u : (unsigned)((double)p * 4294967296.0); }

// seed_ctr (nullable, device): added to the seed when the launch RUNS -- a training step replayed from a hipGraph keeps its
// per-call mask stream by bumping that counter between replays, where an eager step passes a new seed by value
__global__ void __launch_bounds__(256) dropout_apply_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n,
                                                            unsigned long long seed, const unsigned long long* __restrict__ seed_ctr,
                                                            unsigned stream, unsigned thresh, float inv_keep) {
    if (seed_ctr) seed += *seed_ctr;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll)
        dst[i] = src[i] * dropout_keep(seed, stream, (unsigned long long)i, thresh, inv_keep);
}
hipError_t dropout_apply_launch(const float* src, float* dst, long long n, float p, unsigned long long seed, unsigned stream,
                                hipStream_t s, const unsigned long long* seed_ctr) {
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(dropout_apply_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n, seed, seed_ctr, stream, drop_thresh(p),
                       1.0f / (1.0f - p));
    return hipGetLastError();
}

// y = LN(drop(x) + add[m % add_rows]) * gamma + beta; keeps the pre-norm row (sum_out, nullable) and (mean, rstd)
// (the mean / rstd block reduction is layernorm_kernel's, word for word; sharing it through a __forceinline__ helper changed this
// kernel's register allocation and added an instruction, so both kernels keep their own copy)
template <typename TX>
__global__ void __launch_bounds__(256) ln_train_kernel(const TX* __restrict__ x, const float* __restrict__ add, int add_rows,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float eps, float* __restrict__ y, float* __restrict__ sum_out,
                                                       float* __restrict__ stat, int N, unsigned long long seed,
                                                       const unsigned long long* __restrict__ seed_ctr, unsigned stream,
                                                       unsigned thresh, float inv_keep) {
    __shared__ float red[4];
    __shared__ float bc;
    const int m = blockIdx.x, tid = threadIdx.x;
    if (seed_ctr) seed += *seed_ctr;
    const TX* xr = x + (size_t)m * N;
    const float* ar = add ? add + (size_t)(m % add_rows) * N : nullptr;
    float v[8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        v[i] = 0.f;
        if (n < N) {
            float xv = to_f<TX>(xr[n]);
            if (thresh) xv *= dropout_keep(seed, stream, (unsigned long long)m * N + n, thresh, inv_keep);
            v[i] = xv + (ar ? ar[n] : 0.f);
            s += v[i];
            if (sum_out) sum_out[(size_t)m * N + n] = v[i];
        }
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) bc = (red[0] + red[1] + red[2] + red[3]) / (float)N;
    __syncthreads();
    const float mean = bc;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        if (n < N) { const float d = v[i] - mean; q = fmaf(d, d, q); }
    }
    q = wave_sum(q);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    if (tid == 0) {
        bc = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)N + eps);
        stat[(size_t)m * 2 + 0] = mean;
        stat[(size_t)m * 2 + 1] = bc;
    }
    __syncthreads();
    const float rstd = bc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        if (n < N) y[(size_t)m * N + n] = (v[i] - mean) * rstd * gamma[n] + beta[n];
    }
}
hipError_t ln_train_launch(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma, const float* beta,
                           float eps, float* y, float* sum_out, float* stat, int M, int N, float p, unsigned long long seed,
                           unsigned stream, hipStream_t s, const unsigned long long* seed_ctr) {
    if (N > 2048) return hipErrorInvalidValue;
    const unsigned th = drop_thresh(p);
    const float ik = 1.0f / (1.0f - p);
    dispatch_dtype(x_dtype, [&](auto t) {
        using TX = typename decltype(t)::type;
        hipLaunchKernelGGL(ln_train_kernel<TX>, dim3(M), dim3(256), 0, s, (const TX*)x, add, add_rows, gamma, beta, eps, y, sum_out, stat,
                           N, seed, seed_ctr, stream, th, ik);
    });
    return hipGetLastError();
}

// LayerNorm backward.  x: the pre-norm rows (fp32 or, for the embedding norm, TX + add rows); stat: (mean, rstd).
//   dx = rstd (gamma dy - mean_n(gamma dy) - xhat mean_n(gamma dy xhat)),  dgamma = sum_m dy xhat,  dbeta = sum_m dy
// A block walks kLnRows rows and keeps the per-column parameter sums in registers: partial [nblocks][2][N].
constexpr int kLnRows = 8;
template <typename TX>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const float* __restrict__ dy, const TX* __restrict__ x,
                                                     const float* __restrict__ add, int add_rows, const float* __restrict__ stat,
                                                     const float* __restrict__ gamma, float* __restrict__ dx,
                                                     float* __restrict__ partial, int M, int N) {
    __shared__ float r1[4], r2[4];
    __shared__ float b1, b2;
    const int tid = threadIdx.x;
    float gm[8], dgam[8], dbet[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        gm[i] = n < N ? gamma[n] : 0.f;
        dgam[i] = dbet[i] = 0.f;
    }
    for (int rr = 0; rr < kLnRows; ++rr) {
        const int m = blockIdx.x * kLnRows + rr;
        if (m >= M) break;  // uniform
        const float mean = stat[(size_t)m * 2], rstd = stat[(size_t)m * 2 + 1];
        const float* ar = add ? add + (size_t)(m % add_rows) * N : nullptr;
        float g[8], xh[8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = tid + i * 256;
            g[i] = xh[i] = 0.f;
            if (n < N) {
                const float d = dy[(size_t)m * N + n];
                xh[i] = (to_f<TX>(x[(size_t)m * N + n]) + (ar ? ar[n] : 0.f) - mean) * rstd;
                g[i] = d * gm[i];
                s1 += g[i];
                s2 = fmaf(g[i], xh[i], s2);
                dgam[i] = fmaf(d, xh[i], dgam[i]);
                dbet[i] += d;
            }
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        __syncthreads();
        if ((tid & 63) == 0) { r1[tid >> 6] = s1; r2[tid >> 6] = s2; }
        __syncthreads();
        if (tid == 0) { b1 = (r1[0] + r1[1] + r1[2] + r1[3]) / (float)N; b2 = (r2[0] + r2[1] + r2[2] + r2[3]) / (float)N; }
        __syncthreads();
        const float m1 = b1, m2 = b2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = tid + i * 256;
            if (n < N) dx[(size_t)m * N + n] = rstd * (g[i] - m1 - xh[i] * m2);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + i * 256;
        if (n < N) {
            partial[((size_t)blockIdx.x * 2 + 0) * N + n] = dgam[i];
            partial[((size_t)blockIdx.x * 2 + 1) * N + n] = dbet[i];
        }
    }
}
int ln_bwd_nblocks(int M) { return (M + kLnRows - 1) / kLnRows; }
hipError_t ln_bwd_launch(int x_dtype, const float* dy, const void* x, const float* add, int add_rows, const float* stat,
                         const float* gamma, float* dx, float* partial, float* dgamma, float* dbeta, int M, int N, hipStream_t s) {
    if (N > 2048) return hipErrorInvalidValue;
    const int nb = ln_bwd_nblocks(M);
    dispatch_dtype(x_dtype, [&](auto t) {
        using TX = typename decltype(t)::type;
        hipLaunchKernelGGL(ln_bwd_kernel<TX>, dim3(nb), dim3(256), 0, s, dy, (const TX*)x, add, add_rows, stat, gamma, dx, partial, M, N);
    });
    // dgamma / dbeta null (the data-only backward): the per-block partials are left unreduced
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && dgamma) e = colsum_launch(partial, nb, 2ll * N, N, dgamma, s);  // gn_kernels.h
    if (e == hipSuccess && dbeta) e = colsum_launch(partial + N, nb, 2ll * N, N, dbeta, s);
    return e;
}

// gelu_new and its derivative (transformers activations.py:59-66)
__device__ __forceinline__ float dgelu_new_f(float v) {
    const float k = 0.7978845608028654f, a = 0.044715f;
    const float t = tanhf(k * (v + a * v * v * v));
    return 0.5f * (1.0f + t) + 0.5f * v * (1.0f - t * t) * k * (1.0f + 3.0f * a * v * v);
}
// mode 0: dst = gelu_new(src);  mode 1: dst = src * gelu_new'(aux)
__global__ void __launch_bounds__(256) gelu_kernel(const float* __restrict__ src, const float* __restrict__ aux,
                                                   float* __restrict__ dst, long long n, int mode) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll)
        dst[i] = mode ? src[i] * dgelu_new_f(aux[i]) : gelu_new_f(src[i]);
}
hipError_t gelu_launch(const float* src, const float* aux, float* dst, long long n, int mode, hipStream_t s) {
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(gelu_kernel, dim3(blocks), dim3(256), 0, s, src, aux, dst, n, mode);
    return hipGetLastError();
}

// dst[c][r] = f(src[r][c]);  f = identity or gelu_new   (32x32 tiles through LDS)
__global__ void __launch_bounds__(256) transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C,
                                                        int act) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int j = ty; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + tx;
        float v = 0.f;
        if (r < R && c < C) { v = src[(size_t)r * C + c]; if (act) v = gelu_new_f(v); }
        tile[j][tx] = v;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + tx;
        if (r < R && c < C) dst[(size_t)c * R + r] = tile[tx][j];
    }
}
hipError_t transpose_launch(const float* src, float* dst, int R, int C, int act, hipStream_t s) {
    hipLaunchKernelGGL(transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, s, src, dst, R, C, act);
    return hipGetLastError();
}

template <typename T>
__global__ void __launch_bounds__(256) cast_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) dst[i] = to_f<T>(src[i]);
}
hipError_t cast_f32_launch(int dtype, const void* src, float* dst, long long n, hipStream_t s) {
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(cast_f32_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)src, dst, n);
    });
    return hipGetLastError();
}

}  // namespace ddimx
