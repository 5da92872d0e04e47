// Tail of a training step around the network: q-sample, the squared-error loss and its gradient, EMA, and the multi-tensor
// gradient norm / clip / Adam kernels (functions/losses.py, models/ema.py, runners/diffusion.py:155-173).  gfx950 only.
// Every reduction is a fixed-order tree (no float atomics): results are reproducible.
#include "tail_kernels.h"
#include "step_math.h"

namespace ddimx {

// ---- q-sample (functions/losses.py:12-13): x = x0*sqrt(a_t) + e*sqrt(1-a_t), separate fp32 roundings ----
__global__ void __launch_bounds__(256) qsample_kernel(const float* __restrict__ x0, const float* __restrict__ e,
                                                      const float* __restrict__ alphas, const int64_t* __restrict__ t,
                                                      float* __restrict__ x, long long per) {
    const int b = blockIdx.y;
    const float a = alphas[t[b]];
    const float sa = __fsqrt_rn(a), sb = __fsqrt_rn(__fsub_rn(1.0f, a));
    const size_t base = (size_t)b * per;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long long)gridDim.x * 256)
        x[base + i] = qsample_x(x0[base + i], e[base + i], sa, sb);  // step_math.h: no contraction
}
hipError_t qsample_launch(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, int B,
                          long long per, hipStream_t s) {
    const int blocks = (int)((per + 255) / 256 < 1024 ? (per + 255) / 256 : 1024);
    hipLaunchKernelGGL(qsample_kernel, dim3(blocks, B), dim3(256), 0, s, x0, e, alphas, t, x, per);
    return hipGetLastError();
}

// ---- loss (functions/losses.py:15-18): per-sample sum of squared error, then batch mean --------------
int sqerr_nparts() { return kSqParts; }
__global__ void __launch_bounds__(256) sqerr_part_kernel(const float* __restrict__ e, const float* __restrict__ o,
                                                         float* __restrict__ partial, long long per) {
    sqerr_part_body([=](size_t at) { return e[at] - o[at]; }, partial, per);  // tail_kernels.h: the only copy of the reduction
}
__global__ void sqerr_final_kernel(const float* __restrict__ partial, float* __restrict__ loss, int B) {
    // one wave: loss[b] = sum of parts; loss[B] = mean over the batch
    sqerr_final_body([](int, float S) { return S; }, partial, loss, B);
}
hipError_t sqerr_part_launch(const float* e, const float* out, float* partial, int B, long long per, hipStream_t s) {
    hipLaunchKernelGGL(sqerr_part_kernel, dim3(kSqParts, B), dim3(256), 0, s, e, out, partial, per);
    return hipGetLastError();
}
hipError_t sqerr_launch(const float* e, const float* out, float* partial, float* loss_per, int B, long long per,
                        hipStream_t s) {
    sqerr_part_launch(e, out, partial, B, per, s);
    hipLaunchKernelGGL(sqerr_final_kernel, dim3(1), dim3(64), 0, s, partial, loss_per, B);
    return hipGetLastError();
}

// ---- EMA (models/ema.py:16-23): shadow = (1-mu)*p + mu*shadow over all tensors in one launch ----------
constexpr int kEmaBlock = 4096;
int ema_block_elems() { return kEmaBlock; }
__global__ void __launch_bounds__(256) ema_multi_kernel(const long long* __restrict__ shadow_ptrs,
                                                        const long long* __restrict__ param_ptrs,
                                                        const long long* __restrict__ sizes,
                                                        const int* __restrict__ blk_tensor,
                                                        const long long* __restrict__ blk_off, float c_p, float c_s) {
    const int ti = blk_tensor[blockIdx.x];
    float* sh = (float*)shadow_ptrs[ti];
    const float* p = (const float*)param_ptrs[ti];
    const long long n = sizes[ti], off = blk_off[blockIdx.x];
    for (int i = threadIdx.x; i < kEmaBlock; i += 256) {
        const long long k = off + i;
        if (k < n) sh[k] = __fadd_rn(__fmul_rn(c_p, p[k]), __fmul_rn(c_s, sh[k]));
    }
}
hipError_t ema_multi_launch(const long long* shadow_ptrs, const long long* param_ptrs, const long long* sizes,
                            const int* blk_tensor, const long long* blk_off, int nblocks, float c_p, float c_s, hipStream_t s) {
    hipLaunchKernelGGL(ema_multi_kernel, dim3(nblocks), dim3(256), 0, s, shadow_ptrs, param_ptrs, sizes, blk_tensor,
                       blk_off, c_p, c_s);
    return hipGetLastError();
}


// =====================================================================================================
// training-step tail (runners/diffusion.py:155-173): multi-tensor kernels over pointer tables, one launch each
// =====================================================================================================
// sum of squares of all gradient tensors: per-block partials (fixed order) then one block finishes:
// out[0] = total L2 norm, out[1] = clip coefficient min(1, max_norm / (norm + 1e-6))  (torch clip_grad_norm_)
__global__ void __launch_bounds__(256) sqnorm_multi_kernel(const long long* __restrict__ ptrs, const long long* __restrict__ sizes,
                                                           const int* __restrict__ blk_tensor, const long long* __restrict__ blk_off,
                                                           float* __restrict__ partial) {
    __shared__ float red[4];
    const int ti = blk_tensor[blockIdx.x];
    const float* g = (const float*)ptrs[ti];
    const long long n = sizes[ti], off = blk_off[blockIdx.x];
    float s = 0.f;
    for (int i = threadIdx.x; i < kEmaBlock; i += 256) {
        const long long k = off + i;
        if (k < n) s = fmaf(g[k], g[k], s);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void __launch_bounds__(256) sqnorm_final_kernel(const float* __restrict__ partial, int n, float max_norm,
                                                           float* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
        const float coef = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = coef < 1.0f ? coef : 1.0f;
    }
}
hipError_t grad_norm_multi_launch(const long long* ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                                  int nblocks, float max_norm, float* partial, float* out, hipStream_t s) {
    hipLaunchKernelGGL(sqnorm_multi_kernel, dim3(nblocks), dim3(256), 0, s, ptrs, sizes, blk_tensor, blk_off, partial);
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, s, partial, nblocks, max_norm, out);
    return hipGetLastError();
}

// decoupled = 2: AdaBelief (Zhuang et al. 2020, weight_decouple, no rectification, no amsgrad): v <- b2 v + (1-b2)(g-m)^2 + eps.
// g' = g * coef[1] in registers (the clip coefficient stays on the device: no host sync), then Adam / AdamW (torch semantics,
// amsgrad off): decoupled: p *= 1 - lr*wd ; else g += wd*p.  m = m + (1-b1)(g - m); v = b2*v + (1-b2) g*g;
// p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  bc1 = 1 - b1^t, bc2s = sqrt(1 - b2^t) from the host.
__global__ void __launch_bounds__(256) adam_multi_kernel(const AdamArgs a) {
    const int ti = a.blk_tensor[blockIdx.x];
    float* p = (float*)a.p[ti];
    const float* g = (const float*)a.g[ti];  // never written: torch.optim leaves p.grad alone (clip / L2 terms stay in registers)
    float* m = (float*)a.m[ti];
    float* v = (float*)a.v[ti];
    const long long n = a.sizes[ti], off = a.blk_off[blockIdx.x];
    const float cc = a.clip ? a.clip[1] : 1.0f;
    const float lr = a.dyn ? a.dyn[0] : a.lr, bc1 = a.dyn ? a.dyn[1] : a.bc1, bc2s = a.dyn ? a.dyn[2] : a.bc2s;
    const float step_size = lr / bc1;
    for (int i = threadIdx.x; i < kEmaBlock; i += 256) {
        const long long k = off + i;
        if (k >= n) continue;
        float gk = __fmul_rn(g[k], cc);
        float pk = p[k];
        if (a.decoupled) pk = __fmul_rn(pk, 1.0f - lr * a.wd);
        else gk = fmaf(a.wd, pk, gk);
        const float mk = fmaf(1.0f - a.b1, __fsub_rn(gk, m[k]), m[k]);
        float vk;
        if (a.decoupled == 2) {  // AdaBelief: the second moment follows (g - m)^2 and absorbs eps every step
            const float r = __fsub_rn(gk, mk);
            vk = __fadd_rn(fmaf(__fmul_rn(r, r), 1.0f - a.b2, __fmul_rn(v[k], a.b2)), a.eps);
        } else {
            vk = fmaf(__fmul_rn(gk, gk), 1.0f - a.b2, __fmul_rn(v[k], a.b2));
        }
        const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vk), bc2s), a.eps);
        pk = fmaf(-step_size, __fdiv_rn(mk, denom), pk);
        m[k] = mk; v[k] = vk; p[k] = pk;
    }
}
__global__ void __launch_bounds__(256) scale_multi_kernel(const long long* __restrict__ ptrs, const long long* __restrict__ sizes,
                                                          const int* __restrict__ blk_tensor, const long long* __restrict__ blk_off,
                                                          const float* __restrict__ coef) {
    const int ti = blk_tensor[blockIdx.x];
    float* g = (float*)ptrs[ti];
    const long long n = sizes[ti], off = blk_off[blockIdx.x];
    const float c = coef[0];
    if (c == 1.0f) return;  // torch multiplies by the clamped coefficient; x * 1.0f is the identity
    for (int i = threadIdx.x; i < kEmaBlock; i += 256) {
        const long long k = off + i;
        if (k < n) g[k] = __fmul_rn(g[k], c);
    }
}
hipError_t scale_multi_launch(const long long* ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                              int nblocks, const float* coef, hipStream_t s) {
    hipLaunchKernelGGL(scale_multi_kernel, dim3(nblocks), dim3(256), 0, s, ptrs, sizes, blk_tensor, blk_off, coef);
    return hipGetLastError();
}
hipError_t adam_multi_launch(const AdamArgs& a, int nblocks, hipStream_t s) {
    hipLaunchKernelGGL(adam_multi_kernel, dim3(nblocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// d(out)[b] = 2 * g[b] * (out[b] - e[b])   (functions/losses.py:18: per-sample sum of squares; g = upstream gradient per sample)
// with_mean: g has B + 1 entries, the last one the upstream gradient of the batch MEAN (the loss vector's [B] entry): + g[B] / B per sample
__global__ void __launch_bounds__(256) sqerr_bwd_kernel(const float* __restrict__ e, const float* __restrict__ o,
                                                        const float* __restrict__ g, float* __restrict__ d, long long per, int with_mean) {
    const int b = blockIdx.y;
    const float c = sqerr_bwd_c0(g, b, gridDim.y, with_mean);
    const size_t base = (size_t)b * per;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < per; i += gridDim.x * 256ll) d[base + i] = c * (o[base + i] - e[base + i]);
}
hipError_t sqerr_bwd_launch(const float* e, const float* out, const float* g, float* d, int B, long long per, hipStream_t s, int with_mean) {
    const int blocks = sqerr_bwd_blocks(per);
    hipLaunchKernelGGL(sqerr_bwd_kernel, dim3(blocks, B), dim3(256), 0, s, e, out, g, d, per, with_mean);
    return hipGetLastError();
}

}  // namespace ddimx
