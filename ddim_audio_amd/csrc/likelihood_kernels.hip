// Log-likelihood along the probability-flow ODE (ddim_audio_amd/likelihood.py; Song et al. 2021, appendix D.2, with the
// Skilling-Hutchinson trace estimator): the element-wise arithmetic of one network evaluation and its double-precision sums.
//
// include/features/lkx_likelihood.h has the row, the rounding contract and the probe.  All three walking kernels have the grid
// (lkx_blocks(per_sample), B): a block walks its sample's float4s grid-stride, so a thread's elements, the block's tree and the
// order in which the finishing thread adds the blocks depend on per_sample alone -- a sample's sums are the same bits in any
// batch.  Streaming kernels: 16-byte accesses, LDS for the block's four wave sums only, no scratch, no atomics, vector stores only.
// u is written only by a row that commits, k1 only by one that saves and read only where wk != 0: the branches are uniform over
// the launch (they come from the row), so a buffer a row does not need may be anything.
#include "likelihood_kernels.h"
#include "noise.h"

namespace ddimx {

__global__ void __launch_bounds__(kLkxThreads) lkx_probe_fill_kernel(float* __restrict__ r, long long n4, unsigned k0, unsigned k1,
                                                                     unsigned first_sample, unsigned probe) {
    const unsigned sample = first_sample + blockIdx.y;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kLkxThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kLkxThreads) {
        float v[4];
        probe_signs4((unsigned)i, sample, probe, k0, k1, v);
        store4(r, base + (size_t)i, v);
    }
}

__global__ void __launch_bounds__(kLkxThreads) lkx_stage_kernel(float* __restrict__ u, float* __restrict__ k1buf,
                                                                const float* __restrict__ e, const float* __restrict__ g,
                                                                float* __restrict__ xin, double* __restrict__ partial,
                                                                const float* __restrict__ coef, const int* __restrict__ step,
                                                                long long n4, unsigned k0, unsigned k1, unsigned first_sample,
                                                                unsigned probe) {
    __shared__ double red[4];
    const float* c = coef + (size_t)step[0] * kLkxStride;
    const float wk = c[1], we = c[2], an = c[3];
    const int flags = (int)c[5];
    const bool use_k = wk != 0.f, save = (flags & kLkxSave) != 0, commit = (flags & kLkxCommit) != 0;
    const unsigned sample = first_sample + blockIdx.y;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kLkxThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kLkxThreads) {
        const size_t at = base + (size_t)i;
        float r[4], uv[4], ev[4], gv[4], kv[4] = {0.f, 0.f, 0.f, 0.f}, xv[4];
        probe_signs4((unsigned)i, sample, probe, k0, k1, r);
        load4(u, at, uv);
        load4(e, at, ev);
        load4(g, at, gv);
        if (use_k) load4(k1buf, at, kv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float b = use_k ? fmaf(wk, kv[j], uv[j]) : uv[j];
            uv[j] = fmaf(we, ev[j], b);
            xv[j] = __fmul_rn(an, uv[j]);
            acc += (double)r[j] * (double)gv[j];  // r = +-1: the product is exact
        }
        store4(xin, at, xv);
        if (save) store4(k1buf, at, ev);
        if (commit) store4(u, at, uv);
    }
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

__global__ void __launch_bounds__(kLkxThreads) lkx_sumsq_part_kernel(const float* __restrict__ x, double* __restrict__ partial,
                                                                     long long n4) {
    __shared__ double red[4];
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kLkxThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kLkxThreads) {
        float v[4];
        load4(x, base + (size_t)i, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)v[j] * (double)v[j];  // 48 bits at most: the square is exact
    }
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// one thread per sample adds its sample's nb partials in block order
__global__ void __launch_bounds__(64) lkx_finish_kernel(const double* __restrict__ partial, double* __restrict__ acc,
                                                        const double* __restrict__ wd, const int* __restrict__ step, int B, int nb) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* p = partial + (size_t)b * nb;
    double s = p[0];
    for (int k = 1; k < nb; ++k) s += p[k];
    if (wd) {
#pragma clang fp contract(off)  // the product and the sum each rounded once (step_math.h: qsample_x has the reason for the pragma)
        const double term = wd[step[0]] * s;
        acc[b] = acc[b] + term;
    } else {
        acc[b] = s;
    }
}

static bool lkx_shape_ok(int B, long long per_sample) { return B >= 1 && B <= 65535 && per_sample > 0 && per_sample % 4 == 0; }
static bool lkx_probe_ok(int B, long long per_sample, unsigned first_sample) {
    return per_sample / 4 <= (1LL << 32) && (unsigned long long)first_sample + (unsigned long long)B <= (1ULL << 32);
}

hipError_t lkx_probe_fill_launch(float* r, int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned probe,
                                 hipStream_t s) {
    if (!lkx_shape_ok(B, per_sample) || !lkx_probe_ok(B, per_sample, first_sample)) return hipErrorInvalidValue;
    const dim3 grid(lkx_blocks(per_sample), B), block(kLkxThreads);
    hipLaunchKernelGGL(lkx_probe_fill_kernel, grid, block, 0, s, r, per_sample / 4, (unsigned)(seed & 0xffffffffULL),
                       (unsigned)(seed >> 32), first_sample, probe);
    return hipGetLastError();
}

hipError_t lkx_stage_launch(float* u, float* k1, const float* e, const float* g, float* xin, double* partial, const float* coef,
                            const int* step, int B, long long per_sample, unsigned long long seed, unsigned first_sample,
                            unsigned probe, hipStream_t s) {
    if (!lkx_shape_ok(B, per_sample) || !lkx_probe_ok(B, per_sample, first_sample)) return hipErrorInvalidValue;
    const dim3 grid(lkx_blocks(per_sample), B), block(kLkxThreads);
    hipLaunchKernelGGL(lkx_stage_kernel, grid, block, 0, s, u, k1, e, g, xin, partial, coef, step, per_sample / 4,
                       (unsigned)(seed & 0xffffffffULL), (unsigned)(seed >> 32), first_sample, probe);
    return hipGetLastError();
}

hipError_t lkx_finish_launch(const double* partial, double* acc, const double* wd, const int* step, int B, int nb, hipStream_t s) {
    if (B < 1 || B > 65535 || nb < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lkx_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, partial, acc, wd, step, B, nb);
    return hipGetLastError();
}

hipError_t lkx_sumsq_part_launch(const float* x, double* partial, int B, long long per_sample, hipStream_t s) {
    if (!lkx_shape_ok(B, per_sample)) return hipErrorInvalidValue;
    const dim3 grid(lkx_blocks(per_sample), B), block(kLkxThreads);
    hipLaunchKernelGGL(lkx_sumsq_part_kernel, grid, block, 0, s, x, partial, per_sample / 4);
    return hipGetLastError();
}

}  // namespace ddimx
