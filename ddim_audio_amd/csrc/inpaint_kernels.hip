// Masked DDIM inpainting (ddim_audio_amd/inpaint.py): the element-wise arithmetic of one guided / replacement step.
//
// Both kernels read their scalars from the coefficient row of the device step counter (kInpaintStride floats:
// t, s1 = sqrt(1-at), s2 = sqrt(at), s3 = sqrt(at_next), c2, c1, k1 = -2 s1/s2, k2 = 2/s2, zeta), so one captured step replays
// for every iteration.  The grid is (blocks per sample, B): every block belongs to one sample, whose per_sample elements
// (a multiple of 4) it walks in float4s, grid-stride like ddim_update_kernel, whose arithmetic (step_math.h) both use.  The per-sample norm is reduced without atomics:
// the residual kernel writes one fp32 partial per (sample, block) and every block of the update kernel adds its sample's
// partials in the same fixed order, so results are bitwise reproducible and identical between eager and replayed steps.
#include "inpaint_kernels.h"

namespace ddimx {

__global__ void __launch_bounds__(kInpaintThreads) inpaint_residual_kernel(
    const float* __restrict__ xt, const float* __restrict__ et, const float* __restrict__ y, const float* __restrict__ m,
    float* __restrict__ x0, float* __restrict__ seed, float* __restrict__ partials, const float* __restrict__ coef,
    const int* __restrict__ step, long long n4) {
    __shared__ float red[kInpaintThreads / 64];
    const float* c = coef + (size_t)step[0] * kInpaintStride;
    const float s1 = c[1], s2 = c[2], k1 = c[6];
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInpaintThreads) {
        const size_t j = base + (size_t)i;
        const float4 x4 = ((const float4*)xt)[j], e4 = ((const float4*)et)[j];
        const float4 y4 = ((const float4*)y)[j], m4 = ((const float4*)m)[j];
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, es[4] = {e4.x, e4.y, e4.z, e4.w};
        const float ys[4] = {y4.x, y4.y, y4.z, y4.w}, ms[4] = {m4.x, m4.y, m4.z, m4.w};
        float p0[4], sd[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = ddim_x0(xs[k], es[k], s1, s2);
            const float r = inpaint_residual(v, ys[k], ms[k]);
            acc = fmaf(r, r, acc);
            p0[k] = v;
            sd[k] = inpaint_seed(r, ms[k], k1);
        }
        ((float4*)x0)[j] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        ((float4*)seed)[j] = make_float4(sd[0], sd[1], sd[2], sd[3]);
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

template <bool GUIDED, bool REPLACE>
__global__ void __launch_bounds__(kInpaintThreads) inpaint_update_kernel(
    float* __restrict__ xt, const float* __restrict__ et, const float* __restrict__ noise, float* __restrict__ x0,
    const float* __restrict__ y, const float* __restrict__ m, const float* __restrict__ dx, const float* __restrict__ partials,
    int nparts, const float* __restrict__ coef, const int* __restrict__ step, long long n4) {
    __shared__ float red[kInpaintThreads / 64];
    const float* c = coef + (size_t)step[0] * kInpaintStride;
    const float s1 = c[1], s2 = c[2], s3 = c[3], c2 = c[4], c1 = c[5], k2 = c[7], zeta = c[8];
    float w = 0.f;  // zeta / sqrt(L_b); 0 = no guidance term (L_b = 0 or zeta = 0)
    if (GUIDED) {
        // the sample's partials, in the same order in every block: thread i adds partials i, i + 256, ... (nparts <=
        // kInpaintMaxBlocks), then the block sum
        const float* ps = partials + (size_t)blockIdx.y * nparts;
        float v = 0.f;
        for (int p = threadIdx.x; p < nparts; p += kInpaintThreads) v += ps[p];
        const float L = block_sum(v, red);
        // in double, rounded once to fp32: the same value on every device and in a host replay of the arithmetic
        if (L > 0.f && zeta != 0.f) w = (float)((double)zeta / sqrt((double)L));
    }
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInpaintThreads) {
        const size_t j = base + (size_t)i;
        const float4 e4 = ((const float4*)et)[j];
        const float es[4] = {e4.x, e4.y, e4.z, e4.w};
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (noise) { const float4 z = ((const float4*)noise)[j]; nz[0] = z.x; nz[1] = z.y; nz[2] = z.z; nz[3] = z.w; }
        float ys[4] = {0.f, 0.f, 0.f, 0.f}, ms[4] = {0.f, 0.f, 0.f, 0.f};
        if (GUIDED || REPLACE) {
            const float4 y4 = ((const float4*)y)[j], m4 = ((const float4*)m)[j];
            ys[0] = y4.x; ys[1] = y4.y; ys[2] = y4.z; ys[3] = y4.w;
            ms[0] = m4.x; ms[1] = m4.y; ms[2] = m4.z; ms[3] = m4.w;
        }
        float p0[4];
        if (GUIDED) {
            const float4 v4 = ((const float4*)x0)[j];  // written by the residual kernel
            p0[0] = v4.x; p0[1] = v4.y; p0[2] = v4.z; p0[3] = v4.w;
        } else {
            const float4 x4 = ((const float4*)xt)[j];
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) p0[k] = ddim_x0(xs[k], es[k], s1, s2);
            ((float4*)x0)[j] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        }
        float gs[4] = {0.f, 0.f, 0.f, 0.f};
        if (GUIDED && w != 0.f) {
            const float4 d4 = ((const float4*)dx)[j];
            gs[0] = d4.x; gs[1] = d4.y; gs[2] = d4.z; gs[3] = d4.w;
        }
        float out[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float u = ddim_next(p0[k], es[k], s3, c2);
            if (noise) u = fmaf(nz[k], c1, u);
            // g = d L_b / d xt = k2 m^2 (x0 - y) + J_eps^T seed  (seed = k1 m^2 (x0 - y), d_x its data-only backward)
            if (GUIDED && w != 0.f) u = inpaint_guide(u, p0[k], ys[k], ms[k], gs[k], k2, w);
            if (REPLACE) {
                // the known content taken along the same deterministic DDIM path; exactly u where m = 0, exactly k where m = 1
                float kv = ddim_next(ys[k], es[k], s3, c2);
                if (noise) kv = fmaf(nz[k], c1, kv);
                u = inpaint_replace(u, kv, ms[k]);
            }
            out[k] = u;
        }
        ((float4*)xt)[j] = make_float4(out[0], out[1], out[2], out[3]);
    }
}

hipError_t inpaint_residual_launch(const float* xt, const float* et, const float* y, const float* m, float* x0, float* seed,
                                   float* partials, const float* coef, const int* step, int B, long long per_sample, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    const int nb = sample_blocks(B, per_sample, kInpaintMaxBlocks);
    hipLaunchKernelGGL(inpaint_residual_kernel, dim3(nb, B), dim3(kInpaintThreads), 0, s, xt, et, y, m, x0, seed, partials, coef,
                       step, per_sample / 4);
    return hipGetLastError();
}

hipError_t inpaint_update_launch(float* xt, const float* et, const float* noise, float* x0, const float* y, const float* m,
                                 const float* dx, const float* partials, const float* coef, const int* step, int B,
                                 long long per_sample, int flags, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4 || (flags & ~3)) return hipErrorInvalidValue;
    const int nb = sample_blocks(B, per_sample, kInpaintMaxBlocks);
    const long long n4 = per_sample / 4;
    const dim3 grid(nb, B), block(kInpaintThreads);
    switch (flags) {
        case 0: hipLaunchKernelGGL((inpaint_update_kernel<false, false>), grid, block, 0, s, xt, et, noise, x0, y, m, dx, partials,
                                   nb, coef, step, n4); break;
        case 1: hipLaunchKernelGGL((inpaint_update_kernel<false, true>), grid, block, 0, s, xt, et, noise, x0, y, m, dx, partials,
                                   nb, coef, step, n4); break;
        case 2: hipLaunchKernelGGL((inpaint_update_kernel<true, false>), grid, block, 0, s, xt, et, noise, x0, y, m, dx, partials,
                                   nb, coef, step, n4); break;
        default: hipLaunchKernelGGL((inpaint_update_kernel<true, true>), grid, block, 0, s, xt, et, noise, x0, y, m, dx, partials,
                                    nb, coef, step, n4); break;
    }
    return hipGetLastError();
}

}  // namespace ddimx
