// Masked DDIM inpainting (ddim_audio_amd/inpaint.py): the element-wise arithmetic of one guided / replacement step.
//
// Both kernels read their scalars from the coefficient row of the device step counter (kInpaintStride floats:
// t, s1 = sqrt(1-at), s2 = sqrt(at), s3 = sqrt(at_next), c2, c1, k1 = -2 s1/s2, k2 = 2/s2, zeta), so one captured step replays
// for every iteration; the residual kernel takes the row's stride, because the multistep sampler (inpaint_solver_kernels.hip)
// runs it on its wider row, whose first nine floats are these.  The grid is (blocks per sample, B): every block belongs to
// one sample, whose per_sample elements (a multiple of 4) it walks in float4s, grid-stride like ddim_update_kernel.  The
// arithmetic is inpaint_kernels.h's device
// functions, shared with the canvas kernels of window_inpaint_kernels.hip.  The per-sample norm is reduced without atomics:
// the residual kernel writes one fp32 partial per (sample, block) and every block of the update kernel adds its sample's
// partials in the same fixed order, so results are bitwise reproducible and identical between eager and replayed steps.
#include "inpaint_kernels.h"

namespace ddimx {

__global__ void __launch_bounds__(kInpaintThreads) inpaint_residual_kernel(
    const float* __restrict__ xt, const float* __restrict__ et, const float* __restrict__ y, const float* __restrict__ m,
    float* __restrict__ x0, float* __restrict__ seed, float* __restrict__ partials, const float* __restrict__ coef,
    const int* __restrict__ step, long long n4, int stride) {
    __shared__ float red[kInpaintThreads / 64];
    const InpaintRow c = load_inpaint_row(coef, step, stride);
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInpaintThreads) {
        const size_t at = base + (size_t)i;
        float xs[4], es[4], ys[4], ms[4], p0[4], sd[4];
        load4(xt, at, xs);
        load4(et, at, es);
        load4(y, at, ys);
        load4(m, at, ms);
        inpaint_residual4(xs, es, ys, ms, c, p0, sd, acc);
        store4(x0, at, p0);
        store4(seed, at, sd);
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
    const InpaintRow c = load_inpaint_row(coef, step);
    const float w = GUIDED ? inpaint_weight(partials + (size_t)blockIdx.y * nparts, nparts, c.zeta, red) : 0.f;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInpaintThreads) {
        const size_t at = base + (size_t)i;
        float es[4], p0[4], gs[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f};
        float ys[4] = {0.f, 0.f, 0.f, 0.f}, ms[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
        load4(et, at, es);
        if (noise) load4(noise, at, nz);
        if (GUIDED || REPLACE) {
            load4(y, at, ys);
            load4(m, at, ms);
        }
        if (GUIDED) {
            load4(x0, at, p0);  // written by the residual kernel
            if (w != 0.f) load4(dx, at, gs);  // the data-only backward of the seeds
        } else {
            float xs[4];
            load4(xt, at, xs);
#pragma unroll
            for (int q = 0; q < 4; ++q) p0[q] = ddim_x0(xs[q], es[q], c.s1, c.s2);
            store4(x0, at, p0);
        }
        inpaint_update4<GUIDED, REPLACE>(p0, es, ys, ms, gs, nz, noise != nullptr, w, c, out);
        store4(xt, at, out);
    }
}

hipError_t inpaint_residual_launch(const float* xt, const float* et, const float* y, const float* m, float* x0, float* seed,
                                   float* partials, const float* coef, const int* step, int B, long long per_sample, hipStream_t s,
                                   int stride) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    if (stride != kInpaintStride && stride != kInpaintSolverStride) return hipErrorInvalidValue;
    const int nb = sample_blocks(B, per_sample, kInpaintMaxBlocks);
    hipLaunchKernelGGL(inpaint_residual_kernel, dim3(nb, B), dim3(kInpaintThreads), 0, s, xt, et, y, m, x0, seed, partials, coef,
                       step, per_sample / 4, stride);
    return hipGetLastError();
}

hipError_t inpaint_update_launch(float* xt, const float* et, const float* noise, float* x0, const float* y, const float* m,
                                 const float* dx, const float* partials, const float* coef, const int* step, int B,
                                 long long per_sample, int flags, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4 || (flags & ~3)) return hipErrorInvalidValue;
    const int nb = sample_blocks(B, per_sample, kInpaintMaxBlocks);
    dispatch_inpaint_flags(flags, [&](auto guided, auto replace) {
        hipLaunchKernelGGL((inpaint_update_kernel<decltype(guided)::value, decltype(replace)::value>), dim3(nb, B), dim3(kInpaintThreads), 0,
                           s, xt, et, noise, x0, y, m, dx, partials, nb, coef, step, per_sample / 4);
    });
    return hipGetLastError();
}

}  // namespace ddimx
