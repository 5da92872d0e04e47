// Multistep (DPM-Solver++) inpainting (ddim_audio_amd/inpaint_solver.py): the element-wise arithmetic of one step, orders 1-3,
// with a mask, reconstruction guidance folded into the data prediction and the known region on its own exact path.
//
// The scalars come from row step[0] of the table (kInpaintSolverStride floats: t, s1, s2, s3, c2, c1, k1, k2, rho, cx, w0, w1, w2 --
// schedule.inpaint_solver_coefficients), so one captured step replays for every iteration; the order of an iteration, whether it
// adds noise and whether it is guided live in the table.  The layout is inpaint_update_kernel's: the grid is (blocks per sample,
// B), every block belongs to one sample, whose per_sample elements (a multiple of 4) it walks in float4s, grid-stride; every
// block adds its sample's partials (the residual pass's, one per block) in the same fixed order, so results are bitwise
// reproducible and identical between eager and replayed steps.  The scalar operations are step_math.h's, the weight is
// inpaint_weight (inpaint_kernels.h); the operation order is written out in include/ddimx_inpaint_solver.h.  The noise is
// sde_multistep_update_kernel's: noise[i] when the caller hands a buffer, else noise_normals4 (noise.h) for the counter (group of
// four, first_sample + b, draw_base + step[0], tag 0).  No atomics, vector stores only; a sample's result depends on its own
// elements, (seed, its global index) and on nothing else of the batch.
//
// Memory-bound: per element a guided order-3 step with replacement reads xt, eps, x0, y, mask, d_x, h1, h2 (+ noise when handed)
// and writes xt, h1, h2; a buffer whose term is off in the row is not touched.
#include "inpaint_solver_kernels.h"
#include "noise.h"

namespace ddimx {

constexpr unsigned kInpaintSolverTagStep = 0u;  // noise.py TAG_STEP: the noise a sampler step adds

template <bool GUIDED, bool REPLACE>
__global__ void __launch_bounds__(kInpaintThreads) inpaint_multistep_update_kernel(
    float* __restrict__ xt, const float* __restrict__ et, const float* __restrict__ noise, float* __restrict__ x0, float* __restrict__ h1,
    float* __restrict__ h2, const float* __restrict__ y, const float* __restrict__ m, const float* __restrict__ dx,
    const float* __restrict__ partials, int nparts, const float* __restrict__ coef, const int* __restrict__ step, long long n4,
    unsigned k0, unsigned k1, unsigned first_sample, unsigned draw_base) {
    __shared__ float red[kInpaintThreads / 64];
    const int pos = step[0];
    const InpaintSolverRow c = load_inpaint_solver_row(coef, pos);
    const float w = GUIDED ? inpaint_weight(partials + (size_t)blockIdx.y * nparts, nparts, c.r.zeta, red) : 0.f;
    const bool fold = GUIDED && w != 0.f;
    const bool use1 = c.w1 != 0.f, use2 = c.w2 != 0.f && h2 != nullptr, load1 = use1 || use2, add_z = c.r.c1 != 0.f;
    const bool load_z = add_z && noise != nullptr, draw_z = add_z && noise == nullptr;
    const unsigned sample = first_sample + blockIdx.y, draw = draw_base + (unsigned)pos;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kInpaintThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInpaintThreads) {
        const size_t at = base + (size_t)i;
        float xs[4] = {0.f, 0.f, 0.f, 0.f}, es[4], p0[4], gs[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        float ys[4] = {0.f, 0.f, 0.f, 0.f}, ms[4] = {0.f, 0.f, 0.f, 0.f}, m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
        float mt[4], out[4];
        load4(et, at, es);
        if (!GUIDED || REPLACE) load4(xt, at, xs);
        if (load_z) load4(noise, at, z);
        if (draw_z) noise_normals4((unsigned)i, sample, draw, kInpaintSolverTagStep, k0, k1, z);
        if (GUIDED || REPLACE) {
            load4(y, at, ys);
            load4(m, at, ms);
        }
        if (GUIDED) {
            load4(x0, at, p0);  // written by the residual pass
            if (fold) load4(dx, at, gs);  // the data-only backward of the seeds
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) p0[q] = ddim_x0(xs[q], es[q], c.r.s1, c.r.s2);
            store4(x0, at, p0);
        }
        if (load1) load4(h1, at, m1);
        if (use2) load4(h2, at, m2);
        inpaint_multistep4<GUIDED, REPLACE>(xs, es, p0, ys, ms, gs, z, m1, m2, w, use1, use2, add_z, c, mt, out);
        if (h2 && load1) store4(h2, at, m1);
        store4(h1, at, mt);
        store4(xt, at, out);
    }
}

hipError_t inpaint_multistep_update_launch(float* xt, const float* et, const float* noise, float* x0, float* h1, float* h2,
                                           const float* y, const float* m, const float* dx, const float* partials, const float* coef,
                                           const int* step, int B, long long per_sample, int flags, unsigned long long seed,
                                           unsigned first_sample, unsigned draw_base, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4 || (flags & ~3)) return hipErrorInvalidValue;
    const long long n4 = per_sample / 4;
    if (n4 > (1LL << 32) || (unsigned long long)first_sample + (unsigned long long)B > (1ULL << 32)) return hipErrorInvalidValue;
    const int nb = sample_blocks(B, per_sample, kInpaintMaxBlocks);  // = the residual pass's: one partial per block
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    dispatch_inpaint_flags(flags, [&](auto guided, auto replace) {
        hipLaunchKernelGGL((inpaint_multistep_update_kernel<decltype(guided)::value, decltype(replace)::value>), dim3(nb, B),
                           dim3(kInpaintThreads), 0, s, xt, et, noise, x0, h1, h2, y, m, dx, partials, nb, coef, step, n4, k0, k1,
                           first_sample, draw_base);
    });
    return hipGetLastError();
}

}  // namespace ddimx
