// Launch wrappers of the masked-inpainting sampler kernels (inpaint_kernels.hip) and the one copy of a step's arithmetic on
// registers.  Same rules as step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include <type_traits>
#include "step_math.h"

namespace ddimx {

// coefficient rows of the inpainting sampler: (t, s1, s2, s3, c2, c1, k1, k2, zeta) fp32, indexed by the device step counter
constexpr int kInpaintStride = 9;
constexpr int kInpaintThreads = kSampleThreads;  // block_sum
// blocks per sample of both kernels (= partials per sample), sample_blocks(B, per_sample, kInpaintMaxBlocks): each update thread
// adds at most 4 partials (in a fixed order)
constexpr int kInpaintMaxBlocks = 1024;
static_assert(kInpaintThreads == 256, "block_sum reduces exactly 4 waves of 64");
static_assert(kInpaintMaxBlocks <= 4 * kInpaintThreads, "the update kernel adds at most 4 partials per thread");

// ---- the arithmetic of one step, shared with the canvas kernels (window_inpaint_kernels.hip): a kernel keeps only where its
// eps, x0 and d come from, so "one window == inpaint_steps" holds by construction (step_math.h: the rounding contract)
struct InpaintRow { float s1, s2, s3, c2, c1, k1, k2, zeta; };
// `stride`: the floats per row of the table, whose first kInpaintStride are the row above (the multistep table is wider)
__device__ __forceinline__ InpaintRow load_inpaint_row(const float* __restrict__ coef, const int* __restrict__ step,
                                                       int stride = kInpaintStride) {
    const float* c = coef + (size_t)step[0] * stride;
    return {c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
}
// coefficient rows of the multistep inpainting sampler (inpaint_solver_kernels.hip): the row above, its zeta the guidance scale
// rho of the folded form, then (cx, w0, w1, w2) -- schedule.inpaint_solver_coefficients
constexpr int kInpaintSolverStride = 13;
struct InpaintSolverRow { InpaintRow r; float cx, w0, w1, w2; };
__device__ __forceinline__ InpaintSolverRow load_inpaint_solver_row(const float* __restrict__ coef, int pos) {
    const float* c = coef + (size_t)pos * kInpaintSolverStride;
    return {{c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]}, c[9], c[10], c[11], c[12]};
}
// The guidance weight zeta / sqrt(L) of the sample whose nparts (<= kInpaintMaxBlocks) partials start at ps; 0 = no guidance term
// (L = 0 or zeta = 0).  The same order in every block: thread i adds partials i, i + 256, ..., then the block sum.  The quotient
// is taken in double and rounded once to fp32: the same value on every device and in a host replay of the arithmetic.
__device__ __forceinline__ float inpaint_weight(const float* __restrict__ ps, int nparts, float zeta, float* red) {
    float v = 0.f;
    for (int p = threadIdx.x; p < nparts; p += kInpaintThreads) v += ps[p];
    const float L = block_sum(v, red);
    return L > 0.f && zeta != 0.f ? (float)((double)zeta / sqrt((double)L)) : 0.f;
}
// four elements of the residual pass: x0, the seed of the data-only backward, and r^2 added to the thread's partial
__device__ __forceinline__ void inpaint_residual4(const float x[4], const float e[4], const float y[4], const float m[4],
                                                  const InpaintRow& c, float x0[4], float sd[4], float& acc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        x0[q] = ddim_x0(x[q], e[q], c.s1, c.s2);
        const float r = inpaint_residual(x0[q], y[q], m[q]);
        acc = fmaf(r, r, acc);
        sd[q] = inpaint_seed(r, m[q], c.k1);
    }
}
// four elements of the update behind x0: the DDIM step (+ c1 z where add_z), the guidance term where w != 0 -- g = d L / d x =
// k2 m^2 (x0 - y) + d, d the data-only backward of the seeds -- and the replacement: the known content taken along the same DDIM
// path, exactly u where m = 0 and exactly kv where m = 1.  A term that is off is not applied at all.
template <bool GUIDED, bool REPLACE>
__device__ __forceinline__ void inpaint_update4(const float x0[4], const float e[4], const float y[4], const float m[4], const float d[4],
                                                const float z[4], bool add_z, float w, const InpaintRow& c, float out[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float u = ddim_next(x0[q], e[q], c.s3, c.c2);
        if (add_z) u = fmaf(z[q], c.c1, u);
        if (GUIDED && w != 0.f) u = inpaint_guide(u, x0[q], y[q], m[q], d[q], c.k2, w);
        if (REPLACE) {
            float kv = ddim_next(y[q], e[q], c.s3, c.c2);
            if (add_z) kv = fmaf(z[q], c.c1, kv);
            u = inpaint_replace(u, kv, m[q]);
        }
        out[q] = u;
    }
}
// four elements of the multistep update (inpaint_solver_kernels.hip, and on the canvas window_inpaint_kernels.hip) behind m0 = p0:
// the guided prediction mt -- the network's, moved down the gradient of the sample's masked residual norm where w != 0 --, the
// DDIM step, the fold and history terms on mt, the noise, and the known region on its exact path kv = cx x + w0 y (+ c1 z).  The
// operation order is include/ddimx_inpaint_solver.h's; a term that is off is not applied and its operand may hold anything.
template <bool GUIDED, bool REPLACE>
__device__ __forceinline__ void inpaint_multistep4(const float x[4], const float e[4], const float p0[4], const float y[4],
                                                   const float m[4], const float d[4], const float z[4], const float m1[4],
                                                   const float m2[4], float w, bool use1, bool use2, bool add_z,
                                                   const InpaintSolverRow& c, float mt[4], float out[4]) {
    const bool fold = GUIDED && w != 0.f, use_x = c.cx != 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mt[q] = fold ? inpaint_guide(p0[q], p0[q], y[q], m[q], d[q], c.r.k2, w) : p0[q];
        float u = ddim_next(p0[q], e[q], c.r.s3, c.r.c2);
        if (fold) u = fmaf(c.w0, __fsub_rn(mt[q], p0[q]), u);
        if (use1) u = fmaf(c.w1, __fsub_rn(mt[q], m1[q]), u);
        if (use2) u = fmaf(c.w2, __fsub_rn(m1[q], m2[q]), u);
        if (add_z) u = fmaf(z[q], c.r.c1, u);
        if (REPLACE) {
            float kv = inpaint_known(x[q], y[q], c.cx, c.w0, use_x);
            if (add_z) kv = fmaf(z[q], c.r.c1, kv);
            u = inpaint_replace(u, kv, m[q]);
        }
        out[q] = u;
    }
}
// fn(guided, replace) as std::bool_constant for flags (1 = replace, 2 = guided): the launch of an update kernel<..., GUIDED, REPLACE>
template <class Fn>
void dispatch_inpaint_flags(int flags, Fn&& fn) {
    switch (flags & 3) {
        case 0: fn(std::false_type{}, std::false_type{}); break;
        case 1: fn(std::false_type{}, std::true_type{}); break;
        case 2: fn(std::true_type{}, std::false_type{}); break;
        default: fn(std::true_type{}, std::true_type{});
    }
}

// guided path: x0 = (xt - s1 eps) / s2, seed = k1 m^2 (x0 - y), partials[b][blk] = sum of (m (x0 - y))^2 over the block's elements;
// stride: kInpaintStride, or kInpaintSolverStride for the multistep sampler's table (the same kernel on the wider row)
hipError_t inpaint_residual_launch(const float* xt, const float* et, const float* y, const float* m, float* x0, float* seed,
                                   float* partials, const float* coef, const int* step, int B, long long per_sample, hipStream_t s,
                                   int stride = kInpaintStride);
// the DDIM update (+ guidance term, + replacement), in place on xt; flags: 1 = replace, 2 = guided (x0 read, not computed)
hipError_t inpaint_update_launch(float* xt, const float* et, const float* noise, float* x0, const float* y, const float* m,
                                 const float* dx, const float* partials, const float* coef, const int* step, int B,
                                 long long per_sample, int flags, hipStream_t s);

}  // namespace ddimx
