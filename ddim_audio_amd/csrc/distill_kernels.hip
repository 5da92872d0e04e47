// SNR loss weighting and the target of progressive distillation (Salimans & Ho 2022; min-SNR: Hang et al. 2023); at the end of the
// file, the training kernels of consistency distillation (Song et al. 2023).  gfx950 only.
//
// Weighted loss.  The per-sample sum of squares is ddimx_sqerr_loss's, bit for bit: the same first launch (sqerr_part_launch,
// tail_kernels.hip) writes the same parts, and one wave sums them as sqerr_final_kernel does.  The weight is row t[b] of a table --
// t is the int64 timestep tensor the network was given, device memory read when the launch RUNS, so one captured launch serves
// every replay of a graphed training step.  A t[b] outside the table reads no row and weighs the sample with NaN.  Every
// reduction is in a fixed order (no float atomics); with a table of ones both kernels give the unweighted kernels' bits
// (rn(1 v) = v).
//
// Distillation target.  A student learns to do in ONE DDIM step t -> t'' what its teacher does in two, t -> t' -> t''.  With m0
// the teacher's x0 prediction at (z, t) and m1 the one at (z', t'), z' = alpha' m0 + sigma' eps0, the x0 target whose single step
// lands on the teacher's z'' is the convex combination x = m1 + omega (m0 - m1) (omega in [0, 0.5), from the host in the row):
// the direct form (z'' - r z) / (alpha'' - r alpha) cancels in its denominator for short steps and is never evaluated; z'' is
// never materialised.  Two kernels, one on each side of the teacher's second forward; both read z and leave it alone (the
// student reads it too).  Their grids are (blocks per sample, B) like vpred_kernels.hip's: every block belongs to one sample, whose
// float4s it walks grid-stride.  No LDS, no atomics, vector stores only; every element is read before it is written by the
// same thread, so target may alias m0; a sample's result does not depend on B or on the grid.
#include "distill_kernels.h"

namespace ddimx {

__device__ __forceinline__ float table_weight(const float* __restrict__ wtab, int n_table, int64_t tb) {
    return (tb < 0 || tb >= (int64_t)n_table) ? __int_as_float(0x7FC00000) : wtab[tb];
}

__global__ void sqerr_w_final_kernel(const float* __restrict__ partial, const float* __restrict__ wtab, int n_table,
                                     const int64_t* __restrict__ t, float* __restrict__ loss, int B) {
    // one wave, as sqerr_final_kernel: loss[b] = w * (sum of parts); loss[B] = mean of the weighted values over the batch.
    // contract(off), here and in sqerr_final_body: the sum takes the ROUNDED products loss[b] (to this compiler __fmul_rn is a
    // plain operator, and w * S + tot would become one fma)
    sqerr_final_body([=](int b, float S) {
#pragma clang fp contract(off)
        const float v = table_weight(wtab, n_table, t[b]) * S;
        return v;
    }, partial, loss, B);
}

__global__ void __launch_bounds__(256) sqerr_w_bwd_kernel(const float* __restrict__ e, const float* __restrict__ o,
                                                          const float* __restrict__ g, const float* __restrict__ wtab, int n_table,
                                                          const int64_t* __restrict__ t, float* __restrict__ d, long long per) {
    const int b = blockIdx.y;
    const float c = __fmul_rn(table_weight(wtab, n_table, t[b]), sqerr_bwd_c0(g, b, gridDim.y, 1));
    const size_t base = (size_t)b * per;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < per; i += gridDim.x * 256ll) d[base + i] = c * (o[base + i] - e[base + i]);
}

hipError_t sqerr_w_launch(const float* target, const float* out, const float* wtab, int n_table, const int64_t* t, float* partial,
                          float* loss, int B, long long per, hipStream_t s) {
    sqerr_part_launch(target, out, partial, B, per, s);
    hipLaunchKernelGGL(sqerr_w_final_kernel, dim3(1), dim3(64), 0, s, partial, wtab, n_table, t, loss, B);
    return hipGetLastError();
}

hipError_t sqerr_w_bwd_launch(const float* target, const float* out, const float* g, const float* wtab, int n_table, const int64_t* t,
                              float* d, int B, long long per, hipStream_t s) {
    hipLaunchKernelGGL(sqerr_w_bwd_kernel, dim3(sqerr_bwd_blocks(per), B), dim3(256), 0, s, target, out, g, wtab, n_table, t, d, per);
    return hipGetLastError();
}

__global__ void __launch_bounds__(kDistillThreads) distill_half_kernel(const float* __restrict__ z, const float* __restrict__ eps0,
                                                                       const float* __restrict__ rows, float* __restrict__ zmid,
                                                                       float* __restrict__ m0, long long n4) {
    const int b = blockIdx.y;
    const float* c = rows + (size_t)b * kDistillStride;
    const float s1 = c[1], s2 = c[2], s3 = c[3], c2 = c[4];
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kDistillThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kDistillThreads) {
        const size_t at = base + (size_t)i;
        const float4 x = ((const float4*)z)[at];
        const float4 e = ((const float4*)eps0)[at];
        const float xs[4] = {x.x, x.y, x.z, x.w}, es[4] = {e.x, e.y, e.z, e.w};
        float p0[4], zm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p0[j] = ddim_x0(xs[j], es[j], s1, s2);  // step_math.h: ddim_update_kernel's x0 prediction and x_{t'}
            zm[j] = ddim_next(p0[j], es[j], s3, c2);
        }
        ((float4*)m0)[at] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        ((float4*)zmid)[at] = make_float4(zm[0], zm[1], zm[2], zm[3]);
    }
}

__global__ void __launch_bounds__(kDistillThreads) distill_target_kernel(const float* __restrict__ z, const float* __restrict__ zmid,
                                                                         const float* __restrict__ eps1, const float* m0,
                                                                         const float* __restrict__ rows, float* target,
                                                                         float* __restrict__ x0_target, long long n4) {
    const int b = blockIdx.y;
    const float* c = rows + (size_t)b * kDistillStride;
    const float s1 = c[6], s2 = c[7], omega = c[8], cz = c[9], cx = c[10];
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kDistillThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kDistillThreads) {
        const size_t at = base + (size_t)i;
        const float4 x = ((const float4*)z)[at];
        const float4 y = ((const float4*)zmid)[at];
        const float4 e = ((const float4*)eps1)[at];
        const float4 p = ((const float4*)m0)[at];
        const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w}, es[4] = {e.x, e.y, e.z, e.w}, ps[4] = {p.x, p.y, p.z, p.w};
        float xt[4], tg[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m1 = ddim_x0(ys[j], es[j], s1, s2);
            xt[j] = fmaf(omega, __fsub_rn(ps[j], m1), m1);
            tg[j] = fmaf(xt[j], cx, __fmul_rn(xs[j], cz));
        }
        if (x0_target) ((float4*)x0_target)[at] = make_float4(xt[0], xt[1], xt[2], xt[3]);
        ((float4*)target)[at] = make_float4(tg[0], tg[1], tg[2], tg[3]);
    }
}

static bool distill_shape_ok(int B, long long per_sample) { return B >= 1 && B <= 65535 && per_sample > 0 && per_sample % 4 == 0; }

hipError_t distill_half_launch(const float* z, const float* eps0, const float* rows, float* zmid, float* m0, int B, long long per_sample,
                               hipStream_t s) {
    if (!distill_shape_ok(B, per_sample)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kDistillThreads);
    hipLaunchKernelGGL(distill_half_kernel, grid, block, 0, s, z, eps0, rows, zmid, m0, per_sample / 4);
    return hipGetLastError();
}

hipError_t distill_target_launch(const float* z, const float* zmid, const float* eps1, const float* m0, const float* rows, float* target,
                                 float* x0_target, int B, long long per_sample, hipStream_t s) {
    if (!distill_shape_ok(B, per_sample)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kDistillThreads);
    hipLaunchKernelGGL(distill_target_kernel, grid, block, 0, s, z, zmid, eps1, m0, rows, target, x0_target, per_sample / 4);
    return hipGetLastError();
}

// ---- consistency distillation (Song et al. 2023, Luo et al. 2023; ddim_audio_amd/consistency.py, include/cmx_consistency.h)
// The consistency function is f = p x + q out with (p, q) row t[b] of a table (schedule.consistency_table), read when the launch
// runs; a t[b] outside the table reads no row and gives NaN.  f = consistency_f (step_math.h): fma(q, out, rn(p x)).  The loss
// never materialises f: its first stage is sqerr_part_body on y - f, so a table of (0, 1) rows gives ddimx_sqerr_loss's parts,
// and its second stage sqerr_final_body on the distance of the sample's sum.  Scalar loads in the loss (the summation order is
// the squared-error loss's), float4 walks on a (blocks per sample, B) grid elsewhere; every element is read before the same
// thread writes it, so f may alias out.
struct CmRow { float p, q; };
__device__ __forceinline__ CmRow cm_row(const float* __restrict__ tab, int n_table, int64_t tb) {
    const float nan = __int_as_float(0x7FC00000);
    return (tb < 0 || tb >= (int64_t)n_table) ? CmRow{nan, nan} : CmRow{tab[2 * tb], tab[2 * tb + 1]};
}

__global__ void __launch_bounds__(kDistillThreads) cm_out_kernel(const float* __restrict__ x, const float* out,
                                                                 const float* __restrict__ tab, int n_table,
                                                                 const int64_t* __restrict__ t, float* f, long long n4) {
    const int b = blockIdx.y;
    const CmRow r = cm_row(tab, n_table, t[b]);
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kDistillThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kDistillThreads) {
        float xs[4], os[4], fs[4];
        load4(x, base + (size_t)i, xs);
        load4(out, base + (size_t)i, os);
#pragma unroll
        for (int j = 0; j < 4; ++j) fs[j] = consistency_f(xs[j], os[j], r.p, r.q);
        store4(f, base + (size_t)i, fs);
    }
}

__global__ void __launch_bounds__(256) cm_loss_part_kernel(const float* __restrict__ x, const float* __restrict__ o,
                                                           const float* __restrict__ y, const float* __restrict__ tab, int n_table,
                                                           const int64_t* __restrict__ t, float* __restrict__ partial, long long per) {
    const CmRow r = cm_row(tab, n_table, t[blockIdx.y]);
    sqerr_part_body([=](size_t at) { return y[at] - consistency_f(x[at], o[at], r.p, r.q); }, partial, per);
}

__global__ void cm_loss_final_kernel(const float* __restrict__ partial, float huber_c, float* __restrict__ loss, int B) {
    sqerr_final_body([=](int, float S) {
#pragma clang fp contract(off)
        if (!(huber_c > 0.f)) return S;
        const float cc = huber_c * huber_c;
        const float r = __fsqrt_rn(S + cc);
        const float den = r + huber_c;
        return S / den;
    }, partial, loss, B);
}

__global__ void __launch_bounds__(kDistillThreads) cm_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ o,
                                                                      const float* __restrict__ y, const float* __restrict__ tab,
                                                                      int n_table, const int64_t* __restrict__ t, float huber_c,
                                                                      const float* __restrict__ loss, const float* __restrict__ g,
                                                                      float* __restrict__ d, long long n4) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const CmRow r = cm_row(tab, n_table, t[b]);
    float k = sqerr_bwd_c0(g, b, gridDim.y, 1);
    if (huber_c > 0.f) {
        const float root = loss[b] + huber_c;  // sqrt(S_b + c^2) = S_b / (sqrt(S_b + c^2) + c) + c
        const float two = 2.0f * root;
        k = k / two;
    }
    const float c = r.q * k;
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kDistillThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kDistillThreads) {
        float xs[4], os[4], ys[4], ds[4];
        load4(x, base + (size_t)i, xs);
        load4(o, base + (size_t)i, os);
        load4(y, base + (size_t)i, ys);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float diff = consistency_f(xs[j], os[j], r.p, r.q) - ys[j];
            ds[j] = c * diff;
        }
        store4(d, base + (size_t)i, ds);
    }
}

hipError_t cm_out_launch(const float* x, const float* out, const float* tab, int n_table, const int64_t* t, float* f, int B,
                         long long per_sample, hipStream_t s) {
    if (!distill_shape_ok(B, per_sample) || n_table < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cm_out_kernel, dim3(sample_blocks(B, per_sample), B), dim3(kDistillThreads), 0, s, x, out, tab, n_table, t, f,
                       per_sample / 4);
    return hipGetLastError();
}

hipError_t cm_loss_launch(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t,
                          float huber_c, float* partial, float* loss, int B, long long per_sample, hipStream_t s) {
    if (!distill_shape_ok(B, per_sample) || n_table < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cm_loss_part_kernel, dim3(kSqParts, B), dim3(256), 0, s, x, out, y, tab, n_table, t, partial, per_sample);
    hipLaunchKernelGGL(cm_loss_final_kernel, dim3(1), dim3(64), 0, s, partial, huber_c, loss, B);
    return hipGetLastError();
}

hipError_t cm_loss_bwd_launch(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t,
                              float huber_c, const float* loss, const float* g, float* d, int B, long long per_sample, hipStream_t s) {
    if (!distill_shape_ok(B, per_sample) || n_table < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cm_loss_bwd_kernel, dim3(sample_blocks(B, per_sample), B), dim3(kDistillThreads), 0, s, x, out, y, tab, n_table,
                       t, huber_c, loss, g, d, per_sample / 4);
    return hipGetLastError();
}

}  // namespace ddimx
