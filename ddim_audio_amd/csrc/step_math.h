// The arithmetic and the launch shape every sampler update kernel shares (step_, solver_, sde_, pool_, window_, inpaint_ and
// invert_kernels.hip; noise_kernels.hip for the launch shape).  The only copy of each: the scalar operations below, and -- for the
// kernels that apply one coefficient row to a sample's float4s (ddim_update_kernel, multistep_update_kernel,
// sde_multistep_update_kernel, pool_update_kernel, unic_multistep_update_kernel) -- the whole body of an update, update4h (update4
// without a third history term), whose arithmetic on registers (update4_core3, update4_core without that term) the two canvas
// kernels share (window_update_kernel, window_multistep_update_kernel): update4_core3 is the only
// DDIM update in the library.  Single copies that live beside their kernels: the canvas row locator, the clamped cover loads, the
// blend and the cover-count dispatch (WindowRow, window_load_cover, window_blend4, dispatch_cover: window_kernels.h); one
// inpainting step on registers and its flag dispatch (InpaintRow, inpaint_weight, inpaint_residual4, inpaint_update4,
// dispatch_inpaint_flags: inpaint_kernels.h), which inpaint_kernels.hip and window_inpaint_kernels.hip both call; the multistep
// inpainting update (inpaint_solver_kernels.hip) takes the weight, the flag dispatch and the scalar operations below from the same
// places and has its own body, because its history and its known-region path are no part of that step.
//
// Rounding contract.  Every operation is rounded once, to nearest, in this order and with no contraction beyond the fmaf written
// here, so the same inputs give the same bits in every kernel ("order 1 == generalized_steps", "one window ==
// generalized_steps", "empty mask == generalized_steps" rest on it):
//   x0 = (x - s1 e) / s2      reference  xt.add_(et, alpha=-sqrt(1-at)).div_(sqrt(at))
//   x' = s3 x0 + c2 e         reference  xt.mul_(sqrt(at_next)).add_(et, alpha=c2);  a noise term is one more fmaf(z, c1, x')
//   e  = s1 x + s2 v          the eps of a network that predicts v = sqrt(at) e - sqrt(1-at) x0 (vpred_kernels.hip): two roundings
// The x0 clip / dynamic threshold (threshold_kernels.hip) between the network's eps and the update, in this order:
//   x0 = ddim_x0(x, e, s1, s2)                     the prediction above; q = the order statistic of |x0| at the host's rank
//   s  = min(max(q, floor), ceil)                  comparisons only: a NaN q gives floor;  r = rn(floor / s)
//   c  = rn(min(max(x0, -s), s) r)                 comparisons, then one product
//   e' = e if c has x0's bits, else rn(fma(c, -s2, x) / s1)    the eps whose prediction is c, up to these two roundings and ddim_x0's
#pragma once
#include "common.h"

namespace ddimx {

__device__ __forceinline__ float ddim_x0(float x, float e, float s1, float s2) { return __fdiv_rn(fmaf(e, -s1, x), s2); }
__device__ __forceinline__ float ddim_next(float x0, float e, float s3, float c2) { return fmaf(e, c2, __fmul_rn(x0, s3)); }
__device__ __forceinline__ float v_to_eps(float x, float v, float s1, float s2) { return fmaf(v, s2, __fmul_rn(x, s1)); }
// the consistency function f = p x + q out of a consistency model (distill_kernels.hip, sde_kernels.hip): v_to_eps's two roundings
// on the row (p, q) of schedule.consistency_table, fma(q, out, rn(p x))
__device__ __forceinline__ float consistency_f(float x, float out, float p, float q) { return v_to_eps(x, out, p, q); }
__device__ __forceinline__ float x0_scale(float q, float floor, float ceil) {
    const float s = q > floor ? q : floor;
    return s < ceil ? s : ceil;
}
__device__ __forceinline__ float x0_clip(float x0, float s, float r) {
    const float lo = x0 < -s ? -s : x0;
    return __fmul_rn(lo > s ? s : lo, r);
}
__device__ __forceinline__ float x0_to_eps(float x, float e, float x0, float c, float s1, float s2) {
    return __float_as_uint(c) == __float_as_uint(x0) ? e : __fdiv_rn(fmaf(c, -s2, x), s1);
}

// ---- masked inpainting with reconstruction guidance (inpaint_kernels.hip, window_inpaint_kernels.hip), per element, in this order:
//   r    = m (x0 - y)                              the masked residual; L = sum of r^2 per sample, fmaf(r, r, acc) per thread
//   seed = k1 (m r)                                what the data-only backward is seeded with
//   u    = u - w (k2 (m (m (x0 - y))) + d)         fmaf(-w, fmaf(k2, q, d), u): the guidance term, d the backward's result
//   x'   = kv if m == 1, u if m == 0, else fmaf(m, kv, (1 - m) u)     the replacement: exact selects at both ends of the mask
__device__ __forceinline__ float inpaint_residual(float x0, float y, float m) { return __fmul_rn(m, __fsub_rn(x0, y)); }
__device__ __forceinline__ float inpaint_seed(float r, float m, float k1) { return __fmul_rn(k1, __fmul_rn(m, r)); }
__device__ __forceinline__ float inpaint_guide(float u, float x0, float y, float m, float d, float k2, float w) {
    const float q = __fmul_rn(m, __fmul_rn(m, __fsub_rn(x0, y)));
    return fmaf(-w, fmaf(k2, q, d), u);
}
__device__ __forceinline__ float inpaint_replace(float u, float kv, float m) {
    return m == 1.f ? kv : m == 0.f ? u : fmaf(m, kv, __fmul_rn(__fsub_rn(1.f, m), u));
}
// The multistep inpainting step (inpaint_solver_kernels.hip) takes the known content along the exact solution of the sampler's
// ODE / SDE for the constant data prediction y, not along the network's eps:
//   kv = w0 y + cx x          fmaf(cx, x, w0 y); the x term only where use_x (cx != 0): a final row, cx = 0 and w0 = 1, gives y's bits
// with cx = c2 / s1 and w0 = s3 - c2 s2 / s1 from the row (schedule.inpaint_solver_coefficients).
__device__ __forceinline__ float inpaint_known(float x, float y, float cx, float w0, bool use_x) {
    const float k = __fmul_rn(w0, y);
    return use_x ? fmaf(cx, x, k) : k;
}

// ---- one update on one coefficient row: the body of ddim_update_kernel (step_kernels.hip), multistep_update_kernel
// (solver_kernels.hip), sde_multistep_update_kernel (sde_kernels.hip), pool_update_kernel (pool_kernels.hip) and
// unic_multistep_update_kernel (unic_kernels.hip)
// The row is (t, s1, s2, s3, c2, c1, w1, w2) -- schedule.dpm_coefficients; a DDIM row (schedule.ddim_coefficients) ends at c1, a
// corrector row (schedule.unic_coefficients) has a ninth column w3, which load_row3 reads and every other row leaves 0.
struct StepRow { float s1, s2, s3, c2, c1, w1, w2, w3; };
__device__ __forceinline__ StepRow load_row(const float* __restrict__ c, bool has_w) {
    return {c[1], c[2], c[3], c[4], c[5], has_w ? c[6] : 0.f, has_w ? c[7] : 0.f, 0.f};
}
__device__ __forceinline__ StepRow load_row3(const float* __restrict__ c) {
    return {c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
}
// a float4 at index `at` <-> four floats
__device__ __forceinline__ void load4(const float* p, size_t at, float v[4]) {
    const float4 q = ((const float4*)p)[at];
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void store4(float* p, size_t at, const float v[4]) { ((float4*)p)[at] = make_float4(v[0], v[1], v[2], v[3]); }

// Float4 `at` of one update.  With m1 = x0[at] (the previous iteration's prediction, still in the buffer), m2 = hist[at] (the
// one before) and m3 = hist2[at] (the one before that) on entry, per element and in this order:
//   m0 = (x - s1 e) / s2                       ddim_x0
//   u  = s3 m0 + c2 e                          ddim_next
//   u  = u + w1 (m0 - m1)     if use1          fmaf(w1, __fsub_rn(m0, m1), u)
//   u  = u + w2 (m1 - m2)     if use2          fmaf(w2, __fsub_rn(m1, m2), u)
//   u  = u + w3 (m2 - m3)     if use3          fmaf(w3, __fsub_rn(m2, m3), u)
//   u  = u + c1 z             if add_z         fmaf(z, c1, u)
//   xt <- u, x0 <- m0, hist <- m1 (when hist is given), hist2 <- m2 (when hist2 is given)
// The flags are the caller's and uniform over its block; each kernel says how it forms them.  A term whose flag is off is not
// applied at all (fmaf(z, 0, u) is not u at u = -0), and what it would have read is not read: m1 is loaded iff load1 (which use1,
// use2 and a non-null hist need), m2 iff use2, use3 or a non-null hist2 (its shift), m3 iff use3 -- a first iteration finds the
// buffers uninitialised, and they never enter u.  So equal rows, flags and z give equal bits in all five kernels: a row with
// w1 = w2 = 0 is the DDIM step, one with c1 = 0 the deterministic solver's, one with w3 = 0 and no hist2 the solver's too.
// The arithmetic alone, on registers: x <- u and m0 <- the prediction, from x, e, m1, m2, m3 (and z) as above.  update4h below
// and window_update_kernel / window_multistep_update_kernel (window_*kernels.hip), whose e is blended rather than loaded, are its
// callers.
__device__ __forceinline__ void update4_core3(float x[4], const float e[4], const float m1[4], const float m2[4], const float m3[4],
                                              float m0[4], const StepRow& r, bool use1, bool use2, bool use3, bool add_z,
                                              const float z[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m0[j] = ddim_x0(x[j], e[j], r.s1, r.s2);
        float u = ddim_next(m0[j], e[j], r.s3, r.c2);
        if (use1) u = fmaf(r.w1, __fsub_rn(m0[j], m1[j]), u);
        if (use2) u = fmaf(r.w2, __fsub_rn(m1[j], m2[j]), u);
        if (use3) u = fmaf(r.w3, __fsub_rn(m2[j], m3[j]), u);
        if (add_z) u = fmaf(z[j], r.c1, u);
        x[j] = u;
    }
}
// the update without a third history term: what every kernel but the corrector's calls
__device__ __forceinline__ void update4_core(float x[4], const float e[4], const float m1[4], const float m2[4], float m0[4],
                                             const StepRow& r, bool use1, bool use2, bool add_z, const float z[4]) {
    update4_core3(x, e, m1, m2, m2, m0, r, use1, use2, false, add_z, z);
}
__device__ __forceinline__ void update4h(float* xt, const float* et, float* x0, float* hist, float* hist2, size_t at, const StepRow& r,
                                         bool load1, bool use1, bool use2, bool use3, bool add_z, const float z[4]) {
    float x[4], e[4], m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f}, m3[4] = {0.f, 0.f, 0.f, 0.f}, m0[4];
    load4(xt, at, x);
    load4(et, at, e);
    if (load1) load4(x0, at, m1);
    if (use2 || use3 || hist2) load4(hist, at, m2);
    if (use3) load4(hist2, at, m3);
    update4_core3(x, e, m1, m2, m3, m0, r, use1, use2, use3, add_z, z);
    if (hist2) store4(hist2, at, m2);
    if (hist) store4(hist, at, m1);
    store4(x0, at, m0);
    store4(xt, at, x);
}
__device__ __forceinline__ void update4(float* xt, const float* et, float* x0, float* hist, size_t at, const StepRow& r, bool load1,
                                        bool use1, bool use2, bool add_z, const float z[4]) {
    update4h(xt, et, x0, hist, nullptr, at, r, load1, use1, use2, false, add_z, z);
}

// The q-sample x = x0 sqrt(a) + e sqrt(1 - a) (functions/losses.py:12-13) as torch evaluates it: both products and the sum rounded
// separately.  Plain operators under contract(off): the __f*_rn wrappers are plain operators to this compiler, which fused one
// product into the sum in the paired trips of qsample_kernel's unrolled loop -- every element of a thread's trips but an odd last
// one then missed the reference's bits (tests/test_gpu_tail_kernels.py::test_qsample at 1024 * 256 + 5 elements).
__device__ __forceinline__ float qsample_x(float x0, float e, float sa, float sb) {
#pragma clang fp contract(off)
    const float p = x0 * sa, q = e * sb;
    return p + q;
}

constexpr int kSampleThreads = 256;  // 4 waves of 64: block_sum
constexpr int kSampleBlocks = 2048;  // blocks of one launch, about: one sample still fills the chip

// sum over the block (kSampleThreads threads) in a fixed order; every thread gets the result
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();  // red may still be read by an earlier call
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// blocks per sample of a (blocks per sample, B) grid whose blocks walk one sample's float4s grid-stride: about kSampleBlocks in
// all, at most one float4 per thread and pass, at most max_blocks (kernels that keep one partial per block bound it).  No
// kernel's values depend on it.
inline int sample_blocks(int B, long long per_sample, int max_blocks = kSampleBlocks) {
    const long long need = (per_sample / 4 + kSampleThreads - 1) / kSampleThreads;
    long long nb = kSampleBlocks / (B > 0 ? B : 1);
    if (nb < 1) nb = 1;
    if (nb > max_blocks) nb = max_blocks;
    if (nb > need) nb = need;
    return (int)(nb < 1 ? 1 : nb);
}

}  // namespace ddimx
