// The arithmetic and the launch shape every sampler update kernel shares (step_kernels.hip's ddim_update_kernel, solver_, window_,
// inpaint_ and invert_kernels.hip; noise_kernels.hip for the launch shape).  The only copy of each.
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
