// Launch wrappers of the training-step tail kernels (tail_kernels.hip):
// enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

hipError_t qsample_launch(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, int B,
                          long long per, hipStream_t s);
hipError_t sqerr_launch(const float* e, const float* out, float* partial, float* loss_per, int B, long long per,
                        hipStream_t s);
int sqerr_nparts();
constexpr int kSqParts = 64;  // partials per sample of the loss: one wave finishes a sample
// the first of sqerr_launch's two launches alone: partial[b][kSqParts], the per-sample sums of squares in fixed-order parts (the
// weighted loss of distill_kernels.hip finishes them its own way)
hipError_t sqerr_part_launch(const float* e, const float* out, float* partial, int B, long long per, hipStream_t s);
// The two stages of that reduction, the only copy of each (sqerr_part_kernel / sqerr_final_kernel, the weighted loss's and the
// consistency loss's kernels in distill_kernels.hip).  First stage, grid (kSqParts, B) of 256 threads: sample b's elements are cut
// into kSqParts chunks, a thread sums d^2 (d = diff(index), fmaf(d, d, s)) over its chunk's elements 256 apart, then one fixed
// tree over the block.  Second stage, one wave: S_b = the sum of sample b's parts, loss[b] = value(b, S_b), loss[B] = (the sum
// of the loss[b] in b order) / B.  contract(off): the sum takes the ROUNDED value(b, S_b).
template <class Diff>
__device__ __forceinline__ void sqerr_part_body(Diff diff, float* __restrict__ partial, long long per) {
    __shared__ float red[4];
    const int b = blockIdx.y, part = blockIdx.x;
    const long long chunk = (per + kSqParts - 1) / kSqParts;
    const long long lo = part * chunk, hi = (lo + chunk < per) ? lo + chunk : per;
    const size_t base = (size_t)b * per;
    float s = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) { const float d = diff(base + i); s = fmaf(d, d, s); }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[b * kSqParts + part] = (red[0] + red[1]) + (red[2] + red[3]);
}
template <class Value>
__device__ __forceinline__ void sqerr_final_body(Value value, const float* __restrict__ partial, float* __restrict__ loss, int B) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    float tot = 0.f;
    for (int b = 0; b < B; ++b) {
        const float v = value(b, wave_sum(lane < kSqParts ? partial[b * kSqParts + lane] : 0.f));
        if (lane == 0) loss[b] = v;
        tot += v;
    }
    if (lane == 0) loss[B] = tot / (float)B;
}
hipError_t ema_multi_launch(const long long* shadow_ptrs, const long long* param_ptrs, const long long* sizes,
                            const int* blk_tensor, const long long* blk_off, int nblocks, float c_p, float c_s, hipStream_t s);
int ema_block_elems();
// training-step tail (multi-tensor, pointer tables as for ema_multi)
hipError_t grad_norm_multi_launch(const long long* ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                                  int nblocks, float max_norm, float* partial, float* out, hipStream_t s);
struct AdamArgs {
    const long long* p; const long long* g; const long long* m; const long long* v; const long long* sizes;
    const int* blk_tensor; const long long* blk_off; const float* clip;
    float lr, b1, b2, eps, wd, bc1, bc2s; int decoupled;
    const float* dyn;  // nullable, device: {lr, bc1, bc2s} read when the kernel RUNS (graph-replayed steps) instead of the values above
};
hipError_t adam_multi_launch(const AdamArgs& a, int nblocks, hipStream_t s);
hipError_t scale_multi_launch(const long long* ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                              int nblocks, const float* coef, hipStream_t s);
// d_out[b] = 2 g[b] (out[b] - e[b]); g: upstream gradient of the per-sample losses [B]
hipError_t sqerr_bwd_launch(const float* e, const float* out, const float* g, float* d, int B, long long per, hipStream_t s, int with_mean = 0);
// the scalar of sample b in d_out[b] = c0 (out[b] - e[b]).  with_mean: g has B + 1 entries, the last one the upstream gradient of the
// batch MEAN (the loss vector's [B] entry): + g[B] / B per sample.  The only copy (sqerr_bwd_kernel, sqerr_w_bwd_kernel).
__device__ __forceinline__ float sqerr_bwd_c0(const float* __restrict__ g, int b, int B, int with_mean) {
    return 2.0f * (g[b] + (with_mean ? g[B] / (float)B : 0.f));
}
// blocks per sample of sqerr_bwd_kernel's grid (and of the weighted twin's)
inline int sqerr_bwd_blocks(long long per) { return (int)((per + 255) / 256 < 1024 ? (per + 255) / 256 : 1024); }

}  // namespace ddimx
