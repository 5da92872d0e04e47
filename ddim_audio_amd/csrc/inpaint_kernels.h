// Launch wrappers of the masked-inpainting sampler kernels (inpaint_kernels.hip).  Same rules as step_kernels.h: enqueue on the given
// stream, never allocate or synchronise.
#pragma once
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

// guided path: x0 = (xt - s1 eps) / s2, seed = k1 m^2 (x0 - y), partials[b][blk] = sum of (m (x0 - y))^2 over the block's elements
hipError_t inpaint_residual_launch(const float* xt, const float* et, const float* y, const float* m, float* x0, float* seed,
                                   float* partials, const float* coef, const int* step, int B, long long per_sample, hipStream_t s);
// the DDIM update (+ guidance term, + replacement), in place on xt; flags: 1 = replace, 2 = guided (x0 read, not computed)
hipError_t inpaint_update_launch(float* xt, const float* et, const float* noise, float* x0, const float* y, const float* m,
                                 const float* dx, const float* partials, const float* coef, const int* step, int B,
                                 long long per_sample, int flags, hipStream_t s);

}  // namespace ddimx
