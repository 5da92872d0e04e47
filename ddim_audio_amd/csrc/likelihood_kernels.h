// Launch wrappers of the likelihood kernels (likelihood_kernels.hip; ddim_audio_amd/likelihood.py, include/features/lkx_likelihood.h
// has the arithmetic).  Same rules as step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"

namespace ddimx {

constexpr int kLkxStride = 8;                  // floats per row of schedule.likelihood_coefficients (LKX_STRIDE)
constexpr int kLkxSave = 1, kLkxCommit = 2;    // the row's flags (LKX_SAVE, LKX_COMMIT)
constexpr int kLkxThreads = kSampleThreads;    // the grid of the walking kernels: (lkx_blocks, B)
constexpr int kLkxMaxBlocks = 256;             // blocks per sample at most: one finishing thread sums that many partials
constexpr int kLkxPerThread = 4;               // float4s per thread, about, before a sample gets another block

// blocks that walk one sample: a function of per_sample ALONE (a partial sum's order, so a sample's result, must not depend on B)
inline int lkx_blocks(long long per_sample) {
    const long long per_block = (long long)kLkxThreads * kLkxPerThread;
    const long long nb = (per_sample / 4 + per_block - 1) / per_block;
    return (int)(nb < 1 ? 1 : nb > kLkxMaxBlocks ? kLkxMaxBlocks : nb);
}

// every launcher: hipErrorInvalidValue for B outside 1..65535 or per_sample not a positive multiple of 4; the two that draw the
// probe also for per_sample / 4 > 2^32 or first_sample + B > 2^32
hipError_t lkx_probe_fill_launch(float* r, int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned probe,
                                 hipStream_t s);
hipError_t lkx_stage_launch(float* u, float* k1, const float* e, const float* g, float* xin, double* partial, const float* coef,
                            const int* step, int B, long long per_sample, unsigned long long seed, unsigned first_sample,
                            unsigned probe, hipStream_t s);
// acc[b] += wd[step[0]] * (partial[b][0 .. nb - 1] summed in order); wd null: acc[b] = that sum
hipError_t lkx_finish_launch(const double* partial, double* acc, const double* wd, const int* step, int B, int nb, hipStream_t s);
hipError_t lkx_sumsq_part_launch(const float* x, double* partial, int B, long long per_sample, hipStream_t s);

}  // namespace ddimx
