// Launch wrappers of the DDIM-inversion update and of the latent slerp (invert_kernels.hip).  Same rules as step_kernels.h: enqueue on
// the given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"

namespace ddimx {

// coefficient rows of the inversion: (t, s1, s2, p, q, first) fp32, one row per network evaluation, indexed by the device counter
constexpr int kInvertStride = 6;
constexpr int kInvertThreads = kSampleThreads;   // block_sum
constexpr int kSlerpChunk = 64;                  // interpolation weights whose coefficients one block keeps in LDS at a time

// blocks per sample (per pair) of the element-wise kernels = partials per sample, sample_blocks(B, per_sample, kInvertMaxBlocks)
constexpr int kInvertMaxBlocks = 1024;

// One row of the inversion table, in place on xt: x0 <- (xt - s1 eps) / s2, xt <- p base + q eps, base <- xt first on a row whose
// `first` flag is set; partials [B][blocks][2] double: the block sums of (x_new - x_old)^2 and x_new^2; a second, small launch adds
// them in a fixed order and writes log[step][b] = sqrt(sum0) / sqrt(sum1) (0 when sum1 = 0).  A counter outside 0 .. rows - 1
// makes both launches no-ops: nothing is read or written beyond the table and the log.
hipError_t invert_update_launch(float* xt, const float* et, float* base, float* x0, double* partials, float* log, int rows,
                                const float* coef, const int* step, int B, long long per_sample, hipStream_t s);

// Spherical interpolation of P pairs at M weights: out [P][M][per_sample]; partials [P][blocks][3] double (the block sums of
// z1 z2, z1^2, z2^2).  Two launches: the sums, then the blend (every block adds its pair's partials in the same fixed order).
hipError_t slerp_launch(const float* z1, const float* z2, const float* weights, int M, float* out, double* partials, int P,
                        long long per_sample, hipStream_t s);

}  // namespace ddimx
