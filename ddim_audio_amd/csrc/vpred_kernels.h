// Launch wrappers of the v-prediction kernels (vpred_kernels.hip; ddim_audio_amd/sampler.py, losses.py).  Same rules as
// step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"

namespace ddimx {

constexpr int kVpredThreads = kSampleThreads;  // the grid of either kernel: (sample_blocks, B)

// eps[b] = s1 x[b] + s2 v[b] (v_to_eps, step_math.h) with (s1, s2) = row t[b] of vtab [n_table][2]; a t[b] outside
// 0 .. n_table - 1 leaves eps[b] alone and reads no row.  eps may be v.  hipErrorInvalidValue for B outside 1..65535,
// per_sample not a positive multiple of 4 or n_table < 1.
hipError_t v_to_eps_launch(const float* x, const float* v, float* eps, const float* vtab, int n_table, const int64_t* t, int B,
                           long long per_sample, hipStream_t s);
// x[b] = x0[b] sqrt(a) + e[b] sqrt(1 - a) (qsample_kernel's bits) and v[b] = e[b] sqrt(a) - x0[b] sqrt(1 - a), a = alphas[t[b]],
// in one pass.  hipErrorInvalidValue for B outside 1..65535 or per_sample not a positive multiple of 4.
hipError_t qsample_v_launch(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, float* v, int B,
                            long long per_sample, hipStream_t s);

}  // namespace ddimx
