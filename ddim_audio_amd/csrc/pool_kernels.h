// Launch wrappers of the sampler pool's step (pool_kernels.hip; ddim_audio_amd/pool.py).  Same rules as step_kernels.h: enqueue on the
// given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"

namespace ddimx {

// coefficient arena [n_slots][max_steps][kPoolStride] fp32: rows (t, s1, s2, s3, c2, c1, w1, w2), the solver's row layout
constexpr int kPoolStride = 8;
// slot table [n_slots][kPoolSlotWords] int32: pos, len, seed_lo, seed_hi, sample, draw_base, two reserved words.  A slot is
// active iff 0 <= pos < len <= max_steps; every kernel below leaves an idle slot's memory alone
constexpr int kPoolSlotWords = 8;

// t[b] = the t of slot b's current row, 0 for an idle slot
hipError_t pool_begin_launch(const float* arena, const int* slots, int64_t* t, int n_slots, int max_steps, hipStream_t s);
// one update of every active slot's sample, in place on xt[b]; x0[b] <- its x0 prediction, hist[b] <- the previous one.
// hipErrorInvalidValue for n_slots outside 1..65535, max_steps < 1, per_sample not a positive multiple of 4 or per_sample / 4 > 2^32
hipError_t pool_update_launch(float* xt, const float* et, float* x0, float* hist, const float* arena, const int* slots, int n_slots,
                              int max_steps, long long per_sample, hipStream_t s);
// pos[b] += 1 for every active slot
hipError_t pool_end_launch(int* slots, int n_slots, int max_steps, hipStream_t s);

}  // namespace ddimx
