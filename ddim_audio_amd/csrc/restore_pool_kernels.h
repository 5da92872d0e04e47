// Launch wrapper of the restoring pool's update (restore_pool_kernels.hip; ddim_audio_amd/restore_pool.py).  Same rules as
// pool_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "pool_kernels.h"

namespace ddimx {

// second arena [n_slots][max_steps][kRpxKnownStride] fp32: rows (cx, w0) beside the pool's rows (schedule.inpaint_solver_coefficients)
constexpr int kRpxKnownStride = 2;
// word kRpxFlagsWord of a slot-table row (reserved and zero for the pool's own kernels) holds the flags; kRpxKnown: the slot has a
// known clip and a mask
constexpr int kRpxFlagsWord = 6;
constexpr int kRpxKnown = 1;

// pool_update_launch on the slots without kRpxKnown; on the others the same update with the known region put back along its exact
// path.  hipErrorInvalidValue for what pool_update_launch refuses
hipError_t rpx_pool_update_launch(float* xt, const float* et, float* x0, float* hist, const float* y, const float* m, const float* arena,
                                  const float* known, const int* slots, int n_slots, int max_steps, long long per_sample, hipStream_t s);

}  // namespace ddimx
