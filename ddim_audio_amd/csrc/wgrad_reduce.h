// Dispatch and slab reduction of the MFMA weight gradients (wgrad_reduce.hip):
// enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "wgrad_mfma.h"

namespace ddimx {

// dispatch on dtype to wgrad_inst_*.hip; ci = channels of `a`, co = channels of `du`
hipError_t wgrad_geometry(int dtype, int mode, int ci, int co, WgradGeom* g);
hipError_t wgrad_launch(int dtype, int mode, int ci, int co, const WgradArgs& a, int nsplit, hipStream_t s);
// dst[co][ci][tap] (+)= sum_s partial[s][tap][co][ci]   (fixed order; dst is the fp32 parameter-gradient tensor).  The kernel is
// picked by wgrad_reduce_kind: KS threads per output for KS4 / KS16, 16 threads per output quad for QUAD.
enum { WGRAD_REDUCE_KS4 = 0, WGRAD_REDUCE_KS16 = 1, WGRAD_REDUCE_QUAD = 2 };
int wgrad_reduce_kind(int nsplit, int ntaps, int co, int ci);
hipError_t wgrad_reduce_launch(const float* partial, int nsplit, int ntaps, int co, int ci, float* dst, hipStream_t s);

}  // namespace ddimx
