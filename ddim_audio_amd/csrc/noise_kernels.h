// Launch wrapper of the seeded noise fill (noise_kernels.hip; the stream itself is defined in noise.h).  Same rules as step_kernels.h:
// enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"

namespace ddimx {

constexpr int kNoiseThreads = kSampleThreads;  // the grid: (sample_blocks, B), one group of four per thread and pass
constexpr int kNoiseNormals = 0, kNoiseWords = 1;  // `kind`: fp32 normals | the raw Philox words as uint32

// out[b][4 q + j] = output j of Philox4x32-10(key = seed, counter = (q, first_sample + b, draw_base + (step ? step[0] : 0), tag));
// step is read when the launch runs.  hipErrorInvalidValue for B outside 1..65535, per_sample not a positive multiple of 4,
// per_sample / 4 > 2^32, first_sample + B > 2^32 or an unknown kind.
hipError_t noise_fill_launch(void* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample, const int* step,
                             unsigned draw_base, unsigned tag, int kind, hipStream_t s);

}  // namespace ddimx
