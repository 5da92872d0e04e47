// Launch wrapper of the seeded noise fill (noise_kernels.hip; the stream itself is defined in noise.h).  Same rules as kernels.h:
// enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

constexpr int kNoiseThreads = 256;
constexpr int kNoiseNormals = 0, kNoiseWords = 1;  // `kind`: fp32 normals | the raw Philox words as uint32

// blocks per sample: about 2048 blocks in all (so B = 1 still fills the chip), at most one group of four per thread and pass.
// The values do not depend on it.
inline int noise_blocks(int B, long long per_sample) {
    const long long need = (per_sample / 4 + kNoiseThreads - 1) / kNoiseThreads;
    long long nb = 2048 / (B > 0 ? B : 1);
    if (nb < 1) nb = 1;
    if (nb > need) nb = need;
    return (int)(nb < 1 ? 1 : nb);
}

// out[b][4 q + j] = output j of Philox4x32-10(key = seed, counter = (q, first_sample + b, draw_base + (step ? step[0] : 0), tag));
// step is read when the launch runs.  hipErrorInvalidValue for B outside 1..65535, per_sample not a positive multiple of 4,
// per_sample / 4 > 2^32, first_sample + B > 2^32 or an unknown kind.
hipError_t noise_fill_launch(void* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample, const int* step,
                             unsigned draw_base, unsigned tag, int kind, hipStream_t s);

}  // namespace ddimx
