// Launch wrappers of the x0 clip / dynamic threshold kernels (threshold_kernels.hip; ddim_audio_amd/sampler.py).  Same rules as
// step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"

namespace ddimx {

constexpr int kThreshThreads = kSampleThreads;  // the grid of the selection passes and of the rewrite: (sample_blocks, B)
// The key of an element is the bit pattern of |x0| (31 bits; unsigned order = float order, NaN and inf sort by their bits above
// every finite value).  Three digits, most significant first: bits 30..20, 19..10, 9..0.  Every digit value has a bin.
constexpr int kBins0 = 2048, kBins12 = 1024;
constexpr int kQuantileWords = kBins0 + 2 * kBins12;  // unsigned counts of one sample: the three histograms, in pass order

// Bytes of the work buffer of x0_quantile_launch for a batch of B: B * kQuantileWords counts.
// ZERO CONTRACT: every word is 0 before the first call (the caller zeroes the buffer once, when it allocates it), and every call
// leaves every word 0 again -- the finishing kernel, the only launch that runs after the last reader of a sample's histograms,
// clears them with vector stores -- so one buffer serves any number of consecutive calls and graph replays with no host work and
// no memset node between them.  The samples whose t[b] is outside the table are not counted and their words stay 0.  The buffer
// is 16-byte aligned (the histograms are read as uint4).
inline long long quantile_work_bytes(int B) { return (long long)B * kQuantileWords * (long long)sizeof(unsigned); }

// scale[b] = (s, r) of x0_scale / floor / s (step_math.h) for q = the element of rank `rank` (0-based, ascending) among the
// per_sample values |ddim_x0(x, eps, s1, s2)| of sample b, (s1, s2) = row t[b] of tab [n_table][2]; x0 is recomputed from (x, eps)
// in every pass and never stored.  Exact: a three-pass radix select on the bit patterns -- per pass every block counts the elements
// that carry the digits chosen so far in an LDS histogram and adds its non-empty bins to the sample's global one with integer
// atomics (counts do not depend on the order of arrival: no float atomics, the result is bit-reproducible and does not depend on B
// or on the grid); the blocks of the next pass each scan the previous histograms themselves.  Four launches: three passes over
// (sample_blocks, B), then one finishing block per sample.  A t[b] outside 0 .. n_table - 1 leaves scale[b] alone and reads no row.
// hipErrorInvalidValue for B outside 1..65535, per_sample not a positive multiple of 4 or >= 2^31, rank outside 0 .. per_sample - 1
// or n_table < 1.
hipError_t x0_quantile_launch(const float* x, const float* eps, const float* tab, int n_table, const int64_t* t, long long rank,
                              float floor, float ceil, void* work, float* scale, int B, long long per_sample, hipStream_t s);
// eps_out[b] = x0_to_eps(x, eps_in, x0, x0_clip(x0, s, r), s1, s2) with x0 = ddim_x0(x, eps_in, s1, s2), (s, r) = scale[b] and
// (s1, s2) = row t[b] of tab: an element whose clipped prediction has the bits of the prediction keeps its eps bit for bit.  One
// pass; every element is read before the same thread writes it, so eps_out may be eps_in.  A t[b] outside the table leaves
// eps_out[b] alone.  hipErrorInvalidValue as above (no rank).
hipError_t threshold_eps_launch(const float* x, const float* eps_in, float* eps_out, const float* scale, const float* tab, int n_table,
                                const int64_t* t, int B, long long per_sample, hipStream_t s);

}  // namespace ddimx
