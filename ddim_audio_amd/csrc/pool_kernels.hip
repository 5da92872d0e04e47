// Sampler pool (ddim_audio_amd/pool.py): the three launches that frame the forward of a batch whose samples each follow their own
// schedule -- DDIM with any eta or DPM-Solver++ of orders 1-3 -- from their own position in it.
//
// Slot b's scalars come from row pos[b] of its own block of the coefficient arena ([n_slots][max_steps][kPoolStride] fp32, the
// solver's row (t, s1, s2, s3, c2, c1, w1, w2)); pos, the schedule's length and the slot's noise identity live in the slot table
// ([n_slots][kPoolSlotWords] int32: pos, len, seed_lo, seed_hi, sample, draw_base, 2 reserved).  Both are device memory read when
// the launch RUNS, so one captured step serves every mix of requests.  A slot is active iff 0 <= pos < len <= max_steps; no kernel
// reads or writes the sample, the prediction or the history of an idle slot, and none reads the arena beyond an active row.
//
// pool_update_kernel is update4 (step_math.h) on an active slot's row.  Every slot keeps a history: the previous prediction is
// always read and always kept; a history term is applied iff its weight is non-zero and the noise term iff c1 != 0, so a DDIM row
// gives ddim_update_kernel's bits and a solver row multistep_update_kernel's.  z is noise_normals4 (noise.h) for the counter (group
// of four, sample, draw_base + pos, tag 0) under the key (seed_lo, seed_hi) -- what noise_fill_kernel writes for that sample and
// draw -- so there is no noise buffer and no fill launch.  The grid is (blocks per sample, n_slots) like noise_fill_kernel's; every
// block reads its slot's header and row once and walks the sample's float4s grid-stride.  No atomics, no LDS, vector stores only;
// a sample's result depends on its own slot's words and nothing else.
#include "pool_kernels.h"
#include "noise.h"

namespace ddimx {

constexpr unsigned kPoolTagStep = 0u;  // noise.py TAG_STEP: the noise a sampler step adds

// the position of slot b in its schedule, or -1 when the slot is idle
__device__ __forceinline__ int pool_pos(const int* __restrict__ slots, int b, int max_steps) {
    const int pos = slots[(size_t)b * kPoolSlotWords], len = slots[(size_t)b * kPoolSlotWords + 1];
    return (pos >= 0 && pos < len && len <= max_steps) ? pos : -1;
}

__global__ void pool_begin_kernel(const float* __restrict__ arena, const int* __restrict__ slots, int64_t* __restrict__ t,
                                  int n_slots, int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_slots) return;
    const int pos = pool_pos(slots, b, max_steps);
    t[b] = pos < 0 ? (int64_t)0 : (int64_t)arena[((size_t)b * max_steps + pos) * kPoolStride];
}

__global__ void pool_end_kernel(int* __restrict__ slots, int n_slots, int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_slots) return;
    const int pos = pool_pos(slots, b, max_steps);
    if (pos >= 0) slots[(size_t)b * kPoolSlotWords] = pos + 1;
}

__global__ void __launch_bounds__(kSampleThreads) pool_update_kernel(float* __restrict__ xt, const float* __restrict__ et,
                                                                     float* __restrict__ x0, float* __restrict__ hist,
                                                                     const float* __restrict__ arena, const int* __restrict__ slots,
                                                                     int max_steps, long long n4) {
    const int b = blockIdx.y;
    const int pos = pool_pos(slots, b, max_steps);
    if (pos < 0) return;  // idle slot: nothing of it is touched
    const int* h = slots + (size_t)b * kPoolSlotWords;
    const StepRow r = load_row(arena + ((size_t)b * max_steps + pos) * kPoolStride, true);
    const bool use1 = r.w1 != 0.f, use2 = r.w2 != 0.f, draw_z = r.c1 != 0.f;
    const unsigned k0 = (unsigned)h[2], k1 = (unsigned)h[3], sample = (unsigned)h[4], draw = (unsigned)h[5] + (unsigned)pos;
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kSampleThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kSampleThreads) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (draw_z) noise_normals4((unsigned)i, sample, draw, kPoolTagStep, k0, k1, z);
        update4(xt, et, x0, hist, base + (size_t)i, r, true, use1, use2, draw_z, z);
    }
}

static bool pool_shape_ok(int n_slots, int max_steps) { return n_slots >= 1 && n_slots <= 65535 && max_steps >= 1; }

hipError_t pool_begin_launch(const float* arena, const int* slots, int64_t* t, int n_slots, int max_steps, hipStream_t s) {
    if (!pool_shape_ok(n_slots, max_steps)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_begin_kernel, dim3((n_slots + 63) / 64), dim3(64), 0, s, arena, slots, t, n_slots, max_steps);
    return hipGetLastError();
}

hipError_t pool_update_launch(float* xt, const float* et, float* x0, float* hist, const float* arena, const int* slots, int n_slots,
                              int max_steps, long long per_sample, hipStream_t s) {
    if (!pool_shape_ok(n_slots, max_steps) || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    const long long n4 = per_sample / 4;
    if (n4 > (1LL << 32)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(n_slots, per_sample), n_slots), block(kSampleThreads);
    hipLaunchKernelGGL(pool_update_kernel, grid, block, 0, s, xt, et, x0, hist, arena, slots, max_steps, n4);
    return hipGetLastError();
}

hipError_t pool_end_launch(int* slots, int n_slots, int max_steps, hipStream_t s) {
    if (!pool_shape_ok(n_slots, max_steps)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_end_kernel, dim3((n_slots + 63) / 64), dim3(64), 0, s, slots, n_slots, max_steps);
    return hipGetLastError();
}

}  // namespace ddimx
