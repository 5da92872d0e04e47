// Sampler pool (ddim_audio_amd/pool.py): the three launches that frame the forward of a batch whose samples each follow their own
// schedule -- DDIM with any eta or DPM-Solver++ of orders 1-3 -- from their own position in it.
//
// Slot b's scalars come from row pos[b] of its own block of the coefficient arena ([n_slots][max_steps][kPoolStride] fp32, the
// solver's row (t, s1, s2, s3, c2, c1, w1, w2)); pos, the schedule's length and the slot's noise identity live in the slot table
// ([n_slots][kPoolSlotWords] int32: pos, len, seed_lo, seed_hi, sample, draw_base, 2 reserved).  Both are device memory read when
// the launch RUNS, so one captured step serves every mix of requests.  A slot is active iff 0 <= pos < len <= max_steps; no kernel
// reads or writes the sample, the prediction or the history of an idle slot, and none reads the arena beyond an active row.
//
// pool_update_kernel, per element of an active slot and in this order (m1 = x0 on entry, m2 = hist on entry):
//   m0 = (x - s1 e) / s2                       ddim_x0    (step_math.h)
//   u  = s3 m0 + c2 e                          ddim_next
//   u  = u + w1 (m0 - m1)     if w1 != 0       fmaf(w1, __fsub_rn(m0, m1), u)
//   u  = u + w2 (m1 - m2)     if w2 != 0       fmaf(w2, __fsub_rn(m1, m2), u)
//   u  = u + c1 z             if c1 != 0       fmaf(z, c1, u)
//   xt <- u, x0 <- m0, hist <- m1
// the operations and the order of ddim_update_kernel (c1) and multistep_update_kernel (w1, w2), whose bits it gives row for row.
// z is the normal of noise.h for the counter (group of four, sample, draw_base + pos, tag 0) under the key (seed_lo, seed_hi):
// element for element what noise_fill_kernel writes for that sample and draw, formed here from the same two functions, so there
// is no noise buffer and no fill launch.  All conditions are uniform over a block (the row's scalars).  The grid is (blocks per
// sample, n_slots) like noise_fill_kernel's; every block reads its slot's header and row once and walks the sample's float4s
// grid-stride.  No atomics, no LDS, vector stores only; a sample's result depends on its own slot's words and nothing else.
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
    const float* c = arena + ((size_t)b * max_steps + pos) * kPoolStride;
    const float s1 = c[1], s2 = c[2], s3 = c[3], c2 = c[4], c1 = c[5], w1 = c[6], w2 = c[7];
    const bool use1 = w1 != 0.f, use2 = w2 != 0.f, draw_z = c1 != 0.f;
    const unsigned k0 = (unsigned)h[2], k1 = (unsigned)h[3], sample = (unsigned)h[4], draw = (unsigned)h[5] + (unsigned)pos;
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kSampleThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kSampleThreads) {
        const size_t at = base + (size_t)i;
        const float4 x = ((const float4*)xt)[at];
        const float4 e = ((const float4*)et)[at];
        const float4 p = ((const float4*)x0)[at];
        const float xs[4] = {x.x, x.y, x.z, x.w}, es[4] = {e.x, e.y, e.z, e.w}, m1[4] = {p.x, p.y, p.z, p.w};
        float m2[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        if (use2) { const float4 v = ((const float4*)hist)[at]; m2[0] = v.x; m2[1] = v.y; m2[2] = v.z; m2[3] = v.w; }
        if (draw_z) {
            unsigned w[4] = {(unsigned)i, sample, draw, kPoolTagStep};
            philox4x32_10(w, k0, k1);
            noise_pair(w[0], w[1], z[0], z[1]);
            noise_pair(w[2], w[3], z[2], z[3]);
        }
        float p0[4], out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m0 = ddim_x0(xs[j], es[j], s1, s2);
            float u = ddim_next(m0, es[j], s3, c2);
            if (use1) u = fmaf(w1, __fsub_rn(m0, m1[j]), u);
            if (use2) u = fmaf(w2, __fsub_rn(m1[j], m2[j]), u);
            if (draw_z) u = fmaf(z[j], c1, u);
            p0[j] = m0;
            out[j] = u;
        }
        ((float4*)hist)[at] = make_float4(m1[0], m1[1], m1[2], m1[3]);
        ((float4*)x0)[at] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        ((float4*)xt)[at] = make_float4(out[0], out[1], out[2], out[3]);
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
