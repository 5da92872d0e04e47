// Restoring pool (ddim_audio_amd/restore_pool.py): the update launch of a pool whose slots each follow their own schedule and
// some of which restore -- they carry a known clip y and a mask m, and their known region follows its exact path
// kv = cx x_t + w0 y (+ c1 z) (inpaint_solver_kernels.hip, replacement only: no guidance, no backward).
//
// The tables are the pool's (pool_kernels.hip): slot b's scalars come from row pos[b] of its block of the arena, pos / len / the
// noise identity from the slot table, both read when the launch RUNS.  Word kRpxFlagsWord of the slot's header row holds the
// flags; with kRpxKnown the same row of a second arena ([n_slots][max_steps][kRpxKnownStride]) holds (cx, w0).  pool_begin_kernel
// and pool_end_kernel read neither and frame the forward unchanged.
//
// rpx_pool_update_kernel has pool_update_kernel's grid (blocks per sample, n_slots) and its walk: every block reads its slot's
// header and rows once -- the flags are uniform over the block -- and walks the sample's float4s grid-stride.  Without kRpxKnown
// the body is update4 (step_math.h) with pool_update_kernel's arguments: its bits.  With it, per float4: x stays in registers,
// update4_core gives u and m0 from the pool's history (m1 = x0, m2 = hist; a term is applied iff its weight is non-zero, z is
// noise_normals4 for the slot's identity exactly as in pool_update_kernel), then kv = inpaint_known(x, y, cx, w0, cx != 0),
// kv = fmaf(z, c1, kv) iff c1 != 0, u = inpaint_replace(u, kv, m): inpaint_multistep4<false, true>'s operation order with mt = m0,
// every scalar operation step_math.h's.  A final row (cx = 0, w0 = 1) gives y's bits where m == 1.
//
// Nothing of an idle slot is touched; y and m of a slot without kRpxKnown are not read; hist is read iff w2 != 0.  No atomics, no
// LDS, vector loads and stores only; a sample's result depends on its own slot's words and nothing else.
//
// Memory-bound: per element a known slot reads xt, eps, x0, y, m (+ hist at order 3) and writes xt, x0, hist -- 8 or 9 sample-sized
// passes against pool_update_kernel's 6 or 7.
#include "restore_pool_kernels.h"
#include "noise.h"

namespace ddimx {

constexpr unsigned kRpxTagStep = 0u;  // noise.py TAG_STEP: the noise a sampler step adds

// the position of slot b in its schedule, or -1 when the slot is idle: pool_kernels.hip's rule for the same two words
__device__ __forceinline__ int rpx_pos(const int* __restrict__ h, int max_steps) {
    const int pos = h[0], len = h[1];
    return (pos >= 0 && pos < len && len <= max_steps) ? pos : -1;
}

__global__ void __launch_bounds__(kSampleThreads) rpx_pool_update_kernel(float* __restrict__ xt, const float* __restrict__ et,
                                                                         float* __restrict__ x0, float* __restrict__ hist,
                                                                         const float* __restrict__ y, const float* __restrict__ m,
                                                                         const float* __restrict__ arena, const float* __restrict__ known,
                                                                         const int* __restrict__ slots, int max_steps, long long n4) {
    const int b = blockIdx.y;
    const int* h = slots + (size_t)b * kPoolSlotWords;
    const int pos = rpx_pos(h, max_steps);
    if (pos < 0) return;  // idle slot: nothing of it is touched
    const size_t row = (size_t)b * max_steps + pos;
    const StepRow r = load_row(arena + row * kPoolStride, true);
    const bool use1 = r.w1 != 0.f, use2 = r.w2 != 0.f, draw_z = r.c1 != 0.f;
    const unsigned k0 = (unsigned)h[2], k1 = (unsigned)h[3], sample = (unsigned)h[4], draw = (unsigned)h[5] + (unsigned)pos;
    const size_t base = (size_t)b * (size_t)n4;
    const long long first = (long long)blockIdx.x * kSampleThreads + threadIdx.x, stride = (long long)gridDim.x * kSampleThreads;
    if (!(h[kRpxFlagsWord] & kRpxKnown)) {  // pool_update_kernel's body
        for (long long i = first; i < n4; i += stride) {
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (draw_z) noise_normals4((unsigned)i, sample, draw, kRpxTagStep, k0, k1, z);
            update4(xt, et, x0, hist, base + (size_t)i, r, true, use1, use2, draw_z, z);
        }
        return;
    }
    const float cx = known[row * kRpxKnownStride], w0 = known[row * kRpxKnownStride + 1];
    const bool use_x = cx != 0.f;
    for (long long i = first; i < n4; i += stride) {
        const size_t at = base + (size_t)i;
        float x[4], u[4], e[4], ys[4], ms[4], m1[4], m2[4] = {0.f, 0.f, 0.f, 0.f}, m0[4], z[4] = {0.f, 0.f, 0.f, 0.f};
        load4(xt, at, x);
        load4(et, at, e);
        load4(x0, at, m1);  // always read and always kept, as in update4h with a history buffer
        if (use2) load4(hist, at, m2);
        load4(y, at, ys);
        load4(m, at, ms);
        if (draw_z) noise_normals4((unsigned)i, sample, draw, kRpxTagStep, k0, k1, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = x[q];
        update4_core(u, e, m1, m2, m0, r, use1, use2, draw_z, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float kv = inpaint_known(x[q], ys[q], cx, w0, use_x);
            if (draw_z) kv = fmaf(z[q], r.c1, kv);
            u[q] = inpaint_replace(u[q], kv, ms[q]);
        }
        store4(hist, at, m1);
        store4(x0, at, m0);
        store4(xt, at, u);
    }
}

hipError_t rpx_pool_update_launch(float* xt, const float* et, float* x0, float* hist, const float* y, const float* m, const float* arena,
                                  const float* known, const int* slots, int n_slots, int max_steps, long long per_sample, hipStream_t s) {
    if (n_slots < 1 || n_slots > 65535 || max_steps < 1 || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    const long long n4 = per_sample / 4;
    if (n4 > (1LL << 32)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(n_slots, per_sample), n_slots), block(kSampleThreads);
    hipLaunchKernelGGL(rpx_pool_update_kernel, grid, block, 0, s, xt, et, x0, hist, y, m, arena, known, slots, max_steps, n4);
    return hipGetLastError();
}

}  // namespace ddimx
