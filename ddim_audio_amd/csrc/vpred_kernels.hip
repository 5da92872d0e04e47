// v-prediction (Salimans & Ho 2022): v = sqrt(a) e - sqrt(1 - a) x0, so x0 = s2 x - s1 v and eps = s1 x + s2 v with
// s1 = sqrt(1 - a_t), s2 = sqrt(a_t).
//
// v_to_eps_kernel turns the output of a network that predicts v into the eps every update kernel reads, in fp32 and in one launch
// between the forward and the update: the update arithmetic (step_math.h) keeps its one copy, and an error d of the network
// output reaches the x0 prediction as (s1 / s2) s2 d = s1 d.  Sample b's scalars are row t[b] of the table [n_table][2] -- t is
// the int64 timestep tensor the network itself was given, device memory read when the launch RUNS, so one captured launch serves
// every replay and every stepper (one counter, windows, the pool's slots).  A t[b] outside the table leaves the sample alone.
//
// qsample_v_kernel is the training side: the noised sample (qsample_kernel's bits) and the v target from one read of x0 and e.
//
// Both grids are (blocks per sample, B) like noise_fill_kernel's: every block belongs to one sample, whose float4s it walks
// grid-stride, consecutive threads on consecutive groups.  No LDS, no atomics, vector stores only; every element is read before
// it is written by the same thread, so eps may alias v; a sample's result does not depend on B or on the grid.
#include "vpred_kernels.h"

namespace ddimx {

__global__ void __launch_bounds__(kVpredThreads) v_to_eps_kernel(const float* __restrict__ x, const float* v, float* eps,
                                                                 const float* __restrict__ vtab, int n_table,
                                                                 const int64_t* __restrict__ t, long long n4) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    if (tb < 0 || tb >= (int64_t)n_table) return;  // uniform over the block
    const float s1 = vtab[2 * tb], s2 = vtab[2 * tb + 1];
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kVpredThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kVpredThreads) {
        const size_t at = base + (size_t)i;
        const float4 xv = ((const float4*)x)[at];
        const float4 vv = ((const float4*)v)[at];
        ((float4*)eps)[at] = make_float4(v_to_eps(xv.x, vv.x, s1, s2), v_to_eps(xv.y, vv.y, s1, s2), v_to_eps(xv.z, vv.z, s1, s2),
                                         v_to_eps(xv.w, vv.w, s1, s2));
    }
}

// The two outputs of the q-sample.  Plain operators under contract(off): every operation written here is rounded once and none is
// fused (the pragma does not reach into the __f*_rn wrappers, whose bodies carry their own header's setting).
__device__ __forceinline__ float qsample_v_target(float x0, float e, float sa, float sb) {
#pragma clang fp contract(off)
    return e * sa - x0 * sb;
}
// x is ddimx_qsample's bit for bit: both kernels take it from qsample_x (step_math.h).  tests/test_gpu_vpred.py::test_qsample_v pins it.

__global__ void __launch_bounds__(kVpredThreads) qsample_v_kernel(const float* __restrict__ x0, const float* __restrict__ e,
                                                                  const float* __restrict__ alphas, const int64_t* __restrict__ t,
                                                                  float* __restrict__ x, float* __restrict__ v, long long n4) {
    const int b = blockIdx.y;
    const float a = alphas[t[b]];
    const float sa = __fsqrt_rn(a), sb = __fsqrt_rn(__fsub_rn(1.0f, a));  // qsample_kernel's
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kVpredThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kVpredThreads) {
        const size_t at = base + (size_t)i;
        const float4 p = ((const float4*)x0)[at];
        const float4 q = ((const float4*)e)[at];
        const float ps[4] = {p.x, p.y, p.z, p.w}, qs[4] = {q.x, q.y, q.z, q.w};
        float xs[4], vs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xs[j] = qsample_x(ps[j], qs[j], sa, sb);
            vs[j] = qsample_v_target(ps[j], qs[j], sa, sb);
        }
        ((float4*)x)[at] = make_float4(xs[0], xs[1], xs[2], xs[3]);
        ((float4*)v)[at] = make_float4(vs[0], vs[1], vs[2], vs[3]);
    }
}

static bool vpred_shape_ok(int B, long long per_sample) { return B >= 1 && B <= 65535 && per_sample > 0 && per_sample % 4 == 0; }

hipError_t v_to_eps_launch(const float* x, const float* v, float* eps, const float* vtab, int n_table, const int64_t* t, int B,
                           long long per_sample, hipStream_t s) {
    if (!vpred_shape_ok(B, per_sample) || n_table < 1) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kVpredThreads);
    hipLaunchKernelGGL(v_to_eps_kernel, grid, block, 0, s, x, v, eps, vtab, n_table, t, per_sample / 4);
    return hipGetLastError();
}

hipError_t qsample_v_launch(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, float* v, int B,
                            long long per_sample, hipStream_t s) {
    if (!vpred_shape_ok(B, per_sample)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kVpredThreads);
    hipLaunchKernelGGL(qsample_v_kernel, grid, block, 0, s, x0, e, alphas, t, x, v, per_sample / 4);
    return hipGetLastError();
}

}  // namespace ddimx
