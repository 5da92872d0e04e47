// SDE-DPM-Solver++ on one Brownian path (BrownianStream in ddim_audio_amd/noise.py; include/ddimx_brownian.h states the path and the
// plan row): the noise of the step i -> j is z = (P(j) - P(i)) g, P(t) = W(u_t) the value at level t of
// one Brownian motion per element, so runs of different step counts from one seed follow the same path.
//
// P(t) is a pure function of (seed, global sample, element, t): the descent from the root of a virtual binary tree over the timestep
// index, one Brownian-bridge midpoint per node, whose normal is noise_normals4 (noise.h) for the counter (group of four, sample,
// node id, tag 2).  The host (schedule.brownian_plan) lists, per step, the records (node id, rho, s, enter) of the two descents and
// how many leading ones they share; the kernel stages that row -- uniform over the launch -- in LDS once per block and walks it
// per group of four elements: the shared records once, then the rest of either descent.  Every operation is rounded once and in the
// header's order, and P(t) is always the whole descent, so its bits do not depend on the step that asks for it.
//
// The update is update4 (step_math.h) on row step[0] of the solver's table, as in sde_kernels.hip, with the same flags, grid and
// block.  No atomics, no LDS writes but the staging of the row, no noise buffer, no fill launch, vector stores only; a sample's
// result depends on (seed, its global index) and on nothing else of the batch.
#include "brownian_kernels.h"
#include "noise.h"

namespace ddimx {

constexpr unsigned kBrownianTag = 2u;  // DDIMXB_NOISE_TAG, noise.py TAG_PATH
enum { kEnterAnchor = 0, kEnterRoot = 1, kEnterLeft = 2, kEnterRight = 3 };  // DDIMXB_ENTER_*

// the ends a, b of the current node's interval and its midpoint m, for four elements
struct BrownianState { float a[4], b[4], m[4]; };

// the row of a launch into LDS, once per block
__device__ __forceinline__ void brownian_stage(int* row, const int* __restrict__ src) {
    for (int k = threadIdx.x; k < kBrownianStride; k += kSampleThreads) row[k] = src[k];
    __syncthreads();
}

// records [from, to) of one descent (rec: its record 0 in the staged row) on the state the records before them left
__device__ __forceinline__ void brownian_walk(const int* rec, int from, int to, unsigned q, unsigned sample, unsigned k0, unsigned k1,
                                              BrownianState& p) {
#pragma clang fp contract(off)
    for (int r = from; r < to; ++r) {
        const int node = rec[4 * r], enter = rec[4 * r + 3];
        const float rho = __int_as_float(rec[4 * r + 1]), s = __int_as_float(rec[4 * r + 2]);
        float xi[4];
        noise_normals4(q, sample, (unsigned)node, kBrownianTag, k0, k1, xi);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (enter == kEnterAnchor) {  // P(0) = sqrt(u0) xi_0, P(N) = 0
                p.m[j] = __fmul_rn(s, xi[j]);
                p.a[j] = p.m[j];
                p.b[j] = 0.f;
            } else {
                if (enter == kEnterLeft) p.b[j] = p.m[j];
                if (enter == kEnterRight) p.a[j] = p.m[j];
                const float d = __fsub_rn(p.a[j], p.b[j]);
                p.m[j] = fmaf(s, xi[j], fmaf(rho, d, p.b[j]));
            }
        }
    }
}

// P(i) and P(j) of the staged row for group q of `sample`: the shared records once, then the rest of either descent.  The counts
// are clamped to the row's extent, so no word outside the staged row is read whatever the table holds.
__device__ __forceinline__ void brownian_eval4(const int* row, unsigned q, unsigned sample, unsigned k0, unsigned k1, float pi[4],
                                               float pj[4]) {
    const int ni = min(max(row[1], 0), kBrownianRecords), nj = min(max(row[2], 0), kBrownianRecords);
    const int share = min(max(row[0], 0), min(ni, nj));
    const int* ri = row + 4;
    const int* rj = row + 4 + 4 * kBrownianRecords;
    BrownianState sj = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    brownian_walk(rj, 0, share, q, sample, k0, k1, sj);
    BrownianState si = sj;
    brownian_walk(ri, share, ni, q, sample, k0, k1, si);
    brownian_walk(rj, share, nj, q, sample, k0, k1, sj);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pi[j] = si.m[j];
        pj[j] = sj.m[j];
    }
}

// z = (P(j) - P(i)) g
__device__ __forceinline__ void brownian_increment4(const int* row, unsigned q, unsigned sample, unsigned k0, unsigned k1, float z[4]) {
#pragma clang fp contract(off)
    float pi[4], pj[4];
    brownian_eval4(row, q, sample, k0, k1, pi, pj);
    const float g = __int_as_float(row[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = __fmul_rn(__fsub_rn(pj[j], pi[j]), g);
}

__global__ void __launch_bounds__(kSampleThreads) brownian_multistep_update_kernel(float* __restrict__ xt, const float* __restrict__ et,
                                                                                   float* __restrict__ x0, float* __restrict__ hist,
                                                                                   const float* __restrict__ coef,
                                                                                   const int* __restrict__ plan,
                                                                                   const int* __restrict__ step, long long n4, unsigned k0,
                                                                                   unsigned k1, unsigned first_sample) {
    __shared__ int row[kBrownianStride];
    const int pos = step[0];
    brownian_stage(row, plan + (size_t)pos * kBrownianStride);
    const StepRow r = load_row(coef + (size_t)pos * kSolverStride, true);
    const bool use1 = r.w1 != 0.f, use2 = r.w2 != 0.f && hist != nullptr, add_z = r.c1 != 0.f;
    const bool load1 = use1 || use2 || hist != nullptr;
    const unsigned sample = first_sample + blockIdx.y;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kSampleThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kSampleThreads) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (add_z) brownian_increment4(row, (unsigned)i, sample, k0, k1, z);
        update4(xt, et, x0, hist, base + (size_t)i, r, load1, use1, use2, add_z, z);
    }
}

__global__ void __launch_bounds__(kSampleThreads) brownian_path_fill_kernel(float* __restrict__ out, const int* __restrict__ plan_row,
                                                                            long long n4, unsigned k0, unsigned k1, unsigned first_sample,
                                                                            int kind) {
    __shared__ int row[kBrownianStride];
    brownian_stage(row, plan_row);
    const unsigned sample = first_sample + blockIdx.y;
    const size_t base = (size_t)blockIdx.y * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kSampleThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kSampleThreads) {
        float pi[4], v[4];
        if (kind == kBrownianIncrement)
            brownian_increment4(row, (unsigned)i, sample, k0, k1, v);
        else
            brownian_eval4(row, (unsigned)i, sample, k0, k1, pi, v);
        store4(out, base + (size_t)i, v);
    }
}

static bool brownian_shape_ok(int B, long long per_sample, unsigned first_sample) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return false;
    return per_sample / 4 <= (1LL << 32) && (unsigned long long)first_sample + (unsigned long long)B <= (1ULL << 32);
}

hipError_t brownian_multistep_update_launch(float* xt, const float* et, float* x0, float* hist, const float* coef, const int* plan,
                                            const int* step, int B, long long per_sample, unsigned long long seed, unsigned first_sample,
                                            hipStream_t s) {
    if (!brownian_shape_ok(B, per_sample, first_sample)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kSampleThreads);
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    hipLaunchKernelGGL(brownian_multistep_update_kernel, grid, block, 0, s, xt, et, x0, hist, coef, plan, step, per_sample / 4, k0, k1,
                       first_sample);
    return hipGetLastError();
}

hipError_t brownian_path_fill_launch(float* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample,
                                     const int* plan_row, int kind, hipStream_t s) {
    if (!brownian_shape_ok(B, per_sample, first_sample) || (kind != kBrownianPath && kind != kBrownianIncrement))
        return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kSampleThreads);
    const unsigned k0 = (unsigned)(seed & 0xffffffffULL), k1 = (unsigned)(seed >> 32);
    hipLaunchKernelGGL(brownian_path_fill_kernel, grid, block, 0, s, out, plan_row, per_sample / 4, k0, k1, first_sample, kind);
    return hipGetLastError();
}

}  // namespace ddimx
