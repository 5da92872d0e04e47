// Static clipping and dynamic thresholding of the x0 prediction (Saharia et al. 2022, section 2.3; the reason DPM-Solver++ is
// written in its data-prediction form, Lu et al. 2022, section 4), between the network's eps and the unchanged update kernels.
// gfx950 only.  The arithmetic and its rounding contract are step_math.h's.
//
// The dynamic threshold needs, per sample, the exact order statistic of |x0| at a rank the host computed.  x0_hist_kernel<PASS>
// is one digit pass of a radix select on the keys bits(x0) & 0x7FFFFFFF (threshold_kernels.h): it recomputes x0 for its float4s
// from (x, eps), keeps the elements whose higher digits equal the ones chosen so far, counts them by this pass's digit in LDS and
// adds its non-empty bins to the sample's global histogram with integer atomics.  What was chosen so far is not handed over by
// the previous launch: every block scans the previous histograms (at most 12 KB, served by L2) itself -- the consumer-folds idiom of
// gn_fused.h.  x0_finish_kernel scans all three, writes (s, r) and clears the sample's histograms (the zero contract of
// threshold_kernels.h).  threshold_eps_kernel rewrites eps in one pass.
//
// Grids are (blocks per sample, B) like v_to_eps_kernel's: every block belongs to one sample, whose float4s it walks grid-stride
// with unconditional loads; what an element contributes is decided by select after the loads.  Sample b's scalars are row t[b] of
// the table, read when the launch RUNS; a t[b] outside the table makes every block of the sample return at once.  Vector stores
// only; a sample's result does not depend on B or on the grid.
#include "threshold_kernels.h"

namespace ddimx {

// The bin d of hist[NB] with cum(d - 1) <= rank < cum(d), to every thread; rank becomes rank - cum(d - 1), the rank among the
// elements of that bin.  Thread i sums bins [i PER, (i + 1) PER), the block scans the sums, and the one thread whose range holds
// the rank walks its own bins.  sh: 6 words of LDS.
template <int NB>
__device__ __forceinline__ unsigned select_bin(const unsigned* hist, unsigned& rank, unsigned* sh) {
    constexpr int PER = NB / kThreshThreads;
    static_assert(PER % 4 == 0 && PER * kThreshThreads == NB, "uint4 loads, every bin read once");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned c[PER];
#pragma unroll
    for (int j = 0; j < PER / 4; ++j) {
        const uint4 v = ((const uint4*)hist)[tid * (PER / 4) + j];
        c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
    }
    unsigned local = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) local += c[j];
    unsigned inc = local;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    __syncthreads();  // sh may still be read by an earlier call
    if (lane == 63) sh[w] = inc;
    if (tid == 0) sh[4] = sh[5] = 0;
    __syncthreads();
    unsigned excl = inc - local;
    for (int i = 0; i < w; ++i) excl += sh[i];
    if (rank >= excl && rank - excl < local) {  // one thread at the most; the zeros above are behind the barrier
        unsigned rem = rank - excl, d = 0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const bool here = !found && rem < c[j];
            d = here ? (unsigned)j : d;
            rem = (found || here) ? rem : rem - c[j];
            found = found || here;
        }
        sh[4] = (unsigned)tid * PER + d;
        sh[5] = rem;
    }
    __syncthreads();
    rank = sh[5];
    return sh[4];
}

template <int PASS>
__global__ void __launch_bounds__(kThreshThreads) x0_hist_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                                 const float* __restrict__ tab, int n_table,
                                                                 const int64_t* __restrict__ t, unsigned* work, unsigned rank,
                                                                 long long n4) {
    constexpr int NB = PASS == 0 ? kBins0 : kBins12;
    constexpr int OUT = PASS == 0 ? 0 : (PASS == 1 ? kBins0 : kBins0 + kBins12);
    __shared__ unsigned bins[NB];
    __shared__ unsigned sh[6];
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    if (tb < 0 || tb >= (int64_t)n_table) return;  // uniform over the block
    const float s1 = tab[2 * tb], s2 = tab[2 * tb + 1];
    unsigned* hist = work + (size_t)b * kQuantileWords;
    for (int i = threadIdx.x; i < NB; i += kThreshThreads) bins[i] = 0;
    unsigned prefix = 0;  // the digits chosen so far, in place
    if (PASS >= 1) prefix = select_bin<kBins0>(hist, rank, sh) << 20;
    if (PASS >= 2) prefix |= select_bin<kBins12>(hist + kBins0, rank, sh) << 10;
    __syncthreads();
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kThreshThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kThreshThreads) {
        const size_t at = base + (size_t)i;
        const float4 xv = ((const float4*)x)[at];
        const float4 ev = ((const float4*)eps)[at];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, es[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned key = __float_as_uint(ddim_x0(xs[j], es[j], s1, s2)) & 0x7FFFFFFFu;
            if (PASS == 0) {
                atomicAdd(&bins[key >> 20], 1u);
            } else if (PASS == 1) {
                if ((key >> 20) == (prefix >> 20)) atomicAdd(&bins[(key >> 10) & 1023u], 1u);
            } else {
                if ((key >> 10) == (prefix >> 10)) atomicAdd(&bins[key & 1023u], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NB; i += kThreshThreads) {
        const unsigned c = bins[i];
        if (c) atomicAdd(&hist[OUT + i], c);
    }
}

__global__ void __launch_bounds__(kThreshThreads) x0_finish_kernel(const float* __restrict__ tab, int n_table,
                                                                   const int64_t* __restrict__ t, unsigned* work, unsigned rank,
                                                                   float floor, float ceil, float* __restrict__ scale) {
    __shared__ unsigned sh[6];
    const int b = blockIdx.x;
    const int64_t tb = t[b];
    if (tb < 0 || tb >= (int64_t)n_table) return;
    unsigned* hist = work + (size_t)b * kQuantileWords;
    unsigned key = select_bin<kBins0>(hist, rank, sh) << 20;
    key |= select_bin<kBins12>(hist + kBins0, rank, sh) << 10;
    key |= select_bin<kBins12>(hist + kBins0 + kBins12, rank, sh);
    if (threadIdx.x == 0) {
        const float s = x0_scale(__uint_as_float(key), floor, ceil);
        scale[2 * b] = s;
        scale[2 * b + 1] = __fdiv_rn(floor, s);
    }
    // every thread's loads of the histograms lie in front of select_bin's last barrier
    for (int i = threadIdx.x; i < kQuantileWords / 4; i += kThreshThreads) ((uint4*)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void __launch_bounds__(kThreshThreads) threshold_eps_kernel(const float* __restrict__ x, const float* eps_in, float* eps_out,
                                                                       const float* __restrict__ scale, const float* __restrict__ tab,
                                                                       int n_table, const int64_t* __restrict__ t, long long n4) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    if (tb < 0 || tb >= (int64_t)n_table) return;  // uniform over the block
    const float s1 = tab[2 * tb], s2 = tab[2 * tb + 1];
    const float s = scale[2 * b], r = scale[2 * b + 1];
    const size_t base = (size_t)b * (size_t)n4;
    for (long long i = (long long)blockIdx.x * kThreshThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kThreshThreads) {
        const size_t at = base + (size_t)i;
        const float4 xv = ((const float4*)x)[at];
        const float4 ev = ((const float4*)eps_in)[at];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, es[4] = {ev.x, ev.y, ev.z, ev.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x0 = ddim_x0(xs[j], es[j], s1, s2);
            o[j] = x0_to_eps(xs[j], es[j], x0, x0_clip(x0, s, r), s1, s2);
        }
        ((float4*)eps_out)[at] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

static bool thresh_shape_ok(int B, long long per_sample, int n_table) {
    return B >= 1 && B <= 65535 && per_sample > 0 && per_sample % 4 == 0 && per_sample < (1LL << 31) && n_table >= 1;
}

hipError_t x0_quantile_launch(const float* x, const float* eps, const float* tab, int n_table, const int64_t* t, long long rank,
                              float floor, float ceil, void* work, float* scale, int B, long long per_sample, hipStream_t s) {
    if (!thresh_shape_ok(B, per_sample, n_table) || rank < 0 || rank >= per_sample) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kThreshThreads);
    unsigned* w = (unsigned*)work;
    const unsigned k = (unsigned)rank;
    hipLaunchKernelGGL(x0_hist_kernel<0>, grid, block, 0, s, x, eps, tab, n_table, t, w, k, per_sample / 4);
    hipLaunchKernelGGL(x0_hist_kernel<1>, grid, block, 0, s, x, eps, tab, n_table, t, w, k, per_sample / 4);
    hipLaunchKernelGGL(x0_hist_kernel<2>, grid, block, 0, s, x, eps, tab, n_table, t, w, k, per_sample / 4);
    hipLaunchKernelGGL(x0_finish_kernel, dim3(B), block, 0, s, tab, n_table, t, w, k, floor, ceil, scale);
    return hipGetLastError();
}

hipError_t threshold_eps_launch(const float* x, const float* eps_in, float* eps_out, const float* scale, const float* tab, int n_table,
                                const int64_t* t, int B, long long per_sample, hipStream_t s) {
    if (!thresh_shape_ok(B, per_sample, n_table)) return hipErrorInvalidValue;
    const dim3 grid(sample_blocks(B, per_sample), B), block(kThreshThreads);
    hipLaunchKernelGGL(threshold_eps_kernel, grid, block, 0, s, x, eps_in, eps_out, scale, tab, n_table, t, per_sample / 4);
    return hipGetLastError();
}

}  // namespace ddimx
