// Weight gradients of the MFMA convolutions (wgrad_mfma.h), the part that is not a template instance: the dtype dispatch
// over wgrad_inst_*.hip and the fixed-order reduction of the per-workgroup partial slabs.  gfx950 only.
#include "wgrad_reduce.h"

namespace ddimx {

hipError_t wgrad_geometry_bf16(int, int, int, WgradGeom*);
hipError_t wgrad_geometry_f32(int, int, int, WgradGeom*);
hipError_t wgrad_launch_bf16(int, int, int, const WgradArgs&, int, hipStream_t);
hipError_t wgrad_launch_f32(int, int, int, const WgradArgs&, int, hipStream_t);
hipError_t wgrad_geometry(int dtype, int mode, int ci, int co, WgradGeom* g) {
    return dtype == DT_BF16 ? wgrad_geometry_bf16(mode, ci, co, g) : wgrad_geometry_f32(mode, ci, co, g);
}
hipError_t wgrad_launch(int dtype, int mode, int ci, int co, const WgradArgs& a, int nsplit, hipStream_t s) {
    return dtype == DT_BF16 ? wgrad_launch_bf16(mode, ci, co, a, nsplit, s) : wgrad_launch_f32(mode, ci, co, a, nsplit, s);
}

// dst[co][ci][tap] = sum_s partial[s][tap][co][ci]; KS threads share an output (splits s = q, q+KS, ...: loads unrolled so
// that eight are in flight per thread), folded in a fixed order through LDS
template <int KS>
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ partial, int nsplit, int ntaps, int co,
                                                           int ci, float* __restrict__ dst) {
    constexpr int OUT = 256 / KS;
    __shared__ double red[KS][OUT];
    const int n = ntaps * co * ci;
    const int ol = threadIdx.x % OUT, q = threadIdx.x / OUT;
    const int i = blockIdx.x * OUT + ol;
    double s = 0.0;
    if (i < n) {  // strided_sum8<KS> (common.h), kept as a copy: through the helper one of two timed runs fell outside the copy's spread
        int k = q;
        for (; k + 7 * KS < nsplit; k += 8 * KS) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(k + u * KS) * n + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (double)v[u];
        }
        for (; k < nsplit; k += KS) s += (double)partial[(size_t)k * n + i];
    }
    red[q][ol] = s;
    __syncthreads();
    if (q == 0 && i < n) {
        s = 0.0;
#pragma unroll
        for (int k = 0; k < KS; ++k) s += red[k][ol];
        const int c = i % ci, o = (i / ci) % co, tap = i / (ci * co);
        dst[((size_t)o * ci + c) * ntaps + tap] = (float)s;
    }
}
// The same sums in the same order (split s = q, q + 16, ... per thread, then the 16 partial sums in order), four consecutive
// outputs per thread: a 16-byte load per split instead of four 4-byte ones, 256 contiguous bytes of a slab per workgroup
// instead of 64 (the scalar form moved 19 MB of level-0 slabs in 21 us; round 3: 48 launches per step).  n % 4 == 0.
__global__ void __launch_bounds__(256) wgrad_reduce4_kernel(const float* __restrict__ partial, int nsplit, int ntaps, int co, int ci,
                                                            float* __restrict__ dst) {
    constexpr int KS = 16, OG = 16;  // 16 split groups x 16 output quads = 64 outputs per workgroup
    __shared__ double red[KS][OG * 4];
    const int n = ntaps * co * ci;
    const int og = threadIdx.x % OG, q = threadIdx.x / OG;
    const int i0 = (blockIdx.x * OG + og) * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (i0 < n) {
        int k = q;
        for (; k + 7 * KS < nsplit; k += 8 * KS) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *(const float4*)(partial + (size_t)(k + u * KS) * n + i0);
#pragma unroll
            for (int u = 0; u < 8; ++u) { s0 += (double)v[u].x; s1 += (double)v[u].y; s2 += (double)v[u].z; s3 += (double)v[u].w; }
        }
        for (; k < nsplit; k += KS) {
            const float4 v = *(const float4*)(partial + (size_t)k * n + i0);
            s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
        }
    }
    red[q][og * 4 + 0] = s0; red[q][og * 4 + 1] = s1; red[q][og * 4 + 2] = s2; red[q][og * 4 + 3] = s3;
    __syncthreads();
    const int ol = threadIdx.x, i = blockIdx.x * OG * 4 + ol;
    if (ol < OG * 4 && i < n) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < KS; ++k) t += red[k][ol];
        const int c = i % ci, o = (i / ci) % co, tap = i / (ci * co);
        dst[((size_t)o * ci + c) * ntaps + tap] = (float)t;
    }
}
int wgrad_reduce_kind(int nsplit, int ntaps, int co, int ci) {
    const int n = ntaps * co * ci;
    if (nsplit >= 64 && n % 4 == 0) return WGRAD_REDUCE_QUAD;  // many thin slabs (levels 0-2): 16 threads per output quad
    return nsplit >= 64 ? WGRAD_REDUCE_KS16 : WGRAD_REDUCE_KS4;
}
hipError_t wgrad_reduce_launch(const float* partial, int nsplit, int ntaps, int co, int ci, float* dst, hipStream_t s) {
    const int n = ntaps * co * ci;
    switch (wgrad_reduce_kind(nsplit, ntaps, co, ci)) {
    case WGRAD_REDUCE_QUAD:
        hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3((n + 63) / 64), dim3(256), 0, s, partial, nsplit, ntaps, co, ci, dst);
        break;
    case WGRAD_REDUCE_KS16:
        hipLaunchKernelGGL(wgrad_reduce_kernel<16>, dim3((n + 15) / 16), dim3(256), 0, s, partial, nsplit, ntaps, co, ci, dst);
        break;
    default:
        hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3((n + 63) / 64), dim3(256), 0, s, partial, nsplit, ntaps, co, ci, dst);
    }
    return hipGetLastError();
}

}  // namespace ddimx
