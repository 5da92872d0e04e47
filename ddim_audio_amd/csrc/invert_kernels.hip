// DDIM inversion with fixed-point refinement (ddim_audio_amd/invert.py) and the spherical interpolation of latents.
//
// invert_update_kernel: one row of the inversion table (kInvertStride floats: t, s1 = sqrt(1-a_i), s2 = sqrt(a_i),
// p = sqrt(a_i / a_j), q = s1 - p sqrt(1-a_j), first -- schedule.invert_coefficients), selected by the device counter, so one
// captured step replays for every network evaluation of every level.  With x_old = xt on entry, per element and in this order:
//   base = x_old (and base <- x_old)   if the row's `first` flag is set (uniform), else base is read: the first evaluation of a
//                                       level never depends on what the buffer held
//   x0    = (x_old - s1 e) / s2         ddim_x0 (step_math.h)
//   x_new = p base + q e                fmaf(e, q, __fmul_rn(p, base))         xt <- x_new
// and the residual of the fixed-point iteration, r = |x_new - x_old|_2 / |x_new|_2 per sample, for the log: the grid is
// (blocks per sample, B) like the inpainting kernels', every block writes its two sums as doubles (the difference of two fp32
// values and the square of one are formed in double: no rounding that an fp64 restatement would not make too), and
// invert_residual_kernel adds a sample's partials in one fixed order.  No atomics.  xt and x0 never depend on the sums.
//
// slerp: cos(theta) = <z1, z2> / (|z1| |z2|) over the whole pair, out[m] = a_m z1 + b_m z2 with a_m = sin((1 - w_m) theta) /
// sin(theta), b_m = sin(w_m theta) / sin(theta); the three sums as above, theta and the coefficients in double and rounded once.
#include "invert_kernels.h"

namespace ddimx {

// a sample's `nparts` partials of sum `which` (of `nsums` interleaved ones), thread i adding partials i, i + 256, ... first
__device__ __forceinline__ double invert_partials_sum(const double* ps, int nparts, int nsums, int which, double* red) {
    double v = 0.0;
    for (int p = threadIdx.x; p < nparts; p += kInvertThreads) v += ps[(size_t)p * nsums + which];
    return block_sum(v, red);
}

template <bool NT>
__global__ void __launch_bounds__(kInvertThreads) invert_update_kernel(
    float* __restrict__ xt, const float* __restrict__ et, float* __restrict__ base, float* __restrict__ x0,
    double* __restrict__ partials, int rows, const float* __restrict__ coef, const int* __restrict__ step, long long n4) {
    __shared__ double red[kInvertThreads / 64];
    const int row = step[0];
    if (row < 0 || row >= rows) return;  // uniform: the whole grid leaves
    const float* c = coef + (size_t)row * kInvertStride;
    const float s1 = c[1], s2 = c[2], p = c[3], q = c[4];
    const bool first = c[5] != 0.f;
    const size_t off = (size_t)blockIdx.y * (size_t)n4;
    double dd = 0.0, nn = 0.0;
    for (long long i = (long long)blockIdx.x * kInvertThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInvertThreads) {
        const size_t j = off + (size_t)i;
        const float4 x4 = ((const float4*)xt)[j];
        float xs[4] = {x4.x, x4.y, x4.z, x4.w}, es[4], bs[4], p0[4];
        Piece<float>::unpack(NT ? nt_load16((const float4*)et + j) : *(const uint4*)((const float4*)et + j), es);
        if (first) {
            // written once per level, read by its later iterations only: past the cache when the tensors do not fit it
            if (NT) nt_store16((float4*)base + j, Piece<float>::pack(xs));
            else ((float4*)base)[j] = x4;
            bs[0] = xs[0]; bs[1] = xs[1]; bs[2] = xs[2]; bs[3] = xs[3];
        } else {
            Piece<float>::unpack(NT ? nt_load16((const float4*)base + j) : *(const uint4*)((const float4*)base + j), bs);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p0[k] = ddim_x0(xs[k], es[k], s1, s2);
            const float u = fmaf(es[k], q, __fmul_rn(p, bs[k]));
            const double d = (double)u - (double)xs[k];
            dd = fma(d, d, dd);
            nn = fma((double)u, (double)u, nn);
            xs[k] = u;
        }
        if (NT) nt_store16((float4*)x0 + j, Piece<float>::pack(p0));  // read by the host copy at a selected level only
        else ((float4*)x0)[j] = make_float4(p0[0], p0[1], p0[2], p0[3]);
        ((float4*)xt)[j] = make_float4(xs[0], xs[1], xs[2], xs[3]);  // the next forward's input: default policy
    }
    const double sd = block_sum(dd, red), sn = block_sum(nn, red);
    if (threadIdx.x == 0) {
        double* out = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        out[0] = sd;
        out[1] = sn;
    }
}

// one block per sample: log[step][b] = |x_new - x_old| / |x_new| from the sample's partials
__global__ void __launch_bounds__(kInvertThreads) invert_residual_kernel(const double* __restrict__ partials, int nparts,
                                                                         float* __restrict__ log, int rows,
                                                                         const int* __restrict__ step) {
    __shared__ double red[kInvertThreads / 64];
    const int row = step[0];
    if (row < 0 || row >= rows) return;
    const double* ps = partials + (size_t)blockIdx.x * nparts * 2;
    const double sd = invert_partials_sum(ps, nparts, 2, 0, red), sn = invert_partials_sum(ps, nparts, 2, 1, red);
    if (threadIdx.x == 0) log[(size_t)row * gridDim.x + blockIdx.x] = sn > 0.0 ? (float)(sqrt(sd) / sqrt(sn)) : 0.f;
}

hipError_t invert_update_launch(float* xt, const float* et, float* base, float* x0, double* partials, float* log, int rows,
                                const float* coef, const int* step, int B, long long per_sample, hipStream_t s) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4 || rows < 1) return hipErrorInvalidValue;
    const int nb = sample_blocks(B, per_sample, kInvertMaxBlocks);
    const long long n4 = per_sample / 4;
    if (nt_streaming((size_t)B * (size_t)per_sample * 4))
        hipLaunchKernelGGL(invert_update_kernel<true>, dim3(nb, B), dim3(kInvertThreads), 0, s, xt, et, base, x0, partials, rows, coef,
                           step, n4);
    else
        hipLaunchKernelGGL(invert_update_kernel<false>, dim3(nb, B), dim3(kInvertThreads), 0, s, xt, et, base, x0, partials, rows, coef,
                           step, n4);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(invert_residual_kernel, dim3(B), dim3(kInvertThreads), 0, s, partials, nb, log, rows, step);
    return hipGetLastError();
}

// ---- slerp -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kInvertThreads) slerp_sums_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                                    double* __restrict__ partials, long long n4) {
    __shared__ double red[kInvertThreads / 64];
    const size_t off = (size_t)blockIdx.y * (size_t)n4;
    double s12 = 0.0, s11 = 0.0, s22 = 0.0;
    for (long long i = (long long)blockIdx.x * kInvertThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInvertThreads) {
        const float4 a4 = ((const float4*)z1)[off + (size_t)i], b4 = ((const float4*)z2)[off + (size_t)i];
        const double as[4] = {a4.x, a4.y, a4.z, a4.w}, bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s12 = fma(as[k], bs[k], s12);
            s11 = fma(as[k], as[k], s11);
            s22 = fma(bs[k], bs[k], s22);
        }
    }
    const double t12 = block_sum(s12, red), t11 = block_sum(s11, red), t22 = block_sum(s22, red);
    if (threadIdx.x == 0) {
        double* out = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        out[0] = t12;
        out[1] = t11;
        out[2] = t22;
    }
}

template <bool NT>
__global__ void __launch_bounds__(kInvertThreads) slerp_blend_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                                     const float* __restrict__ weights, int M,
                                                                     float* __restrict__ out, const double* __restrict__ partials,
                                                                     int nparts, long long n4) {
    __shared__ double red[kInvertThreads / 64];
    __shared__ float ca[kSlerpChunk], cb[kSlerpChunk];
    const double* ps = partials + (size_t)blockIdx.y * nparts * 3;
    const double s12 = invert_partials_sum(ps, nparts, 3, 0, red), s11 = invert_partials_sum(ps, nparts, 3, 1, red),
                 s22 = invert_partials_sum(ps, nparts, 3, 2, red);
    // theta = 0 (parallel inputs: sqrt(s11 s22) returns s11 exactly when z1 = z2) or a zero input: sin(theta) = 0 and the formula
    // is 0 / 0 -- the straight line instead
    double theta = 0.0, st = 0.0;
    if (s11 > 0.0 && s22 > 0.0) {
        double c = s12 / sqrt(s11 * s22);
        c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
        theta = acos(c);
        st = sin(theta);
    }
    const bool line = !(st > 0.0);
    const size_t off = (size_t)blockIdx.y * (size_t)n4;
    for (int m0 = 0; m0 < M; m0 += kSlerpChunk) {
        const int mc = M - m0 < kSlerpChunk ? M - m0 : kSlerpChunk;
        __syncthreads();  // the previous chunk's coefficients are no longer read
        if ((int)threadIdx.x < mc) {
            const double w = (double)weights[m0 + threadIdx.x];
            ca[threadIdx.x] = (float)(line ? 1.0 - w : sin((1.0 - w) * theta) / st);
            cb[threadIdx.x] = (float)(line ? w : sin(w * theta) / st);
        }
        __syncthreads();
        for (long long i = (long long)blockIdx.x * kInvertThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kInvertThreads) {
            const float4 a4 = ((const float4*)z1)[off + (size_t)i], b4 = ((const float4*)z2)[off + (size_t)i];
            const float as[4] = {a4.x, a4.y, a4.z, a4.w}, bs[4] = {b4.x, b4.y, b4.z, b4.w};
            for (int m = 0; m < mc; ++m) {
                const float a = ca[m], b = cb[m];
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = fmaf(b, bs[k], __fmul_rn(a, as[k]));
                float4* dst = (float4*)out + ((size_t)blockIdx.y * M + (size_t)(m0 + m)) * (size_t)n4 + (size_t)i;
                if (NT) nt_store16(dst, Piece<float>::pack(o));
                else *dst = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
}

hipError_t slerp_launch(const float* z1, const float* z2, const float* weights, int M, float* out, double* partials, int P,
                        long long per_sample, hipStream_t s) {
    if (P < 1 || P > 65535 || M < 1 || per_sample <= 0 || per_sample % 4) return hipErrorInvalidValue;
    const int nb = sample_blocks(P, per_sample, kInvertMaxBlocks);
    const long long n4 = per_sample / 4;
    hipLaunchKernelGGL(slerp_sums_kernel, dim3(nb, P), dim3(kInvertThreads), 0, s, z1, z2, partials, n4);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (nt_streaming((size_t)P * (size_t)M * (size_t)per_sample * 4))
        hipLaunchKernelGGL(slerp_blend_kernel<true>, dim3(nb, P), dim3(kInvertThreads), 0, s, z1, z2, weights, M, out, partials, nb, n4);
    else
        hipLaunchKernelGGL(slerp_blend_kernel<false>, dim3(nb, P), dim3(kInvertThreads), 0, s, z1, z2, weights, M, out, partials, nb, n4);
    return hipGetLastError();
}

}  // namespace ddimx
