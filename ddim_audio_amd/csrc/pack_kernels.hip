// Weight packing (fp32 parameters -> the internal layouts of the conv / FNet kernels) and the NCHW <-> NHWC layout
// converters.  gfx950 only.
#include "pack_kernels.h"

namespace ddimx {

// =====================================================================================================
// weight packing (fp32 parameters -> internal layouts)
// =====================================================================================================
__global__ void pack_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}
hipError_t pack_copy_launch(const float* src, float* dst, long long n, hipStream_t s) {
    const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(pack_copy_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}

// many small fp32 copies in one launch: the (src, dst, n) triples travel as kernel arguments
__global__ void __launch_bounds__(256) pack_copy_multi_kernel(const PackCopyBatch b) {
    const float* src = b.src[blockIdx.y];
    float* dst = b.dst[blockIdx.y];
    const long long n = b.n[blockIdx.y];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}
hipError_t pack_copy_multi_launch(const PackCopyBatch& b, hipStream_t s) {
    if (b.count < 1) return hipSuccess;
    long long mx = 0;
    for (int i = 0; i < b.count; ++i) if (b.n[i] > mx) mx = b.n[i];
    const int bx = (int)((mx + 255) / 256 < 256 ? (mx + 255) / 256 : 256);
    hipLaunchKernelGGL(pack_copy_multi_kernel, dim3(bx, b.count), dim3(256), 0, s, b);
    return hipGetLastError();
}

template <typename T>
__global__ void pack_conv_kernel(const float* __restrict__ w, T* __restrict__ dst, int O, int I, int KK) {
    const long long n = (long long)KK * O * I;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ci = i % I, co = (i / I) % O, tap = i / ((long long)I * O);
        dst[i] = from_f<T>(w[((size_t)co * I + ci) * KK + tap]);
    }
}
hipError_t pack_conv_launch(int dtype, const float* w, void* dst, int O, int I, int KH, int KW, hipStream_t s) {
    const long long n = (long long)KH * KW * O * I;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(pack_conv_kernel<T>, dim3(blocks), dim3(256), 0, s, w, (T*)dst, O, I, KH * KW);
    });
    return hipGetLastError();
}

// many conv-weight packings in one launch (a training step re-packs every conv after its optimizer step: 143 launches of 4 us
// otherwise).  mode 0: the forward layout of pack_conv_kernel, dst[tap][co][ci] = w[co][ci][tap]; mode 1: the data-gradient
// packing of a 3x3 conv (pack_conv_dgrad_kernel: transposed and flipped), dst[tp][ci][co] = w[co][ci][8 - tp].
template <typename T>
__device__ __forceinline__ void pack_conv_entry(const float* __restrict__ w, T* __restrict__ dst, int O, int I, int KK, int mode) {
    const int n = KK * O * I;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (mode == 0) {
            const int ci = i % I, co = (i / I) % O, tap = i / (I * O);
            dst[i] = from_f<T>(w[((size_t)co * I + ci) * KK + tap]);
        } else {
            const int co = i % O, ci = (i / O) % I, tp = i / (O * I);
            dst[i] = from_f<T>(w[((size_t)co * I + ci) * 9 + (8 - tp)]);
        }
    }
}
__global__ void __launch_bounds__(256) pack_conv_multi_kernel(const PackConvBatch b) {
    const int e = blockIdx.y;
    if (b.f32[e]) pack_conv_entry<float>(b.src[e], (float*)b.dst[e], b.O[e], b.I[e], b.KK[e], b.mode[e]);
    else pack_conv_entry<__bf16>(b.src[e], (__bf16*)b.dst[e], b.O[e], b.I[e], b.KK[e], b.mode[e]);
}
hipError_t pack_conv_multi_launch(const PackConvBatch& b, hipStream_t s) {
    if (b.count < 1) return hipSuccess;
    long long mx = 0;
    for (int i = 0; i < b.count; ++i) {
        const long long n = (long long)b.KK[i] * b.O[i] * b.I[i];
        if (n > mx) mx = n;
    }
    const int bx = (int)((mx + 255) / 256 < 64 ? (mx + 255) / 256 : 64);
    hipLaunchKernelGGL(pack_conv_multi_kernel, dim3(bx, b.count), dim3(256), 0, s, b);
    return hipGetLastError();
}

// conv weight [O][I][KH][KW] fp32 (KK = KH * KW taps, row-major) -> bf16 in MFMA fragment order (conv_wreg.h):
//   dst[step = tap * (I/16) + kg][nb][lane = h * 32 + l31][j]  =  w[co = nb * 32 + l31][ci = kg * 16 + h * 8 + j][tap]
__global__ void pack_conv_frag_kernel(const float* __restrict__ w, __bf16* __restrict__ dst, int O, int I, int KK) {
    const int KG = I / 16, NBLK = O / 32;
    const long long n = (long long)KK * O * I;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
        const long long blk = i >> 9;
        const int nb = (int)(blk % NBLK), st = (int)(blk / NBLK);
        const int tap = st / KG, kg = st % KG;
        const int co = nb * 32 + (lane & 31), ci = kg * 16 + (lane >> 5) * 8 + j;
        dst[i] = (__bf16)w[((size_t)co * I + ci) * KK + tap];
    }
}
hipError_t pack_conv_frag_launch(const float* w, void* dst, int O, int I, int KK, hipStream_t s) {
    if (O % 32 || I % 16) return hipErrorInvalidValue;
    const long long n = (long long)KK * O * I;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(pack_conv_frag_kernel, dim3(blocks), dim3(256), 0, s, w, (__bf16*)dst, O, I, KK);
    return hipGetLastError();
}

// packed taps [ntaps][NOUT][CIN] bf16 -> fragment order [ntaps * CIN/16][NOUT/32][64][8] (conv_wreg.h)
__global__ void pack_frag_from_taps_kernel(const __bf16* __restrict__ src, __bf16* __restrict__ dst, int ntaps, int NOUT, int CIN) {
    const int KG = CIN / 16, NBLK = NOUT / 32;
    const long long n = (long long)ntaps * NOUT * CIN;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
        const long long blk = i >> 9;
        const int nb = (int)(blk % NBLK), st = (int)(blk / NBLK);
        const int tap = st / KG, kg = st % KG;
        const int co = nb * 32 + (lane & 31), ci = kg * 16 + (lane >> 5) * 8 + j;
        dst[i] = src[((size_t)tap * NOUT + co) * CIN + ci];
    }
}
hipError_t pack_frag_from_taps_launch(const void* src, void* dst, int ntaps, int NOUT, int CIN, hipStream_t s) {
    if (NOUT % 32 || CIN % 16) return hipErrorInvalidValue;
    const long long n = (long long)ntaps * NOUT * CIN;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(pack_frag_from_taps_kernel, dim3(blocks), dim3(256), 0, s, (const __bf16*)src, (__bf16*)dst, ntaps, NOUT, CIN);
    return hipGetLastError();
}

// ConvTranspose2d(k4,s2,p1) weight [I][O][4][4] -> sub-pixel form [a][tap=(dyi,dx)][vc=b*O+co][ci]:
// output (2py+a, 2px+b) reads input (py+dy-1, px+dx-1) through kernel element kh = 3+a-2dy, kw = 3+b-2dx
// (dy = a+dyi in {a,a+1}; dx in {0,1,2}); combinations whose kw falls outside 0..3 are zero.
template <typename T>
__global__ void pack_convT_kernel(const float* __restrict__ w, T* __restrict__ dst, int I, int O) {
    const long long n = 2LL * 6 * 2 * O * I;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ci = i % I;
        const int vc = (i / I) % (2 * O);
        const int tap = (i / ((long long)I * 2 * O)) % 6;
        const int a = i / ((long long)I * 2 * O * 6);
        const int b = vc / O, co = vc % O;
        const int dy = a + tap / 3, dx = tap % 3;
        const int kh = 3 + a - 2 * dy, kw = 3 + b - 2 * dx;
        float v = 0.f;
        if (kw >= 0 && kw < 4 && kh >= 0 && kh < 4) v = w[(((size_t)ci * O + co) * 4 + kh) * 4 + kw];
        dst[i] = from_f<T>(v);
    }
}
hipError_t pack_convT_launch(int dtype, const float* w, void* dst, int I, int O, hipStream_t s) {
    const long long n = 2LL * 6 * 2 * O * I;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(pack_convT_kernel<T>, dim3(blocks), dim3(256), 0, s, w, (T*)dst, I, O);
    });
    return hipGetLastError();
}

__global__ void pack_perm_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int C, int Fr) {
    const long long n = (long long)rows * C * Fr;
    const int Wd = C * Fr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int col = i % Wd;
        const long long r = i / Wd;
        const int f = col / C, c = col % C;
        dst[i] = src[r * Wd + (long long)c * Fr + f];
    }
}
hipError_t pack_perm_cols_launch(const float* src, float* dst, int rows, int C, int Fr, hipStream_t s) {
    const long long n = (long long)rows * C * Fr;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(pack_perm_cols_kernel, dim3(blocks), dim3(256), 0, s, src, dst, rows, C, Fr);
    return hipGetLastError();
}
__global__ void pack_perm_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int Fr, int K) {
    const long long n = (long long)C * Fr * K;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int k = i % K;
        const int row = i / K;
        const int f = row / C, c = row % C;
        dst[i] = src[((long long)c * Fr + f) * K + k];
    }
}
hipError_t pack_perm_rows_launch(const float* src, float* dst, int C, int Fr, int K, hipStream_t s) {
    const long long n = (long long)C * Fr * K;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(pack_perm_rows_kernel, dim3(blocks), dim3(256), 0, s, src, dst, C, Fr, K);
    return hipGetLastError();
}

// =====================================================================================================
// data-gradient weights: the transposed, spatially flipped 3x3 kernel in the forward conv's packed layout
//   dst[tap'][ci][co] = w[co][ci][8 - tap']        (w: Conv2d.weight [O][I][3][3]; dst: [9][I][O] as T)
// =====================================================================================================
template <typename T>
__global__ void pack_conv_dgrad_kernel(const float* __restrict__ w, T* __restrict__ dst, int O, int I) {
    const int n = 9 * O * I;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int co = i % O, ci = (i / O) % I, tp = i / (O * I);
        dst[i] = from_f<T>(w[((size_t)co * I + ci) * 9 + (8 - tp)]);
    }
}
hipError_t pack_conv_dgrad_launch(int dtype, const float* w, void* dst, int O, int I, hipStream_t s) {
    const int n = 9 * O * I;
    const int blocks = (n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(pack_conv_dgrad_kernel<T>, dim3(blocks), dim3(256), 0, s, w, (T*)dst, O, I);
    });
    return hipGetLastError();
}

// ---- layout converters (test / boundary helpers) -------------------------------------------------------
template <typename T>
__global__ void to_nhwc_kernel(const float* __restrict__ in, T* __restrict__ out, int C, int HW, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = i % C;
        const long long p = (i / C) % HW, b = i / ((long long)C * HW);
        out[i] = from_f<T>(in[(b * C + c) * HW + p]);
    }
}
template <typename T>
__global__ void from_nhwc_kernel(const T* __restrict__ in, float* __restrict__ out, int C, int HW, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long p = i % HW;
        const int c = (i / HW) % C;
        const long long b = i / ((long long)C * HW);
        out[i] = to_f<T>(in[(b * HW + p) * C + c]);
    }
}
hipError_t to_nhwc_launch(int dtype, const float* in, void* out, int B, int C, int HW, hipStream_t s) {
    const long long n = (long long)B * C * HW;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(to_nhwc_kernel<T>, dim3(blocks), dim3(256), 0, s, in, (T*)out, C, HW, n);
    });
    return hipGetLastError();
}
hipError_t from_nhwc_launch(int dtype, const void* in, float* out, int B, int C, int HW, hipStream_t s) {
    const long long n = (long long)B * C * HW;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(from_nhwc_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)in, out, C, HW, n);
    });
    return hipGetLastError();
}

}  // namespace ddimx
