// The U-Net's two edge convolutions (C_io = 2 side, HBM-bound; models/diffusion.py:189-208), forward and backward:
// in-conv (NCHW fp32 -> NHWC T + statistics partials), out-conv ((a + b) NHWC T -> NCHW fp32), their data gradients and
// the weight gradient of both as one correlation.  gfx950 only.  Every reduction is a fixed-order tree (no float atomics).
#include "edge_conv.h"
#include "gn_fused.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace ddimx {

// =====================================================================================================
// launch constants: what the kernels below and edge_plan at the bottom share
// =====================================================================================================
constexpr int kInPixPerBlock = 1024;     // in-conv: pixels of one workgroup (one statistics part)
constexpr int kTileH = 8, kTileW = 32;   // out-conv and the in-conv's data gradient: output pixels of one workgroup
constexpr int kEdgeT = 16;               // tiled weight gradient: a 16 x 16 tile
constexpr int kEdgeChunk = 32;           // strip weight gradient: rows of S staged per LDS tile,
constexpr int kStripRows = 128;          //   rows of one strip,
static inline int edge_pixb(int dtype) { return dtype == DT_BF16 ? 64 : 32; }  //   pixel columns of one strip
int conv_in_nparts(int H, int W) { return (int)(((long long)H * W + kInPixPerBlock - 1) / kInPixPerBlock); }

// =====================================================================================================
// in-conv: Conv2d(cin -> C0, k3, p1) reading NCHW fp32, writing NHWC T (+ per-channel stats partials)
// (conv_in_kernel and conv_in_mfma_kernel add their four per-wave partials in different orders in the channel-format tail:
// real statistics would move by an ulp if the two tails were merged, so each keeps its own)
// =====================================================================================================
template <typename T>
__global__ void __launch_bounds__(256) conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, T* __restrict__ out,
                                                      float* __restrict__ stats, int cin, int C0, int H, int W,
                                                      int groups) {
    constexpr int EPB = Piece<T>::N;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* wl = lds;                       // [cin*9][C0]
    float* red = lds + cin * 9 * C0;       // [4 waves][C0][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OPP = C0 / EPB, PPP = 256 / OPP;
    const int b = blockIdx.y, part = blockIdx.x;
    for (int i = tid; i < cin * 9 * C0; i += 256) {
        const int co = i % C0, r = i / C0;  // r = ci*9 + tap
        wl[i] = w[(size_t)co * cin * 9 + r];
    }
    __syncthreads();
    const int c = tid % OPP, pslot = tid / OPP;
    float s[EPB], q[EPB], bv[EPB];
#pragma unroll
    for (int j = 0; j < EPB; ++j) { s[j] = q[j] = 0.f; bv[j] = bias[c * EPB + j]; }
    const int HW = H * W;
    const float* xb = x + (size_t)b * cin * HW;
    for (int it = 0; it < kInPixPerBlock / PPP; ++it) {
        const int pix = part * kInPixPerBlock + it * PPP + pslot;
        if (pix >= HW) break;
        const int py = pix / W, px = pix % W;
        float acc[EPB];
#pragma unroll
        for (int j = 0; j < EPB; ++j) acc[j] = bv[j];
        for (int ci = 0; ci < cin; ++ci) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int gy = py + k / 3 - 1, gx = px + k % 3 - 1;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(size_t)ci * HW + (size_t)gy * W + gx];
                const float* wr = wl + (ci * 9 + k) * C0 + c * EPB;
#pragma unroll
                for (int j = 0; j < EPB; ++j) acc[j] = fmaf(v, wr[j], acc[j]);
            }
        }
        uint4 pv = Piece<T>::pack(acc);
        Piece<T>::unpack(pv, acc);  // statistics of the stored values
        *(uint4*)(out + ((size_t)b * HW + pix) * C0 + c * EPB) = pv;
#pragma unroll
        for (int j = 0; j < EPB; ++j) { s[j] += acc[j]; q[j] = fmaf(acc[j], acc[j], q[j]); }
    }
    if (stats) {
        for (int o = OPP; o < 64; o <<= 1) {
#pragma unroll
            for (int j = 0; j < EPB; ++j) { s[j] += __shfl_xor(s[j], o, 64); q[j] += __shfl_xor(q[j], o, 64); }
        }
        if (lane < OPP) {
#pragma unroll
            for (int j = 0; j < EPB; ++j) {
                red[(wave * C0 + c * EPB + j) * 2 + 0] = s[j];
                red[(wave * C0 + c * EPB + j) * 2 + 1] = q[j];
            }
        }
        __syncthreads();
        if (groups) {  // group-format partials (gn_fused.h)
            if (wave == 0) gn_bins_store<4>(red, C0 * 2, C0, 0, C0, stats + ((size_t)b * gridDim.x + part) * kGnSlab, lane);
        } else {
            for (int i = tid; i < C0 * 2; i += 256) {
                const float t = red[i] + red[C0 * 2 + i] + red[2 * C0 * 2 + i] + red[3 * C0 * 2 + i];
                stats[(((size_t)b * gridDim.x + part) * C0) * 2 + i] = t;
            }
        }
    }
}

// ---- MFMA path (C0 = 32, cin = 2): the 18-term dot products run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: A = weights,
// rows = cout; B = im2col of the input, columns = 32 consecutive pixels).  MFMA step i multiplies tap i, its two k are the two
// input channels: lane half h handles channel h (any assignment of the 18 products to (step, half) is valid as long as A and B
// agree), so the tap geometry is a compile-time constant and the channel one per-lane offset; the bias is a tenth step against
// a column of ones (exact).  A wave walks 32-pixel blocks; the nine input loads of the block two ahead are issued before the current
// block is multiplied and stored: the lane-per-pixel kernel this one replaced was a chain of {18 loads, wait -- which also waits
// for the previous stores, vmcnt is in-order -- 576 FMAs, LDS, 4 stores} per 64 pixels and reached 1.7 TB/s of the 8.  Loads are
// unconditional (padding taps read the centre pixel and are zeroed by select): a load under a branch is waited for at once.
template <typename T>
__global__ void __launch_bounds__(256, 4) conv_in_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, T* __restrict__ out,
                                                              float* __restrict__ stats, int H, int W, int groups) {
    constexpr int C0 = 32, CIN = 2, KT = CIN * 9;
    constexpr int ROWB = C0 * (int)sizeof(T), PCS = ROWB / 16;  // bytes / 16-byte pieces per pixel
    constexpr int NBLK = kInPixPerBlock / (4 * 32);              // 32-pixel blocks per wave
    __shared__ float red[4][C0 * 2];
    __shared__ __attribute__((aligned(16))) char otile[4][32 * (ROWB + 16)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, part = blockIdx.x;
    const int HW = H * W;
    const float* xb = x + (size_t)b * CIN * HW;
    float wa[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wa[i] = w[l31 * KT + h * 9 + i];
    const float wbias = h == 0 ? bias[l31] : 0.f;
    const int hoff = h * HW;  // this lane half's input channel (32-bit element offsets against the uniform base xb)
    const int wshift = (W & (W - 1)) == 0 ? __builtin_ctz(W) : -1;  // uniform
    // accumulator register r of a lane holds cout 8*(r/4) + 4*h + r%4 of pixel l31 (32x32 MFMA output layout)
    float s[16], q[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = q[r] = 0.f;
    float nxt[2][9];  // the blocks one and two ahead
    auto load_block = [&](int blk, float (&dst)[9]) __attribute__((always_inline)) {
        const int p = part * kInPixPerBlock + (blk * 4 + wave) * 32 + l31;
        const int pc = p < HW ? p : HW - 1;
        const int py = wshift >= 0 ? pc >> wshift : pc / W, px = pc - py * W;
        const int ctr = hoff + pc;  // the pixel itself: always a valid element
        const bool vy[3] = {py > 0, true, py < H - 1}, vx[3] = {px > 0, true, px < W - 1};
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int dy = i / 3 - 1, dx = i % 3 - 1;
            const bool inb = vy[dy + 1] && vx[dx + 1];
            const float v = xb[inb ? ctr + dy * W + dx : ctr];
            dst[i] = inb ? v : 0.f;
        }
    };
    load_block(0, nxt[0]);
    load_block(1, nxt[1]);
    char* const tile = otile[wave];
#pragma unroll 1
    for (int blk = 0; blk < NBLK; ++blk) {
        const int pix0 = part * kInPixPerBlock + (blk * 4 + wave) * 32;  // first pixel of this block (uniform per wave)
        if (pix0 >= HW) break;
        const bool valid = pix0 + l31 < HW;
        float cur[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { cur[i] = nxt[0][i]; nxt[0][i] = nxt[1][i]; }
        load_block(blk + 2, nxt[1]);  // (past the workgroup's range / the image: clamped addresses, results unused)
        f32x16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wbias, 1.0f, acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 9; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[i], cur[i], acc, 0, 0, 0);
        char* my = tile + l31 * (ROWB + 16);
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            float f[4] = {acc[4 * qd], acc[4 * qd + 1], acc[4 * qd + 2], acc[4 * qd + 3]};
            if constexpr (sizeof(T) == 2) {
                const uint32_t lo = Piece<__bf16>::pk(f[0], f[1]), hi = Piece<__bf16>::pk(f[2], f[3]);
                *(uint2*)(my + (8 * qd + 4 * h) * 2) = make_uint2(lo, hi);
                f[0] = __uint_as_float(lo << 16); f[1] = __uint_as_float(lo & 0xffff0000u);  // the values as stored
                f[2] = __uint_as_float(hi << 16); f[3] = __uint_as_float(hi & 0xffff0000u);
            } else {
                *(float4*)(my + (8 * qd + 4 * h) * 4) = make_float4(f[0], f[1], f[2], f[3]);
            }
            if (valid) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { s[4 * qd + j] += f[j]; q[4 * qd + j] = fmaf(f[j], f[j], q[4 * qd + j]); }
            }
        }
        // LDS operations of one wave execute in order: the writes above are visible to the reads below without a fence (a
        // wavefront-scope fence also waits for the global stores of the previous block)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // the block's 32 pixels are consecutive in memory: PCS / 2 store instructions of 1 KiB contiguous each
        char* obase = (char*)(out + ((size_t)b * HW + pix0) * C0);
        const int npix = HW - pix0 < 32 ? HW - pix0 : 32;
#pragma unroll
        for (int k = 0; k < PCS / 2; ++k) {
            const int idx = k * 64 + lane;           // piece index inside the block
            const int pp = idx / PCS, pc = idx % PCS;
            const uint4 vv = *(const uint4*)(tile + pp * (ROWB + 16) + pc * 16);
            if (pp < npix) *(uint4*)(obase + (size_t)idx * 16) = vv;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the tile has been read before the next block overwrites it
        __builtin_amdgcn_wave_barrier();
    }
    if (stats) {
        // lanes of one half hold the same 16 couts for 32 different pixels: butterflies over the five pixel bits
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) { s[r] += __shfl_xor(s[r], o, 64); q[r] += __shfl_xor(q[r], o, 64); }
            if (l31 == 0) {
                const int c = 8 * (r / 4) + 4 * h + (r % 4);
                red[wave][c * 2] = s[r]; red[wave][c * 2 + 1] = q[r];
            }
        }
        __syncthreads();
        if (groups) {  // group-format partials (gn_fused.h)
            if (wave == 0) gn_bins_store<4>(&red[0][0], C0 * 2, C0, 0, C0, stats + ((size_t)b * gridDim.x + part) * kGnSlab, lane);
        } else if (tid < C0 * 2) {
            stats[(((size_t)b * gridDim.x + part) * C0) * 2 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        }
    }
}

hipError_t conv_in_launch(int dtype, const float* x, const float* w, const float* bias, void* out, float* stats, int B,
                          int cin, int C0, int H, int W, hipStream_t s, int groups) {
    EdgePlan p;
    if (edge_plan(EDGE_CONV_IN, dtype, B, C0, cin, H, W, groups, &p)) return hipErrorInvalidValue;
    const dim3 grid(p.grid_x, p.grid_y);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (p.variant) hipLaunchKernelGGL(conv_in_mfma_kernel<T>, grid, dim3(256), 0, s, x, w, bias, (T*)out, stats, H, W, groups);
        else hipLaunchKernelGGL(conv_in_kernel<T>, grid, dim3(256), p.lds, s, x, w, bias, (T*)out, stats, cin, C0, H, W, groups);
    });
    return hipGetLastError();
}

// =====================================================================================================
// out-conv: Conv2d(C0 -> cout, k3, p1) on (a + b) NHWC T, writing NCHW fp32
// =====================================================================================================
template <typename T>
__global__ void __launch_bounds__(256) conv_out_kernel(const T* __restrict__ a, const T* __restrict__ b2,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int C0, int cout, int H, int W,
                                                       int tiles_x, int tiles_y) {
    constexpr int EPB = Piece<T>::N;
    constexpr int IH = kTileH + 2, IW = kTileW + 2;
    extern __shared__ __attribute__((aligned(16))) float tile[];  // [IH*IW][C0+1]
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = ty * kTileH, x0 = tx * kTileW;
    const int CPP = C0 / EPB, LS = C0 + 1;
    for (int i = tid; i < IH * IW * CPP; i += 256) {
        const int c = i % CPP, pix = i / CPP;
        const int gy = y0 - 1 + pix / IW, gx = x0 - 1 + pix % IW;
        float f[EPB];
#pragma unroll
        for (int j = 0; j < EPB; ++j) f[j] = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t g = (((size_t)b * H + gy) * W + gx) * C0 + c * EPB;
            float k[EPB];
            Piece<T>::unpack(*(const uint4*)(a + g), f);
            Piece<T>::unpack(*(const uint4*)(b2 + g), k);
#pragma unroll
            for (int j = 0; j < EPB; ++j) f[j] += k[j];  // x + hidden[0], kept in fp32
        }
#pragma unroll
        for (int j = 0; j < EPB; ++j) tile[pix * LS + c * EPB + j] = f[j];
    }
    __syncthreads();
    const int py = tid / kTileW, px = tid % kTileW;
    float acc[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[o] = (o < cout) ? bias[o] : 0.f;
    for (int ci = 0; ci < C0; ++ci) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float v = tile[((py + k / 3) * IW + px + k % 3) * LS + ci];
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (o < cout) acc[o] = fmaf(v, w[((size_t)k * cout + o) * C0 + ci], acc[o]);
        }
    }
    const int gy = y0 + py, gx = x0 + px;
    if (gy < H && gx < W) {
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (o < cout) out[(((size_t)b * cout + o) * H + gy) * W + gx] = acc[o];
    }
}

// ---- the tile walk of both fixed-width 3x3 convs that read NHWC T and write NCHW fp32 (C0 -> NO): the out-conv's fast path (TWO:
// the operand is a + b, added in fp32 and re-rounded to T; BIAS) and the in-conv's data gradient (one operand, its bits staged
// unchanged; no bias).  The 10 x 34 halo tile is staged once into LDS in the activation dtype with a pixel stride of C0*es+16 bytes
// (conflict-free b128 reads), one lane = one output pixel, weights wave-uniform.
template <typename T, int C0, int NO, bool TWO, bool BIAS>
__device__ __forceinline__ void edge_tile_conv(const T* __restrict__ a, const T* __restrict__ b2, const float* __restrict__ w,
                                               const float* __restrict__ bias, float* __restrict__ out, int H, int W, int tiles_x,
                                               int tiles_y) {
    constexpr int EPB = Piece<T>::N, ES = sizeof(T);
    constexpr int IH = kTileH + 2, IW = kTileW + 2;
    constexpr int CPP = C0 / EPB, PS = C0 * ES + 16;
    __shared__ __attribute__((aligned(16))) char tile[IH * IW * PS];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = ty * kTileH, x0 = tx * kTileW;
    // halo staging: all loads of the tile are issued before the first use, unconditionally (out-of-image pieces read a clamped
    // address and are zeroed by select) -- under `if (inside) load` every piece was a round trip of its own, six in a row per thread
    constexpr int NPIECE = IH * IW * CPP, NIT = (NPIECE + 255) / 256;
    uint4 va[NIT], vb[TWO ? NIT : 1];
    bool inb[NIT];
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int i0 = tid + u * 256, i = i0 < NPIECE ? i0 : NPIECE - 1;
        const int c = i % CPP, pix = i / CPP;
        const int gy = y0 - 1 + pix / IW, gx = x0 - 1 + pix % IW;
        inb[u] = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int gyc = gy < 0 ? 0 : (gy >= H ? H - 1 : gy), gxc = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);
        const size_t g = (((size_t)b * H + gyc) * W + gxc) * C0 + c * EPB;
        va[u] = *(const uint4*)(a + g);
        if constexpr (TWO) vb[u] = *(const uint4*)(b2 + g);
    }
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int i = tid + u * 256;
        uint4 v;
        if constexpr (TWO) {
            float f[EPB], k[EPB];
            Piece<T>::unpack(va[u], f);
            Piece<T>::unpack(vb[u], k);
#pragma unroll
            for (int j = 0; j < EPB; ++j) f[j] += k[j];
            v = Piece<T>::pack(f);
            if (!inb[u]) v = make_uint4(0, 0, 0, 0);
        } else {
            v = inb[u] ? va[u] : make_uint4(0, 0, 0, 0);
        }
        if (i < NPIECE) *(uint4*)(tile + (i / CPP) * PS + (i % CPP) * 16) = v;
    }
    __syncthreads();
    const int py = tid / kTileW, px = tid % kTileW;
    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = BIAS ? bias[o] : 0.f;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {  // w: [tap][NO][C0], NO * C0 contiguous wave-uniform floats per tap
        const char* tp = tile + ((py + k / 3) * IW + px + k % 3) * PS;
        const float* wk = w + k * NO * C0;
#pragma unroll
        for (int c = 0; c < CPP; ++c) {
            float f[EPB];
            Piece<T>::unpack(*(const uint4*)(tp + c * 16), f);
#pragma unroll
            for (int j = 0; j < EPB; ++j)
#pragma unroll
                for (int o = 0; o < NO; ++o) acc[o] = fmaf(f[j], wk[o * C0 + c * EPB + j], acc[o]);
        }
    }
    const int gy = y0 + py, gx = x0 + px;
    if (gy < H && gx < W) {
#pragma unroll
        for (int o = 0; o < NO; ++o) out[(((size_t)b * NO + o) * H + gy) * W + gx] = acc[o];
    }
}

// fast path (C0 = 32, cout = 2): the tile walk over a + b, with the bias
template <typename T, int C0, int COUT>
__global__ void __launch_bounds__(256) conv_out_fast_kernel(const T* __restrict__ a, const T* __restrict__ b2,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ out, int H, int W, int tiles_x,
                                                            int tiles_y) {
    edge_tile_conv<T, C0, COUT, true, true>(a, b2, w, bias, out, H, W, tiles_x, tiles_y);
}

hipError_t conv_out_launch(int dtype, const void* a, const void* b, const float* w, const float* bias, float* out, int B,
                           int C0, int cout, int H, int W, hipStream_t s) {
    EdgePlan p;
    if (edge_plan(EDGE_CONV_OUT, dtype, B, C0, cout, H, W, 0, &p)) return hipErrorInvalidValue;
    const dim3 grid(p.grid_x);
    const int tiles_x = p.tiles_x, tiles_y = p.tiles_y;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (p.variant)
            hipLaunchKernelGGL((conv_out_fast_kernel<T, 32, 2>), grid, dim3(256), 0, s, (const T*)a, (const T*)b, w, bias, out, H, W,
                               tiles_x, tiles_y);
        else
            hipLaunchKernelGGL(conv_out_kernel<T>, grid, dim3(256), p.lds, s, (const T*)a, (const T*)b, w, bias, out, C0, cout, H, W,
                               tiles_x, tiles_y);
    });
    return hipGetLastError();
}

// =====================================================================================================
// data gradients of both convs
// =====================================================================================================
// data gradient of the output conv: ds[b][y][x][c] = sum_{k,o} d_eps[b][o][y-ky+1][x-kx+1] * w[k][o][c]   (w: packed [9][cout][C0])
// (d_eps NCHW fp32, ds NHWC T; it is the gradient of BOTH summands of `x + hidden[0]`, :284)
template <typename T>
__global__ void __launch_bounds__(256) conv_out_bwd_data_kernel(const float* __restrict__ de, const float* __restrict__ w,
                                                                T* __restrict__ ds, int C0, int cout, int H, int W) {
    constexpr int EPB = Piece<T>::N;
    extern __shared__ float wl[];  // [k][o][c]: the forward's packed layout, copied as is
    for (int i = threadIdx.x; i < 9 * cout * C0; i += 256) wl[i] = w[i];
    __syncthreads();
    const int CPP = C0 / EPB;
    const long long pieces = (long long)H * W * CPP;
    const int b = blockIdx.y;
    for (long long pc = blockIdx.x * 256ll + threadIdx.x; pc < pieces; pc += gridDim.x * 256ll) {
        const int c0 = (int)(pc % CPP) * EPB;
        const long long pix = pc / CPP;
        const int y = (int)(pix / W), x = (int)(pix % W);
        float acc[EPB];
#pragma unroll
        for (int j = 0; j < EPB; ++j) acc[j] = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const size_t off = ok ? (size_t)yy * W + xx : 0;
            for (int o = 0; o < cout; ++o) {
                const float dv = de[((size_t)b * cout + o) * H * W + off];
                const float d = ok ? dv : 0.f;
                const float* wp = wl + (k * cout + o) * C0 + c0;
#pragma unroll
                for (int j = 0; j < EPB; ++j) acc[j] = fmaf(d, wp[j], acc[j]);
            }
        }
        *(uint4*)(ds + ((size_t)b * H * W + pix) * C0 + c0) = Piece<T>::pack(acc);
    }
}
// Fast path (C0 = 32, cout = 2): every thread keeps the 9 x 2 x EPB weights of its channel piece in registers and walks
// pixels; the 18 d_eps values of a pixel are shared by the piece lanes (same address: one transaction).
template <typename T>
__global__ void __launch_bounds__(256) conv_out_bwd_data_reg_kernel(const float* __restrict__ de, const float* __restrict__ w,
                                                                    T* __restrict__ ds, int H, int W) {
    constexpr int C0 = 32, COUT = 2, EPB = Piece<T>::N, PPB = C0 / EPB, PIX = 256 / PPB;
    const int j = threadIdx.x % PPB, pl = threadIdx.x / PPB, b = blockIdx.y;
    float wr[9 * COUT][EPB];
#pragma unroll
    for (int ko = 0; ko < 9 * COUT; ++ko)
#pragma unroll
        for (int e = 0; e < EPB; ++e) wr[ko][e] = w[ko * C0 + j * EPB + e];
    const long long HW = (long long)H * W;
    const float* d0 = de + (size_t)b * COUT * HW;
    for (long long pix = (long long)blockIdx.x * PIX + pl; pix < HW; pix += (long long)gridDim.x * PIX) {
        const int y = (int)(pix / W), x = (int)(pix % W);
        float dv[9 * COUT];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const size_t off = ok ? (size_t)yy * W + xx : 0;
#pragma unroll
            for (int o = 0; o < COUT; ++o) {
                const float v = d0[(size_t)o * HW + off];
                dv[k * COUT + o] = ok ? v : 0.f;
            }
        }
        float acc[EPB];
#pragma unroll
        for (int e = 0; e < EPB; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ko = 0; ko < 9 * COUT; ++ko)
#pragma unroll
            for (int e = 0; e < EPB; ++e) acc[e] = fmaf(dv[ko], wr[ko][e], acc[e]);
        *(uint4*)(ds + ((size_t)b * HW + pix) * C0 + j * EPB) = Piece<T>::pack(acc);
    }
}
hipError_t conv_out_bwd_data_launch(int dtype, const float* d_eps, const float* w, void* ds, int B, int C0, int cout, int H,
                                    int W, hipStream_t s) {
    EdgePlan p;
    if (edge_plan(EDGE_CONV_OUT_BWD_DATA, dtype, B, C0, cout, H, W, 0, &p)) return hipErrorInvalidValue;
    const dim3 grid(p.grid_x, p.grid_y);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (p.variant) hipLaunchKernelGGL(conv_out_bwd_data_reg_kernel<T>, grid, dim3(256), 0, s, d_eps, w, (T*)ds, H, W);
        else hipLaunchKernelGGL(conv_out_bwd_data_kernel<T>, grid, dim3(256), p.lds, s, d_eps, w, (T*)ds, C0, cout, H, W);
    });
    return hipGetLastError();
}

// data gradient of the input conv (:255-256, the gradient w.r.t. the network input x):
//   dx[b][i][y][x] = sum_{k,c} dy[b][y+ky-1][x+kx-1][c] * w[k][i][c]      (zero padding of dy)
// w = pack_conv_dgrad(DT_F32, W_in, .., O = C0, I = NI): [9][NI][C0] fp32, W_in transposed and spatially flipped, so this is a
// plain 3x3 forward conv C0 -> NI over dy.  dy NHWC T, dx NCHW fp32, WRITTEN.
// Fast path (C0 = 32, NI = 2): the out-conv's tile walk (edge_tile_conv) over the one operand dy, without a bias.
template <typename T, int C0, int NI>
__global__ void __launch_bounds__(256) conv_in_bwd_data_fast_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                                    float* __restrict__ dx, int H, int W, int tiles_x, int tiles_y) {
    edge_tile_conv<T, C0, NI, false, false>(dy, nullptr, w, nullptr, dx, H, W, tiles_x, tiles_y);
}
// any other (C0, NI <= 4): one thread per output pixel straight from global memory.  (Its tap loop encloses its channel loop, the
// generic conv_out_kernel's channel loop its tap loop: real outputs would move if one were written as the other, so both stay)
template <typename T>
__global__ void __launch_bounds__(256) conv_in_bwd_data_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                               float* __restrict__ dx, int C0, int NI, int H, int W) {
    const long long HW = (long long)H * W;
    const int b = blockIdx.y;
    for (long long pix = blockIdx.x * 256ll + threadIdx.x; pix < HW; pix += gridDim.x * 256ll) {
        const int y = (int)(pix / W), x = (int)(pix % W);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 9; ++k) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const T* p = dy + (((size_t)b * H + yy) * W + xx) * C0;
            for (int c = 0; c < C0; ++c) {
                const float d = to_f<T>(p[c]);
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (o < NI) acc[o] = fmaf(d, w[(k * NI + o) * C0 + c], acc[o]);
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (o < NI) dx[((size_t)b * NI + o) * HW + pix] = acc[o];
    }
}
hipError_t conv_in_bwd_data_launch(int dtype, const void* dy, const float* w, float* dx, int B, int C0, int NI, int H, int W,
                                   hipStream_t s) {
    EdgePlan p;
    if (edge_plan(EDGE_CONV_IN_BWD_DATA, dtype, B, C0, NI, H, W, 0, &p)) return hipErrorInvalidValue;
    const dim3 grid(p.grid_x, p.grid_y);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (p.variant)
            hipLaunchKernelGGL((conv_in_bwd_data_fast_kernel<T, 32, 2>), grid, dim3(256), 0, s, (const T*)dy, w, dx, H, W, p.tiles_x,
                               p.tiles_y);
        else
            hipLaunchKernelGGL(conv_in_bwd_data_kernel<T>, grid, dim3(256), 0, s, (const T*)dy, w, dx, C0, NI, H, W);
    });
    return hipGetLastError();
}

// =====================================================================================================
// weight gradients of both convs as one correlation:
//   R[kk][i][c] = sum_{b,y,x} G[b][y][x][c] * S[b][i][y + ky - 1][x + kx - 1]     (zero padding of S)
// G = g1 (+ g2): NHWC T with C channels; S: NCHW fp32 with NI <= 4 planes.
//   input conv : G = d(hidden[0]), S = x       -> dW_in[c][i][kk]  = R[kk][i][c],     db_in[c]  = sumG[c]
//   output conv: G = x + hidden[0], S = d_eps  -> dW_out[i][c][kk] = R[8 - kk][i][c], db_out[i] = sumS[i]
// persistent blocks over 16x16 tiles; partial [nblocks][9*NI*C + C + NI]; edge_wgrad_reduce maps to the layouts.
// =====================================================================================================
template <typename T>
__global__ void __launch_bounds__(288) edge_wgrad_kernel(const T* __restrict__ g1, const T* __restrict__ g2,
                                                         const float* __restrict__ S, float* __restrict__ partial, int C, int NI,
                                                         int H, int W, int tiles_x, int tiles_y, int total_tiles) {
    extern __shared__ float sm[];
    float* Gt = sm;                                   // [256][C + 1]
    float* St = sm + 256 * (C + 1);                   // [NI][18][18]
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int items = 9 * C;
    float acc[2][4];  // up to 2 items per thread (items <= 2 * blockDim), NI <= 4
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[q][i] = 0.f;
    float sumg = 0.f, sums = 0.f;
    for (int t = blockIdx.x; t < total_tiles; t += gridDim.x) {
        const int b = t / (tiles_x * tiles_y), tt = t % (tiles_x * tiles_y);
        const int y0 = (tt / tiles_x) * kEdgeT, x0 = (tt % tiles_x) * kEdgeT;
        __syncthreads();
        for (int i = tid; i < 256 * C; i += nthr) {
            const int c = i % C, p = i / C;
            const int y = y0 + p / kEdgeT, x = x0 + p % kEdgeT;
            float v = 0.f;
            if (y < H && x < W) {
                const size_t e = (((size_t)b * H + y) * W + x) * C + c;
                v = to_f<T>(g1[e]);
                if (g2) v += to_f<T>(g2[e]);
            }
            Gt[p * (C + 1) + c] = v;
        }
        for (int i = tid; i < NI * 18 * 18; i += nthr) {
            const int xx = i % 18, yy = (i / 18) % 18, pl = i / 324;
            const int y = y0 + yy - 1, x = x0 + xx - 1;
            St[i] = (y >= 0 && y < H && x >= 0 && x < W) ? S[(((size_t)b * NI + pl) * H + y) * W + x] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int it = tid + q * nthr;
            if (it >= items) break;
            const int c = it % C, kk = it / C;
            const int ky = kk / 3, kx = kk % 3;
            for (int p = 0; p < 256; ++p) {
                const float gv = Gt[p * (C + 1) + c];
                const int so = (p / kEdgeT + ky) * 18 + p % kEdgeT + kx;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < NI) acc[q][i] = fmaf(gv, St[i * 324 + so], acc[q][i]);
            }
        }
        if (tid < C) {
            for (int p = 0; p < 256; ++p) sumg += Gt[p * (C + 1) + tid];
        } else if (tid - C < NI) {
            const int pl = tid - C;
            for (int p = 0; p < 256; ++p) sums += St[pl * 324 + (p / kEdgeT + 1) * 18 + p % kEdgeT + 1];
        }
    }
    float* out = partial + (size_t)blockIdx.x * (9 * NI * C + C + NI);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int it = tid + q * nthr;
        if (it >= items) break;
        const int c = it % C, kk = it / C;
        for (int i = 0; i < NI; ++i) out[(kk * NI + i) * C + c] = acc[q][i];
    }
    if (tid < C) out[9 * NI * C + tid] = sumg;
    else if (tid - C < NI) out[9 * NI * C + C + tid - C] = sums;
}
// Fast path for the reference shape (C = 32 channels, NI = 2 planes).  A block owns a strip of PIXB columns x `rows`
// rows of one sample; thread = (pixel column, 16-byte channel piece): G is read with one 16-byte load per pixel, the
// 3x3xNI neighbourhood of S comes from an LDS tile (staged 32 rows at a time), and each thread keeps EPB x 9 x NI
// accumulators in registers for the whole strip.  The pixel lanes are folded at the end (wave shuffles, then LDS).
template <typename T>
__global__ void __launch_bounds__(256) edge_wgrad_strip_kernel(const T* __restrict__ g1, const T* __restrict__ g2,
                                                               const float* __restrict__ S, float* __restrict__ partial, int H,
                                                               int W, int rows, int sx, int sy) {
    constexpr int C = 32, NI = 2, EPB = Piece<T>::N, PPB = C / EPB, PIXB = 256 / PPB, SW = PIXB + 2;
    constexpr int NACC = EPB * 9 * NI;
    __shared__ float St[NI][kEdgeChunk + 2][SW];
    __shared__ float red[4][PPB][NACC + EPB + NI];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = tid % PPB, p = tid / PPB;
    const int strip = blockIdx.x;
    const int b = strip / (sx * sy), x0 = (strip % sx) * PIXB, y0 = ((strip / sx) % sy) * rows;
    const int y1 = y0 + rows < H ? y0 + rows : H;
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
    float sumg[EPB], sums[NI];
#pragma unroll
    for (int e = 0; e < EPB; ++e) sumg[e] = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) sums[i] = 0.f;
    const int x = x0 + p;
    const bool xok = x < W;
    for (int yc = y0; yc < y1; yc += kEdgeChunk) {
        const int nr = y1 - yc < kEdgeChunk ? y1 - yc : kEdgeChunk;
        __syncthreads();
        for (int i = tid; i < NI * (kEdgeChunk + 2) * SW; i += 256) {
            const int cx = i % SW, ry = (i / SW) % (kEdgeChunk + 2), pl = i / (SW * (kEdgeChunk + 2));
            const int gy = yc - 1 + ry, gx = x0 - 1 + cx;
            const bool ok = ry < nr + 2 && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float v = S[(((size_t)b * NI + pl) * H + (ok ? gy : 0)) * W + (ok ? gx : 0)];
            St[pl][ry][cx] = ok ? v : 0.f;
        }
        __syncthreads();
        // G pieces are requested one row ahead of their use (clamped address, masked after the load)
        const size_t ebase = (((size_t)b * H + yc) * W + (xok ? x : x0)) * C + j * EPB;
        const size_t rstride = (size_t)W * C;
        uint4 n1 = *(const uint4*)(g1 + ebase), n2 = make_uint4(0, 0, 0, 0);
        if (g2) n2 = *(const uint4*)(g2 + ebase);
#pragma unroll 1
        for (int r = 0; r < nr; ++r) {
            const uint4 c1 = n1, c2 = n2;
            const size_t en = ebase + (size_t)(r + 1 < nr ? r + 1 : r) * rstride;
            n1 = *(const uint4*)(g1 + en);
            if (g2) n2 = *(const uint4*)(g2 + en);
            float g[EPB];
            Piece<T>::unpack(c1, g);
            if (g2) {
                float g2v[EPB];
                Piece<T>::unpack(c2, g2v);
#pragma unroll
                for (int q = 0; q < EPB; ++q) g[q] += g2v[q];
            }
            if (!xok) {
#pragma unroll
                for (int q = 0; q < EPB; ++q) g[q] = 0.f;
            }
#pragma unroll
            for (int q = 0; q < EPB; ++q) sumg[q] += g[q];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if (xok) sums[i] += St[i][r + 1][p + 1];
#pragma unroll
                for (int kk = 0; kk < 9; ++kk) {
                    const float sv = St[i][r + kk / 3][p + kk % 3];
#pragma unroll
                    for (int q = 0; q < EPB; ++q) acc[(q * 9 + kk) * NI + i] = fmaf(g[q], sv, acc[(q * 9 + kk) * NI + i]);
                }
            }
        }
    }
    // fold the pixel lanes of a wave (lanes with equal j: xor over the lane bits above log2(PPB)), then the 4 waves
    auto fold = [&](float v) __attribute__((always_inline)) -> float {
#pragma unroll
        for (int o = PPB; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = fold(acc[k]);
#pragma unroll
    for (int q = 0; q < EPB; ++q) sumg[q] = fold(sumg[q]);
#pragma unroll
    for (int i = 0; i < NI; ++i) sums[i] = fold(sums[i]);
    __syncthreads();
    if (lane < PPB) {
#pragma unroll
        for (int k = 0; k < NACC; ++k) red[wave][lane][k] = acc[k];
#pragma unroll
        for (int q = 0; q < EPB; ++q) red[wave][lane][NACC + q] = sumg[q];
#pragma unroll
        for (int i = 0; i < NI; ++i) red[wave][lane][NACC + EPB + i] = sums[i];
    }
    __syncthreads();
    float* out = partial + (size_t)blockIdx.x * (9 * NI * C + C + NI);
    for (int k = tid; k < PPB * (NACC + EPB); k += 256) {
        const int jj = k / (NACC + EPB), r = k % (NACC + EPB);
        const float v = (red[0][jj][r] + red[1][jj][r]) + (red[2][jj][r] + red[3][jj][r]);
        if (r < NACC) {
            const int i = r % NI, kk = (r / NI) % 9, q = r / (NI * 9);
            out[(kk * NI + i) * C + jj * EPB + q] = v;
        } else {
            out[9 * NI * C + jj * EPB + (r - NACC)] = v;
        }
    }
    if (tid < NI)  // every piece lane of a pixel added the same S values: take piece 0
        out[9 * NI * C + C + tid] = (red[0][0][NACC + EPB + tid] + red[1][0][NACC + EPB + tid]) +
                                    (red[2][0][NACC + EPB + tid] + red[3][0][NACC + EPB + tid]);
}

// mode 0 (input conv): dW[c][i][kk], db[c] = sumG;  mode 1 (output conv): dW[i][c][kk] = R[8-kk], db[i] = sumS
__global__ void __launch_bounds__(256) edge_wgrad_reduce_kernel(const float* __restrict__ partial, int nblocks, int C, int NI,
                                                                int mode, float* __restrict__ dW, float* __restrict__ db) {
    __shared__ double red[4][64];
    const int per = 9 * NI * C + C + NI;
    const int o64 = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + o64;
    double s = 0.0;
    if (i < per) s = strided_sum8<4>(q, nblocks, [&](int k) { return partial[(size_t)k * per + i]; });
    red[q][o64] = s;
    __syncthreads();
    if (q != 0 || i >= per) return;
    s = (red[0][o64] + red[1][o64]) + (red[2][o64] + red[3][o64]);
    if (i < 9 * NI * C) {
        const int c = i % C, pl = (i / C) % NI, kk = i / (C * NI);
        if (mode == 0) dW[((size_t)c * NI + pl) * 9 + kk] = (float)s;
        else dW[((size_t)pl * C + c) * 9 + (8 - kk)] = (float)s;
    } else if (i < 9 * NI * C + C) {
        if (mode == 0) db[i - 9 * NI * C] = (float)s;
    } else if (mode == 1) {
        db[i - 9 * NI * C - C] = (float)s;
    }
}
size_t edge_wgrad_partial_floats(int dtype, int B, int C, int NI, int H, int W) {
    EdgePlan p;
    if (edge_plan(EDGE_WGRAD, dtype, B, C, NI, H, W, 0, &p)) return 0;
    return (size_t)p.partial_blocks * (9 * NI * C + C + NI);
}
hipError_t edge_wgrad_launch(int dtype, int mode, const void* g1, const void* g2, const float* S, float* partial, float* dW,
                             float* db, int B, int C, int NI, int H, int W, hipStream_t s) {
    EdgePlan p;
    if (edge_plan(EDGE_WGRAD, dtype, B, C, NI, H, W, 0, &p)) return hipErrorInvalidValue;
    const int nb = p.partial_blocks;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (p.variant)
            hipLaunchKernelGGL(edge_wgrad_strip_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)g1, (const T*)g2, S, partial, H, W,
                               kStripRows, p.tiles_x, p.tiles_y);
        else
            hipLaunchKernelGGL(edge_wgrad_kernel<T>, dim3(nb), dim3(288), p.lds, s, (const T*)g1, (const T*)g2, S, partial, C, NI, H, W,
                               p.tiles_x, p.tiles_y, B * p.tiles_x * p.tiles_y);
    });
    hipLaunchKernelGGL(edge_wgrad_reduce_kernel, dim3(p.reduce_blocks), dim3(256), 0, s, partial, nb, C, NI, mode, dW, db);
    return hipGetLastError();
}

// =====================================================================================================
// launch geometry of every launcher above, and what each refuses (host only)
// =====================================================================================================
static const char* edge_why(const char* fmt, ...) {
    static thread_local char buf[200];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}
const char* edge_plan(int op, int dtype, int B, int C0, int Cio, int H, int W, int groups, EdgePlan* p) {
    memset(p, 0, sizeof(*p));
    constexpr long long kIntMax = 0x7fffffffll, kLds = 64 * 1024;
    constexpr int kGridY = 65535;
    if (dtype != DT_F32 && dtype != DT_BF16) return edge_why("dtype %d is neither DDIMX_F32 nor DDIMX_BF16", dtype);
    if (B < 1 || H < 1 || W < 1 || C0 < 1 || Cio < 1)
        return edge_why("B = %d, H = %d, W = %d, C0 = %d, Cio = %d: each must be at least 1", B, H, W, C0, Cio);
    // tile and strip origins plus their halo (at most H + 160, W + 66) are int; element offsets are 64-bit
    if (H > kIntMax - 256 || W > kIntMax - 256) return edge_why("H = %d, W = %d: tile origins plus halo overflow int", H, W);
    if ((double)B * H * W * (C0 > Cio ? C0 : Cio) >= 4.0e18) return edge_why("B H W C = %g elements overflow 64-bit byte offsets", (double)B * H * W * (C0 > Cio ? C0 : Cio));
    const int epb = epb_of(dtype);
    const long long HW = (long long)H * W;
    const bool fixed = C0 == 32 && Cio == 2;  // the reference's widths: every op has a kernel of its own for them
    p->variant = fixed ? 1 : 0;
    p->threads = 256;
    p->grid_y = 1;
    p->trips = 1;
    auto cdiv = [](long long a, long long b) { return (a + b - 1) / b; };
    switch (op) {
    case EDGE_CONV_IN: {
        const int opp = C0 / epb;
        if (C0 % epb || opp > 64 || (opp & (opp - 1)))
            return edge_why("C0 = %d: must be %d times a power of two up to 64", C0, epb);
        if (groups && C0 % kGroups) return edge_why("C0 = %d: group-format statistics need a multiple of %d", C0, kGroups);
        if (B > kGridY) return edge_why("B = %d exceeds the grid's y limit %d", B, kGridY);
        // generic: int pix < parts * 1024 <= H W + 1023.  MFMA: the int offset hoff + pc + W + 1 reaches 2 H W - 1
        const long long lim = fixed ? (1ll << 30) : kIntMax - (kInPixPerBlock - 1);
        if (HW > lim) return edge_why("H W = %lld exceeds %lld, the kernel's int pixel offsets", HW, lim);
        const long long lds = fixed ? 0 : ((long long)Cio * 9 * C0 + 4 * C0 * 2) * 4;
        if (lds > kLds) return edge_why("Cin = %d, C0 = %d: %lld bytes of LDS exceed %lld", Cio, C0, lds, kLds);
        p->lds = (int)lds;
        p->grid_x = (unsigned)cdiv(HW, kInPixPerBlock);
        p->grid_y = B;
        p->tiles_x = (int)p->grid_x;
        p->tiles_y = 1;
        const long long full = HW < kInPixPerBlock ? HW : kInPixPerBlock;  // pixels of the fullest part
        // MFMA: wave 0's 32-pixel blocks; generic: pixels per slot of 256 / opp slots
        p->trips = (int)(fixed ? cdiv(cdiv(full, 32), 4) : cdiv(full, 256 / opp));
        return nullptr;
    }
    case EDGE_CONV_OUT:
    case EDGE_CONV_IN_BWD_DATA: {
        const bool out = op == EDGE_CONV_OUT;
        if (Cio > 4) return edge_why("%s = %d: at most 4", out ? "Cout" : "Cin", Cio);
        if (out && C0 % 8) return edge_why("C0 = %d: must be a multiple of 8", C0);
        if (!out && C0 % epb) return edge_why("C0 = %d: must be a multiple of %d", C0, epb);
        const long long lds = (long long)(kTileH + 2) * (kTileW + 2) * (C0 + 1) * 4;
        if (out && lds > kLds) return edge_why("C0 = %d: %lld bytes of LDS exceed %lld", C0, lds, kLds);
        if (out || fixed) {  // one block per 8 x 32 tile, the sample folded into grid.x: int tile arithmetic
            const long long tx = cdiv(W, kTileW), ty = cdiv(H, kTileH);
            if (tx * ty > kIntMax || tx * ty * B > kIntMax)
                return edge_why("B = %d x %lld x %lld tiles exceed the int tile index", B, ty, tx);
            p->tiles_x = (int)tx;
            p->tiles_y = (int)ty;
            p->grid_x = (unsigned)(tx * ty * B);
            p->lds = out && !fixed ? (int)lds : 0;
            return nullptr;
        }
        if (B > kGridY) return edge_why("B = %d exceeds the grid's y limit %d", B, kGridY);
        p->grid_x = (unsigned)(cdiv(HW, 256) < 4096 ? cdiv(HW, 256) : 4096);  // pixel indices are 64-bit
        p->grid_y = B;
        p->trips = (int)cdiv(HW, p->grid_x * 256ll);
        return nullptr;
    }
    case EDGE_CONV_OUT_BWD_DATA: {
        if (B > kGridY) return edge_why("B = %d exceeds the grid's y limit %d", B, kGridY);
        p->grid_y = B;
        if (fixed) {  // pixel indices are 64-bit
            const int pixb = edge_pixb(dtype);
            const long long want = cdiv(HW, pixb * 8);  // ~8 pixels per thread
            p->grid_x = (unsigned)(want > 4096 ? 4096 : want);
            p->trips = (int)cdiv(HW, (long long)p->grid_x * pixb);
            return nullptr;
        }
        if (C0 % epb) return edge_why("C0 = %d: must be a multiple of %d", C0, epb);
        const long long lds = 9ll * Cio * C0 * 4;
        if (lds > kLds) return edge_why("Cout = %d, C0 = %d: %lld bytes of LDS exceed %lld", Cio, C0, lds, kLds);
        const long long pieces = HW * (C0 / epb);  // 64-bit in the kernel
        p->lds = (int)lds;
        p->grid_x = (unsigned)(cdiv(pieces, 256) < 4096 ? cdiv(pieces, 256) : 4096);
        p->trips = (int)cdiv(pieces, p->grid_x * 256ll);
        return nullptr;
    }
    case EDGE_WGRAD: {
        if (Cio > 4) return edge_why("Cio = %d: at most 4 planes", Cio);
        long long nb;
        if (fixed) {
            const int pb = edge_pixb(dtype);
            const long long sx = cdiv(W, pb), sy = cdiv(H, kStripRows);
            nb = sx * sy * B;
            if (sx * sy > kIntMax || nb > kIntMax - 1024) return edge_why("B = %d x %lld x %lld strips exceed the int block index", B, sy, sx);
            p->tiles_x = (int)sx;
            p->tiles_y = (int)sy;
            p->grid_x = (unsigned)nb;
            p->trips = (int)cdiv(H < kStripRows ? H : kStripRows, kEdgeChunk);  // chunks of the tallest strip
        } else {
            if (9 * C0 > 2 * 288 || C0 + Cio > 288) return edge_why("C0 = %d: more than two of 9 C0 items per thread", C0);
            const long long lds = (256ll * (C0 + 1) + Cio * 324) * 4;
            if (lds > kLds) return edge_why("C0 = %d, Cio = %d: %lld bytes of LDS exceed %lld", C0, Cio, lds, kLds);
            const long long tx = cdiv(W, kEdgeT), ty = cdiv(H, kEdgeT), tiles = tx * ty * B;
            // the tile loop's int counter runs to tiles + grid - 1
            if (tx * ty > kIntMax || tiles > kIntMax - 1024) return edge_why("B = %d x %lld x %lld tiles exceed the int tile index", B, ty, tx);
            nb = tiles < 1024 ? tiles : 1024;
            p->tiles_x = (int)tx;
            p->tiles_y = (int)ty;
            p->grid_x = (unsigned)nb;
            p->threads = 288;
            p->lds = (int)lds;
            p->trips = (int)cdiv(tiles, nb);
        }
        p->partial_blocks = (int)nb;
        p->reduce_blocks = (9 * Cio * C0 + C0 + Cio + 63) / 64;
        // the reduce's quarter 0 takes partials 0, 4, 8, ..: eight per unrolled trip while k + 28 < nb, one per trip after
        p->reduce_unrolled = nb > 28 ? (int)cdiv(nb - 28, 32) : 0;
        p->reduce_tail = (int)cdiv(nb - 32ll * p->reduce_unrolled > 0 ? nb - 32ll * p->reduce_unrolled : 0, 4);
        return nullptr;
    }
    }
    return edge_why("op %d is no edge launcher", op);
}

}  // namespace ddimx
