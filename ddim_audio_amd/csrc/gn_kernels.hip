// GroupNorm around the fused convolutions, forward and backward: finalisation of the statistics partials, the residual
// pass, per-channel tensor statistics, the three backward steps and the column / part sums of their parameter gradients.
// All element-wise passes share one partitioning of a sample (elem_geom) and one reduction of it to a slab (slab_reduce).
// gfx950 only.
// Every reduction is a fixed-order tree (no float atomics): results are reproducible.  The reference obtains the backward
// from autograd (runners/diffusion.py:150 `loss.backward()`) over models/diffusion.py:42-56 (Residual_Block).
#include "gn_kernels.h"

namespace ddimx {

// =====================================================================================================
// GroupNorm finalisation: partial (sum, sumsq) slabs -> per-(sample, channel) scale / shift
//   scale = rstd_g * gamma_c ; shift = beta_c - mean_g * scale     (torch.nn.GroupNorm, biased variance)
// =====================================================================================================
// One 256-thread block per (group, sample): every thread sums a strided share of the (sum, sumsq) pairs in fp64 (8-byte loads,
// up to four issued before the first use), then wave butterflies + one LDS exchange (fixed order) give the group's totals.
__global__ void __launch_bounds__(256) gn_finalize_kernel(const float* __restrict__ stats, int nparts, int Cs, int C,
                                                          double count, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          float* __restrict__ scale, float* __restrict__ shift,
                                                          float* __restrict__ mr_out) {
    __shared__ double rs[4], rq[4];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int GS = C / kGroups, reps = Cs / C;
    const int per_part = reps * GS, total = nparts * per_part;
    const float2* base = (const float2*)stats + (size_t)b * nparts * Cs;
    double s = 0.0, q = 0.0;
    for (int i0 = tid; i0 < total; i0 += 256 * 4) {
        float2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 256;
            v[u] = make_float2(0.f, 0.f);
            if (i < total) {
                const int part = i / per_part, r = i - part * per_part;
                const int rep = r / GS;
                v[u] = base[(size_t)part * Cs + rep * C + g * GS + (r - rep * GS)];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { s += (double)v[u].x; q += (double)v[u].y; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
    if ((tid & 63) == 0) { rs[tid >> 6] = s; rq[tid >> 6] = q; }
    __syncthreads();
    const double S = (rs[0] + rs[1]) + (rs[2] + rs[3]), Q = (rq[0] + rq[1]) + (rq[2] + rq[3]);
    const double mean = S / count;
    double var = Q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float mf = (float)mean, rf = (float)(1.0 / sqrt(var + (double)eps));
    if (mr_out && tid == 0) {  // saved for the backward pass: [B][groups][2] = (mean, rstd)
        mr_out[((size_t)b * kGroups + g) * 2 + 0] = mf;
        mr_out[((size_t)b * kGroups + g) * 2 + 1] = rf;
    }
    for (int i = tid; i < GS; i += 256) {
        const int c = g * GS + i;
        const float sc = rf * gamma[c];
        scale[(size_t)b * C + c] = sc;
        shift[(size_t)b * C + c] = (beta ? beta[c] : 0.f) - mf * sc;
    }
}

hipError_t gn_finalize_launch(const float* stats, int nparts, int Cs, int C, double count, const float* gamma,
                              const float* beta, float eps, float* scale, float* shift, int B, hipStream_t s, float* mr_out) {
    if (C % kGroups || Cs % C) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(kGroups, B), dim3(256), 0, s, stats, nparts, Cs, C, count, gamma, beta,
                       eps, scale, shift, mr_out);
    return hipGetLastError();
}

// The same from group-format partials (gn_fused.h) -- used where a sample has more than kGnFuseMaxParts partials (long
// spectrograms at the shallow levels), so that consumers need not re-read them per workgroup.  One block per sample.
__global__ void __launch_bounds__(1024) gn_finalize_groups_kernel(const GnIn gn, int C, float* __restrict__ scale,
                                                                  float* __restrict__ shift) {
    __shared__ float scr[16 * kGroups * 2];
    const int b = blockIdx.x, tid = threadIdx.x, bd = blockDim.x;
    GnInLoads ld;
    gn_in_issue(gn, b, tid, bd, ld);
    gn_in_reduce(gn, b, tid, bd, ld, scr);
    __syncthreads();
    for (int c = tid; c < C; c += bd) {
        float m, r;
        gn_in_group(gn, scr, bd >> 6, c / (C / kGroups), &m, &r);
        const float sc = r * gn.gamma[c];
        scale[(size_t)b * C + c] = sc;
        shift[(size_t)b * C + c] = fmaf(-m, sc, gn.beta ? gn.beta[c] : 0.f);
    }
}
// nthreads: the block size of the consumer this replaces the in-kernel finalisation of (64 .. 1024, a multiple of 64) -- the
// reduction order, and with it every bit of the result, is a function of (gn.np, nthreads)
hipError_t gn_finalize_groups_launch(const GnIn& gn, int C, float* scale, float* shift, int B, int nthreads, hipStream_t s) {
    if (C % kGroups || nthreads < 64 || nthreads > 1024 || nthreads % 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_finalize_groups_kernel, dim3(B), dim3(nthreads), 0, s, gn, C, scale, shift);
    return hipGetLastError();
}

// =====================================================================================================
// the element-wise passes over a sample (resid, tensor_stats, gn_bwd_stats, gn_bwd_apply): one launch geometry,
// one slab reduction (resid, gn_bwd_apply)
// =====================================================================================================
constexpr int kResidIters = 16;  // at most: 16-byte pieces per thread
// iters, pieces per thread: 16 where the sample is large, fewer on the deep levels so that a sample still spreads over >= 64
// workgroups -- with 16 the level-5 tensor (8 192 pieces) was two workgroups per sample, each a chain of 16 dependent load round
// trips.  The partition is a function of the sample's size only (never of the batch): a sample's partial sums do not depend on the
// batch it is in.
struct ElemGeom {
    int epb, cpp;      // elements of a 16-byte piece, pieces per pixel
    int bd, rows;      // block size, pixels (rows of the LDS table) a block covers per iteration
    int iters, nparts, nt;
    dim3 grid;         // (nparts, B)
    size_t lds1, lds2; // bytes of a [rows][C] table of single sums / of (sum, sumsq) pairs
    bool ok;           // whole pieces per pixel, whole pixels per block
};
static ElemGeom elem_geom(int dtype, int B, int HW, int C) {
    ElemGeom g;
    g.epb = epb_of(dtype);
    g.cpp = C / g.epb;
    g.bd = (g.cpp % 3 == 0) ? 192 : 256;
    g.ok = C % g.epb == 0 && g.cpp > 0 && g.bd % g.cpp == 0;
    g.rows = g.cpp > 0 ? g.bd / g.cpp : 0;
    const long long pieces = (long long)HW * g.cpp;
    const long long it = pieces / ((long long)g.bd * 64);
    g.iters = (int)(it < 1 ? 1 : it > kResidIters ? kResidIters : it);
    const int per_block = g.bd * g.iters;
    g.nparts = (int)((pieces + per_block - 1) / per_block);
    g.nt = nt_streaming((size_t)B * HW * C * esz(dtype));
    g.grid = dim3(g.nparts, B);
    g.lds1 = (size_t)g.rows * C * 4;
    g.lds2 = 2 * g.lds1;
    return g;
}
int resid_threads(int dtype, int C) { return elem_geom(dtype, 1, 1, C).bd; }
int resid_iters(int dtype, int HW, int C) { return elem_geom(dtype, 1, HW, C).iters; }
int resid_nparts(int dtype, int HW, int C) { return elem_geom(dtype, 1, HW, C).nparts; }

// The sample walk of those passes is written out in each kernel (workgroup `part` of a sample takes the pieces pc0 + it * bd,
// it < iters, pc0 = part * iters * bd + tid, NIT iterations' loads issued together): through one helper taking the loads and their
// use as callables, gn_bwd_stats ran 4-14 % and tensor_stats 2-3 % slower at the level-0 and level-2 shapes.

// Per-thread sums of EPB channels to the workgroup's slab `stats[slab]`, W = 2: pairs (a, b) -> [C][2], W = 1: a alone -> [C].
// One row of LDS per pixel of the block, a barrier, then every column added over the rows in the order 0 .. R-1: every producer
// of a slab over this partition reduces in this order.  TAIL and groups: the slab is folded to the group format (gn_fused.h)
// instead.  red: [R][C*W] floats, + [C*W] with TAIL (only a kernel whose launcher adds that room instantiates it).
// resid_kernel and both reductions of gn_bwd_apply_kernel call it; tensor_stats_kernel and gn_bwd_stats_kernel hold the same
// reduction as copies (see there), and tests/test_gpu_gn_kernels.py pins that all of them give the same bits.
template <int EPB, int W, bool TAIL = false>
__device__ __forceinline__ void slab_reduce(float* red, const float* a, const float* b, int C, int bd, float* __restrict__ stats, int groups = 0) {
    static_assert(!TAIL || W == 2, "the group format holds (sum, sumsq) pairs");
    if (!TAIL) groups = 0;
    const int tid = threadIdx.x;
    const int CPP = C / EPB, R = bd / CPP, row = tid / CPP, c = tid % CPP;
    const size_t slab = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int j = 0; j < EPB; ++j) {
        red[(row * C + c * EPB + j) * W] = a[j];
        if (W == 2) red[(row * C + c * EPB + j) * W + 1] = b[j];
    }
    __syncthreads();
    float* const chan = red + R * C * W;  // the workgroup's per-channel totals (group format)
    for (int i = tid; i < C * W; i += bd) {
        float t = 0.f;
#pragma unroll 8
        for (int r = 0; r < R; ++r) t += red[r * C * W + i];
        if (groups) chan[i] = t;
        else stats[slab * C * W + i] = t;
    }
    if (groups) {
        __syncthreads();
        if (tid < 64) gn_bins_store<1>(chan, 0, C, 0, C, stats + slab * kGnSlab, tid);
    }
}

// =====================================================================================================
// residual pass: y = x + (h*scale + shift)   or   y = x + h(fp32)
// =====================================================================================================
// LDS: [R][C*2] per-row channel sums | [C*2] workgroup totals | [4 waves][8][2] floats (fused GroupNorm input)
template <typename T, bool HF32, bool HSILU = false>
__global__ void __launch_bounds__(256) resid_kernel(const T* x, const void* __restrict__ hv,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    T* y, float* __restrict__ stats, int HW, int C, const GnIn gn, int groups, int iters,
                                                    int nt) {
    constexpr int EPB = Piece<T>::N;
    extern __shared__ __attribute__((aligned(16))) float red[];  // [R][C*2]
    const int tid = threadIdx.x, bd = blockDim.x;
    const int CPP = C / EPB;
    const int c = tid % CPP;
    const int b = blockIdx.y, part = blockIdx.x;
    const long long pieces = (long long)HW * CPP;
    float* const scr = red + (bd / CPP) * C * 2 + C * 2;
    float sc[EPB], sh[EPB], s[EPB], q[EPB];
#pragma unroll
    for (int j = 0; j < EPB; ++j) { s[j] = q[j] = 0.f; sc[j] = 1.f; sh[j] = 0.f; }
    // one 16-byte piece of x and of h per thread and iteration
    constexpr int HN = HF32 ? EPB / 4 : 1;
    const size_t sbase = (size_t)b * HW * C;
    auto load = [&](size_t e, uint4& vx, uint4 (&vh)[HN]) __attribute__((always_inline)) {
        vx = nt ? nt_load16(x + e) : *(const uint4*)(x + e);  // (nt: uniform)
        if constexpr (HF32) {
#pragma unroll
            for (int k = 0; k < HN; ++k) vh[k] = *(const uint4*)((const float*)hv + e + 4 * k);
        } else {
            vh[0] = nt ? nt_load16((const T*)hv + e) : *(const uint4*)((const T*)hv + e);
        }
    };
    auto process = [&](size_t e, const uint4& vx, const uint4 (&vh)[HN]) __attribute__((always_inline)) {
        float fx[EPB], fh[EPB];
        Piece<T>::unpack(vx, fx);
        if constexpr (HF32) {
#pragma unroll
            for (int k = 0; k < HN; ++k) {
                fh[4 * k] = __uint_as_float(vh[k].x); fh[4 * k + 1] = __uint_as_float(vh[k].y);
                fh[4 * k + 2] = __uint_as_float(vh[k].z); fh[4 * k + 3] = __uint_as_float(vh[k].w);
            }
        } else {
            Piece<T>::unpack(vh[0], fh);
        }
#pragma unroll
        for (int j = 0; j < EPB; ++j) fx[j] = fx[j] + fmaf(HSILU ? silu_f(fh[j]) : fh[j], sc[j], sh[j]);
        const uint4 pv = Piece<T>::pack(fx);
        if (nt) nt_store16(y + e, pv);
        else *(uint4*)(y + e) = pv;
        Piece<T>::unpack(pv, fx);
#pragma unroll
        for (int j = 0; j < EPB; ++j) { s[j] += fx[j]; q[j] = fmaf(fx[j], fx[j], q[j]); }
    };
    if (!HF32) {
        if (gn.stats) {  // uniform: finish the GroupNorm of h here (gn_fused.h)
            float gam[EPB], bet[EPB];
            GnInLoads ld;
            gn_in_issue(gn, b, tid, bd, ld);
            gn_in_params<EPB>(gn, c * EPB, gam, bet);
            gn_in_reduce(gn, b, tid, bd, ld, scr);
            __syncthreads();
            gn_in_fold<EPB>(gn, scr, bd >> 6, C, c * EPB, gam, bet, sc, sh);
        } else {
#pragma unroll
            for (int j = 0; j < EPB; ++j) {
                sc[j] = scale[(size_t)b * C + c * EPB + j];
                sh[j] = shift[(size_t)b * C + c * EPB + j];
            }
        }
    }
    // four iterations' loads are issued together (unconditionally: out-of-range slots re-read piece 0 and are dropped; a load
    // under a branch is waited for at once, and the loop used to be one load round trip + one store acknowledgement per
    // iteration), then the four are processed and stored.  x may alias y: a thread only ever touches its own pieces.
    const long long pc0 = (long long)part * iters * bd + tid;
    for (int it0 = 0; it0 < iters; it0 += 4) {
        uint4 vx[4], vh[4][HN];
        size_t e[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long pc = pc0 + (long long)(it0 + u) * bd;
            ok[u] = it0 + u < iters && pc < pieces;
            e[u] = sbase + (size_t)(ok[u] ? pc : 0) * EPB;
            load(e[u], vx[u], vh[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ok[u]) process(e[u], vx[u], vh[u]);
    }
    if (stats) slab_reduce<EPB, 2, true>(red, s, q, C, bd, stats, groups);
}

hipError_t resid_launch(int dtype, const void* x, const void* h, int h_f32, const float* scale, const float* shift,
                        void* y, float* stats, int B, int HW, int C, hipStream_t s, const GnIn* gn, int groups) {
    const ElemGeom eg = elem_geom(dtype, B, HW, C);
    if (!eg.ok || C % kGroups) return hipErrorInvalidValue;
    GnIn g = {};
    if (gn) g = *gn;
    if (g.stats && (h_f32 == 1 || g.np > kGnFuseMaxParts)) return hipErrorInvalidValue;
    const size_t lds = eg.lds2 + (size_t)C * 2 * 4 + 4 * kGroups * 2 * 4;  // + the workgroup's totals + the fused GroupNorm input
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        auto launch = [&](auto k) {
            hipLaunchKernelGGL(k, eg.grid, dim3(eg.bd), lds, s, (const T*)x, h, scale, shift, (T*)y, stats, HW, C, g, groups, eg.iters, eg.nt);
        };
        if (h_f32 == 2) launch(resid_kernel<T, false, true>);  // training forward: h holds the pre-activation, y = x + SiLU(h)*scale + shift
        else if (h_f32) launch(resid_kernel<T, true>);
        else launch(resid_kernel<T, false>);
    });
    return hipGetLastError();
}


// ---- per-channel statistics of an NHWC tensor (used when a tensor arrives without producer stats) ----
template <typename T>
__global__ void __launch_bounds__(256) tensor_stats_kernel(const T* __restrict__ x, float* __restrict__ stats, int HW,
                                                           int C, int groups, int iters) {
    constexpr int EPB = Piece<T>::N;
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int tid = threadIdx.x, bd = blockDim.x;
    const int CPP = C / EPB, c = tid % CPP, b = blockIdx.y, part = blockIdx.x;
    const long long pieces = (long long)HW * CPP;
    float s[EPB], q[EPB];
#pragma unroll
    for (int j = 0; j < EPB; ++j) s[j] = q[j] = 0.f;
    for (int it = 0; it < iters; ++it) {
        const long long pc = ((long long)part * iters + it) * bd + tid;
        if (pc >= pieces) break;
        float f[EPB];
        Piece<T>::unpack(*(const uint4*)(x + (size_t)b * HW * C + (size_t)pc * EPB), f);
#pragma unroll
        for (int j = 0; j < EPB; ++j) { s[j] += f[j]; q[j] = fmaf(f[j], f[j], q[j]); }
    }
    // slab_reduce<EPB, 2, true>, kept as a copy: through the helper the level-0 shape timed 0.2-0.9 % above the copy's spread
    const int R = bd / CPP, row = tid / CPP;
#pragma unroll
    for (int j = 0; j < EPB; ++j) {
        red[(row * C + c * EPB + j) * 2 + 0] = s[j];
        red[(row * C + c * EPB + j) * 2 + 1] = q[j];
    }
    __syncthreads();
    float* const chan = red + R * C * 2;
    for (int i = tid; i < C * 2; i += bd) {
        float t = 0.f;
#pragma unroll 8
        for (int r = 0; r < R; ++r) t += red[r * C * 2 + i];
        if (groups) chan[i] = t;
        else stats[(((size_t)b * gridDim.x + part) * C) * 2 + i] = t;
    }
    if (groups) {
        __syncthreads();
        if (tid < 64) gn_bins_store<1>(chan, 0, C, 0, C, stats + ((size_t)b * gridDim.x + part) * kGnSlab, tid);
    }
}
hipError_t tensor_stats_launch(int dtype, const void* x, float* stats, int B, int HW, int C, hipStream_t s, int groups) {
    const ElemGeom eg = elem_geom(dtype, B, HW, C);
    if (!eg.ok || (groups && C % kGroups)) return hipErrorInvalidValue;
    const size_t lds = eg.lds2 + (size_t)C * 2 * 4;  // + the workgroup's totals
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(tensor_stats_kernel<T>, eg.grid, dim3(eg.bd), lds, s, (const T*)x, stats, HW, C, groups, eg.iters);
    });
    return hipGetLastError();
}

// =====================================================================================================
// GroupNorm backward, step 1: per-(sample, channel) partial sums  P = sum g' ,  Q = sum g' * v
//   MODE 0 (GroupNorm fed by SiLU(u): GN1, GN2):   g' = g,                          v = SiLU(u)
//   MODE 1 (GroupNorm followed by SiLU: GN0):      g' = g * SiLU'(scale*x + shift), v = x      (u = x)
// same partitioning as tensor_stats / resid (resid_nparts), output [B][nparts][C][2]
// =====================================================================================================
template <typename T, int MODE>
__global__ void __launch_bounds__(256) gn_bwd_stats_kernel(const T* __restrict__ g, const T* __restrict__ u,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           float* __restrict__ stats, int HW, int C, int iters, int nt) {
    constexpr int EPB = Piece<T>::N;
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int tid = threadIdx.x, bd = blockDim.x;
    const int CPP = C / EPB, c = tid % CPP, b = blockIdx.y, part = blockIdx.x;
    const long long pieces = (long long)HW * CPP;
    float sc[EPB], sh[EPB], P[EPB], Q[EPB];
#pragma unroll
    for (int j = 0; j < EPB; ++j) {
        P[j] = Q[j] = 0.f;
        sc[j] = MODE == 1 ? scale[(size_t)b * C + c * EPB + j] : 1.f;
        sh[j] = MODE == 1 ? shift[(size_t)b * C + c * EPB + j] : 0.f;
    }
    // four iterations' loads are issued together, unconditionally (out-of-range slots re-read piece 0 and are dropped): one
    // load round trip per four iterations instead of one per iteration
    const long long pc0 = (long long)part * iters * bd + tid;
    const size_t sbase = (size_t)b * HW * C;
    for (int it0 = 0; it0 < iters; it0 += 4) {
        uint4 vg[4], vu[4];
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long pc = pc0 + (long long)(it0 + k) * bd;
            ok[k] = it0 + k < iters && pc < pieces;
            const size_t e = sbase + (size_t)(ok[k] ? pc : 0) * EPB;
            vg[k] = nt ? nt_load16(g + e) : *(const uint4*)(g + e);
            vu[k] = nt ? nt_load16(u + e) : *(const uint4*)(u + e);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            float fg[EPB], fu[EPB];
            Piece<T>::unpack(vg[k], fg);
            Piece<T>::unpack(vu[k], fu);
#pragma unroll
            for (int j = 0; j < EPB; ++j) {
                float gp, v;
                if (MODE == 0) { gp = fg[j]; v = silu_f(fu[j]); }
                else { gp = fg[j] * dsilu_f(fmaf(fu[j], sc[j], sh[j])); v = fu[j]; }
                P[j] += gp;
                Q[j] = fmaf(gp, v, Q[j]);
            }
        }
    }
    // slab_reduce<EPB, 2>, kept as a copy: through the helper mode 1 at the level-2 shape timed 1-2 % above the copy's spread
    const int R = bd / CPP, row = tid / CPP;
#pragma unroll
    for (int j = 0; j < EPB; ++j) {
        red[(row * C + c * EPB + j) * 2 + 0] = P[j];
        red[(row * C + c * EPB + j) * 2 + 1] = Q[j];
    }
    __syncthreads();
    for (int i = tid; i < C * 2; i += bd) {
        float t = 0.f;
        for (int r = 0; r < R; ++r) t += red[r * C * 2 + i];
        stats[(((size_t)b * gridDim.x + part) * C) * 2 + i] = t;
    }
}
hipError_t gn_bwd_stats_launch(int dtype, int mode, const void* g, const void* u, const float* scale, const float* shift,
                               float* stats, int B, int HW, int C, hipStream_t s) {
    const ElemGeom eg = elem_geom(dtype, B, HW, C);
    if (!eg.ok) return hipErrorInvalidValue;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        auto k = mode ? gn_bwd_stats_kernel<T, 1> : gn_bwd_stats_kernel<T, 0>;
        hipLaunchKernelGGL(k, eg.grid, dim3(eg.bd), eg.lds2, s, (const T*)g, (const T*)u, scale, shift, stats, HW, C, eg.iters, eg.nt);
    });
    return hipGetLastError();
}

// =====================================================================================================
// GroupNorm backward, step 2: partial sums -> per-(sample, channel) coefficients of
//     d(input of the norm) = ca * g' + cb * v + cc
// and the per-sample parameter-gradient terms  dgamma_b[b][c] = rstd (Q - mean P),  dbeta_b[b][c] = P.
//   S1 = sum_{c in group} gamma_c P_c,  S2 = sum_{c in group} gamma_c rstd (Q_c - mean P_c),  N = elements per group
//   ca = gamma_c rstd,  cb = -rstd^2 S2 / N,  cc = -rstd S1 / N + mean rstd^2 S2 / N
// grid (groups, B)
// =====================================================================================================
__global__ void __launch_bounds__(256) gn_bwd_finalize_kernel(const float* __restrict__ stats, int nparts, int C, double count,
                                                              const float* __restrict__ gamma, const float* __restrict__ mr,
                                                              float* __restrict__ coef /*[B][3][C]*/, float* __restrict__ dgb /*[B][2][C]*/) {
    __shared__ double rp[8][32], rq[8][32];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int GS = C / kGroups;  // <= 32
    const float mean = mr[((size_t)b * kGroups + g) * 2 + 0], rstd = mr[((size_t)b * kGroups + g) * 2 + 1];
    const int ch = tid & 31, pl = tid >> 5;  // 8 part-lanes per channel
    const int c = g * GS + ch;
    double P = 0.0, Q = 0.0;
    {   // eight partials per thread in flight, unconditionally (clamped index, dropped by select), added in the original order: the
        // loop with a run-time trip count was one load round trip per partial, and this kernel is nothing else
        // (partsum_block's loop over (P, Q) pairs; kept apart: shared with it through a helper templated on the entry, the compiler
        // emitted nine load instructions for this kernel where this copy has ten)
        const int cs = ch < GS ? c : g * GS;
        for (int p0 = pl; p0 < nparts; p0 += 64) {
            float2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int p = p0 + 8 * u;
                v[u] = *(const float2*)(stats + (((size_t)b * nparts + (p < nparts ? p : nparts - 1)) * C + cs) * 2);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool in = ch < GS && p0 + 8 * u < nparts;
                P += in ? (double)v[u].x : 0.0;
                Q += in ? (double)v[u].y : 0.0;
            }
        }
    }
    rp[pl][ch] = P; rq[pl][ch] = Q;
    __syncthreads();
    if (tid >= 64) return;
    P = Q = 0.0;
    if (tid < GS) {
        for (int k = 0; k < 8; ++k) { P += rp[k][tid]; Q += rq[k][tid]; }
    }
    const int cc = g * GS + tid;
    const double gm = tid < GS ? (double)gamma[cc] : 0.0;
    const double dg = (double)rstd * (Q - (double)mean * P);
    double s1 = gm * P, s2 = gm * dg;
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (tid < GS) {
        const double r = (double)rstd;
        coef[((size_t)b * 3 + 0) * C + cc] = (float)(gm * r);
        coef[((size_t)b * 3 + 1) * C + cc] = (float)(-r * r * s2 / count);
        coef[((size_t)b * 3 + 2) * C + cc] = (float)(-r * s1 / count + (double)mean * r * r * s2 / count);
        dgb[((size_t)b * 2 + 0) * C + cc] = (float)dg;
        dgb[((size_t)b * 2 + 1) * C + cc] = (float)P;
    }
}
hipError_t gn_bwd_finalize_launch(const float* stats, int nparts, int C, double count, const float* gamma, const float* mr,
                                  float* coef, float* dgb, int B, hipStream_t s) {
    if (C % kGroups || C / kGroups > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(kGroups, B), dim3(256), 0, s, stats, nparts, C, count, gamma, mr, coef, dgb);
    return hipGetLastError();
}

// the column sums of the reductions below: column cl of the row lanes' partial sums red[N][M], added in row order
template <int N, int M>
__device__ __forceinline__ double fold_rows(const double (&red)[N][M], int cl) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) s += red[k][cl];
    return s;
}
// dst[c] = sum_b src[b * stride + c]: 16 columns x 16 row slices per block, slices folded in a fixed order
__global__ void __launch_bounds__(256) colsum_kernel(const float* __restrict__ src, int B, long long stride, int C,
                                                     float* __restrict__ dst) {
    __shared__ double red[16][16];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    red[rl][cl] = c < C ? strided_sum8<16>(rl, B, [&](int b) { return src[(size_t)b * stride + c]; }) : 0.0;
    __syncthreads();
    if (rl == 0 && c < C) dst[c] = (float)fold_rows(red, cl);
}
hipError_t colsum_launch(const float* src, int B, long long stride, int C, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(colsum_kernel, dim3((C + 15) / 16), dim3(256), 0, s, src, B, stride, C, dst);
    return hipGetLastError();
}
// the same sums for up to kMax (src, dst) pairs in one launch (the entries travel as kernel arguments): the backward defers
// its per-block parameter-gradient batch sums and flushes them together.  32 columns x 8 row lanes per block: another order of
// addition than colsum_kernel's
__global__ void __launch_bounds__(256) colsum_multi_kernel(const ColsumBatch q) {
    __shared__ double red[8][32];
    const int e = blockIdx.y;
    const int C = q.C[e], B = q.B[e];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    if (blockIdx.x * 32 >= C) return;  // uniform
    const float* src = q.src[e];
    const long long stride = q.stride[e];
    double s = 0.0;
    if (c < C)
        for (int b = rl; b < B; b += 8) s += (double)src[(size_t)b * stride + c];
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < C) q.dst[e][c] = (float)fold_rows(red, cl);
}
hipError_t colsum_multi_launch(const ColsumBatch& q, hipStream_t s) {
    if (q.count < 1) return hipSuccess;
    int mx = 0;
    for (int i = 0; i < q.count; ++i) if (q.C[i] > mx) mx = q.C[i];
    hipLaunchKernelGGL(colsum_multi_kernel, dim3((mx + 31) / 32, q.count), dim3(256), 0, s, q);
    return hipGetLastError();
}
// dst[b][c] = sum_p src[((b*nparts + p)*C + c) * src_step]
__device__ __forceinline__ void partsum_block(const float* __restrict__ src, int nparts, int C, float* __restrict__ dst,
                                              long long dst_stride, int src_step) {
    __shared__ double red[8][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl, b = blockIdx.y;
    double s = 0.0;
    {   // eight partials per thread in flight (see gn_bwd_finalize_kernel), same order of addition
        const int cs = c < C ? c : C - 1;
        for (int p0 = rl; p0 < nparts; p0 += 64) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int p = p0 + 8 * u;
                v[u] = src[(((size_t)b * nparts + (p < nparts ? p : nparts - 1)) * C + cs) * src_step];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (c < C && p0 + 8 * u < nparts) ? (double)v[u] : 0.0;
        }
    }
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < C) dst[(size_t)b * dst_stride + c] = (float)fold_rows(red, cl);
}
__global__ void __launch_bounds__(256) partsum_kernel(const float* __restrict__ src, int nparts, int C, float* __restrict__ dst,
                                                      long long dst_stride, int src_step) {
    partsum_block(src, nparts, C, dst, dst_stride, src_step);
}
__global__ void __launch_bounds__(256) partsum_multi_kernel(const PartsumBatch q) {
    const int e = blockIdx.z;
    if ((int)blockIdx.y >= q.B[e] || (int)blockIdx.x * 32 >= q.C[e]) return;  // uniform
    partsum_block(q.src[e], q.nparts[e], q.C[e], q.dst[e], q.dst_stride[e], 1);
}
hipError_t partsum_multi_launch(const PartsumBatch& q, hipStream_t s) {
    if (q.count < 1) return hipSuccess;
    int cm = 0, bm = 0;
    for (int i = 0; i < q.count; ++i) { if (q.C[i] > cm) cm = q.C[i]; if (q.B[i] > bm) bm = q.B[i]; }
    hipLaunchKernelGGL(partsum_multi_kernel, dim3((cm + 31) / 32, bm, q.count), dim3(256), 0, s, q);
    return hipGetLastError();
}
hipError_t partsum_launch(const float* src, int B, int nparts, int C, float* dst, long long dst_stride, hipStream_t s,
                          int src_step) {
    hipLaunchKernelGGL(partsum_kernel, dim3((C + 31) / 32, B), dim3(256), 0, s, src, nparts, C, dst, dst_stride, src_step);
    return hipGetLastError();
}

// =====================================================================================================
// GroupNorm backward, step 3 (elementwise):
//   MODE 0:  du = (ca*g + cb*SiLU(u) + cc) * SiLU'(u)                 + per-(sample, part, channel) sums of du
//   MODE 1:  dx = gy + ca*(g*SiLU'(scale*x+shift)) + cb*x + cc [+ extra]          (x = u)
//            + (nstats != null) the first statistics pass of the block that reads dx as ITS dy: P = sum dx, Q = sum dx * SiLU(nu),
//              nu = that block's saved u2 -- same partition, same per-thread order of additions and the same rounded dx values as
//              gn_bwd_stats_kernel<T, 0> over (dx, nu), and the same order of reduction, so the slabs are bit-identical to that pass
//              and it need not run
// =====================================================================================================
template <typename T, int MODE>
__global__ void __launch_bounds__(256) gn_bwd_apply_kernel(const T* __restrict__ g, const T* __restrict__ u,
                                                           const T* __restrict__ gy, const T* __restrict__ extra,
                                                           const float* __restrict__ coef, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, T* __restrict__ out,
                                                           float* __restrict__ sums, int HW, int C, int iters,
                                                           const T* __restrict__ nu, float* __restrict__ nstats, int nt) {
    constexpr int EPB = Piece<T>::N;
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int tid = threadIdx.x, bd = blockDim.x;
    const int CPP = C / EPB, c = tid % CPP, b = blockIdx.y, part = blockIdx.x;
    const long long pieces = (long long)HW * CPP;
    float ca[EPB], cb[EPB], cc[EPB], sc[EPB], sh[EPB], acc[EPB];
    float nP[MODE == 1 ? EPB : 1], nQ[MODE == 1 ? EPB : 1];
    const bool chain = MODE == 1 && nstats != nullptr;  // uniform
    if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < EPB; ++j) nP[j] = nQ[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < EPB; ++j) {
        const int ch = c * EPB + j;
        ca[j] = coef[((size_t)b * 3 + 0) * C + ch];
        cb[j] = coef[((size_t)b * 3 + 1) * C + ch];
        cc[j] = coef[((size_t)b * 3 + 2) * C + ch];
        sc[j] = MODE == 1 ? scale[(size_t)b * C + ch] : 1.f;
        sh[j] = MODE == 1 ? shift[(size_t)b * C + ch] : 0.f;
        acc[j] = 0.f;
    }
    // NIT iterations' loads are issued together, unconditionally (out-of-range slots re-read piece 0 and are dropped; an
    // absent `extra` reads g in its place): one load round trip per NIT iterations instead of one per iteration
    constexpr int NIT = MODE == 0 ? 4 : 2;
    const long long pc0 = (long long)part * iters * bd + tid;
    const size_t sbase = (size_t)b * HW * C;
    const T* const pex = (MODE == 1 && extra) ? extra : g;
    for (int it0 = 0; it0 < iters; it0 += NIT) {
        uint4 vg[NIT], vu[NIT], vy[MODE == 1 ? NIT : 1], ve[MODE == 1 ? NIT : 1], vn[MODE == 1 ? NIT : 1];
        size_t e[NIT];
        bool ok[NIT];
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const long long pc = pc0 + (long long)(it0 + k) * bd;
            ok[k] = it0 + k < iters && pc < pieces;
            e[k] = sbase + (size_t)(ok[k] ? pc : 0) * EPB;
            if (nt) {  // (uniform) streamed once: keep the lines out of the caches' replacement order
                vg[k] = nt_load16(g + e[k]);
                vu[k] = nt_load16(u + e[k]);
            } else {
                vg[k] = *(const uint4*)(g + e[k]);
                vu[k] = *(const uint4*)(u + e[k]);
            }
            if (MODE == 1) {
                vy[k] = nt ? nt_load16(gy + e[k]) : *(const uint4*)(gy + e[k]);
                ve[k] = nt ? nt_load16(pex + e[k]) : *(const uint4*)(pex + e[k]);
                if (chain) vn[k] = nt ? nt_load16(nu + e[k]) : *(const uint4*)(nu + e[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            if (!ok[k]) continue;
            float fg[EPB], fu[EPB], fo[EPB];
            Piece<T>::unpack(vg[k], fg);
            Piece<T>::unpack(vu[k], fu);
            if (MODE == 0) {
#pragma unroll
                for (int j = 0; j < EPB; ++j) {
                    const float sg = sigmoid_f(fu[j]);
                    const float ds = fmaf(ca[j], fg[j], fmaf(cb[j], fu[j] * sg, cc[j]));
                    fo[j] = ds * (sg * fmaf(fu[j], 1.0f - sg, 1.0f));
                }
            } else {
                float fy[EPB], fe[EPB];
                Piece<T>::unpack(vy[k], fy);
                Piece<T>::unpack(ve[k], fe);
#pragma unroll
                for (int j = 0; j < EPB; ++j) {
                    const float gp = fg[j] * dsilu_f(fmaf(fu[j], sc[j], sh[j]));
                    fo[j] = fy[j] + fmaf(ca[j], gp, fmaf(cb[j], fu[j], cc[j]));
                    if (extra) fo[j] += fe[j];
                }
            }
            const uint4 pv = Piece<T>::pack(fo);
            if (nt) nt_store16(out + e[k], pv);
            else *(uint4*)(out + e[k]) = pv;
            if (MODE == 1 && chain) {
                float fn[EPB];
                Piece<T>::unpack(pv, fo);  // the values as stored: what the separate pass would read
                Piece<T>::unpack(vn[k], fn);
#pragma unroll
                for (int j = 0; j < EPB; ++j) {
                    nP[j] += fo[j];
                    nQ[j] = fmaf(fo[j], silu_f(fn[j]), nQ[j]);
                }
            }
            if (MODE == 0) {
                Piece<T>::unpack(pv, fo);  // sums of the values as stored (what the weight-gradient kernel will read)
#pragma unroll
                for (int j = 0; j < EPB; ++j) acc[j] += fo[j];
            }
        }
    }
    if (MODE == 0 && sums) slab_reduce<EPB, 1>(red, acc, nullptr, C, bd, sums);
    if (MODE == 1 && chain) slab_reduce<EPB, 2>(red, nP, nQ, C, bd, nstats);
}
hipError_t gn_bwd_apply_launch(int dtype, int mode, const void* g, const void* u, const void* gy, const void* extra,
                               const float* coef, const float* scale, const float* shift, void* out, float* sums, int B,
                               int HW, int C, hipStream_t s, const void* nu, float* nstats) {
    const ElemGeom eg = elem_geom(dtype, B, HW, C);
    if (!eg.ok || (nstats && (mode != 1 || !nu))) return hipErrorInvalidValue;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        auto k = mode ? gn_bwd_apply_kernel<T, 1> : gn_bwd_apply_kernel<T, 0>;
        hipLaunchKernelGGL(k, eg.grid, dim3(eg.bd), nstats ? eg.lds2 : eg.lds1, s, (const T*)g, (const T*)u, (const T*)gy, (const T*)extra, coef,
                           scale, shift, (T*)out, sums, HW, C, eg.iters, (const T*)nu, nstats, eg.nt);
    });
    return hipGetLastError();
}

}  // namespace ddimx
