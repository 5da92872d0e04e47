// Launch wrappers of the GroupNorm kernels (gn_kernels.hip): enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"
#include "gn_fused.h"

namespace ddimx {

// ---- GroupNorm statistics -> folded per-(sample, channel) scale / shift ---------------------------
// stats [B][nparts][Cs][2]; channel vc of the slab is real channel vc % C.  count = elements per group.
hipError_t gn_finalize_launch(const float* stats, int nparts, int Cs, int C, double count, const float* gamma,
                              const float* beta /*nullable*/, float eps, float* scale, float* shift, int B,
                              hipStream_t s, float* mean_rstd_out /*[B][8][2], nullable*/ = nullptr);
// the same from group-format partials (gn.stats [B][gn.np][8][2])
hipError_t gn_finalize_groups_launch(const GnIn& gn, int C, float* scale, float* shift, int B, int nthreads, hipStream_t s);
int resid_threads(int dtype, int C);  // block size of resid_kernel / tensor_stats for C channels

// ---- residual pass: y = x + (h*scale + shift)  (block tail, models/diffusion.py:54-56), or y = x + h ----
// h_f32 = 1: h is fp32 (FNet output) and no affine is applied; h_f32 = 2: y = x + SiLU(h)*scale + shift (training
// forward, h = pre-activation).  stats nullable.  Elements per sample = HW*C.
// gn != null (gn->stats set): scale / shift are derived in-kernel from the group partials of h (consumer-side finalisation)
hipError_t resid_launch(int dtype, const void* x, const void* h, int h_f32, const float* scale, const float* shift,
                        void* y, float* stats, int B, int HW, int C, hipStream_t s, const GnIn* gn = nullptr, int groups = 0);
int resid_nparts(int dtype, int HW, int C);
int resid_iters(int dtype, int HW, int C);  // 16-byte pieces per thread of the element-wise passes (sample size only)
// per-channel (sum, sumsq) partials of an NHWC tensor, same partitioning as resid_nparts
hipError_t tensor_stats_launch(int dtype, const void* x, float* stats, int B, int HW, int C, hipStream_t s, int groups = 0);

// ---- GroupNorm backward around the fused convolutions (three steps; see gn_kernels.hip) -----------------
// mode 0: the norm is fed by SiLU(u) (GN1, GN2); mode 1: the norm is followed by SiLU and fed by x = u (GN0)
hipError_t gn_bwd_stats_launch(int dtype, int mode, const void* g, const void* u, const float* scale, const float* shift,
                               float* stats /*[B][nparts][C][2]*/, int B, int HW, int C, hipStream_t s);
// mr: saved (mean, rstd) [B][8][2]; coef out [B][3][C]; dgb out [B][2][C] = per-sample (dgamma, dbeta) terms
hipError_t gn_bwd_finalize_launch(const float* stats, int nparts, int C, double count, const float* gamma, const float* mr,
                                  float* coef, float* dgb, int B, hipStream_t s);
// mode 0: out = (ca*g + cb*SiLU(u) + cc)*SiLU'(u), sums [B][nparts][C] of out (nullable)
// mode 1: out = gy + ca*(g*SiLU'(scale*u+shift)) + cb*u + cc (+ extra); with nstats (and nu) also the slabs gn_bwd_stats_launch(mode 0)
//         would write for (g = out, u = nu): the first statistics pass of the block that takes `out` as its dy, bit for bit
hipError_t gn_bwd_apply_launch(int dtype, int mode, const void* g, const void* u, const void* gy, const void* extra,
                               const float* coef, const float* scale, const float* shift, void* out, float* sums, int B,
                               int HW, int C, hipStream_t s, const void* nu = nullptr, float* nstats = nullptr);
hipError_t colsum_launch(const float* src, int B, long long stride, int C, float* dst, hipStream_t s);
struct ColsumBatch {
    static constexpr int kMax = 96;
    const float* src[kMax]; float* dst[kMax]; long long stride[kMax]; int B[kMax]; int C[kMax]; int count;
};
hipError_t colsum_multi_launch(const ColsumBatch& q, hipStream_t s);
// dst[b][c] = sum_p src[((b*nparts + p)*C + c) * src_step]   (src_step = 2 reads the `sum` half of (sum, sumsq) slabs)
hipError_t partsum_launch(const float* src, int B, int nparts, int C, float* dst, long long dst_stride, hipStream_t s,
                          int src_step = 1);
// the same for many (src, dst) pairs in one launch (src_step 1): the backward defers the per-sample channel sums of its blocks
// (conv.1.bias and timestep-embedding terms: nothing on the data-gradient chain reads them) and flushes them with the batch sums
struct PartsumBatch {
    static constexpr int kMax = 32;
    const float* src[kMax]; float* dst[kMax]; long long dst_stride[kMax]; int nparts[kMax], C[kMax], B[kMax]; int count;
};
hipError_t partsum_multi_launch(const PartsumBatch& q, hipStream_t s);

}  // namespace ddimx
