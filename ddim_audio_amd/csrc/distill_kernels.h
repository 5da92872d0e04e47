// Launch wrappers of the SNR-weighted loss, the progressive-distillation target kernels and the training kernels of consistency
// distillation (distill_kernels.hip; ddim_audio_amd/losses.py, distill.py, consistency.py).  Same rules as step_kernels.h: enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "step_math.h"
#include "tail_kernels.h"

namespace ddimx {

constexpr int kDistillThreads = kSampleThreads;  // the grid of the two target kernels: (sample_blocks, B)
constexpr int kDistillStride = 12;               // floats per row of schedule.distill_coefficients (DDIMX_DISTILL_STRIDE)

// loss[b] = rn(w S_b), w = wtab[t[b]], S_b the per-sample sum ddimx_sqerr_loss forms (sqerr_part_launch's parts, summed by one
// wave); loss[B] = (sum of the weighted values in b order) / B.  A t[b] outside 0 .. n_table - 1 reads no row: w = NaN.
hipError_t sqerr_w_launch(const float* target, const float* out, const float* wtab, int n_table, const int64_t* t, float* partial,
                          float* loss, int B, long long per, hipStream_t s);
// d[b] = c (out[b] - target[b]), c = rn(w c0), c0 = sqerr_bwd_c0(g, b, B, 1) (tail_kernels.h), w as above
hipError_t sqerr_w_bwd_launch(const float* target, const float* out, const float* g, const float* wtab, int n_table, const int64_t* t,
                              float* d, int B, long long per, hipStream_t s);
// rows: [B][kDistillStride], sample b's row (t, s1, s2, s3, c2, t', s1', s2', omega, cz, cx, 0).
// m0[b] = ddim_x0(z, eps0, s1, s2), zmid[b] = ddim_next(m0, eps0, s3, c2) (step_math.h).  hipErrorInvalidValue for B outside
// 1..65535 or per_sample not a positive multiple of 4.
hipError_t distill_half_launch(const float* z, const float* eps0, const float* rows, float* zmid, float* m0, int B, long long per_sample,
                               hipStream_t s);
// m1 = ddim_x0(zmid, eps1, s1', s2'); x = fma(omega, m0 - m1, m1); target = fma(x, cx, z cz); x0_target (nullable) = x.
// target may be m0.
hipError_t distill_target_launch(const float* z, const float* zmid, const float* eps1, const float* m0, const float* rows, float* target,
                                 float* x0_target, int B, long long per_sample, hipStream_t s);

// ---- consistency distillation (include/cmx_consistency.h has the arithmetic).  tab: [n_table][2] rows (p, q); t: int64 [B], read
// when the launch runs; a t[b] outside the table gives NaN.  hipErrorInvalidValue for B outside 1..65535, per_sample not a positive
// multiple of 4 or n_table < 1.
// f = consistency_f(x, out, p, q) (step_math.h); f may be out
hipError_t cm_out_launch(const float* x, const float* out, const float* tab, int n_table, const int64_t* t, float* f, int B,
                         long long per_sample, hipStream_t s);
// loss[b] = the distance of S_b = sum (y - f)^2 (sqerr_part_body / sqerr_final_body, tail_kernels.h), loss[B] their mean;
// partial: [B][kSqParts]
hipError_t cm_loss_launch(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t,
                          float huber_c, float* partial, float* loss, int B, long long per_sample, hipStream_t s);
// d = rn(q k_b) (f - y); k_b = sqerr_bwd_c0(g, b, B, 1), divided by 2 (loss[b] + huber_c) when huber_c > 0
hipError_t cm_loss_bwd_launch(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t,
                              float huber_c, const float* loss, const float* g, float* d, int B, long long per_sample, hipStream_t s);

}  // namespace ddimx
