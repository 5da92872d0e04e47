/* libddimx -- second public header: SNR loss weighting and the target of progressive distillation.
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is ddimxd_: the dynamic symbols named ddimx_* are exactly
 * the declarations of ddimx.h (tests/test_host_cpu.py holds the library to that), and these are declared here.
 */
#ifndef DDIMX_DISTILL_H
#define DDIMX_DISTILL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* floats per row of schedule.distill_coefficients:
 * (t, s1, s2, s3, c2, t', s1', s2', omega, cz, cx, 0) */
#define DDIMX_DISTILL_STRIDE 12

/* ---- SNR loss weighting (ddim_audio_amd/losses.py; min-SNR: Hang et al. 2023, truncated SNR: Salimans & Ho 2022) -------------
 * The squared-error loss of ddimx_sqerr_loss with one weight per sample, w = wtab[t[b]]: wtab is fp32 [n_table]
 * (schedule.loss_weight_table) and t the int64 [B] timestep tensor the network was given, read when the launch RUNS, so a
 * captured launch serves every replay of a graphed training step.
 *   ddimxd_sqerr_loss_w: loss[b] = rn(w S_b), S_b the per-sample sum of ddimx_sqerr_loss bit for bit (the same first launch);
 *     loss[B] = the sum of the weighted values in b order, divided by B.  partial: [B*64] scratch.
 *   ddimxd_sqerr_loss_w_bwd_mean: d_out[b] = c (out[b] - target[b]), c = rn(w c0), c0 = 2 (g[b] + g[B] / B) the scalar of
 *     ddimx_sqerr_loss_bwd_mean; g: [B + 1], the upstream gradient of the loss vector.
 * A t[b] outside 0 .. n_table - 1 reads no row and weighs the sample with NaN: NaN in loss[b] and loss[B], a NaN row d_out[b].
 * With a table of ones both are bit-identical to the unweighted pair.  Fixed-order reductions, no float atomics.  Arguments are
 * validated before the launch: nulls, 1 <= B <= 65535, per_sample positive, n_table >= 1. */
int ddimxd_sqerr_loss_w(const float* target, const float* out, const float* wtab, int n_table, const int64_t* t, float* partial,
                        float* loss, int B, long long per_sample, void* stream);
int ddimxd_sqerr_loss_w_bwd_mean(const float* target, const float* out, const float* g, const float* wtab, int n_table,
                                 const int64_t* t, float* d_out, int B, long long per_sample, void* stream);

/* ---- progressive distillation (ddim_audio_amd/distill.py; Salimans & Ho 2022) ----------------------------------------------
 * A student does in one DDIM step t -> t'' what its teacher does in the two steps t -> t' -> t'' (eta = 0).  rows is fp32
 * [B][DDIMX_DISTILL_STRIDE]: sample b's row of schedule.distill_coefficients, GATHERED by the caller (the step index of a sample
 * is known on the host, which builds t and t' from the same rows; no index reaches the kernels).  z, eps0, eps1, zmid, m0, target
 * and x0_target are fp32 [B][per_sample]; eps0 / eps1 are the teacher's eps at (z, t) / (zmid, t') (a v teacher's outputs go
 * through ddimx_v_to_eps first).
 *   ddimxd_distill_half: m0 = (z - s1 eps0) / s2 and zmid = s3 m0 + c2 eps0 with the arithmetic and rounding of
 *     ddimx_ddim_update (its x0 and x_{t-1} bit for bit), the row chosen per sample.
 *   ddimxd_distill_target: m1 = (zmid - s1' eps1) / s2', x = fma(omega, m0 - m1, m1), target = fma(x, cx, rn(z cz)); x0_target,
 *     if not null, receives x.  x is the x0 whose single step from z lands on the teacher's z'' (never materialised); (cz, cx)
 *     turn it into the student's training target: (1/s1, -s2/s1) for an eps student, (s2/s1, -1/s1) for a v student.
 * Both leave z alone.  target may be m0 (in place); x0_target aliases nothing.  A sample's result does not depend on B.
 * Arguments are validated before the launch: nulls (x0_target alone may be null), 1 <= B <= 65535, per_sample a positive
 * multiple of 4. */
int ddimxd_distill_half(const float* z, const float* eps0, const float* rows, float* zmid, float* m0, int B, long long per_sample,
                        void* stream);
int ddimxd_distill_target(const float* z, const float* zmid, const float* eps1, const float* m0, const float* rows, float* target,
                          float* x0_target, int B, long long per_sample, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_DISTILL_H */
