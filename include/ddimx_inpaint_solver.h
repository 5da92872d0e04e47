/* libddimx -- ninth public header: the multistep (DPM-Solver++) inpainting step, the kernels of
 * ddim_audio_amd.inpaint_solver_steps: a mask, reconstruction guidance folded into the data prediction, and the known region
 * on its own exact path.
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is ddimxi_, for the reason ddimxs_ exists (ddimx_sde.h).
 */
#ifndef DDIMX_INPAINT_SOLVER_H
#define DDIMX_INPAINT_SOLVER_H

#ifdef __cplusplus
extern "C" {
#endif

/* fp32 values per row of the coefficient table (schedule.inpaint_solver_coefficients):
 *     t, s1, s2, s3, c2, c1, k1, k2, rho, cx, w0, w1, w2
 * Columns 0-5, w1 and w2 are the solver's (ddimxs_multistep_update: schedule.dpm_coefficients), k1 and k2 the inpainting
 * sampler's (ddimx_inpaint_residual), rho the guidance scale of the row's step; cx = c2 / s1 and w0 = s3 - c2 s2 / s1 are the
 * coefficients of x_t and of a constant data prediction in the exact solution of the sampler's ODE / SDE over the step.
 * ddimx_step_begin_ex(coef, DDIMXI_STRIDE, ...) fills t. */
#define DDIMXI_STRIDE 13
/* flags of ddimxi_multistep_update: the values of DDIMX_INPAINT_REPLACE / DDIMX_INPAINT_GUIDED (ddimx.h) */
#define DDIMXI_REPLACE 1
#define DDIMXI_GUIDED 2

/* ddimx_inpaint_residual on a row of DDIMXI_STRIDE floats (columns 0-8 are that function's row, rho where it has zeta): the same
 * kernel and the same bits.  Guided step, between the tape-keeping forward and ddimx_unet_bwd_ex(DDIMX_BWD_DATA_ONLY):
 *     x0 = (xt - s1 eps) / s2,  r = mask (x0 - y),  seed = k1 mask r,  partials = per-block sums of r^2
 * partials holds ddimx_inpaint_partials_floats(B, per_sample) floats. */
int ddimxi_residual(const float* xt, const float* eps, const float* y, const float* mask, float* x0, float* seed, float* partials,
                    const float* coef, const int* step, int B, long long per_sample, void* stream);

/* One step, in place on xt, over NCHW fp32 [B][per_sample] tensors.  coef holds rows of DDIMXI_STRIDE fp32; step is a device int32
 * whose value, read when the launch RUNS, selects the row, so one captured launch serves every replay.  h1 holds the guided
 * prediction of the previous iteration, h2 (nullable: orders 1-2) the one before.  Per element, with x = xt, m1 = h1 and m2 = h2
 * on entry, every operation rounded once and in this order (the scalar operations are those of ddimx_ddim_update,
 * ddimxs_multistep_update and ddimx_inpaint_update):
 *     m0 = (x - s1 eps) / s2                          without DDIMXI_GUIDED: computed, and written to x0;
 *                                                     with it: read from x0, where ddimxi_residual put it
 *     wq = fp32(rho / sqrt(L))                        DDIMXI_GUIDED: L = the sample's partials added in their fixed order, the
 *                                                     quotient in double, rounded once; 0 when L = 0 or rho = 0, and without the flag
 *     mt = fma(-wq, fma(k2, mask (mask (m0 - y)), d_x), m0)   if wq != 0, else mt = m0: the guided prediction
 *     u  = fma(eps, c2, s3 m0)                        the DDIM update
 *     u  = fma(w0, mt - m0, u)                        if wq != 0
 *     u  = fma(w1, mt - m1, u)                        if w1 != 0
 *     u  = fma(w2, m1 - m2, u)                        if w2 != 0 and h2 is given
 *     u  = fma(z, c1, u)                              if c1 != 0
 *     DDIMXI_REPLACE:
 *         kv = w0 y;  kv = fma(cx, x, kv) if cx != 0;  kv = fma(z, c1, kv) if c1 != 0
 *         u  = kv where mask = 1, u where mask = 0, else fma(mask, kv, (1 - mask) u)
 *     xt <- u;  h2 <- m1 if h2 is given and m1 was read;  h1 <- mt
 * A term that is off is not applied at all, and what it would have read is not read: m1 is read iff w1 != 0 or the w2 term is on,
 * m2 iff the w2 term is on, d_x iff wq != 0, xt iff a flag needs it (REPLACE, or no GUIDED), noise iff c1 != 0 -- the first
 * iteration finds h1 and h2 uninitialised, and their contents never enter u.  A final row (c2 = c1 = 0, s3 = 1: cx = 0, w0 = 1)
 * makes kv = y bit for bit.  With mask = 0 everywhere and rho = 0 the result is ddimxs_multistep_update's, bit for bit.
 * z is noise[i] when noise is given; with noise null and c1 != 0 the kernel draws it as ddimxs_multistep_update does: the normals
 * of the seeded stream (ddimx_noise_fill) for the counter (group of four, first_sample + b, draw_base + step[0], tag 0) under
 * `seed`.  y / mask are needed by either flag, d_x / partials by DDIMXI_GUIDED.
 * Arguments are validated before the launch, and a refused call writes nothing: nulls (noise, h2 and what the flags do not need
 * excepted), unknown flags, 1 <= B <= 65535, per_sample a positive multiple of 4 with at most 2^32 groups of four,
 * first_sample + B <= 2^32. */
int ddimxi_multistep_update(float* xt, const float* eps, const float* noise, float* x0, float* h1, float* h2, const float* y,
                            const float* mask, const float* d_x, const float* partials, const float* coef, const int* step, int B,
                            long long per_sample, int flags, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_INPAINT_SOLVER_H */
