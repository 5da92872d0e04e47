/* libddimx -- eighth public header: the multistep update with the UniC corrector of UniPC (Zhao et al. 2023) folded in, the
 * update of ddim_audio_amd.dpm_solver_steps(corrector=True).
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The function lives in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by it.  Its prefix is ddimxu_, for the reason ddimxs_ exists (ddimx_sde.h).
 */
#ifndef DDIMX_UNIC_H
#define DDIMX_UNIC_H

#ifdef __cplusplus
extern "C" {
#endif

/* fp32 values per row of the corrector's coefficient table (schedule.unic_coefficients): t, s1, s2, s3, c2, c1, w1', w2', w3 */
#define DDIMXU_STRIDE 9

/* One step, in place on xt.  xt, eps, x0, hist and hist2 hold n fp32 each; coef holds rows of DDIMXU_STRIDE fp32; step is a device
 * int32 whose value, read when the launch RUNS, selects the row, so one captured launch serves every replay.  Predictor and
 * corrector are linear in the sample and in the x0 predictions, so "correct the sample with this step's prediction, then predict
 * from the corrected sample" is ddimx_multistep_update with other history weights and one more history term: no second sample
 * buffer and no second pass.  Per element, with m1 = x0, m2 = hist and m3 = hist2 on entry, every operation rounded once and in
 * this order (the arithmetic of ddimx_ddim_update, ddimx_multistep_update, ddimxs_multistep_update and ddimx_pool_update):
 *     m0 = (x - s1 eps) / s2
 *     u  = s3 m0 + c2 eps
 *     u  = fma(w1, m0 - m1, u)     if w1 != 0
 *     u  = fma(w2, m1 - m2, u)     if w2 != 0 and hist is given
 *     u  = fma(w3, m2 - m3, u)     if w3 != 0 and hist2 is given
 *     xt <- u, x0 <- m0, hist <- m1 (when hist is given), hist2 <- m2 (when hist2 is given)
 * A history buffer is read only if a term or a shift needs it: the first iterations find the buffers uninitialised, and their
 * contents never enter u.  A row with w3 = 0 and hist2 null gives ddimx_multistep_update's bits; c1 is not read (no noise).
 * hist and hist2 may be null, hist2 only together with hist.  Arguments are validated before the launch, and a refused call
 * writes nothing: nulls (hist and hist2 excepted), hist2 without hist, n a positive multiple of 4. */
int ddimxu_multistep_update(float* xt, const float* eps, float* x0, float* hist, float* hist2, const float* coef, const int* step,
                            long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_UNIC_H */
