/* libddimx -- fourth public header: the stochastic multistep update of SDE-DPM-Solver++ (Lu et al. 2022, appendix; known as
 * "DPM++ 2M SDE" and "3M SDE"), the update of ddim_audio_amd.dpm_solver_steps(tau > 0).
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The function lives in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by it.  Its prefix is ddimxs_: the dynamic symbols named ddimx_* are exactly
 * the declarations of ddimx.h (tests/test_host_cpu.py holds the library to that), and this one is declared here.
 */
#ifndef DDIMX_SDE_H
#define DDIMX_SDE_H

#ifdef __cplusplus
extern "C" {
#endif

/* One step of every sample, in place on xt.  xt, eps, noise, x0 and hist are fp32 [B][per_sample]; coef holds rows of 8 fp32
 * (t, s1, s2, s3, c2, c1, w1, w2) (schedule.dpm_coefficients(tau=)); step is a device int32 whose value, read when the launch RUNS,
 * selects the row, so one captured launch serves every replay.  Per element, with m1 = x0 and m2 = hist on entry, every operation
 * rounded once and in this order (the arithmetic of ddimx_ddim_update, ddimx_multistep_update and ddimx_pool_update):
 *     m0 = (x - s1 eps) / s2
 *     u  = s3 m0 + c2 eps
 *     u  = fma(w1, m0 - m1, u)     if w1 != 0
 *     u  = fma(w2, m1 - m2, u)     if w2 != 0 and hist is given
 *     u  = fma(z, c1, u)           if c1 != 0
 *     xt <- u, x0 <- m0, hist <- m1 (when hist is given)
 * A row with c1 = 0 gives ddimx_multistep_update's bits, a row with w1 = w2 = 0 ddimx_ddim_update's on the same noise.
 * z: noise[i] when noise is non-null; otherwise the normal of the seeded stream (ddimx_noise_fill, DDIMX_NOISE_NORMALS) for the
 * counter (group of four elements, first_sample + b, draw_base + step[0], tag 0) under the key of seed, drawn inside the kernel:
 * element for element what ddimx_noise_fill would have written for the same (seed, first_sample, step, draw_base), with no noise
 * buffer and no fill launch.  A sample's result then depends on (seed, first_sample + b) and on nothing else of the batch.
 * hist and noise may be null; seed, first_sample and draw_base are not read when noise is given or the row's c1 is 0.
 * Arguments are validated before the launch: nulls (hist and noise excepted), 1 <= B <= 65535, per_sample a positive multiple of 4
 * with at most 2^32 groups of four, first_sample + B <= 2^32. */
int ddimxs_multistep_update(float* xt, const float* eps, const float* noise, float* x0, float* hist, const float* coef, const int* step,
                            int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_SDE_H */
