/* libddimx -- sixth public header: the kernels of windowed multistep sampling, ddim_audio_amd.windowed_solver_steps --
 * DPM-Solver++ orders 1-3 (deterministic, or SDE-DPM-Solver++) on one long canvas denoised through overlapping windows of the
 * network's own length.
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is ddimxw_: the dynamic symbols named ddimx_* are exactly
 * the declarations of ddimx.h (tests/test_host_cpu.py holds the library to that), and these are declared here.
 *
 * The geometry is ddimx_window_gather's / ddimx_window_update's: canvas [N][C][L][F] fp32, window batch [N W][C][T][F] fp32,
 * window j of canvas sample n = batch sample n W + j = canvas rows [j H, j H + T), L = T + (W - 1) H, F a positive multiple of 4,
 * N W <= 65535, K = ceil(T / H) <= DDIMX_WINDOW_MAX_COVER.  The plan of a canvas row l (schedule.window_plan): the first covering
 * window jfirst[l], the number of covering windows cnt[l] (1 .. K), int32 [L] each, and the normalised weights wt[k][l]
 * (k = 0 .. cnt - 1 in ascending window order; fp32 [K][L], not read and nullable for K = 1).  The blended noise prediction of
 * a canvas element is ddimx_window_update's:
 *     e = eps of window jfirst                                                                   if cnt == 1 (a select, no multiply)
 *     e = fma(wt[c-1], eps[jfirst+c-1], ... fma(wt[1], eps[jfirst+1], wt[0] * eps[jfirst]))      otherwise
 */
#ifndef DDIMX_WINDOW_H
#define DDIMX_WINDOW_H

#ifdef __cplusplus
extern "C" {
#endif

/* One multistep step of the canvas, in place on x, from the window batch's noise predictions eps: the blend above followed by
 * ddimxs_multistep_update's arithmetic (ddimx_sde.h) in one pass.  x, noise, x0 and hist are canvas-shaped; coef holds rows of 8 fp32
 * (t, s1, s2, s3, c2, c1, w1, w2) (schedule.dpm_coefficients(tau=)); step is a device int32 whose value, read when the launch RUNS,
 * selects the row, so one captured launch serves every replay.  Per element, with m1 = x0 and m2 = hist on entry:
 *     m0 = (x - s1 e) / s2
 *     u  = s3 m0 + c2 e
 *     u  = fma(w1, m0 - m1, u)     if w1 != 0
 *     u  = fma(w2, m1 - m2, u)     if w2 != 0 and hist is given
 *     u  = fma(z, c1, u)           if c1 != 0
 *     x <- u, x0 <- m0, hist <- m1 (when hist is given)
 * The result is bit for bit ddimxw_blend followed by ddimxs_multistep_update on the canvas.  x0 is read only where a history term
 * or hist needs it, hist only where w2 != 0: a first iteration may find both uninitialised.
 * z: noise[i] when noise is non-null; otherwise the normal of the seeded stream for the counter (group of four elements inside the
 * canvas sample, first_sample + n, draw_base + step[0], tag 0) under the key of seed, drawn inside the kernel: what ddimx_noise_fill
 * writes into a canvas-shaped buffer.  A canvas sample's result depends on (seed, first_sample + n) and on nothing else of the batch.
 * hist and noise may be null (and wt for K = 1).  Arguments are validated before the launch: nulls, the geometry above, K, and
 * first_sample + N <= 2^32. */
int ddimxw_multistep_update(float* x, const float* eps, const float* noise, float* x0, float* hist, const int* jfirst, const int* cnt,
                            const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F,
                            unsigned long long seed, unsigned first_sample, unsigned draw_base, void* stream);

/* beps [N][C][L][F] <- the blended noise prediction alone, with the same arithmetic: for the callers that need it whole before any
 * canvas element is updated (ddimxq_x0_quantile / ddimxq_threshold_eps on the canvas, ddimxb_multistep_update); the existing
 * update functions then run on (x, beps).  Validated like the function above. */
int ddimxw_blend(const float* eps, float* beps, const int* jfirst, const int* cnt, const float* wt, int N, int W, int C, int L, int T,
                 int H, int F, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_WINDOW_H */
