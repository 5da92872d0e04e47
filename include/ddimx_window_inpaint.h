/* libddimx -- seventh public header: the kernels of windowed inpainting, ddim_audio_amd.windowed_inpaint_steps -- masked DDIM
 * inpainting with reconstruction guidance (ddimx_inpaint_residual / ddimx_inpaint_update) on one long canvas denoised through
 * overlapping windows of the network's own length (ddimx_window_gather / ddimx_window_update).
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is ddimxwi_: the dynamic symbols named ddimx_* are exactly
 * the declarations of ddimx.h, and these are declared here.
 *
 * The geometry and the plan are ddimx_window.h's: canvas [N][C][L][F] fp32, window batch [N W][C][T][F] fp32, window j of canvas
 * sample n = batch sample n W + j = canvas rows [j H, j H + T), L = T + (W - 1) H, F a positive multiple of 4, N W <= 65535,
 * K = ceil(T / H) <= DDIMX_WINDOW_MAX_COVER; per canvas row l the first covering window jfirst[l], the number of covering windows
 * cnt[l] (int32 [L] each) and the normalised weights wt[k][l] (fp32 [K][L], nullable for K = 1 only).  The coefficient rows are
 * ddimx_inpaint_update's: DDIMX_INPAINT_STRIDE fp32 (t, s1, s2, s3, c2, c1, k1, k2, zeta), the row chosen by the device int32
 * `step` when the launch RUNS.  x, y, mask, noise, x0 and beps are canvas-shaped; eps of ddimxwi_residual, seed and d_win are
 * window-batch-shaped.
 */
#ifndef DDIMX_WINDOW_INPAINT_H
#define DDIMX_WINDOW_INPAINT_H

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of `partials` for N canvas samples of per_sample = C L F elements: N times the blocks per canvas sample of both kernels,
 * ddimx_inpaint_partials_floats' count; -1 for N outside 1..65535 or per_sample not a positive multiple of 4. */
long long ddimxwi_partials_floats(int N, long long per_sample);

/* The first pass of a guided step, over the canvas: beps <- the blend of the window batch's eps (ddimxw_blend's arithmetic),
 * x0 <- (x - s1 beps) / s2, r = mask (x0 - y), partials[n][blk] <- the block's sum of r^2 -- the norm L_n belongs to the CANVAS
 * sample --, and the seed of the window batch's data-only backward, the adjoint of the blend: with s = k1 mask r at canvas row l,
 *     seed of window jfirst[l] + k at its row l - (jfirst[l] + k) H  <-  wt[k][l] s     (k < cnt[l]; s itself where cnt[l] == 1).
 * Every element of seed is written exactly once (a window row is one canvas row, and that row is covered by that window): nothing
 * has to be zeroed first.  Validated before the launch: nulls, the geometry above, K. */
int ddimxwi_residual(const float* x, const float* eps, const float* y, const float* mask, float* x0, float* beps, float* seed,
                     float* partials, const int* jfirst, const int* cnt, const float* wt, const float* coef, const int* step, int N,
                     int W, int C, int L, int T, int H, int F, void* stream);

/* ddimx_inpaint_update on the canvas, in place on x; flags are DDIMX_INPAINT_REPLACE | DDIMX_INPAINT_GUIDED (ddimx.h).
 *     not guided: eps is the window batch's and is blended here; x0 <- (x - s1 e) / s2 is written.  With no flag and a zero mask
 *                 the step is ddimx_window_update; in general it is ddimxw_blend followed by ddimx_inpaint_update, bit for bit.
 *     guided:     eps is the canvas-shaped beps and x0 is read, both ddimxwi_residual's; the network term of the gradient at
 *                 canvas row l is the sum of d_win (the data-only backward of seed) over the covering windows in ascending
 *                 window order, ((d[j0] + d[j1]) + d[j2]) ..., every sum rounded once, d[j0] itself where cnt[l] == 1;
 *                 u -= zeta / sqrt(L_n) (k2 mask r + that sum), L_n the canvas sample's partials added in a fixed order,
 *                 the factor formed in double and rounded once; skipped where L_n = 0 or zeta = 0.
 * noise (canvas-shaped) may be null; y and mask may be null only with no flag, d_win and partials only when not guided.  Validated before the
 * launch: nulls, the geometry above, K, unknown flag bits. */
int ddimxwi_update(float* x, const float* eps, const float* noise, float* x0, const float* y, const float* mask, const float* d_win,
                   const float* partials, const int* jfirst, const int* cnt, const float* wt, const float* coef, const int* step, int N,
                   int W, int C, int L, int T, int H, int F, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_WINDOW_INPAINT_H */
