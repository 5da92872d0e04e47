/* libddimx -- fifth public header: SDE-DPM-Solver++ on one Brownian path (ddim_audio_amd.BrownianStream): the noise of a step is
 * the normalised increment of one Brownian motion between the two levels of the step, so runs of different step counts from the
 * same seed follow the same path.
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is ddimxb_, for the reason ddimxs_ exists (ddimx_sde.h).
 *
 * The path.  With T the length of the alphas-cumprod table, D = max(1, ceil(log2 T)) and N = 2^D, the points t = 0 .. N carry the
 * clock u[t] = (a_t / (1 - a_t))^tau (t < T) and u[t] = 0 (T <= t <= N), decreasing in t, and P(t) = W(u[t]) for one standard
 * Brownian motion W per element.  P(N) = 0, P(0) = sqrt(u[0]) xi_0, and every other point is the midpoint m = (a + b) / 2 of one
 * node [a, b] of the binary tree over [0, N] (heap numbering: the root is node 1, the children of n are 2n: [a, m] and 2n + 1:
 * [m, b]), a Brownian bridge with an unequal split:
 *     P(m) = P(b) + rho_n (P(a) - P(b)) + s_n xi_n,   rho_n = (u_m - u_b) / (u_a - u_b),   s_n = sqrt((u_a - u_m)(u_m - u_b) / (u_a - u_b))
 * xi_n for element 4q + j of global sample s is normal j of the seeded stream (ddimx_noise_fill, DDIMX_NOISE_NORMALS) for the
 * counter (q, s, n, tag 2) under the key of seed.  P(t) is reached by the one descent from the root that stops where m = t.
 * In fp32, every operation rounded once:  d = P(a) - P(b);  v = fma(rho, d, P(b));  P(m) = fma(s, xi, v);  P(0) = sqrt(u0) * xi_0;
 * the noise of the step i -> j is z = (P(j) - P(i)) * g, g = 1 / sqrt(u_j - u_i).
 *
 * A plan row (DDIMXB_PLAN_STRIDE 32-bit words, written by the host: schedule.brownian_plan) holds the two descents of one step:
 *     word 0  the number of leading records the two descents share (they are evaluated once)
 *     word 1  the number of records of the descent to i, the level left        (0 .. DDIMXB_MAX_DEPTH + 1)
 *     word 2  the number of records of the descent to j, the level reached     (0 .. DDIMXB_MAX_DEPTH + 1)
 *     word 3  g, fp32
 *     words 4 + 4r ..                               record r of the descent to i
 *     words 4 + 4 (DDIMXB_MAX_DEPTH + 1) + 4r ..    record r of the descent to j
 * A record is (node id: int32, rho: fp32, s: fp32, enter: int32).  enter says how the record's interval follows from the one
 * before: DDIMXB_ENTER_ANCHOR (node 0: P(a) = P(m) = s xi, P(b) = 0), DDIMXB_ENTER_ROOT (node 1: [0, N] as the anchor left it),
 * DDIMXB_ENTER_LEFT (b <- the last midpoint) or DDIMXB_ENTER_RIGHT (a <- the last midpoint).  The value of a descent is its last
 * record's P(m).  A row whose word 2 is 0 is empty: no noise.
 */
#ifndef DDIMX_BROWNIAN_H
#define DDIMX_BROWNIAN_H

#define DDIMXB_MAX_DEPTH 16     /* D at most: tables of up to 65536 timesteps */
#define DDIMXB_PLAN_STRIDE 140  /* 4 + 2 * (DDIMXB_MAX_DEPTH + 1) * 4 */
#define DDIMXB_NOISE_TAG 2      /* the purpose word of the path's counters (0: a step's noise, 1: the initial x_T) */
#define DDIMXB_ENTER_ANCHOR 0
#define DDIMXB_ENTER_ROOT 1
#define DDIMXB_ENTER_LEFT 2
#define DDIMXB_ENTER_RIGHT 3
#define DDIMXB_PATH 0       /* ddimxb_path_fill: out <- the value of the row's descent to j */
#define DDIMXB_INCREMENT 1  /* ddimxb_path_fill: out <- z of the row */

#ifdef __cplusplus
extern "C" {
#endif

/* ddimxs_multistep_update (ddimx_sde.h) with the noise of the step taken from the path: xt, eps, x0 and hist are fp32
 * [B][per_sample]; coef holds rows of 8 fp32 (schedule.dpm_coefficients(tau=)), plan rows of DDIMXB_PLAN_STRIDE words
 * (schedule.brownian_plan); step is a device int32 whose value, read when the launch RUNS, selects the row of both.  The update is
 * that export's, operation for operation, with z the row's increment for (group of four elements, first_sample + b) under the key
 * of seed, evaluated inside the kernel: no noise buffer, no fill launch.  The noise term is added iff the row's c1 != 0; a row with
 * c1 = 0 (and an empty plan row) gives ddimxs_multistep_update's bits.  hist may be null.
 * Arguments are validated before the launch as ddimxs_multistep_update validates them; plan must not be null. */
int ddimxb_multistep_update(float* xt, const float* eps, float* x0, float* hist, const float* coef, const int* plan, const int* step,
                            int B, long long per_sample, unsigned long long seed, unsigned first_sample, void* stream);

/* out [B][per_sample] fp32 <- what the update kernel evaluates for the one plan row at plan_row (DDIMXB_PLAN_STRIDE words):
 * kind DDIMXB_PATH: P of the row's descent to j; DDIMXB_INCREMENT: z.  An empty descent gives 0.  Validation as above. */
int ddimxb_path_fill(float* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample, const int* plan_row,
                     int kind, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_BROWNIAN_H */
