/* libddimx -- feature header: consistency distillation (Song et al. 2023, Algorithm 2, in the discrete-time form of Luo et al.
 * 2023) and few-step consistency sampling; the kernels of ddim_audio_amd.consistency_step and ddim_audio_amd.consistency_steps.
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is cmx_, and this file's name does not start with ddimx: the
 * binding (ddim_audio_amd/_lib.py) keeps such a header in a table of its own, FEATURE_HEADERS, and binds its functions by the same
 * rule on first use.
 *
 * The consistency function of a network with raw output `out` is f(x, t) = p_t x + q_t out, with (p_t, q_t) row t of a table the
 * host writes (schedule.consistency_table: [n_table][2] fp32).  Per element, each operation rounded once:
 *     f = fma(q, out, rn(p x))
 * t is the int64 [B] timestep tensor the network was given, device memory read when the launch RUNS.  A t[b] outside
 * 0 .. n_table - 1 reads no row: that sample's results are NaN.  Every reduction is in a fixed order, with no float atomics; a
 * sample's result does not depend on B.  All four functions validate before the launch: null pointers, 1 <= B <= 65535,
 * per_sample a positive multiple of 4, n_table >= 1 (the first three), huber_c finite and >= 0 (the loss and its backward),
 * at most 2^32 groups of four per sample and first_sample + B <= 2^32 (the update).
 */
#ifndef CMX_CONSISTENCY_H
#define CMX_CONSISTENCY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMX_STRIDE 8 /* floats per row of the sampling table (schedule.consistency_coefficients) */

/* f[b] = fma(q, out[b], rn(p x[b])), (p, q) = tab[t[b]].  x, out, f: fp32 [B][per_sample]; f may alias out. */
int cmx_consistency_out(const float* x, const float* out, const float* tab, int n_table, const int64_t* t, float* f, int B,
                        long long per_sample, void* stream);

/* The distillation loss against the target y (fp32 [B][per_sample], a constant).  f as above, never written to memory;
 * S_b = the sum over the sample of (y - f)^2, reduced exactly as ddimx_sqerr_loss reduces (e - out)^2: d = rn(y - f),
 * fma(d, d, s) per thread over the same elements in the same order, the same two fixed trees (partial: [B][64] fp32 scratch).
 *     huber_c == 0:  loss[b] = S_b
 *     huber_c  > 0:  loss[b] = rn(S_b / rn(rn(sqrt(rn(S_b + rn(c c)))) + c))       the pseudo-Huber sqrt(S + c^2) - c,
 *                                                                                    in the form that does not cancel for S << c^2
 *     loss[B] = rn((sum of loss[b] in b order) / B)
 * loss: fp32 [B + 1].  With a table whose rows are (0, 1) and huber_c = 0 the result is ddimx_sqerr_loss(y, out)'s, bit for bit. */
int cmx_consistency_loss(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t, float huber_c,
                         float* partial, float* loss, int B, long long per_sample, void* stream);

/* Its backward w.r.t. out.  g: fp32 [B + 1], the upstream gradient of the loss vector (g[B] the batch mean's); loss: the
 * forward's vector.  Per sample, each operation rounded once and in this order:
 *     k = 2 (g[b] + g[B] / B)                                       (ddimx_sqerr_loss_bwd_mean's scalar)
 *     k = rn(k / rn(2 rn(loss[b] + c)))        if huber_c > 0       sqrt(S_b + c^2) = loss[b] + c: d loss / d S = 1 / (2 sqrt(S + c^2))
 *     cq = rn(q k)
 * and per element d_out = rn(cq rn(f - y)).  With (0, 1) rows and huber_c = 0: ddimx_sqerr_loss_bwd_mean(y, out, g)'s bits. */
int cmx_consistency_loss_bwd(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t,
                             float huber_c, const float* loss, const float* g, float* d_out, int B, long long per_sample, void* stream);

/* One sampling step of every sample, in place on xt.  xt, out, noise, x0: fp32 [B][per_sample]; out is the network's raw output at
 * (xt, t).  coef holds rows of CMX_STRIDE fp32, (t, p, q, a_next, 0, c1, 0, 0); step is a device int32 whose value, read when the
 * launch RUNS, selects the row, so one captured launch serves every replay.  Per element:
 *     m = fma(q, out, rn(p xt))                 the data prediction f(xt, t)
 *     u = rn(a_next m)
 *     u = fma(z, c1, u)        if c1 != 0       the re-noising to the next level: a_next = sqrt(abar_next), c1 = sqrt(1 - abar_next)
 *     x0 <- m, xt <- u
 * The last row of a run is (t, p, q, 1, 0, 0, 0, 0): xt = x0.  z is noise[i] when noise is non-null; otherwise the normal of
 * the seeded stream (ddimx_noise_fill, DDIMX_NOISE_NORMALS) for the counter (group of four elements, first_sample + b,
 * draw_base + step[0], tag 0) under the key of seed, drawn inside the kernel -- ddimxs_multistep_update's convention: element for
 * element what ddimx_noise_fill would have written, with no noise buffer and no fill launch.  noise may be null; seed,
 * first_sample and draw_base are not read when noise is given or the row's c1 is 0. */
int cmx_consistency_update(float* xt, const float* out, const float* noise, float* x0, const float* coef, const int* step, int B,
                           long long per_sample, unsigned long long seed, unsigned first_sample, unsigned draw_base, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMX_CONSISTENCY_H */
