/* libddimx -- feature header: exact log-likelihood along the probability-flow ODE (Song et al. 2021, section 4.3 and appendix
 * D.2) with the Skilling-Hutchinson trace estimator (Grathwohl et al. 2019); the kernels of ddim_audio_amd.log_likelihood.
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is lkx_, and this file lies in include/features/: the
 * binding (ddim_audio_amd/_lib.py) keeps every header of that directory in a table of its own, FEATURES, and binds its functions
 * by the same rule on first use.  This directory is where feature headers go.
 *
 * The ODE is du/ds = eps(alpha u, t) in u = x / alpha, s = sigma / alpha, walked on the levels of a timestep grid; the
 * divergence of eps is estimated as r . (J^T r) with a Rademacher probe r, J^T r the data-only backward of the seed r.  One
 * network evaluation is one row of the table schedule.likelihood_coefficients writes: LKX_STRIDE fp32,
 *     (t, wk, we, a_next, wd, flags, 0, 0)
 * t is an integer below 2^24, exact in fp32; flags is LKX_SAVE | LKX_COMMIT as a float.  The rounding contract of a row, with e
 * the network's eps and g the backward's output, per element, each operation rounded once and in this order:
 *     un  = fma(we, e, fma(wk, k1, u))        (wk == 0: fma(we, e, u); k1 is not read)
 *     xin = rn(a_next un)                     the next network input
 *     k1 <- e       if flags & LKX_SAVE       (else k1 is not written)
 *     u  <- un      if flags & LKX_COMMIT     (else u is not written)
 * and per sample, in double:  acc[b] += wd (sum of r g over the sample).  wd is NOT column 4 of the fp32 row: lkx_finish reads
 * it from a table of doubles, one per row, that lies beside the fp32 one (schedule.likelihood_coefficients returns both), so the
 * quadrature weights keep their 53 bits.  Column 4 holds their fp32 rounding for inspection only; no kernel reads it.
 *
 * The probe.  Element j of group q (four consecutive elements) of global sample first_sample + b is +1 when bit 31 of word j
 * of Philox4x32-10 at the counter (q, first_sample + b, probe, 3) under the key of seed is clear, else -1: the seeded stream of
 * ddimx_noise.h with the tag 3 (tags 0 to 2 are taken).  lkx_stage regenerates it; it never reads the buffer lkx_probe_fill wrote.
 *
 * Every reduction runs in a fixed order in double with no atomics of any kind; the number of blocks that walk a sample depends
 * on per_sample alone, so a sample's result does not depend on B.  Every function validates before the launch: null pointers,
 * 1 <= B <= 65535, per_sample a positive multiple of 4, at most 2^32 groups of four per sample and first_sample + B <= 2^32
 * (the two that draw the probe), blocks_per_sample >= 1 (lkx_finish).
 */
#ifndef LKX_LIKELIHOOD_H
#define LKX_LIKELIHOOD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LKX_STRIDE 8 /* floats per row of the table (schedule.likelihood_coefficients) */
#define LKX_SAVE 1   /* flags: k1 <- e */
#define LKX_COMMIT 2 /* flags: u <- un */

/* The doubles of the `partial` scratch of lkx_stage / lkx_sumsq for a batch of B: B times the blocks that walk one sample, which
 * depend on per_sample alone -- lkx_partials_doubles(1, per_sample) is lkx_finish's blocks_per_sample.  0 for a bad argument. */
long long lkx_partials_doubles(int B, long long per_sample);

/* r[b] <- the probe of global sample first_sample + b as fp32 +1 / -1.  r: fp32 [B][per_sample]. */
int lkx_probe_fill(float* r, int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned probe, void* stream);

/* The update above on row step[0] of coef (step: a device int32 read when the launch RUNS, so one captured launch serves every
 * replay).  u, k1, e, g, xin: fp32 [B][per_sample]; xin may alias nothing else.  partial: double [lkx_partials_doubles(B,
 * per_sample)], receives per block the sum of r g over the block's elements (each thread its elements in walk order, then the
 * block's fixed tree).  The probe is drawn in the kernel from (seed, first_sample + b, probe). */
int lkx_stage(float* u, float* k1, const float* e, const float* g, float* xin, double* partial, const float* coef, const int* step,
              int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned probe, void* stream);

/* acc[b] += wd[step[0]] (partial[b][0] + partial[b][1] + ... in block order), all in double.  wd: double [rows], the
 * quadrature weights of the rows of coef; acc: double [B]. */
int lkx_finish(const double* partial, double* acc, const double* wd, const int* step, int B, int blocks_per_sample, void* stream);

/* out[b] <- the sum of x[b]^2 in double (every square exact), through the same partial and finish code.  x: fp32
 * [B][per_sample]; partial as lkx_stage's; out: double [B]. */
int lkx_sumsq(const float* x, double* partial, double* out, int B, long long per_sample, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LKX_LIKELIHOOD_H */
