/* libddimx -- feature header: restoration (replacement-only inpainting) requests in the continuous-batching pool; the update
 * kernel of ddim_audio_amd.RestorePool.
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The function lives in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by it.  Its prefix is rpx_, and this file lies in a directory of its own below
 * include/features/: the binding (ddim_audio_amd/_lib.py) parses every include/features/<dir>/<file>.h into the table
 * FEATURE_DIRS["<dir>/<file>"] and binds its functions by the same rule on first use.  A new feature adds a directory.
 *
 * The pool's tables (ddimx.h, ddimx_pool_*) stay as they are: the arena [n_slots][max_steps][DDIMX_POOL_STRIDE] fp32 with rows
 * (t, s1, s2, s3, c2, c1, w1, w2) and the slot table [n_slots][DDIMX_POOL_SLOT_WORDS] int32 (pos, len, seed_lo, seed_hi, sample,
 * draw_base, flags, 0).  Word 6, reserved and zero for ddimx_pool_*, is a flags word here: RPX_KNOWN says that the slot restores --
 * it has a known clip y and a mask m, and every row of it has a companion row (cx, w0) in a second arena `known`
 * [n_slots][max_steps][RPX_KNOWN_STRIDE] fp32 (columns 9 and 10 of schedule.inpaint_solver_coefficients).  ddimx_pool_begin and
 * ddimx_pool_end read words 0-1 and the first arena alone and frame the forward unchanged.
 *
 * rpx_pool_update, for every active slot (0 <= pos < len <= max_steps), on row pos, with m1 = x0[b] and m2 = hist[b] on entry,
 * per element, each operation rounded once and in this order:
 *     m0 = (x - s1 eps) / s2,  u = s3 m0 + c2 eps           (ddimx_ddim_update's operations and rounding)
 *     u  = fma(w1, m0 - m1, u)      if w1 != 0
 *     u  = fma(w2, m1 - m2, u)      if w2 != 0
 *     u  = fma(z, c1, u)            if c1 != 0
 *   and, for a slot with RPX_KNOWN only,
 *     kv = w0 y                     then kv = fma(cx, x, kv) if cx != 0
 *     kv = fma(z, c1, kv)           if c1 != 0
 *     u  = kv if m == 1, u if m == 0, else fma(m, kv, (1 - m) u)
 *     xt <- u, x0 <- m0, hist <- m1
 * z is the normal ddimx_noise_fill writes for (seed = seed_hi << 32 | seed_lo, sample, draw = draw_base + pos, tag 0) at that
 * element, drawn inside the kernel.  A slot without RPX_KNOWN gets ddimx_pool_update's bits in xt, x0 and hist; a slot with it
 * gets, in xt and in the prediction, the bits of ddimxi_multistep_update(flags = DDIMXI_REPLACE) on the row
 * (t, s1, s2, s3, c2, c1, ., ., 0, cx, w0, w1, w2) with the same noise identity.  A final row (cx = 0, w0 = 1) gives y's bits
 * where m == 1.  Nothing of an idle slot is read or written; y and mask of a slot without RPX_KNOWN are not read; a buffer whose
 * term is off is not read for that term (x0 and hist are read for the history shift alone, and never enter u then).
 *
 * Validated before the launch (a refused call writes nothing): null pointers, 1 <= n_slots <= 65535, max_steps >= 1, per_sample a
 * positive multiple of 4 with at most 2^32 groups of four.
 */
#ifndef RPX_RESTORE_POOL_H
#define RPX_RESTORE_POOL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPX_KNOWN_STRIDE 2 /* floats per row of the second arena: (cx, w0) */
#define RPX_FLAGS_WORD 6   /* the word of a slot-table row that holds the flags */
#define RPX_KNOWN 1        /* flags: the slot has y and mask, and rows in the second arena */

/* xt, eps, x0, hist, y, mask: fp32 [n_slots][per_sample]; arena, known, slots: as above. */
int rpx_pool_update(float* xt, const float* eps, float* x0, float* hist, const float* y, const float* mask, const float* arena,
                    const float* known, const int* slots, int n_slots, int max_steps, long long per_sample, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RPX_RESTORE_POOL_H */
