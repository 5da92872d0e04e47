/* libddimx -- third public header: static clipping and dynamic thresholding of the x0 prediction in the DDIM and DPM-Solver++
 * samplers (Saharia et al. 2022, section 2.3; Lu et al. 2022, section 4).
 *
 * The conventions are ddimx.h's: every function returns 0 on success, non-zero on error with the message in
 * ddimx_last_error(); pointers are DEVICE pointers owned by the caller; every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and can be captured into a hipGraph.  The functions live in the same libddimx.so;
 * DDIMX_ABI_VERSION (ddimx.h) is not changed by them.  Their prefix is ddimxq_: the dynamic symbols named ddimx_* are exactly
 * the declarations of ddimx.h (tests/test_host_cpu.py holds the library to that), and these are declared here.
 */
#ifndef DDIMX_THRESHOLD_H
#define DDIMX_THRESHOLD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Both functions sit between the network's eps (after ddimx_v_to_eps, if it predicts v) and the unchanged update kernels, and
 * work per sample.  x, eps, eps_in and eps_out are fp32 [B][per_sample]; tab is fp32 [n_table][2], row t = (s1, s2) =
 * (sqrt(1 - a_t), sqrt(a_t)) (schedule.v_table); t is the int64 [B] timestep tensor the network was given, read when the launch
 * RUNS, so one captured launch serves every replay and the pool's per-slot timesteps.  x0 = (x - s1 eps) / s2 with the arithmetic
 * and rounding of ddimx_ddim_update; it is recomputed wherever it is needed and never stored.  scale is fp32 [B][2], row b =
 * (s, r): the clipped prediction is c = rn(min(max(x0, -s), s) r).
 *
 *   ddimxq_quantile_work_bytes: the size of `work` for a batch of B (16 KiB per sample); -1 for B outside 1..65535.
 *     `work` is 16-byte aligned and holds ZEROS before the first call: the caller clears it once, when it allocates it.  Every call
 *     leaves it all zeros again (its last launch clears what the call counted), so the same buffer serves any number of
 *     consecutive calls and graph replays with no host work in between.
 *   ddimxq_x0_quantile: scale[b] = (s, r), s = min(max(q, floor), ceil), r = rn(floor / s), where q is the element of rank `rank`
 *     (0-based, ascending; the host computes it: schedule.threshold_rank) of the per_sample values |x0| of sample b -- the exact
 *     order statistic, the "lower" quantile, by a radix select on the bit patterns (NaN and inf sort above every finite value; a
 *     NaN q gives s = floor).  Integer atomics only: bit-reproducible, and a sample's row does not depend on B.  Four launches.
 *     ceil may be +inf.
 *   ddimxq_threshold_eps: eps_out = eps_in where c has the bits of x0 (a threshold that does not engage changes nothing, bit for
 *     bit), else rn(fma(c, -s2, x) / s1), the eps whose x0 prediction is c.  One launch.  eps_out may be eps_in.  A static clip
 *     is this call alone with rows (limit, 1) written by the host.
 * A t[b] outside 0 .. n_table - 1 reads no row and leaves scale[b], respectively eps_out[b], untouched.
 * Arguments are validated before any launch: nulls, 1 <= B <= 65535, per_sample a positive multiple of 4 below 2^31,
 * 0 <= rank < per_sample, n_table >= 1, 0 < floor <= ceil. */
long long ddimxq_quantile_work_bytes(int B);
int ddimxq_x0_quantile(const float* x, const float* eps, const float* tab, int n_table, const int64_t* t, long long rank, float floor,
                       float ceil, void* work, float* scale, int B, long long per_sample, void* stream);
int ddimxq_threshold_eps(const float* x, const float* eps_in, float* eps_out, const float* scale, const float* tab, int n_table,
                         const int64_t* t, int B, long long per_sample, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_THRESHOLD_H */
