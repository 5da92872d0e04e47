// Exports of include/features/lkx_likelihood.h: the probe, the row-driven update of one network evaluation with its partial sums of
// r . g, the finishing sum and the per-sample sum of squares of the prior term.
#include "host.h"
#include "../../include/features/lkx_likelihood.h"
#include "likelihood_kernels.h"

static_assert(LKX_STRIDE == kLkxStride && LKX_SAVE == kLkxSave && LKX_COMMIT == kLkxCommit,
              "lkx_likelihood.h and likelihood_kernels.h disagree");

extern "C" {

long long lkx_partials_doubles(int B, long long per_sample) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return 0;
    return (long long)B * lkx_blocks(per_sample);
}

int lkx_probe_fill(float* r, int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned probe, void* stream) {
    if (!r) return fail("lkx_probe_fill: null argument");
    CHK(sample_shape("lkx_probe_fill", B, per_sample));
    CHK(noise_range("lkx_probe_fill", B, per_sample, first_sample));
    HIPCHK(lkx_probe_fill_launch(r, B, per_sample, seed, first_sample, probe, (hipStream_t)stream));
    return 0;
}

int lkx_stage(float* u, float* k1, const float* e, const float* g, float* xin, double* partial, const float* coef, const int* step,
              int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned probe, void* stream) {
    if (!u || !k1 || !e || !g || !xin || !partial || !coef || !step) return fail("lkx_stage: null argument");
    CHK(sample_shape("lkx_stage", B, per_sample));
    CHK(noise_range("lkx_stage", B, per_sample, first_sample));
    HIPCHK(lkx_stage_launch(u, k1, e, g, xin, partial, coef, step, B, per_sample, seed, first_sample, probe, (hipStream_t)stream));
    return 0;
}

int lkx_finish(const double* partial, double* acc, const double* wd, const int* step, int B, int blocks_per_sample, void* stream) {
    if (!partial || !acc || !wd || !step) return fail("lkx_finish: null argument");
    CHK(batch_range("lkx_finish", B));
    if (blocks_per_sample < 1) return fail("lkx_finish: blocks_per_sample = %d must be positive", blocks_per_sample);
    HIPCHK(lkx_finish_launch(partial, acc, wd, step, B, blocks_per_sample, (hipStream_t)stream));
    return 0;
}

int lkx_sumsq(const float* x, double* partial, double* out, int B, long long per_sample, void* stream) {
    if (!x || !partial || !out) return fail("lkx_sumsq: null argument");
    CHK(sample_shape("lkx_sumsq", B, per_sample));
    HIPCHK(lkx_sumsq_part_launch(x, partial, B, per_sample, (hipStream_t)stream));
    HIPCHK(lkx_finish_launch(partial, out, nullptr, nullptr, B, lkx_blocks(per_sample), (hipStream_t)stream));
    return 0;
}

}  // extern "C"
