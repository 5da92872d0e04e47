// Export of include/ddimx_sde.h: the stochastic multistep update (SDE-DPM-Solver++), noise from a buffer or drawn in the kernel; and
// the sampling update of include/cmx_consistency.h, which shares that draw.
#include "host.h"
#include "../../include/ddimx_sde.h"
#include "../../include/cmx_consistency.h"
#include "sde_kernels.h"

static_assert(CMX_STRIDE == kCmStride, "cmx_consistency.h and sde_kernels.h disagree");

extern "C" {

int ddimxs_multistep_update(float* xt, const float* eps, const float* noise, float* x0, float* hist, const float* coef, const int* step,
                            int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                            void* stream) {
    if (!xt || !eps || !x0 || !coef || !step) return fail("ddimxs_multistep_update: null argument");
    CHK(sample_shape("ddimxs_multistep_update", B, per_sample));
    CHK(noise_range("ddimxs_multistep_update", B, per_sample, first_sample));
    HIPCHK(sde_multistep_update_launch(xt, eps, noise, x0, hist, coef, step, B, per_sample, seed, first_sample, draw_base,
                                       (hipStream_t)stream));
    return 0;
}

int cmx_consistency_update(float* xt, const float* out, const float* noise, float* x0, const float* coef, const int* step, int B,
                           long long per_sample, unsigned long long seed, unsigned first_sample, unsigned draw_base, void* stream) {
    if (!xt || !out || !x0 || !coef || !step) return fail("cmx_consistency_update: null argument");
    CHK(sample_shape("cmx_consistency_update", B, per_sample));
    CHK(noise_range("cmx_consistency_update", B, per_sample, first_sample));
    HIPCHK(cm_update_launch(xt, out, noise, x0, coef, step, B, per_sample, seed, first_sample, draw_base, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
