// Export of include/ddimx_sde.h: the stochastic multistep update (SDE-DPM-Solver++), noise from a buffer or drawn in the kernel.
#include "host.h"
#include "../../include/ddimx_sde.h"
#include "sde_kernels.h"

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

}  // extern "C"
