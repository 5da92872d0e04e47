// Export of include/ddimx_sde.h: the stochastic multistep update (SDE-DPM-Solver++), noise from a buffer or drawn in the kernel.
#include "host.h"
#include "../../include/ddimx_sde.h"
#include "sde_kernels.h"

extern "C" {

int ddimxs_multistep_update(float* xt, const float* eps, const float* noise, float* x0, float* hist, const float* coef, const int* step,
                            int B, long long per_sample, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                            void* stream) {
    if (!xt || !eps || !x0 || !coef || !step) return fail("ddimxs_multistep_update: null argument");
    if (B < 1 || B > 65535) return fail("ddimxs_multistep_update: B = %d (1..65535)", B);
    if (per_sample <= 0 || per_sample % 4)
        return fail("ddimxs_multistep_update: per_sample = %lld must be a positive multiple of 4", per_sample);
    if (per_sample / 4 > (1LL << 32))
        return fail("ddimxs_multistep_update: per_sample = %lld has more than 2^32 groups of four", per_sample);
    if ((unsigned long long)first_sample + (unsigned long long)B > (1ULL << 32))
        return fail("ddimxs_multistep_update: first_sample + B = %llu exceeds 2^32", (unsigned long long)first_sample + (unsigned long long)B);
    HIPCHK(sde_multistep_update_launch(xt, eps, noise, x0, hist, coef, step, B, per_sample, seed, first_sample, draw_base,
                                       (hipStream_t)stream));
    return 0;
}

}  // extern "C"
