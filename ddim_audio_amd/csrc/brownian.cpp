// Exports of include/ddimx_brownian.h: the stochastic multistep update with its noise taken from one Brownian path, and the fill that
// materialises the path's values and increments.
#include "host.h"
#include "../../include/ddimx_brownian.h"
#include "brownian_kernels.h"

static_assert(kBrownianMaxDepth == DDIMXB_MAX_DEPTH && kBrownianStride == DDIMXB_PLAN_STRIDE, "ddimx_brownian.h: the plan row");
static_assert(kBrownianPath == DDIMXB_PATH && kBrownianIncrement == DDIMXB_INCREMENT, "ddimx_brownian.h: the fill kinds");

extern "C" {

int ddimxb_multistep_update(float* xt, const float* eps, float* x0, float* hist, const float* coef, const int* plan, const int* step,
                            int B, long long per_sample, unsigned long long seed, unsigned first_sample, void* stream) {
    if (!xt || !eps || !x0 || !coef || !plan || !step) return fail("ddimxb_multistep_update: null argument");
    CHK(sample_shape("ddimxb_multistep_update", B, per_sample));
    CHK(noise_range("ddimxb_multistep_update", B, per_sample, first_sample));
    HIPCHK(brownian_multistep_update_launch(xt, eps, x0, hist, coef, plan, step, B, per_sample, seed, first_sample,
                                            (hipStream_t)stream));
    return 0;
}

int ddimxb_path_fill(float* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample, const int* plan_row,
                     int kind, void* stream) {
    if (!out || !plan_row) return fail("ddimxb_path_fill: null argument");
    if (kind != DDIMXB_PATH && kind != DDIMXB_INCREMENT) return fail("ddimxb_path_fill: kind = %d (DDIMXB_PATH or DDIMXB_INCREMENT)", kind);
    CHK(sample_shape("ddimxb_path_fill", B, per_sample));
    CHK(noise_range("ddimxb_path_fill", B, per_sample, first_sample));
    HIPCHK(brownian_path_fill_launch(out, B, per_sample, seed, first_sample, plan_row, kind, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
