// Export of include/ddimx_unic.h: the multistep update with the folded UniC corrector (a third history term).
#include "host.h"
#include "../../include/ddimx_unic.h"
#include "unic_kernels.h"

static_assert(DDIMXU_STRIDE == ddimx::kUnicStride, "ddimx_unic.h and unic_kernels.h disagree");

extern "C" {

int ddimxu_multistep_update(float* xt, const float* eps, float* x0, float* hist, float* hist2, const float* coef, const int* step,
                            long long n, void* stream) {
    if (!xt || !eps || !x0 || !coef || !step) return fail("ddimxu_multistep_update: null argument");
    if (hist2 && !hist) return fail("ddimxu_multistep_update: hist2 needs hist");
    if (n <= 0 || n % 4) return fail("ddimxu_multistep_update: n = %lld must be a positive multiple of 4", n);
    HIPCHK(unic_multistep_update_launch(xt, eps, x0, hist, hist2, coef, step, n, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
