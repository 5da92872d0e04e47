// Exports of include/ddimx_window.h: the windowed multistep solver's fused blend + update and the blend alone.
#include "host.h"
#include "../../include/ddimx_window.h"
#include "window_solver_kernels.h"

extern "C" {

int ddimxw_multistep_update(float* x, const float* eps, const float* noise, float* x0, float* hist, const int* jfirst, const int* cnt,
                            const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F,
                            unsigned long long seed, unsigned first_sample, unsigned draw_base, void* stream) {
    if (!x || !eps || !x0 || !jfirst || !cnt || !coef || !step) return fail("ddimxw_multistep_update: null argument");
    CHK(window_shape("ddimxw_multistep_update", N, W, C, L, T, H, F));
    CHK(window_cover("ddimxw_multistep_update", wt, T, H));
    CHK(noise_range("ddimxw_multistep_update", N, (long long)C * L * F, first_sample));
    HIPCHK(window_multistep_update_launch(x, eps, noise, x0, hist, jfirst, cnt, wt, coef, step, N, W, C, L, T, H, F, seed, first_sample,
                                          draw_base, (hipStream_t)stream));
    return 0;
}

int ddimxw_blend(const float* eps, float* beps, const int* jfirst, const int* cnt, const float* wt, int N, int W, int C, int L, int T,
                 int H, int F, void* stream) {
    if (!eps || !beps || !jfirst || !cnt) return fail("ddimxw_blend: null argument");
    CHK(window_shape("ddimxw_blend", N, W, C, L, T, H, F));
    CHK(window_cover("ddimxw_blend", wt, T, H));
    HIPCHK(window_blend_launch(eps, beps, jfirst, cnt, wt, N, W, C, L, T, H, F, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
