// Exports of include/ddimx_window_inpaint.h: the two element-wise passes of a windowed inpainting step; and of
// include/ddimx_window_inpaint_solver.h: the same two under the multistep update.
#include "host.h"
#include "../../include/ddimx_inpaint_solver.h"
#include "../../include/ddimx_window_inpaint.h"
#include "../../include/ddimx_window_inpaint_solver.h"
#include "window_inpaint_kernels.h"

extern "C" {

long long ddimxwi_partials_floats(int N, long long per_sample) {
    if (N < 1 || N > 65535 || per_sample <= 0 || per_sample % 4) return -1;
    return (long long)N * window_inpaint_blocks(N, per_sample);
}

int ddimxwi_residual(const float* x, const float* eps, const float* y, const float* mask, float* x0, float* beps, float* seed,
                     float* partials, const int* jfirst, const int* cnt, const float* wt, const float* coef, const int* step, int N,
                     int W, int C, int L, int T, int H, int F, void* stream) {
    if (!x || !eps || !y || !mask || !x0 || !beps || !seed || !partials || !jfirst || !cnt || !coef || !step)
        return fail("ddimxwi_residual: null argument");
    CHK(window_shape("ddimxwi_residual", N, W, C, L, T, H, F));
    CHK(window_cover("ddimxwi_residual", wt, T, H));
    HIPCHK(window_inpaint_residual_launch(x, eps, y, mask, x0, beps, seed, partials, jfirst, cnt, wt, coef, step, N, W, C, L, T, H, F,
                                          (hipStream_t)stream));
    return 0;
}

int ddimxwi_update(float* x, const float* eps, const float* noise, float* x0, const float* y, const float* mask, const float* d_win,
                   const float* partials, const int* jfirst, const int* cnt, const float* wt, const float* coef, const int* step, int N,
                   int W, int C, int L, int T, int H, int F, int flags, void* stream) {
    if (!x || !eps || !x0 || !jfirst || !cnt || !coef || !step) return fail("ddimxwi_update: null argument");
    if (flags & ~(DDIMX_INPAINT_REPLACE | DDIMX_INPAINT_GUIDED)) return fail("ddimxwi_update: unknown flags %d", flags);
    if ((flags & (DDIMX_INPAINT_REPLACE | DDIMX_INPAINT_GUIDED)) && (!y || !mask)) return fail("ddimxwi_update: replace / guided need y and mask");
    if ((flags & DDIMX_INPAINT_GUIDED) && (!d_win || !partials)) return fail("ddimxwi_update: guided needs d_win and partials");
    CHK(window_shape("ddimxwi_update", N, W, C, L, T, H, F));
    CHK(window_cover("ddimxwi_update", wt, T, H));
    HIPCHK(window_inpaint_update_launch(x, eps, noise, x0, y, mask, d_win, partials, jfirst, cnt, wt, coef, step, N, W, C, L, T, H, F, flags,
                                        (hipStream_t)stream));
    return 0;
}

// ---- include/ddimx_window_inpaint_solver.h: the same two passes under the multistep update, rows of DDIMXI_STRIDE floats

int ddimxwis_residual(const float* x, const float* eps, const float* y, const float* mask, float* x0, float* beps, float* seed,
                      float* partials, const int* jfirst, const int* cnt, const float* wt, const float* coef, const int* step, int N,
                      int W, int C, int L, int T, int H, int F, void* stream) {
    if (!x || !eps || !y || !mask || !x0 || !beps || !seed || !partials || !jfirst || !cnt || !coef || !step)
        return fail("ddimxwis_residual: null argument");
    CHK(window_shape("ddimxwis_residual", N, W, C, L, T, H, F));
    CHK(window_cover("ddimxwis_residual", wt, T, H));
    HIPCHK(window_inpaint_residual_launch(x, eps, y, mask, x0, beps, seed, partials, jfirst, cnt, wt, coef, step, N, W, C, L, T, H, F,
                                          (hipStream_t)stream, kInpaintSolverStride));
    return 0;
}

int ddimxwis_multistep_update(float* x, const float* eps, const float* noise, float* x0, float* h1, float* h2, const float* y,
                              const float* mask, const float* d_win, const float* partials, const int* jfirst, const int* cnt,
                              const float* wt, const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F,
                              int flags, unsigned long long seed, unsigned first_sample, unsigned draw_base, void* stream) {
    if (!x || !eps || !x0 || !h1 || !jfirst || !cnt || !coef || !step) return fail("ddimxwis_multistep_update: null argument");
    if (flags & ~(DDIMXI_REPLACE | DDIMXI_GUIDED)) return fail("ddimxwis_multistep_update: unknown flags %d", flags);
    if ((flags & (DDIMXI_REPLACE | DDIMXI_GUIDED)) && (!y || !mask)) return fail("ddimxwis_multistep_update: replace / guided need y and mask");
    if ((flags & DDIMXI_GUIDED) && (!d_win || !partials)) return fail("ddimxwis_multistep_update: guided needs d_win and partials");
    CHK(window_shape("ddimxwis_multistep_update", N, W, C, L, T, H, F));
    CHK(window_cover("ddimxwis_multistep_update", wt, T, H));
    CHK(noise_range("ddimxwis_multistep_update", N, (long long)C * L * F, first_sample));
    HIPCHK(window_inpaint_multistep_launch(x, eps, noise, x0, h1, h2, y, mask, d_win, partials, jfirst, cnt, wt, coef, step, N, W, C, L, T,
                                           H, F, flags, seed, first_sample, draw_base, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
