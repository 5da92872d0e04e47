// Exports of include/ddimx_inpaint_solver.h: the multistep inpainting step -- the residual pass on its wider row and the update.
#include "host.h"
#include "../../include/ddimx_inpaint_solver.h"
#include "inpaint_solver_kernels.h"

static_assert(DDIMXI_STRIDE == ddimx::kInpaintSolverStride, "ddimx_inpaint_solver.h and inpaint_kernels.h disagree");
static_assert(DDIMXI_REPLACE == DDIMX_INPAINT_REPLACE && DDIMXI_GUIDED == DDIMX_INPAINT_GUIDED, "dispatch_inpaint_flags reads ddimx.h's flag bits");

extern "C" {

int ddimxi_residual(const float* xt, const float* eps, const float* y, const float* mask, float* x0, float* seed, float* partials,
                    const float* coef, const int* step, int B, long long per_sample, void* stream) {
    if (!xt || !eps || !y || !mask || !x0 || !seed || !partials || !coef || !step) return fail("ddimxi_residual: null argument");
    CHK(sample_shape("ddimxi_residual", B, per_sample));
    HIPCHK(inpaint_residual_launch(xt, eps, y, mask, x0, seed, partials, coef, step, B, per_sample, (hipStream_t)stream,
                                   kInpaintSolverStride));
    return 0;
}

int ddimxi_multistep_update(float* xt, const float* eps, const float* noise, float* x0, float* h1, float* h2, const float* y,
                            const float* mask, const float* d_x, const float* partials, const float* coef, const int* step, int B,
                            long long per_sample, int flags, unsigned long long seed, unsigned first_sample, unsigned draw_base,
                            void* stream) {
    if (!xt || !eps || !x0 || !h1 || !coef || !step) return fail("ddimxi_multistep_update: null argument");
    if (flags & ~(DDIMXI_REPLACE | DDIMXI_GUIDED)) return fail("ddimxi_multistep_update: unknown flags %d", flags);
    if ((flags & (DDIMXI_REPLACE | DDIMXI_GUIDED)) && (!y || !mask)) return fail("ddimxi_multistep_update: replace / guided need y and mask");
    if ((flags & DDIMXI_GUIDED) && (!d_x || !partials)) return fail("ddimxi_multistep_update: guided needs d_x and partials");
    CHK(sample_shape("ddimxi_multistep_update", B, per_sample));
    CHK(noise_range("ddimxi_multistep_update", B, per_sample, first_sample));
    HIPCHK(inpaint_multistep_update_launch(xt, eps, noise, x0, h1, h2, y, mask, d_x, partials, coef, step, B, per_sample, flags, seed,
                                           first_sample, draw_base, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
