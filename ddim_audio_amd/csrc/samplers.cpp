// Exports of the sampler-step kernel families (DDIM / DDPM, inpainting, multistep solver, inversion, noise, windows, pool)
// and of the loss, EMA and optimizer kernels.
#include "host.h"
#include "inpaint_kernels.h"
#include "solver_kernels.h"
#include "invert_kernels.h"
#include "noise_kernels.h"
#include "window_kernels.h"
#include "pool_kernels.h"
#include "vpred_kernels.h"

extern "C" {

int ddimx_step_begin(const float* coef, const int* step, int64_t* t, int B, void* stream) {
    HIPCHK(step_begin_launch(coef, step, t, B, 6, (hipStream_t)stream));
    return 0;
}
int ddimx_step_begin_ex(const float* coef, int row_stride, const int* step, int64_t* t, int B, void* stream) {
    HIPCHK(step_begin_launch(coef, step, t, B, row_stride, (hipStream_t)stream));
    return 0;
}
int ddimx_ddim_update(float* xt, const float* et, const float* noise, float* x0, const float* coef, const int* step,
                      long long n, void* stream) {
    HIPCHK(ddim_update_launch(xt, et, noise, x0, coef, step, n, (hipStream_t)stream));
    return 0;
}
int ddimx_ddpm_update(const float* x, const float* et, const float* noise, float* x0, float* xn, const float* coef,
                      const int* step, long long n, void* stream) {
    HIPCHK(ddpm_update_launch(x, et, noise, x0, xn, coef, step, n, (hipStream_t)stream));
    return 0;
}
int ddimx_step_end(int* step, void* stream) {
    HIPCHK(step_end_launch(step, (hipStream_t)stream));
    return 0;
}
long long ddimx_inpaint_partials_floats(int B, long long per_sample) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return -1;
    return (long long)B * sample_blocks(B, per_sample, kInpaintMaxBlocks);
}
int ddimx_inpaint_residual(const float* xt, const float* eps, const float* y, const float* mask, float* x0, float* seed,
                           float* partials, const float* coef, const int* step, int B, long long per_sample, void* stream) {
    if (!xt || !eps || !y || !mask || !x0 || !seed || !partials || !coef || !step) return fail("ddimx_inpaint_residual: null argument");
    CHK(sample_shape("ddimx_inpaint_residual", B, per_sample));
    HIPCHK(inpaint_residual_launch(xt, eps, y, mask, x0, seed, partials, coef, step, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_inpaint_update(float* xt, const float* eps, const float* noise, float* x0, const float* y, const float* mask,
                         const float* d_x, const float* partials, const float* coef, const int* step, int B, long long per_sample,
                         int flags, void* stream) {
    if (!xt || !eps || !x0 || !coef || !step) return fail("ddimx_inpaint_update: null argument");
    if (flags & ~(DDIMX_INPAINT_REPLACE | DDIMX_INPAINT_GUIDED)) return fail("ddimx_inpaint_update: unknown flags %d", flags);
    if ((flags & (DDIMX_INPAINT_REPLACE | DDIMX_INPAINT_GUIDED)) && (!y || !mask))
        return fail("ddimx_inpaint_update: replace / guided need y and mask");
    if ((flags & DDIMX_INPAINT_GUIDED) && (!d_x || !partials)) return fail("ddimx_inpaint_update: guided needs d_x and partials");
    CHK(sample_shape("ddimx_inpaint_update", B, per_sample));
    HIPCHK(inpaint_update_launch(xt, eps, noise, x0, y, mask, d_x, partials, coef, step, B, per_sample, flags, (hipStream_t)stream));
    return 0;
}
int ddimx_multistep_update(float* xt, const float* eps, float* x0, float* hist, const float* coef, const int* step, long long n,
                           void* stream) {
    if (!xt || !eps || !x0 || !coef || !step) return fail("ddimx_multistep_update: null argument");
    if (n <= 0 || n % 4) return fail("ddimx_multistep_update: n = %lld must be a positive multiple of 4", n);
    HIPCHK(multistep_update_launch(xt, eps, x0, hist, coef, step, n, (hipStream_t)stream));
    return 0;
}
static_assert(DDIMX_INVERT_STRIDE == kInvertStride, "ddimx.h and invert_kernels.h disagree");
long long ddimx_invert_partials_doubles(int B, long long per_sample) {
    if (B < 1 || B > 65535 || per_sample <= 0 || per_sample % 4) return -1;
    return (long long)B * sample_blocks(B, per_sample, kInvertMaxBlocks) * 3;
}
int ddimx_invert_update(float* xt, const float* eps, float* base, float* x0, double* partials, float* log, int rows,
                        const float* coef, const int* step, int B, long long per_sample, void* stream) {
    if (!xt || !eps || !base || !x0 || !partials || !log || !coef || !step) return fail("ddimx_invert_update: null argument");
    if (rows < 1) return fail("ddimx_invert_update: rows = %d must be positive", rows);
    CHK(sample_shape("ddimx_invert_update", B, per_sample));
    HIPCHK(invert_update_launch(xt, eps, base, x0, partials, log, rows, coef, step, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_slerp(const float* z1, const float* z2, const float* weights, int M, float* out, double* partials, int P,
                long long per_sample, void* stream) {
    if (!z1 || !z2 || !weights || !out || !partials) return fail("ddimx_slerp: null argument");
    if (M < 1) return fail("ddimx_slerp: M = %d weights (at least 1)", M);
    if (P < 1 || P > 65535) return fail("ddimx_slerp: P = %d pairs (1..65535)", P);
    CHK(sample_shape("ddimx_slerp", P, per_sample));
    HIPCHK(slerp_launch(z1, z2, weights, M, out, partials, P, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_noise_fill(void* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample, const int* step,
                     unsigned draw_base, unsigned tag, int kind, void* stream) {
    if (!out) return fail("ddimx_noise_fill: null argument");
    CHK(sample_shape("ddimx_noise_fill", B, per_sample));
    CHK(noise_range("ddimx_noise_fill", B, per_sample, first_sample));
    if (kind != DDIMX_NOISE_NORMALS && kind != DDIMX_NOISE_WORDS) return fail("ddimx_noise_fill: unknown kind %d", kind);
    HIPCHK(noise_fill_launch(out, B, per_sample, seed, first_sample, step, draw_base, tag, kind, (hipStream_t)stream));
    return 0;
}
static_assert(DDIMX_WINDOW_MAX_COVER == kWindowMaxCover, "ddimx.h and window_kernels.h disagree");
int ddimx_window_gather(const float* canvas, float* win, int N, int W, int C, int L, int T, int H, int F, void* stream) {
    if (!canvas || !win) return fail("ddimx_window_gather: null argument");
    CHK(window_shape("ddimx_window_gather", N, W, C, L, T, H, F));
    HIPCHK(window_gather_launch(canvas, win, N, W, C, L, T, H, F, (hipStream_t)stream));
    return 0;
}
int ddimx_window_update(float* x, const float* eps, const float* noise, float* x0, const int* jfirst, const int* cnt, const float* wt,
                        const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, void* stream) {
    if (!x || !eps || !x0 || !jfirst || !cnt || !coef || !step) return fail("ddimx_window_update: null argument");
    CHK(window_shape("ddimx_window_update", N, W, C, L, T, H, F));
    CHK(window_cover("ddimx_window_update", wt, T, H));
    HIPCHK(window_update_launch(x, eps, noise, x0, jfirst, cnt, wt, coef, step, N, W, C, L, T, H, F, (hipStream_t)stream));
    return 0;
}
static_assert(DDIMX_POOL_STRIDE == kPoolStride && DDIMX_POOL_SLOT_WORDS == kPoolSlotWords, "ddimx.h and pool_kernels.h disagree");
static int pool_shape(const char* who, int n_slots, int max_steps) {
    if (n_slots < 1 || n_slots > 65535) return fail("%s: n_slots = %d (1..65535)", who, n_slots);
    if (max_steps < 1) return fail("%s: max_steps = %d must be positive", who, max_steps);
    return 0;
}
int ddimx_pool_begin(const float* arena, const int* slots, int64_t* t, int n_slots, int max_steps, void* stream) {
    if (!arena || !slots || !t) return fail("ddimx_pool_begin: null argument");
    CHK(pool_shape("ddimx_pool_begin", n_slots, max_steps));
    HIPCHK(pool_begin_launch(arena, slots, t, n_slots, max_steps, (hipStream_t)stream));
    return 0;
}
int ddimx_pool_update(float* xt, const float* eps, float* x0, float* hist, const float* arena, const int* slots, int n_slots,
                      int max_steps, long long per_sample, void* stream) {
    if (!xt || !eps || !x0 || !hist || !arena || !slots) return fail("ddimx_pool_update: null argument");
    CHK(pool_shape("ddimx_pool_update", n_slots, max_steps));
    CHK(sample_shape("ddimx_pool_update", n_slots, per_sample));
    CHK(noise_range("ddimx_pool_update", n_slots, per_sample, 0));  // a slot's sample index is a word of the slot table: any value fits
    HIPCHK(pool_update_launch(xt, eps, x0, hist, arena, slots, n_slots, max_steps, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_pool_end(int* slots, int n_slots, int max_steps, void* stream) {
    if (!slots) return fail("ddimx_pool_end: null argument");
    CHK(pool_shape("ddimx_pool_end", n_slots, max_steps));
    HIPCHK(pool_end_launch(slots, n_slots, max_steps, (hipStream_t)stream));
    return 0;
}
int ddimx_v_to_eps(const float* x, const float* v, float* eps, const float* vtab, int n_table, const int64_t* t, int B,
                   long long per_sample, void* stream) {
    if (!x || !v || !eps || !vtab || !t) return fail("ddimx_v_to_eps: null argument");
    CHK(sample_shape("ddimx_v_to_eps", B, per_sample));
    if (n_table < 1) return fail("ddimx_v_to_eps: n_table = %d must be positive", n_table);
    HIPCHK(v_to_eps_launch(x, v, eps, vtab, n_table, t, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_qsample_v(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, float* v, int B,
                    long long per_sample, void* stream) {
    if (!x0 || !e || !alphas || !t || !x || !v) return fail("ddimx_qsample_v: null argument");
    CHK(sample_shape("ddimx_qsample_v", B, per_sample));
    HIPCHK(qsample_v_launch(x0, e, alphas, t, x, v, B, per_sample, (hipStream_t)stream));
    return 0;
}
// the scalar kernels of the training step's tail: any positive per_sample
static int tail_shape(const char* who, int B, long long per_sample) {
    CHK(batch_range(who, B));
    if (per_sample <= 0) return fail("%s: per_sample = %lld must be positive", who, per_sample);
    return 0;
}
// block tables of the multi-tensor kernels: one workgroup per entry, so a negative count is refused and an empty table is no launch
static int table_shape(const char* who, const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks) {
    if (!sizes || !blk_tensor || !blk_off) return fail("%s: null argument", who);
    if (nblocks < 0) return fail("%s: nblocks = %d must not be negative", who, nblocks);
    return 0;
}
int ddimx_qsample(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, int B,
                  long long per_sample, void* stream) {
    if (!x0 || !e || !alphas || !t || !x) return fail("ddimx_qsample: null argument");
    CHK(tail_shape("ddimx_qsample", B, per_sample));
    HIPCHK(qsample_launch(x0, e, alphas, t, x, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_sqerr_loss(const float* e, const float* out, float* partial, float* loss, int B, long long per_sample,
                     void* stream) {
    if (!e || !out || !partial || !loss) return fail("ddimx_sqerr_loss: null argument");
    CHK(tail_shape("ddimx_sqerr_loss", B, per_sample));
    HIPCHK(sqerr_launch(e, out, partial, loss, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_ema_block_elems(void) { return ema_block_elems(); }
int ddimx_ema_update_multi(const long long* shadow_ptrs, const long long* param_ptrs, const long long* sizes,
                           const int* blk_tensor, const long long* blk_off, int nblocks, float mu, void* stream) {
    // 1 - mu from the ALREADY ROUNDED mu: not the reference's fp32(1.0 - mu) of a Python double (see ddimx_ema_update_multi_coef)
    return ddimx_ema_update_multi_coef(shadow_ptrs, param_ptrs, sizes, blk_tensor, blk_off, nblocks, (float)(1.0 - (double)mu), mu,
                                       stream);
}
int ddimx_ema_update_multi_coef(const long long* shadow_ptrs, const long long* param_ptrs, const long long* sizes,
                                const int* blk_tensor, const long long* blk_off, int nblocks, float c_param, float c_shadow,
                                void* stream) {
    if (!shadow_ptrs || !param_ptrs) return fail("ddimx_ema_update_multi: null argument");
    CHK(table_shape("ddimx_ema_update_multi", sizes, blk_tensor, blk_off, nblocks));
    if (nblocks == 0) return 0;
    HIPCHK(ema_multi_launch(shadow_ptrs, param_ptrs, sizes, blk_tensor, blk_off, nblocks, c_param, c_shadow, (hipStream_t)stream));
    return 0;
}

int ddimx_grad_norm_multi(const long long* grad_ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                          int nblocks, float max_norm, float* partial, float* out, void* stream) {
    if (!grad_ptrs || !partial || !out) return fail("ddimx_grad_norm_multi: null argument");
    CHK(table_shape("ddimx_grad_norm_multi", sizes, blk_tensor, blk_off, nblocks));
    if (nblocks == 0) return 0;
    HIPCHK(grad_norm_multi_launch(grad_ptrs, sizes, blk_tensor, blk_off, nblocks, max_norm, partial, out, (hipStream_t)stream));
    return 0;
}
int ddimx_scale_multi(const long long* ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks,
                      const float* coef, void* stream) {
    if (!ptrs || !coef) return fail("ddimx_scale_multi: null argument");
    CHK(table_shape("ddimx_scale_multi", sizes, blk_tensor, blk_off, nblocks));
    if (nblocks == 0) return 0;
    HIPCHK(scale_multi_launch(ptrs, sizes, blk_tensor, blk_off, nblocks, coef, (hipStream_t)stream));
    return 0;
}
// what ddimx_adam_multi and _dyn share; clip is nullable
static int adam_args(const char* who, AdamArgs* a, const long long* param_ptrs, const long long* grad_ptrs, const long long* m_ptrs,
                     const long long* v_ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks,
                     const float* clip, float beta1, float beta2, float eps, float weight_decay, int decoupled) {
    if (!param_ptrs || !grad_ptrs || !m_ptrs || !v_ptrs) return fail("%s: null argument", who);
    CHK(table_shape(who, sizes, blk_tensor, blk_off, nblocks));
    if (decoupled < 0 || decoupled > 2) return fail("%s: decoupled = %d (0 Adam, 1 AdamW, 2 AdaBelief)", who, decoupled);
    a->p = param_ptrs; a->g = grad_ptrs; a->m = m_ptrs; a->v = v_ptrs; a->sizes = sizes; a->blk_tensor = blk_tensor; a->blk_off = blk_off;
    a->clip = clip; a->lr = 0.f; a->b1 = beta1; a->b2 = beta2; a->eps = eps; a->wd = weight_decay; a->decoupled = decoupled;
    a->bc1 = 1.f; a->bc2s = 1.f;
    a->dyn = nullptr;
    return 0;
}
int ddimx_adam_multi(const long long* param_ptrs, const long long* grad_ptrs, const long long* m_ptrs, const long long* v_ptrs,
                     const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks, const float* clip,
                     float lr, float beta1, float beta2, float eps, float weight_decay, int step, int decoupled, void* stream) {
    if (step < 1) return fail("ddimx_adam_multi: step must be >= 1");
    AdamArgs a;
    CHK(adam_args("ddimx_adam_multi", &a, param_ptrs, grad_ptrs, m_ptrs, v_ptrs, sizes, blk_tensor, blk_off, nblocks, clip, beta1, beta2,
                  eps, weight_decay, decoupled));
    if (nblocks == 0) return 0;
    a.lr = lr;
    a.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    a.bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    HIPCHK(adam_multi_launch(a, nblocks, (hipStream_t)stream));
    return 0;
}

int ddimx_adam_multi_dyn(const long long* param_ptrs, const long long* grad_ptrs, const long long* m_ptrs, const long long* v_ptrs,
                         const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks, const float* clip,
                         const float* dyn, float beta1, float beta2, float eps, float weight_decay, int decoupled, void* stream) {
    if (!dyn) return fail("ddimx_adam_multi_dyn: null dyn");
    AdamArgs a;
    CHK(adam_args("ddimx_adam_multi_dyn", &a, param_ptrs, grad_ptrs, m_ptrs, v_ptrs, sizes, blk_tensor, blk_off, nblocks, clip, beta1,
                  beta2, eps, weight_decay, decoupled));
    if (nblocks == 0) return 0;
    a.dyn = dyn;
    HIPCHK(adam_multi_launch(a, nblocks, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
