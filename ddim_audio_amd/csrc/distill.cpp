// Exports of include/ddimx_distill.h: the SNR-weighted loss and the progressive-distillation target kernels; and the training half
// of include/cmx_consistency.h: the consistency function, its loss and the loss's backward.
#include "host.h"
#include "../../include/ddimx_distill.h"
#include "../../include/cmx_consistency.h"
#include "distill_kernels.h"

static_assert(DDIMX_DISTILL_STRIDE == kDistillStride, "ddimx_distill.h and distill_kernels.h disagree");

// ddimx_sqerr_loss's shape rules (scalar kernels: any positive per_sample) plus the table's
static int loss_w_shape(const char* who, int B, long long per_sample, int n_table) {
    CHK(batch_range(who, B));
    if (per_sample <= 0) return fail("%s: per_sample = %lld must be positive", who, per_sample);
    if (n_table < 1) return fail("%s: n_table = %d must be positive", who, n_table);
    return 0;
}

// the consistency kernels' rules: a sample is walked in float4s, the table has a row, the pseudo-Huber constant is finite and >= 0
static int cm_shape(const char* who, int B, long long per_sample, int n_table, float huber_c) {
    CHK(sample_shape(who, B, per_sample));
    if (n_table < 1) return fail("%s: n_table = %d must be positive", who, n_table);
    if (!(huber_c >= 0.f) || isinf(huber_c)) return fail("%s: huber_c = %g must be finite and >= 0", who, (double)huber_c);
    return 0;
}

extern "C" {

int ddimxd_sqerr_loss_w(const float* target, const float* out, const float* wtab, int n_table, const int64_t* t, float* partial,
                        float* loss, int B, long long per_sample, void* stream) {
    if (!target || !out || !wtab || !t || !partial || !loss) return fail("ddimxd_sqerr_loss_w: null argument");
    CHK(loss_w_shape("ddimxd_sqerr_loss_w", B, per_sample, n_table));
    HIPCHK(sqerr_w_launch(target, out, wtab, n_table, t, partial, loss, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimxd_sqerr_loss_w_bwd_mean(const float* target, const float* out, const float* g, const float* wtab, int n_table,
                                 const int64_t* t, float* d_out, int B, long long per_sample, void* stream) {
    if (!target || !out || !g || !wtab || !t || !d_out) return fail("ddimxd_sqerr_loss_w_bwd_mean: null argument");
    CHK(loss_w_shape("ddimxd_sqerr_loss_w_bwd_mean", B, per_sample, n_table));
    HIPCHK(sqerr_w_bwd_launch(target, out, g, wtab, n_table, t, d_out, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimxd_distill_half(const float* z, const float* eps0, const float* rows, float* zmid, float* m0, int B, long long per_sample,
                        void* stream) {
    if (!z || !eps0 || !rows || !zmid || !m0) return fail("ddimxd_distill_half: null argument");
    CHK(sample_shape("ddimxd_distill_half", B, per_sample));
    HIPCHK(distill_half_launch(z, eps0, rows, zmid, m0, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimxd_distill_target(const float* z, const float* zmid, const float* eps1, const float* m0, const float* rows, float* target,
                          float* x0_target, int B, long long per_sample, void* stream) {
    if (!z || !zmid || !eps1 || !m0 || !rows || !target) return fail("ddimxd_distill_target: null argument");
    CHK(sample_shape("ddimxd_distill_target", B, per_sample));
    HIPCHK(distill_target_launch(z, zmid, eps1, m0, rows, target, x0_target, B, per_sample, (hipStream_t)stream));
    return 0;
}

// ---- include/cmx_consistency.h: the training half of consistency distillation (the sampling update is sde.cpp's)
int cmx_consistency_out(const float* x, const float* out, const float* tab, int n_table, const int64_t* t, float* f, int B,
                        long long per_sample, void* stream) {
    if (!x || !out || !tab || !t || !f) return fail("cmx_consistency_out: null argument");
    CHK(cm_shape("cmx_consistency_out", B, per_sample, n_table, 0.f));
    HIPCHK(cm_out_launch(x, out, tab, n_table, t, f, B, per_sample, (hipStream_t)stream));
    return 0;
}
int cmx_consistency_loss(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t, float huber_c,
                         float* partial, float* loss, int B, long long per_sample, void* stream) {
    if (!x || !out || !y || !tab || !t || !partial || !loss) return fail("cmx_consistency_loss: null argument");
    CHK(cm_shape("cmx_consistency_loss", B, per_sample, n_table, huber_c));
    HIPCHK(cm_loss_launch(x, out, y, tab, n_table, t, huber_c, partial, loss, B, per_sample, (hipStream_t)stream));
    return 0;
}
int cmx_consistency_loss_bwd(const float* x, const float* out, const float* y, const float* tab, int n_table, const int64_t* t,
                             float huber_c, const float* loss, const float* g, float* d_out, int B, long long per_sample, void* stream) {
    if (!x || !out || !y || !tab || !t || !loss || !g || !d_out) return fail("cmx_consistency_loss_bwd: null argument");
    CHK(cm_shape("cmx_consistency_loss_bwd", B, per_sample, n_table, huber_c));
    HIPCHK(cm_loss_bwd_launch(x, out, y, tab, n_table, t, huber_c, loss, g, d_out, B, per_sample, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
