// Exports of include/ddimx_threshold.h: the exact per-sample quantile of |x0| and the eps rewrite of the x0 clip / threshold.
#include "host.h"
#include "../../include/ddimx_threshold.h"
#include "threshold_kernels.h"

static int thresh_shape(const char* who, int B, long long per_sample, int n_table) {
    CHK(sample_shape(who, B, per_sample));
    if (per_sample >= (1LL << 31)) return fail("%s: per_sample = %lld must be below 2^31", who, per_sample);
    if (n_table < 1) return fail("%s: n_table = %d must be positive", who, n_table);
    return 0;
}

extern "C" {

long long ddimxq_quantile_work_bytes(int B) { return (B < 1 || B > 65535) ? -1 : quantile_work_bytes(B); }

int ddimxq_x0_quantile(const float* x, const float* eps, const float* tab, int n_table, const int64_t* t, long long rank, float floor,
                       float ceil, void* work, float* scale, int B, long long per_sample, void* stream) {
    if (!x || !eps || !tab || !t || !work || !scale) return fail("ddimxq_x0_quantile: null argument");
    CHK(thresh_shape("ddimxq_x0_quantile", B, per_sample, n_table));
    if (rank < 0 || rank >= per_sample) return fail("ddimxq_x0_quantile: rank = %lld outside 0 .. per_sample - 1 = %lld", rank, per_sample - 1);
    if (!(floor > 0.f) || !(floor <= ceil)) return fail("ddimxq_x0_quantile: floor = %g, ceil = %g (0 < floor <= ceil)", (double)floor, (double)ceil);
    HIPCHK(x0_quantile_launch(x, eps, tab, n_table, t, rank, floor, ceil, work, scale, B, per_sample, (hipStream_t)stream));
    return 0;
}

int ddimxq_threshold_eps(const float* x, const float* eps_in, float* eps_out, const float* scale, const float* tab, int n_table,
                         const int64_t* t, int B, long long per_sample, void* stream) {
    if (!x || !eps_in || !eps_out || !scale || !tab || !t) return fail("ddimxq_threshold_eps: null argument");
    CHK(thresh_shape("ddimxq_threshold_eps", B, per_sample, n_table));
    HIPCHK(threshold_eps_launch(x, eps_in, eps_out, scale, tab, n_table, t, B, per_sample, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
