// Launch wrappers of the FNet's row-wise and element-wise kernels (fnet_pointwise.hip):
// enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

// ---- LayerNorm over rows -----------------------------------------------------------------------------
// y = LN(x [+ add[(m % add_rows)]]) * gamma + beta;  x is T (dtype) or fp32 (dtype = DT_F32)
// chunk_rows > 0: y is written chunk-major for fnet_dense_kernel, rows of a sample = chunk_rows (<= 32)
hipError_t layernorm_launch(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma,
                            const float* beta, float eps, float* y, int M, int N, hipStream_t s, int chunk_rows = 0);

// ---- FNet bottleneck, training ---------------------------------------------------------------------------
// seed_ctr (nullable, device memory): *seed_ctr is added to the seed when the kernel runs (graph-replayed training steps)
hipError_t dropout_apply_launch(const float* src, float* dst, long long n, float p, unsigned long long seed, unsigned stream,
                                hipStream_t s, const unsigned long long* seed_ctr = nullptr);
// y = LN(drop(x) + add[m % add_rows]); sum_out (nullable) keeps the pre-norm rows, stat [M][2] = (mean, rstd)
hipError_t ln_train_launch(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma, const float* beta,
                           float eps, float* y, float* sum_out, float* stat, int M, int N, float p, unsigned long long seed,
                           unsigned stream, hipStream_t s, const unsigned long long* seed_ctr = nullptr);
int ln_bwd_nblocks(int M);
// partial: ln_bwd_nblocks(M) * 2 * N floats; dgamma / dbeta nullable (not reduced)
hipError_t ln_bwd_launch(int x_dtype, const float* dy, const void* x, const float* add, int add_rows, const float* stat,
                         const float* gamma, float* dx, float* partial, float* dgamma, float* dbeta, int M, int N, hipStream_t s);
// mode 0: dst = gelu_new(src); mode 1: dst = src * gelu_new'(aux)
hipError_t gelu_launch(const float* src, const float* aux, float* dst, long long n, int mode, hipStream_t s);
hipError_t transpose_launch(const float* src, float* dst, int R, int C, int act_gelu, hipStream_t s);
hipError_t cast_f32_launch(int dtype, const void* src, float* dst, long long n, hipStream_t s);

}  // namespace ddimx
