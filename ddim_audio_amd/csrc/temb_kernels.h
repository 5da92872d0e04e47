// Launch wrappers of the timestep-embedding kernels (temb_kernels.hip): enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

// ---- small dense layers (timestep embedding MLP, models/diffusion.py:110-120) ------------------------
// y[b][n] = act(sum_k x[row(b)][k] * W[n][k] + bias[n]); row(b) = idx ? idx[b] : b
// in_silu: SiLU is applied to x while it is read (training keeps the pre-activations)
hipError_t linear_rows_launch(const float* x, const int64_t* idx, const float* W, const float* bias, float* y, int B,
                              int N, int K, int act_silu, hipStream_t s, int in_silu = 0);

hipError_t temb_gather_launch(const float* table /*[n_timesteps][E]*/, const int64_t* t, float* out, int B, int E, hipStream_t s);

// ---- timestep-embedding MLP backward -------------------------------------------------------------------------
hipError_t linear_bwd_w_launch(const float* dy, const float* x, const int64_t* idx, float* dW, float* db, int B, int N, int K,
                               int x_silu, hipStream_t s);
hipError_t linear_bwd_x_launch(const float* dy, const float* W, const float* xpre, float* dx, int B, int N, int K, hipStream_t s);

}  // namespace ddimx
