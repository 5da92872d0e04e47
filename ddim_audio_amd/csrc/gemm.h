// Launch wrappers of the MFMA GEMM (gemm.hip) and of the FNet's dense kernels (fnet_dense.hip):
// enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

// ---- "NT" GEMM (gemm.hip): C[z][M][N] (+)= A[z][M][K] * B[z][N][K]^T; fp32 or bf16 MFMA, optional split-K ----
struct GemmArgs {
    const float* A; const float* B; float* C;
    const float* bias;      // [N] or null
    const float* resid;     // same layout as C, added in the epilogue, or null
    float* partial;         // split-K workspace [batch*splitk][M][N] (required when splitk > 1)
    int M, N, K, lda, ldb, ldc;
    long long sA, sB, sC;   // batch strides (elements)
    int batch;
    int splitk;             // K split over blockIdx.z (1 = none)
    int accumulate;         // C += ...
    int act;                // 0 none, 1 gelu_new
    int bf16;               // 1: round operands to bf16 while staging, v_mfma_f32_32x32x16_bf16
};
// One GEMM over dense row-major operands: lda = ldb = K, ldc = N, one batch, everything else zero and set by name.
static inline GemmArgs gemm_nt(const float* A, const float* B, float* C, int M, int N, int K) {
    GemmArgs g = {};
    g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.batch = 1;
    return g;
}
hipError_t gemm_launch(GemmArgs g, hipStream_t s);
int gemm_pick_splitk(int M, int N, int K, int batch, int bf16);
// Z[b] = Re(FFT2(X[b])) + X[b] in one launch (gemm.hip); dft_hidden [2hid][hid] interleaved cos/sin rows, dft_seq [S][2S]
bool fnet_mix_supported(int S, int hid);
hipError_t fnet_mix_launch(const float* dft_hidden, const float* dft_seq, const float* X, float* Z, int B, int S, int hid,
                           hipStream_t s);

// ---- dense layers of the FNet at S <= 32 without split-K workspace / LayerNorm launches (fnet_dense.hip) ----------------
// Layouts: "chunk-major" = [sample][k / 4][32 rows][4 fp32] (bf16: [k / 8][32][8]); statistics [sample][part / 2][32][2 x 2].
struct FnetDenseArgs {
    const void* W;         // FRAGMENT order (fnet_fold_launch); bf16 when the launch is bf16, else fp32
    const float* bias;     // [N]
    const void* X;         // tokens: row-major fp32 [B*S][K], or chunk-major (x_chunk) fp32 / bf16 (x_bf16)
    const float* xstats;   // non-null: the operand is (x - mean_row) * rstd_row, from xnp parts of xn elements each
    int xnp, xn;
    void* out;             // row-major fp32 [B*S][N], or chunk-major (out_chunk) fp32 / bf16 (out_bf16)
    int x_chunk, x_bf16, out_chunk, out_bf16;
    int act;               // 1: gelu_new
    const float* R;        // non-null (chunk-major fp32): + LayerNorm(R)[row][n] * rgamma[n] + rbeta[n], statistics rstats
    const float* rstats; const float* rgamma; const float* rbeta;
    int rnp, rn;
    float* ostats;         // nullable: row statistics of `out` as written, gridDim.x parts of 32 or 64 features
    float eps;
    int S, K, N;
};
// Fourier mixing over those layouts with the previous layer's output LayerNorm taken on the fly (fnet_dense.hip)
struct FnetMixArgs {
    const float* tab;      // hidden-DFT table of this layer, gamma folded in, fragment order (fnet_table_launch)
    const float* dft_seq;  // [S][2S] = [cos | -sin]
    const float* V;        // chunk-major fp32 input rows
    const float* vstats;   // their statistics (16 parts of hid / 16); null: the rows are used as they are
    const float* gamma; const float* beta; const float* bc;  // LayerNorm affine and C_H beta (with vstats)
    float* zc; float* zstats;  // chunk-major Z and its row statistics (hid / 16 parts of 16)
    float eps;
    int S, hid;
};
hipError_t fnet_mix2_launch(const FnetMixArgs& a, int B, hipStream_t s);
hipError_t fnet_table_launch(const float* gamma, const float* beta, float* tab, float* bc, int H, hipStream_t s);
bool fnet_dense_supported(int S, int K, int N);
hipError_t fnet_dense_launch(const FnetDenseArgs& a, int B, int bf16, hipStream_t s);
// Wf = W * diag(gamma) (gamma null: W) in MFMA fragment order, optionally rounded to bf16; bf = bias + W * beta (beta null: not written)
hipError_t fnet_fold_launch(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, int wf_bf16,
                            float* bf, int N, int K, hipStream_t s);
// out = LayerNorm(A*B^T + bias + resid) * gamma + beta (rows of N <= 2048), GEMM via the partial workspace
hipError_t gemm_ln_launch(GemmArgs g, const float* gamma, const float* beta, float eps, float* out, hipStream_t s);

}  // namespace ddimx
