// Launch wrappers of the weight-packing and layout-conversion kernels (pack_kernels.hip):
// enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

// ---- weight packing ------------------------------------------------------------------------------------
hipError_t pack_copy_launch(const float* src, float* dst, long long n, hipStream_t s);
struct PackCopyBatch {
    static constexpr int kMax = 96;
    const float* src[kMax]; float* dst[kMax]; long long n[kMax]; int count;
    // queues one copy; launches the batch when it is full
    hipError_t push(const float* from, float* to, long long len, hipStream_t s);
};
hipError_t pack_copy_multi_launch(const PackCopyBatch& b, hipStream_t s);
inline hipError_t PackCopyBatch::push(const float* from, float* to, long long len, hipStream_t s) {
    src[count] = from; dst[count] = to; n[count] = len;
    if (++count == kMax) { hipError_t e = pack_copy_multi_launch(*this, s); count = 0; return e; }
    return hipSuccess;
}
struct PackConvBatch {
    static constexpr int kMax = 64;
    const float* src[kMax]; void* dst[kMax]; int O[kMax], I[kMax], KK[kMax]; unsigned char mode[kMax], f32[kMax]; int count;
    // queues one packing; launches the batch when it is full
    hipError_t push(const float* w, void* d, int o, int i, int kk, int md, int dtype, hipStream_t s);
};
hipError_t pack_conv_multi_launch(const PackConvBatch& b, hipStream_t s);
inline hipError_t PackConvBatch::push(const float* w, void* d, int o, int i, int kk, int md, int dtype, hipStream_t s) {
    src[count] = w; dst[count] = d; O[count] = o; I[count] = i; KK[count] = kk; mode[count] = (unsigned char)md;
    f32[count] = dtype == DT_F32;
    if (++count == kMax) { hipError_t e = pack_conv_multi_launch(*this, s); count = 0; return e; }
    return hipSuccess;
}
hipError_t pack_conv_launch(int dtype, const float* w /*[O][I][KH][KW]*/, void* dst /*[KH*KW][O][I]*/, int O, int I,
                            int KH, int KW, hipStream_t s);
hipError_t pack_convT_launch(int dtype, const float* w /*[I][O][4][4]*/, void* dst /*[2][6][2*O][I]*/, int I, int O,
                             hipStream_t s);
// dst[r][f*C + c] = src[r][c*Fr + f]   (token-order permutation of the FNet boundary, rows r)
hipError_t pack_perm_cols_launch(const float* src, float* dst, int rows, int C, int Fr, hipStream_t s);
// dst[(f*C + c)][k] = src[(c*Fr + f)][k]
hipError_t pack_perm_rows_launch(const float* src, float* dst, int C, int Fr, int K, hipStream_t s);

// packed tap layout [ntaps][NOUT][CIN] bf16 (ddimx_pack_conv / one row-parity class of ddimx_pack_convT) -> fragment order
hipError_t pack_frag_from_taps_launch(const void* src, void* dst, int ntaps, int NOUT, int CIN, hipStream_t s);
// weights [O][I][KH][KW] fp32 -> bf16 fragment order [KH*KW * I/16][O/32][64][8]  (conv_wreg.h)
hipError_t pack_conv_frag_launch(const float* w, void* dst, int O, int I, int KK, hipStream_t s);

// data-gradient weights of a 3x3 conv: dst[tap'][ci][co] = w[co][ci][8 - tap'] in the activation dtype
hipError_t pack_conv_dgrad_launch(int dtype, const float* w, void* dst, int O, int I, hipStream_t s);

// ---- layout converters (test / boundary helpers) --------------------------------------------------------------
hipError_t to_nhwc_launch(int dtype, const float* in, void* out, int B, int C, int HW, hipStream_t s);
hipError_t from_nhwc_launch(int dtype, const void* in, float* out, int B, int C, int HW, hipStream_t s);

}  // namespace ddimx
