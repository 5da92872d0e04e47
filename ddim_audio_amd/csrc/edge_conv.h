// Launch wrappers of the edge convolutions (edge_conv.hip): enqueue on the given stream, never allocate or synchronise.
#pragma once
#include "common.h"

namespace ddimx {

// ---- launch geometry, host only: the one copy the launchers below, the workspace size and ddimx_debug_edge_plan share ----
enum { EDGE_CONV_IN = 0, EDGE_CONV_OUT = 1, EDGE_CONV_OUT_BWD_DATA = 2, EDGE_CONV_IN_BWD_DATA = 3, EDGE_WGRAD = 4 };  // DDIMX_EDGE_*
struct EdgePlan {
    int variant;          // 0: the kernel for any width; 1: the one for C0 = 32, Cio = 2 (in-conv: MFMA, out-conv: fast, its data
                          // gradient: register, the in-conv's data gradient: tiled, weight gradient: strip)
    unsigned grid_x, grid_y;
    int threads, lds;     // threads per block, dynamic LDS bytes
    int trips;            // the most trips any block makes of its outer loop (pixel slots, grid strides, tiles, strip chunks)
    int tiles_x, tiles_y; // tiles / strips of one sample across and down (in-conv: its 1024-pixel parts, 1)
    int partial_blocks;   // weight gradient: partial slabs fed to the reduce, whose geometry follows
    int reduce_blocks, reduce_unrolled, reduce_tail;  // blocks; 8-deep and single trips of the thread quarter that starts at slab 0
};
// Plans launcher `op` for C0 wide channels and Cio narrow ones.  Returns null, or the reason the launcher refuses the call (a
// thread-local string); every launcher below launches exactly what its plan says and returns hipErrorInvalidValue where it refuses.
const char* edge_plan(int op, int dtype, int B, int C0, int Cio, int H, int W, int groups, EdgePlan* p);

// ---- U-Net edge convolutions (C_io = 2 side; HBM-bound; layout conversion NCHW fp32 <-> NHWC T) ----
// in-conv: reference models/diffusion.py:189-198.  x [B][2][H][W] fp32 -> out [B][H][W][C0] T, + stats partials
hipError_t conv_in_launch(int dtype, const float* x, const float* w /*[C0][cin][3][3]*/, const float* bias, void* out,
                          float* stats, int B, int cin, int C0, int H, int W, hipStream_t s, int groups = 0);
// groups = 1 (here and below): the statistics partials are written folded to the 8 groups, [B][nparts][8][2] (gn_fused.h)
int conv_in_nparts(int H, int W);
// out-conv: models/diffusion.py:199-208 preceded by x + hidden[0] (:284).  (a + b) NHWC T -> eps [B][cout][H][W] fp32
hipError_t conv_out_launch(int dtype, const void* a, const void* b, const float* w /*packed [9][cout][C0] fp32*/,
                           const float* bias, float* out, int B, int C0, int cout, int H, int W, hipStream_t s);

// ---- backward --------------------------------------------------------------------------------------------------
hipError_t conv_out_bwd_data_launch(int dtype, const float* d_eps, const float* w /*packed [9][cout][C0]*/, void* ds, int B, int C0,
                                    int cout, int H, int W, hipStream_t s);
// gradient w.r.t. the network input x of the input conv: dy NHWC [B][H][W][C0] (= d hidden[0]), w = pack_conv_dgrad_launch(DT_F32,
// W_in, .., O = C0, I = NI) [9][NI][C0], dx NCHW fp32 [B][NI][H][W] (written); NI <= 4
hipError_t conv_in_bwd_data_launch(int dtype, const void* dy, const float* w, float* dx, int B, int C0, int NI, int H, int W,
                                   hipStream_t s);
size_t edge_wgrad_partial_floats(int dtype, int B, int C, int NI, int H, int W);
// mode 0: input conv (G = d hidden[0], S = x); mode 1: output conv (G = g1 + g2 = x + hidden[0], S = d_eps)
hipError_t edge_wgrad_launch(int dtype, int mode, const void* g1, const void* g2, const float* S, float* partial, float* dW,
                             float* db, int B, int C, int NI, int H, int W, hipStream_t s);

}  // namespace ddimx
