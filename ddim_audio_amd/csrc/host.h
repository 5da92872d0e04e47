// Internal header of the host side of libddimx (not installed): what the translation units behind include/ddimx.h share --
// error reporting, the context, the workspace / tape layouts, the conv dispatcher and the building blocks.
//   plan.cpp           parameter plan, weight packing, gradient layout
//   conv_dispatch.cpp  conv / weight-gradient planning and launch, the debug-plan exports
//   blocks.cpp         Residual_Block, timestep embedding, FNet (with its GEMM call and Fourier mix), Down / Upsample backward, and
//                      the sizing rules of the scratch these use (statistics slabs, split-K partials)
//   walk_infer.cpp     inference workspace, the forward walk (inference and training), the inference exports
//   walk_train.cpp     tape, training workspace, the training forward's export and the backward chain
//   ops.cpp            per-op exports
//   samplers.cpp       sampler, loss and optimizer kernels' exports
//   distill.cpp        exports of include/ddimx_distill.h (weighted loss, distillation target) and the training half of
//                      include/cmx_consistency.h (its sampling update is sde.cpp's)
//   window_solver.cpp  exports of include/ddimx_window.h (the windowed multistep solver's blend and fused update)
//   window_inpaint.cpp exports of include/ddimx_window_inpaint.h (the windowed inpainting step's residual and update)
#pragma once
#include "../../include/ddimx.h"

#include <stdarg.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "conv_mfma.h"
// launch wrappers, one header per kernel family; all enqueue on the given stream, never allocate or synchronise (graph-capturable)
#include "edge_conv.h"
#include "gn_kernels.h"
#include "fnet_pointwise.h"
#include "gemm.h"
#include "temb_kernels.h"
#include "step_kernels.h"
#include "window_kernels.h"
#include "tail_kernels.h"
#include "pack_kernels.h"
#include "wgrad_reduce.h"
#include "conv_pipe.h"

// ------------------------------------------------------------------------------------------ plan
enum PackKind { PK_COPY, PK_CONV, PK_CONVT, PK_BIAS2, PK_PERM_COLS, PK_PERM_ROWS, PK_CONV_F32 };

struct ParamSpec {
    std::string name;
    long long numel;
    int kind;
    int d0, d1, d2, d3;  // shape (unused dims = 1)
    size_t off, bytes;   // in the packed buffer
};

struct RBW {
    int g0, b0, g1, b1, g2, w0, w1, bias1;  // indices into specs
};

struct ddimx_ctx {
    ddimx_config cfg;
    int dtype;
    int fnet_bf16;  // operands of the FNet's dense-weight GEMMs rounded to bf16 (transformers.dtype), else exact fp32 MFMA
    int L;
    int E;      // total timestep-embedding width
    int width;  // FNet token width
    int Fr;     // frequency bins at the bottleneck
    std::vector<ParamSpec> specs;
    std::vector<long long> grad_off;  // per spec: its offset (floats) in the flat gradient buffer; grad_total: that buffer's size
    long long grad_total;
    std::vector<size_t> frag_off;  // per spec: offset of a second, fragment-order copy of a 3x3 conv weight (conv_wreg.h), 0 = none
    size_t packed_bytes;
    // indices
    int te, tw[3], tb[3];
    int in_w, in_b, out_w, out_b;
    std::vector<std::vector<RBW>> down_rb, up_rb;  // [level][r]
    std::vector<int> down_w, down_b, up_w, up_b;   // per level (level 0 unused)
    int ln0_w, ln0_b, proj_w, proj_b, cout_w, cout_b;
    struct FL { int ln1_w, ln1_b, w1, b1, w2, b2, ln2_w, ln2_b; };
    std::vector<FL> fl;
    // second copies for fnet_dense_kernel (fnet_dense.hip; offsets into the packed buffer, 0 = none): the first FFN matrix with
    // the preceding LayerNorm's gamma folded in (+ the bias with its beta), compute_out likewise with the last layer's output
    // LayerNorm; all of them in MFMA fragment order and -- bf16 FNet -- pre-rounded to bf16
    struct FX { size_t w1f, b1f, w2c, tab, bc; };  // tab / bc: the layer's hidden-DFT table with the PREVIOUS layer's output LayerNorm folded in
    std::vector<FX> fx;
    size_t fx_proj = 0, fx_coutf = 0, fx_coutb = 0;
    bool fx_on = false;
    const void* frag_packed = nullptr;  // the packed buffer whose fragment-order conv copies (frag_off) are current: written by the
                                        // eval-only pack (ddimx_pack_fnet_inference), stale after every ddimx_pack_weights
    const void* fx_packed = nullptr;  // the packed buffer whose fnet_dense copies are current (ddimx_pack_fnet_inference), else null
    std::vector<int> emb_off_down, emb_off_up;  // temb chunk offsets per block, execution order
    const unsigned long long* dropout_ctr = nullptr;  // device counter added to every dropout seed (ddimx_set_dropout_counter)
};

// ddimx_ctx is the type behind the interface's handle; nothing below is part of the interface
#pragma GCC visibility push(hidden)

using namespace ddimx;

// ------------------------------------------------------------------------------------------ errors
int fail(const char* fmt, ...);  // records the message ddimx_last_error returns (per thread); returns 1
#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define CHK(expr)               \
    do {                        \
        int r_ = (expr);        \
        if (r_) return r_;      \
    } while (0)

static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

bool rb_frag_weights(int dtype, int C);

// Split-K of the FNet GEMMs is chosen from the PER-SAMPLE problem (rows of one sample, never the batch): a sample's rows are
// then summed in the same order alone, inside any batch and on any number of GPUs (bit-identical results).
constexpr int kMaxSplitK = 8;
static inline int sample_splitk(int rows_per_sample, int N, int K, int bf16) { return gemm_pick_splitk(rows_per_sample, N, K, 1, bf16); }

// ------------------------------------------------------------------------------------------ workspace
// Every scratch layout of the library (inference workspace, training workspace, tape, the per-op workspaces) is a sequence of
// take() calls.  Two test hooks live here and nowhere else (ops.cpp: ddimx_debug_set_carve_gap, ddimx_debug_layout): a process-wide
// gap of unused bytes behind every region (0 in every product path: the layouts are then what they always were), and a per-thread
// recorder that notes each region's offset and requested size while a layout export carves with a null base.
struct CarveLog { long long *off, *bytes; int cap, n; };
size_t carve_gap();
void carve_note(size_t off, size_t bytes);
struct Carver {
    char* base;
    size_t off;
    void* take(size_t bytes) {
        void* p = base ? base + off : nullptr;
        carve_note(off, bytes);
        off += al256(bytes) + carve_gap();
        return p;
    }
};

// ---- what every whole-network (and FNet) entry point checks before its first launch
// B >= 1, T a positive multiple of 2^(levels - 1) and, where given, the dropout probability in [0, 1)
static inline int check_shape(const ddimx_ctx* c, int B, int T, const float* dropout_p = nullptr) {
    const int m = 1 << (c->L - 1);
    if (B < 1) return fail("batch %d", B);
    if (T < m || T % m) return fail("T=%d must be a positive multiple of %d", T, m);
    if (dropout_p && (*dropout_p < 0.f || *dropout_p >= 1.f)) return fail("dropout probability %g out of [0, 1)", (double)*dropout_p);
    return 0;
}
// ---- what the exports of the per-sample kernels check: the batch is the grid's y extent, a sample is walked in float4s
static inline int batch_range(const char* who, int B) {
    if (B < 1 || B > 65535) return fail("%s: B = %d (1..65535)", who, B);
    return 0;
}
static inline int sample_shape(const char* who, int B, long long per_sample) {
    CHK(batch_range(who, B));
    if (per_sample <= 0 || per_sample % 4) return fail("%s: per_sample = %lld must be a positive multiple of 4", who, per_sample);
    return 0;
}
// the counter of the seeded noise stream (noise.h) holds the group of four and the global sample index in 32 bits each
static inline int noise_range(const char* who, int B, long long per_sample, unsigned first_sample) {
    const unsigned long long end = (unsigned long long)first_sample + (unsigned long long)B;
    if (per_sample / 4 > (1LL << 32)) return fail("%s: per_sample = %lld has more than 2^32 groups of four", who, per_sample);
    if (end > (1ULL << 32)) return fail("%s: first_sample + B = %llu exceeds 2^32", who, end);
    return 0;
}
// the geometry of the windowed samplers' kernels (window_kernels.h: window_shape_ok), each violation by name
static inline int window_shape(const char* who, int N, int W, int C, int L, int T, int H, int F) {
    if (N < 1 || W < 1 || (long long)N * W > 65535) return fail("%s: N = %d canvas samples x W = %d windows (N W in 1..65535)", who, N, W);
    if (C < 1 || F < 4 || F % 4) return fail("%s: C = %d, F = %d (C >= 1, F a positive multiple of 4)", who, C, F);
    if (T < 1 || H < 1 || H > T) return fail("%s: T = %d, H = %d (1 <= H <= T)", who, T, H);
    if ((long long)L != (long long)T + (long long)(W - 1) * H) return fail("%s: L = %d is not T + (W - 1) H = %lld", who, L, (long long)T + (long long)(W - 1) * H);
    if (!window_shape_ok(N, W, C, L, T, H, F)) return fail("%s: one canvas sample has 2^31 or more groups of four elements", who);
    return 0;
}
// K = ceil(T / H) windows cover a canvas row: at most DDIMX_WINDOW_MAX_COVER, and overlapping windows need their weights
static inline int window_cover(const char* who, const float* wt, int T, int H) {
    const int K = (T + H - 1) / H;
    if (K > DDIMX_WINDOW_MAX_COVER) return fail("%s: ceil(T / H) = %d windows cover a row (at most %d)", who, K, DDIMX_WINDOW_MAX_COVER);
    if (K > 1 && !wt) return fail("%s: overlapping windows (H < T) need wt", who);
    return 0;
}
struct TrainTape;
// carves `lay` (Ws / TrainWs: a workspace, TrainTape: a tape) from the caller's buffer and checks the caller's byte count; `who`: the
// export, for the refusal's message
template <class Layout>
static int carve_checked(const char* who, void (*carver)(const ddimx_ctx*, char*, int, int, Layout*), const ddimx_ctx* c, const void* base,
                         long long bytes, int B, int T, Layout* lay) {
    carver(c, (char*)const_cast<void*>(base), B, T, lay);
    if ((long long)lay->total <= bytes) return 0;
    return fail(std::is_same<Layout, TrainTape>::value ? "%s: tape too small: need %zu bytes, got %lld"
                                                              : "%s: workspace too small: need %zu bytes, got %lld", who, lay->total, bytes);
}

// Where the forward walk finds each activation: the timestep embedding and its MLP's two hidden rows (the tape keeps those before
// their SiLU), the input conv's output (hidden[0]) and per level the down / up path's input and each Residual_Block's output.  The
// tape has a buffer per site; the inference workspace one for all of a level's down sites and one for its up sites (blocks run in place).
struct WalkSites {
    float *temb_h1, *temb_h2, *temb;
    void* A;
    std::vector<void*> dn_in, up_in;
    std::vector<std::vector<void*>> dn_y, up_y;  // [level][r]
};
// Scratch of run_fnet (all of it per sample: a batch shard takes its samples' rows of each)
struct FnetWs {
    float *ln0, *X, *Ut, *Z, *Y, *Hb, *O, *gpart;
    float *pz, *pv, *zc, *hc, *vc;  // fnet_dense.hip: row statistics of Z and of the last FFN output; chunk-major Z, FFN hidden, last FFN output
};
struct Ws : WalkSites, FnetWs {
    void *h1, *h2;
    float *stats, *stats2, *scale, *shift;  // stats / stats2: the inference walk alternates (a kernel reads one, writes the other)
    size_t total;
    size_t stats_per_sample, gpart_per_sample;  // floats: the statistics / split-K scratch one sample can need (max over ops)
    size_t h_per_sample;                        // bytes of h1 / h2 one sample can need (its largest level)
    int cmax;
};
void carve(const ddimx_ctx* c, char* base, int B, int T, Ws* w);

// ------------------------------------------------------------------------------------------ conv dispatch
// One fused conv launch.  The first line is what a factory below sets; everything else is optional and set by name.
struct ConvCall {
    int dtype, mode, cin, cout; const void* in; const void* w; void* out; int B, Hin, Win;
    const float* bias = nullptr; const float* chan_add = nullptr; int chan_add_stride = 0;
    const float* in_scale = nullptr; const float* in_shift = nullptr; int xf = XF_NONE; int act = 0;
    const void* skip = nullptr; float* stats = nullptr;
    unsigned long long* stamps = nullptr;
    bool batch_plan = false;  // training: choose the tile variant from the real batch (inference: sample size only)
    const void* aux = nullptr; const float* aux_scale = nullptr; const float* aux_shift = nullptr; int bwd_mode = 0;  // ConvArgs, same names
    GnIn gn = {};             // gn.stats set: the input's GroupNorm is finished inside the kernel (in_scale / in_shift unused)
    bool groups = false;      // statistics partials in group format (gn_fused.h)
    const void* wf = nullptr; // the same weights in MFMA fragment order (conv_wreg.h), if the caller has them
    int kernel_pref = 0;      // 0: the walk's choice; 1: never the software-pipelined kernel (conv_pipe.h); 2: only it (per-op exports)
};

// set for the duration of the whole-network training calls (see ConvCall::batch_plan)
struct BatchPlanScope {  // (the flag itself, thread-local, is private to conv_dispatch.cpp)
    BatchPlanScope();
    ~BatchPlanScope();
};
// Plan of one conv launch: tile configuration and the persistent-workgroup split.
struct ConvPlan { ConvGeom g; int var, Hv, Wv, tiles_x, tiles_y, tiles_per_wg, wgs_per_sample; bool wreg, pipe; };
// CONV3 (3x3, pad 1, C -> C): in and out are both H x W.
ConvCall conv3_call(int dtype, int C, const void* in, const void* w, void* out, int B, int H, int W);
// DOWN4 (Conv2d k4 s2 p1, cin -> cout): H x W is the INPUT's size (both even); out is H/2 x W/2.
ConvCall down4_call(int dtype, int cin, int cout, const void* in, const void* w, void* out, int B, int H, int W);
// UP4 (ConvTranspose2d k4 s2 p1, cin -> cout, + skip): H x W is the INPUT's size, the small side; skip (nullable) and out are 2H x 2W.
ConvCall up4_call(int dtype, int cin, int cout, const void* in, const void* w, const void* skip, void* out, int B, int H, int W);
size_t conv_stats_floats(int dtype, int mode, int cin, int cout, int B, int Hv, int Wv);
int conv_plan(const ConvCall& q, ConvPlan* p);
constexpr int kNumCUs = 256;  // MI355X
// consumer-side GroupNorm finalisation pays 1-1.5 us per round of workgroups (prologue + the producer's tail), a finalize launch
// 5 us + a kernel boundary that the other batch shard partly fills: B = 8 stays launch-free, B >= 32 mostly does not
constexpr int kGnFuseConvRounds = 3, kGnFuseResidRounds = 2;
int conv_rounds(const ConvPlan& p, int B);
bool gn_fuse(int n, int rounds, int max_rounds);
int resid_rounds(int dtype, int C, int B, int H, int W);
int conv_nparts(const ConvPlan& p, bool groups);
int run_conv(const ConvCall& q, hipStream_t s, int* nparts, int* Cs);
void wgrad_plan(const WgradGeom& g, int B, int Hd, int Wd, int* tiles_x, int* tiles_y, int* nsplit, int* per);
size_t wgrad_partial_floats(int dtype, int mode, int ci, int co, int B, int Hd, int Wd);
int run_wgrad(int dtype, int mode, int ci, int co, const void* a_t, const void* du, const float* a_scale,
              const float* a_shift, int xf, float* partial, float* dst, int B, int Hd, int Wd, hipStream_t s);

// ------------------------------------------------------------------------------------------ building blocks
struct RBPtrs {
    const float *g0, *b0, *g1, *b1, *g2, *bias1;
    const void *w0, *w1;
    const void *w0f = nullptr, *w1f = nullptr;  // fragment-order copies (conv_wreg.h) or null
};

// What the training forward of one Residual_Block keeps for its backward: the two pre-activation tensors and the
// GroupNorm constants.  small: [6][B][C] folded (scale, shift) of GN0, GN1, GN2 then [3][B][8][2] (mean, rstd).
struct RBTape {
    void *u1, *u2;
    float* small;
    float* sc(int i, int B, int C) const { return small + (size_t)(2 * i) * B * C; }
    float* sh(int i, int B, int C) const { return small + (size_t)(2 * i + 1) * B * C; }
    float* mr(int i, int B, int C) const { return small + (size_t)6 * B * C + (size_t)i * B * kGroups * 2; }
};
static inline size_t rb_tape_small_floats(int B, int C) { return (size_t)6 * B * C + (size_t)3 * B * kGroups * 2; }

// The weight-gradient branch of the backward (ddimx_unet_bwd_forked).  A conv's weight gradient needs its output gradient `du`
// and the saved forward tensor and feeds nothing but the parameter's gradient slot, so it leaves the data-gradient chain: it is
// issued on a second stream behind an event and the chain goes on.  WHEN it is issued decides what it shares the chip with, and
// that decides whether anything is gained (profiles/r04/wgside/): next to the data-gradient convs (forked as soon as `du`
// exists) both kernels want the same VALU + matrix cycles and each simply takes longer (wgrad 128 -> 204 us, conv 137 -> 196 us
// on average: zero sum); next to the GroupNorm-backward passes (HBM only) the two overlap for real.  So both weight gradients of a
// block are forked behind its LAST data-gradient conv and run beside the block's final apply pass and the next block's statistics
// and first apply pass.  The branch owns its slab buffer and four `du` buffers: a block writes du2 / du1 into the pair of its
// parity, and before the block after next overwrites that pair it waits for the event behind the pair's last reader.  Every fork,
// release and join records an event of its own (nothing is re-recorded inside one capture).
struct WgSide {
    hipStream_t st = nullptr;  // null: one stream, nothing below is used
    void* const* ev = nullptr;
    int n = 0, used = 0;
    // fork each weight gradient as soon as its `du` exists, for the block about to run only (the walk's last block: nothing follows
    // that its branch could run beside)
    bool early_block = false;
    float* partial = nullptr;
    void* du[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t du_free[2] = {nullptr, nullptr};
    int blk = 0;               // Residual_Blocks seen so far (parity -> buffer pair)
    // Weight gradients that wait for the bottleneck: the up path's blocks of the largest levels write their du2 / du1 into buffers
    // of their own (`hold`, non-null for such a block) and queue their launches here; the queue is issued on the branch when the
    // chain enters the FNet backward -- ~3.5 ms of launch-bound kernels at 32 samples, under which these run almost for free.
    void* const* hold = nullptr;
    std::vector<std::function<int()>> held;
    bool on() const { return st != nullptr; }
    int flush_held(hipStream_t s) {
        if (held.empty()) return 0;
        CHK(fork(s));
        for (auto& f : held) CHK(f());
        held.clear();
        return 0;
    }
    int next(hipEvent_t* e) {
        if (used >= n) return fail("ddimx_unet_bwd_forked: %d events are not enough (ddimx_bwd_side_events)", n);
        *e = (hipEvent_t)ev[used++];
        return 0;
    }
    // the branch may read what `s` has produced so far
    int fork(hipStream_t s) {
        hipEvent_t e;
        CHK(next(&e));
        HIPCHK(hipEventRecord(e, s));
        HIPCHK(hipStreamWaitEvent(st, e, 0));
        return 0;
    }
    // everything the branch has been given so far reads buffer pair p no more
    int release(int p) {
        hipEvent_t e;
        CHK(next(&e));
        HIPCHK(hipEventRecord(e, st));
        du_free[p] = e;
        return 0;
    }
    // `s` is about to overwrite buffer pair p
    int claim(int p, hipStream_t s) {
        if (du_free[p]) HIPCHK(hipStreamWaitEvent(s, du_free[p], 0));
        du_free[p] = nullptr;
        return 0;
    }
    int join(hipStream_t s) {
        hipEvent_t e;
        CHK(next(&e));
        HIPCHK(hipEventRecord(e, st));
        HIPCHK(hipStreamWaitEvent(s, e, 0));
        du_free[0] = du_free[1] = nullptr;
        return 0;
    }
};
// The up path's weight gradients of levels < kWgradHoldLevels wait (in `du` buffers of their own, TrainWs::hold: part of the training
// workspace's size) for the bottleneck's backward, whose launch-bound FNet kernels leave the chip idle (WgSide::held).
constexpr int kWgradHoldLevels = 2;

// Gradient destinations of one Residual_Block (fp32, the parameters' own layouts); dtemb: [B][stride] slice.
struct RBGrads {
    float *g0, *b0, *g1, *b1, *g2, *w0, *w1, *bias1;
    float* dtemb; int dtemb_stride;
};
// Scratch of the block backward (carved by the caller)
struct RBBwdWs {
    void *du, *dg;          // activation-sized
    float *stats, *coef, *dgb, *sums, *partial;
    // whole-network backward: the batch sums of the per-sample parameter-gradient terms are deferred and flushed many at
    // a time (colsum_multi); each block then gets its own 4 slots of [B][2][C] floats in `slots` (null: sum immediately)
    ColsumBatch* defer = nullptr;
    float* slots = nullptr;
    // ... and so are the per-sample channel sums of du2 / du1 (conv.1.bias, the timestep-embedding chunk): each block then writes
    // them into two slabs of its own (`sums2`: [2][sums floats]) and queues the reductions (partsum_multi)
    PartsumBatch* pdefer = nullptr;
    float* sums2 = nullptr;
    size_t sums_f = 0;
    // data-only backward (DDIMX_BWD_DATA_ONLY): dx alone -- no weight gradient, no batch or per-sample parameter sums
    bool data_only = false;
};
static inline size_t rb_bwd_stats_floats(int dtype, int B, int HW, int C) { return (size_t)B * resid_nparts(dtype, HW, C) * C * 2; }

static inline const float* pf(const ddimx_ctx* c, const void* packed, int i) {
    return (const float*)((const char*)packed + c->specs[i].off);
}
static inline const void* pv(const ddimx_ctx* c, const void* packed, int i) {
    return (const void*)((const char*)packed + c->specs[i].off);
}
// the fragment-order copy (conv_wreg.h / conv_pipe.h) of conv weight `idx`, if `packed` holds a current one, else null
static inline const void* frag_of(const ddimx_ctx* c, const void* packed, int idx) {
    const bool have = c->frag_packed == packed && (size_t)idx < c->frag_off.size() && c->frag_off[idx];
    return have ? (const char*)packed + c->frag_off[idx] : nullptr;
}

// Extra weight packings the backward needs: data-gradient layouts of the convs and transposed FNet matrices.
struct BwdPack {
    std::vector<std::vector<size_t>> dn_wd0, dn_wd1, up_wd0, up_wd1;  // [level][r] offsets
    std::vector<size_t> down_dg, up_dg;                              // per level (level 0 unused)
    size_t projT, coutT;
    std::vector<size_t> w1T, w2T;
    size_t in_dg;  // input conv, data gradient: [9][in_channels][ch0] fp32 (pack_conv_dgrad of down_modules.0.weight)
    size_t total;
};
void plan_bwd_pack(const ddimx_ctx* c, BwdPack* b);

// What the training forward keeps (carved from the caller's `tape` buffer; depends on B and T).
struct TrainTape : WalkSites {
    std::vector<std::vector<RBTape>> dn_rb, up_rb;
    float *ln0, *ln0_stat, *X0;
    struct FLT { float *Z, *zstat, *Y1, *pre, *s, *sstat, *Xout; };
    std::vector<FLT> fl;
    size_t total;
};
void carve_tape(const ddimx_ctx* c, char* base, int B, int T, TrainTape* t);

// Scratch shared by the training forward and the backward.
struct TrainWs {
    float *stats, *scale, *shift;
    float *Ut, *Hb, *O, *gpart;
    std::vector<void*> Ga, Gb, GS;
    void *gA, *du, *dg, *du_b[3];          // du_b / partial_b: the weight-gradient branch's further `du` buffers and its own slabs (WgSide)
    float *coef, *dgb, *sums, *partial, *partial_b, *slots, *sums_ring;
    size_t sums_f;
    std::vector<std::vector<void*>> hold;  // [level][2 r + {du2, du1}]: the up path's held weight gradients (WgSide::held)
    float *dtemb, *dh2, *dh1;
    float *dO, *dXa, *dXb, *dZ, *dH, *T1, *T2, *lnpart, *dTok, *pgrad;
    size_t total;
};
void carve_train_ws(const ddimx_ctx* c, char* base, int B, int T, TrainWs* w);

// Model.forward (walk_infer.cpp), for inference and for training: what differs between the two is this data.  The caller has
// validated everything: the walk's only refusals are a launch's.
struct FwdWalk {
    const WalkSites* at;
    // Residual_Block scratch.  stats2 set (inference): group-format statistics in two alternating buffers, fragment-order weights
    // where packed; null (training): per-channel statistics in `stats`.  A batch shard's share starts at its first sample x (the per-sample sizes).
    void *h1 = nullptr, *h2 = nullptr; float *stats = nullptr, *stats2 = nullptr, *scale = nullptr, *shift = nullptr;
    size_t stats_per_sample = 0, h_per_sample = 0; int cmax = 0;
    // timestep embedding and bottleneck: over `ws` (inference), or `tape` and `tws` (training: they keep their rows, as every block does)
    const Ws* ws = nullptr; const TrainTape* tape = nullptr; const TrainWs* tws = nullptr; float dropout_p = 0.f; unsigned long long seed = 0;
    // lanes: the whole batch on `s` (fork_mask 0: nothing else is used), or two batch shards on `s` and `sa`
    hipStream_t s = nullptr, sa = nullptr; void* const* events = nullptr; int n_events = 0; unsigned fork_mask = 0;
};
int unet_fwd_walk(const ddimx_ctx* c, const void* packed, const ddimx_tables* tables, const float* x, const int64_t* t, float* eps, int B,
                  int T, const FwdWalk& k);

// Scratch of the Down / Upsample backward: weight-gradient slabs, statistics slabs, per-sample channel sums
struct DuBwdWs { float *partial, *stats, *dgb; size_t total; };

// ---- blocks.cpp
ConvCall rb_conv_call(int dtype, int C, int which, const void* in, const void* w, const void* wf, const float* bias,
                      const float* temb, int temb_stride, float* scale, float* shift, void* out, float* stats, int B, int H, int W);
// One Residual_Block forward.  The first line is what rb_call sets; everything else is set by name.
struct RBCall {
    int dtype, C; const void* x; void* y; int B, H, W; RBPtrs p; hipStream_t s;
    const float* temb = nullptr; int temb_stride = 0;  // this block's chunk of the timestep embedding, [B][stride]
    void *h1 = nullptr, *h2 = nullptr;                 // the convs' outputs (unused with a tape: they go to u1 / u2)
    float *stats = nullptr, *stats2 = nullptr, *scale = nullptr, *shift = nullptr;  // stats2 set: launch-free GroupNorm, group format
    int x_nparts = 0, x_Cs = 0;                        // the partition of x's statistics, which `stats` holds on entry
    bool want_stats = false;                           // leave those of y (in `stats`; with stats2: in `stats2`)
    const RBTape* tape = nullptr;                      // training: keep what the backward needs
};
static inline RBCall rb_call(int dtype, int C, const void* x, void* y, int B, int H, int W, const RBPtrs& p, hipStream_t s) {
    return RBCall{dtype, C, x, y, B, H, W, p, s};
}
int run_resblock(const RBCall& q, int* y_nparts);
size_t rb_stats_floats(int dtype, int B, int C, int H, int W, bool group_floor);
size_t walk_stats_floats(const ddimx_ctx* c, int B, int T, bool group_floor);
// GroupNorm-backward statistics in a data-gradient conv's epilogue: the decision and the set-up (blocks.cpp)
int dgrad_fused_stats(ConvCall& d, const void* aux, const float* asc, const float* ash, int mode, float* stats, int np_resid,
                      int* nparts);
int run_resblock_bwd(int dtype, int C, const void* x, const RBTape& tp, const void* dy, const void* extra, void* dx,
                     const float* gam0, const float* gam1, const float* gam2, const void* wd0, const void* wd1,
                     const RBGrads& gr, const RBBwdWs& w, int B, int H, int W, hipStream_t s, WgSide* sd = nullptr,
                     bool stats_ready = false, const void* next_u2 = nullptr);
RBPtrs rb_ptrs(const ddimx_ctx* c, const void* packed, const RBW& r);
int run_temb(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1,
             const float* b1, const float* w2, const float* b2, float* h1, float* h2, float* out, int B,
             int pos_ch, int emb_ch, int E, hipStream_t s);
int run_temb_train(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1, const float* b1,
                   const float* w2, const float* b2, float* h1_pre, float* h2_pre, float* out, int B, int pos_ch, int emb_ch, int E,
                   hipStream_t s);
int run_temb_bwd(const float* d_out, const float* te, const int64_t* t, const float* w1, const float* w2, const float* h1_pre,
                 const float* h2_pre, float* d_h2, float* d_h1, float* d_w0, float* d_b0, float* d_w1, float* d_b1, float* d_w2,
                 float* d_b2, int B, int pos_ch, int emb_ch, int E, hipStream_t s);
int run_gemm(const GemmArgs& g, float* partial, int rows_per_sample, hipStream_t s);
size_t fnet_partial_floats(const ddimx_ctx* c, int B, int S, bool backward);
int fourier_mix(const float* dft_hidden, const float* dft_seq, const float* X, float* Z, float* Ut, float* partial, int B, int S, int hid,
                bool fused, hipStream_t s);
int run_fnet(const ddimx_ctx* c, const void* packed, const ddimx_tables* tb, const FnetWs& w, const void* x, int B, int S, hipStream_t s);
int fnet_fwd_train_part(const ddimx_ctx* c, const void* packed, const ddimx_tables* tables, const TrainWs& w, const TrainTape& tp,
                        const void* x, int B, int S, float dropout_p, unsigned long long seed, hipStream_t s);
int fnet_bwd_part(const ddimx_ctx* c, const void* packed, const char* pb, const BwdPack& bp, const ddimx_tables* tables,
                  const TrainWs& w, const TrainTape& tp, const void* Dlast, float* grads, int B, int S, float dropout_p,
                  unsigned long long seed, hipStream_t s, bool data_only = false);
// Backward of Downsample (cbig -> csmall; x: its input, 2Hs x 2Ws; dy: Hs x Ws) and of Upsample + skip add (csmall -> cbig; x: its
// input, Hs x Ws; dy: 2Hs x 2Ws): the weight gradient, the bias gradient's sums, then the data-gradient conv into dx (Downsample: on
// top of dx_add, nullable).  sd on: the weight gradient goes to the side stream behind a fork, with the branch's slabs; everything
// else stays on `s`.  data_only: the data-gradient conv alone.
int run_downsample_bwd(int dtype, int cbig, int csmall, const void* x, const void* dy, const void* w_dgrad, const void* dx_add, void* dx,
                       float* d_w, float* d_b, const DuBwdWs& w, int B, int Hs, int Ws, hipStream_t s, WgSide* sd = nullptr,
                       bool data_only = false);
int run_upsample_bwd(int dtype, int csmall, int cbig, const void* x, const void* dy, const void* w_dgrad, void* dx, float* d_w,
                     float* d_b, const DuBwdWs& w, int B, int Hs, int Ws, hipStream_t s, WgSide* sd = nullptr, bool data_only = false);

#pragma GCC visibility pop
