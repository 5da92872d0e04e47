/* libddimx -- C ABI of the MI355X-native DDIM denoising hot path (gfx950).
 *
 * The reference (klae01/ddim-audio) is pure Python and has no FFI of its own; its boundary for this
 * path is the Python API  Model(config) / model(x, t) / generalized_steps(...)  (SURVEY.md section 8b).
 * This header is the native interface introduced *underneath* that API: each entry point names the
 * reference code whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; ddimx_last_error() gives the message;
 *     nothing aborts or exits (the reference's main.py logs exceptions, main.py:212-223).
 *   - all pointers except `ddimx_config*`, host pointer arrays and host scalars are DEVICE pointers
 *     owned by the caller (PyTorch); the library borrows them for the duration of one call, never
 *     allocates device memory, never synchronises: every call only enqueues work on `stream`
 *     (a hipStream_t passed as void*), so call sequences can be captured into a hipGraph.
 *   - activations inside the network are NHWC ([B][T'][F'][C], channels innermost) in the
 *     activation dtype (DDIMX_F32 or DDIMX_BF16); the network boundary is the reference's
 *     NCHW fp32 [B][C][T][F] (models/diffusion.py:238-240).
 */
#ifndef DDIMX_H
#define DDIMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDIMX_ABI_VERSION 2
#define DDIMX_MAX_LEVELS 8
#define DDIMX_F32 0
#define DDIMX_BF16 1

/* config.model.* and config.diffusion.num_diffusion_timesteps as read by Model.__init__
 * (models/diffusion.py:170-235; configs/audio.yml:25-61). */
typedef struct {
    int in_channels;                 /* model.channels (2) */
    int f_size;                      /* model.f_size (256) */
    int n_levels;                    /* len(model.ch) */
    int ch[DDIMX_MAX_LEVELS];        /* model.ch */
    int res[DDIMX_MAX_LEVELS];       /* model.res */
    int krn[DDIMX_MAX_LEVELS];       /* model.krn (3 only) */
    int n_timesteps;                 /* diffusion.num_diffusion_timesteps */
    int fnet_hidden;                 /* transformers.kwargs.hidden_size */
    int fnet_layers;                 /* transformers.kwargs.num_hidden_layers */
    int fnet_inter;                  /* transformers.kwargs.intermediate_size */
    float fnet_ln_eps;               /* transformers.kwargs.layer_norm_eps */
    int act_dtype;                   /* model.dtype: DDIMX_F32 (parity mode) or DDIMX_BF16 */
    int fnet_dtype;                  /* transformers.dtype (models/diffusion.py:242-246): operand type of the FNet's dense-weight
                                        GEMMs.  DDIMX_F32 = the reference's mixed mode (convs in act_dtype, transformer fp32);
                                        DDIMX_BF16 = operands rounded to bf16 (needs act_dtype == DDIMX_BF16).  The DFT factors,
                                        LayerNorms and accumulators are fp32 either way. */
} ddimx_config;

/* Host-built constant tables for a given T (device pointers, fp32):
 *   posenc     [S][width]    Add_Encoding table (models/diffusion.py:81-92,131-140) in NHWC token order
 *   dft_hidden [2*hid][hid]  interleaved rows: 2k = cos(2 pi k n / hid), 2k+1 = sin(2 pi k n / hid)
 *   dft_seq    [S][2*S]      row k = [cos(2 pi k n / S), n < S | -sin(2 pi k n / S), n < S]
 * with S = T / 2^(n_levels-1), width = ch[-1] * f_size / 2^(n_levels-1). */
typedef struct {
    const float* posenc;
    const float* dft_hidden;
    const float* dft_seq;
    const float* temb_table; /* optional (may be null): [n_timesteps][E] = BetaEmbedding(t) for every t (models/diffusion.py:
                                110-120), built once per weight set with ddimx_temb_fwd over t = 0..n_timesteps-1; when given,
                                ddimx_unet_fwd copies row t[b] instead of running the three-layer MLP (eval mode only: the
                                rows are bit-identical to the MLP's, which computes every row independently) */
} ddimx_tables;

typedef struct ddimx_ctx* ddimx_handle;

int ddimx_abi_version(void);
const char* ddimx_last_error(void);

/* Model.__init__ (models/diffusion.py:170-235): validates the configuration, builds the packing and
 * launch plan.  No device memory is allocated. */
int ddimx_create(const ddimx_config* cfg, ddimx_handle* out);
int ddimx_destroy(ddimx_handle h);
/* Training under hipGraph replay: *counter (device memory, or null to switch off) is added to the dropout seed of every
 * launch of the training forward / backward when it RUNS; an eager step passes a fresh seed by value instead. */
int ddimx_set_dropout_counter(ddimx_handle h, const unsigned long long* counter);

/* Number of state_dict entries (388 parameters + temb.te = 389 for configs/audio.yml), in the
 * reference's registration order; name/shape of entry i for cross-checking the host mirror. */
int ddimx_num_params(ddimx_handle h);
int ddimx_param_info(ddimx_handle h, int i, const char** name, long long* numel);

/* Bytes of the packed-weight buffer / of the workspace for a [B,2,T,F] forward. */
long long ddimx_packed_bytes(ddimx_handle h);
long long ddimx_workspace_bytes(ddimx_handle h, int B, int T);

/* Convert the fp32 parameters (device pointers, state_dict order) to the internal layouts
 * (implicit-GEMM conv weights in the activation dtype, sub-pixel ConvTranspose weights, FNet boundary
 * in NHWC token order).  Must be re-run whenever parameters change (optimizer step, load_state_dict,
 * EMAHelper.ema: models/ema.py:25-30). */
int ddimx_pack_weights(ddimx_handle h, const void* const* params, int n_params, void* packed, void* stream);
/* Inference-only second copies, derived from what ddimx_pack_weights wrote into `packed`; call it after ddimx_pack_weights when the
 * weights are packed for eval mode (a training step re-packs after every optimizer step and reads none of them):
 * - the conv weights of Residual_Block / Downsample / Upsample in MFMA fragment order (csrc/conv_wreg.h, conv_pipe.h;
 *   models/diffusion.py:28-40,59-78) -- without them the convolutions run through conv_mfma_kernel's LDS weight path;
 * - the FNet weights for the launch-lean bottleneck path (csrc/fnet_dense.hip: fragment order, the LayerNorms' gamma / beta folded
 *   into the next matrix, one hidden-DFT table per layer; models/diffusion.py:131-167, modeling_fnet.py:138-279) -- without them
 *   the forward takes the GEMM path: 77 launches instead of 39.
 * Same results within rounding either way; a later ddimx_pack_weights into the same buffer invalidates both. */
int ddimx_pack_fnet_inference(ddimx_handle h, void* packed, void* stream);

/* Model.forward (models/diffusion.py:237-294), eval mode: x [B][C][T][F] fp32, t [B] int64 -> eps. */
int ddimx_unet_fwd(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace,
                   long long workspace_bytes, const float* x, const int64_t* t, float* eps, int B, int T,
                   void* stream);

/* The same forward with part of the network run as two batch shards on two streams (samples [0, B/2) on `stream`, [B/2, B) on
 * `aux_stream`, forked and joined with caller-owned hipEvent_t -- one per fork and one per join, at most 2 * n_levels + 4 of them,
 * none recorded twice in a call; everything is joined into `stream` on return, and the calls are capturable into one hipGraph).  fork_mask bit l (0 <= l < n_levels): the ops whose output lives on level l run
 * sharded; bit 16: the FNet bottleneck.  Every op of the path is per sample (GroupNorm / LayerNorm / FFT are per sample:
 * models/diffusion.py:42-56,148-167), so the result is bit-identical for every mask; aux_stream = NULL or fork_mask = 0 is
 * ddimx_unet_fwd. */
int ddimx_unet_fwd_forked(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                          const float* x, const int64_t* t, float* eps, int B, int T, void* stream, void* aux_stream,
                          void* const* events, int n_events, unsigned fork_mask);

/* ---- training: forward that keeps a tape + whole-network backward ------------------------------------
 * The reference trains through autograd: functions/losses.py:12-18 builds the graph of Model.forward
 * (models/diffusion.py:237-294, training mode: dropout hidden_dropout_prob after the FNet projection and after each FNet
 * FFN) and runners/diffusion.py:150 `loss.backward()` walks it.  Here the forward stores, per Residual_Block, the two
 * pre-activation conv outputs and the GroupNorm constants (plus the FNet rows) in `tape`, and ddimx_unet_bwd turns
 * d_eps into all 388 parameter gradients.
 *   packed_bwd : extra weight packings of the backward (data-gradient conv layouts, transposed FNet matrices), built by
 *                ddimx_pack_weights_bwd from the same parameter tensors + the forward's packed buffer;
 *   tape       : ddimx_train_tape_bytes(B, T) bytes, written by the forward, read by the backward;
 *   workspace  : ddimx_train_workspace_bytes(B, T) bytes of scratch (shared by both calls);
 *   grads      : fp32 [ddimx_grad_floats()], parameter i (plan order, as ddimx_param_info) at ddimx_grad_offset(i) in the
 *                parameter's own shape; gradients are WRITTEN (not accumulated); the temb.te buffer's slot is untouched;
 *   dropout    : masks are a pure function of (seed, layer, element), so the backward regenerates them: pass the same
 *                (dropout_p, seed) to both calls.  dropout_p = 0 gives the deterministic function the parity tests use.
 * The gradient w.r.t. the input x is produced by ddimx_unet_bwd_ex only (the training step never needs it). */
long long ddimx_packed_bwd_bytes(ddimx_handle h);
int ddimx_pack_weights_bwd(ddimx_handle h, const void* const* params, int n_params, const void* packed, void* packed_bwd,
                           void* stream);
long long ddimx_train_tape_bytes(ddimx_handle h, int B, int T);
long long ddimx_train_workspace_bytes(ddimx_handle h, int B, int T);
long long ddimx_grad_floats(ddimx_handle h);
long long ddimx_grad_offset(ddimx_handle h, int i);
int ddimx_unet_fwd_train(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace,
                         long long workspace_bytes, void* tape, long long tape_bytes, const float* x, const int64_t* t,
                         float* eps, int B, int T, float dropout_p, unsigned long long seed, void* stream);
int ddimx_unet_bwd(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                   long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                   const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed, void* stream);
/* Data-parallel training (the reference has no counterpart: runners/diffusion.py:216 is a commented DataParallel):
 * the same backward, which additionally records three caller-owned hipEvent_t on `stream` as soon as a bucket of the flat
 * gradient buffer is final -- bucket 0 = up_modules.* (ready after the up path), 1 = transformer.* (after the bottleneck),
 * 2 = temb.* + down_modules.* (at the end) -- so that the caller can all-reduce each bucket on a second stream while the rest of
 * the backward still runs.  ddimx_grad_buckets fills ranges[6] = {begin0, end0, begin1, end1, begin2, end2} (float offsets into
 * the flat gradient buffer, each bucket one contiguous run).  n_events must be 0 (plain ddimx_unet_bwd) or 3. */
int ddimx_grad_buckets(ddimx_handle h, long long* ranges);
int ddimx_unet_bwd_staged(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                          long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                          const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed,
                          void* const* bucket_events, int n_events, void* stream);
/* The same backward with its weight gradients on a second stream (runners/diffusion.py:150 `loss.backward()`; autograd has no
 * counterpart -- it runs one stream).  A conv's weight gradient feeds nothing but its parameter's slot, so it leaves the
 * data-gradient chain: each is issued on `side_stream` behind an event of `side_events` (caller-owned hipEvent_t, at least
 * ddimx_bwd_side_events(h) of them, none re-recorded within one call so that the call can be captured into a hipGraph) while the
 * chain goes on; the branch is joined into `stream` before the call returns.  Results are bit-identical to ddimx_unet_bwd_staged
 * (same kernels, partitions and order of additions).  With n_events = 3, bucket 0's event is recorded on `side_stream` (behind the
 * up path's last weight gradient and the chain's batch sums), buckets 1 and 2 on `stream`.  side_stream null: one stream. */
int ddimx_bwd_side_events(ddimx_handle h);
int ddimx_unet_bwd_forked(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                          long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                          const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed,
                          void* const* bucket_events, int n_events, void* stream, void* side_stream, void* const* side_events,
                          int n_side_events);
/* The same backward with the gradient w.r.t. the network input -- what autograd hands the reference's `x` (models/diffusion.py:
 * 237-256: x feeds nothing but the input conv, Conv2d(channels -> ch[0], k3 p1), so d x is that conv's data gradient of
 * d hidden[0], one launch behind the chain) -- and an optional data-only mode.
 *   d_x   : nullable; fp32 NCHW [B][in_channels][T][F], WRITTEN with d(sum <d_eps, eps>) / d x.
 *   flags : DDIMX_BWD_DATA_ONLY -- no parameter gradient at all (frozen weights, e.g. guidance): every launch that reaches only a
 *           parameter slot is skipped (weight gradients, bias / GroupNorm / LayerNorm sums, the per-sample sums that feed conv.1.bias
 *           and the timestep embedding, the FNet weight GEMMs, the timestep-embedding MLP); `grads` may be null and is not touched;
 *           d_x is required and is bit-identical to a full backward's; bucket_events must be null, n_events 0; side_stream and its
 *           events are not used (there is no branch to fork).
 * Arguments are validated before the first launch.  ddimx_unet_bwd, _staged and _forked are this call with d_x = null, flags = 0. */
#define DDIMX_BWD_DATA_ONLY 1
int ddimx_unet_bwd_ex(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                      long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                      const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed,
                      void* const* bucket_events, int n_events, void* stream, void* side_stream, void* const* side_events,
                      int n_side_events, float* d_x, int flags);
/* backward of the per-sample squared-error loss (functions/losses.py:18): d_out[b] = 2 g[b] (out[b] - e[b]).  Both forms validate
 * their arguments before the launch: nulls, 1 <= B <= 65535, per_sample positive. */
int ddimx_sqerr_loss_bwd(const float* e, const float* out, const float* g_per_sample, float* d_out, int B,
                         long long per_sample, void* stream);
/* the same against the gradient of ddimx_sqerr_loss's whole [B + 1] vector (per-sample losses, then their batch mean --
 * functions/losses.py:16-18 keepdim / mean): d_out[b] = 2 (g[b] + g[B] / B) (out[b] - e[b]) */
int ddimx_sqerr_loss_bwd_mean(const float* e, const float* out, const float* g, float* d_out, int B, long long per_sample, void* stream);

/* ---- per-op entry points (same kernels as ddimx_unet_fwd; used by the parity tests) ------------- */
/* layout helpers: NCHW fp32 <-> NHWC activation dtype */
int ddimx_to_nhwc(int dtype, const float* nchw, void* nhwc, int B, int C, int H, int W, void* stream);
int ddimx_from_nhwc(int dtype, const void* nhwc, float* nchw, int B, int C, int H, int W, void* stream);
/* weight packing of single layers: Conv2d [O][I][KH][KW] -> [KH*KW][O][I]; ConvTranspose2d(k4,s2,p1)
 * [I][O][4][4] -> [2][6][2*O][I] (sub-pixel form, see csrc/pack_kernels.hip) */
int ddimx_pack_conv(int dtype, const float* w, void* dst, int O, int I, int KH, int KW, void* stream);
int ddimx_pack_convT(int dtype, const float* w, void* dst, int I, int O, void* stream);
/* The packing kernels that otherwise run only inside ddimx_pack_weights / ddimx_pack_weights_bwd, one launch (or one batched
 * sequence) at a time, for tests/test_gpu_temb_step_pack.py.  All tensors fp32 unless said otherwise.
 *   ddimx_pack_perm_cols: dst[r][f*C + c] = src[r][c*Fr + f], r < rows -- the token-order permutation of the FNet boundary
 *     (models/diffusion.py:273-278: the reference's order is c*Fr + f, the library's f*C + c).
 *   ddimx_pack_perm_rows: dst[f*C + c][k] = src[c*Fr + f][k], k < K.  With C and Fr swapped either one is the other direction.
 *   ddimx_pack_copy_multi: dsts[i][0 .. ns[i]) = srcs[i][..] for `count` >= 1 entries; srcs / dsts / ns are HOST arrays of device
 *     pointers / lengths, queued as ddimx_pack_weights queues its plain copies: a launch per 96 entries and one for the rest.
 *   ddimx_pack_conv_multi: `count` >= 1 conv-weight packings, queued as ddimx_pack_weights(_bwd) queues them (a launch per 64 entries
 *     and one for the rest).  Entry i reads srcs[i] = Conv2d.weight [O[i]][I[i]][KK[i] taps] and writes dsts[i] in dtype[i]
 *     (DDIMX_F32 / DDIMX_BF16): mode[i] 0 = ddimx_pack_conv's layout [tap][O][I]; 1 = ddimx_pack_conv_dgrad's [tap][I][O] with the taps
 *     reversed (KK = 9 only).  All seven arrays are HOST arrays.
 * Arguments are validated before the first launch: nulls, positive shapes, rows / entries of fewer than 2^31 elements, mode, dtype. */
int ddimx_pack_perm_cols(const float* src, float* dst, int rows, int C, int Fr, void* stream);
int ddimx_pack_perm_rows(const float* src, float* dst, int C, int Fr, int K, void* stream);
int ddimx_pack_copy_multi(const float* const* srcs, float* const* dsts, const long long* ns, int count, void* stream);
int ddimx_pack_conv_multi(const float* const* srcs, void* const* dsts, const int* O, const int* I, const int* KK, const int* mode,
                          const int* dtype, int count, void* stream);
/* Where ddimx_pack_weights puts parameter i (plan order, as ddimx_param_info) in the packed buffer, and in which layout.  Host only,
 * read-only.  *kind = DDIMX_PACK_* below; *offset / *bytes: the region written (bytes without the padding up to the next region);
 * dims[4]: the parameter's own shape, unused dimensions 1.  Layouts, element type fp32 unless said otherwise:
 *   COPY      the parameter as it is
 *   CONV      ddimx_pack_conv in the activation dtype, dims = (O, I, KH, KW)
 *   CONVT     ddimx_pack_convT in the activation dtype, dims = (I, O, 4, 4)
 *   BIAS2     the bias twice, one copy after the other, dims = (O)
 *   PERM_COLS ddimx_pack_perm_cols(rows = dims[0], C = ch[-1], Fr = dims[1] / C)
 *   PERM_ROWS ddimx_pack_perm_rows(C = ch[-1], Fr = dims[0] / C, K = dims[1])
 *   CONV_F32  ddimx_pack_conv in fp32 whatever the activation dtype
 * Any output pointer may be null. */
#define DDIMX_PACK_COPY 0
#define DDIMX_PACK_CONV 1
#define DDIMX_PACK_CONVT 2
#define DDIMX_PACK_BIAS2 3
#define DDIMX_PACK_PERM_COLS 4
#define DDIMX_PACK_PERM_ROWS 5
#define DDIMX_PACK_CONV_F32 6
int ddimx_debug_param_pack(ddimx_handle h, int i, int* kind, long long* offset, long long* bytes, int* dims);
long long ddimx_op_workspace_bytes(int dtype, int B, int C, int H, int W);
/* The scratch layouts, for tests (tests/walk_harness.py); no product path calls any of the three.  Host only.
 * Every workspace and the tape are a sequence of regions, each starting on a 256-byte boundary.
 *   ddimx_debug_set_carve_gap: from now on, in this process, every region of every layout is followed by `bytes` unused bytes (a
 *     non-negative multiple of 256; anything else is refused).  All *_bytes exports and all walks follow.  The default, 0, is the only
 *     value a product uses: set it back before anything else runs.  Not to be changed while a call of another thread is in flight.
 *   ddimx_debug_layout: the regions of ddimx_workspace_bytes (which = DDIMX_LAYOUT_WORKSPACE), ddimx_train_workspace_bytes
 *     (_TRAIN_WORKSPACE) or ddimx_train_tape_bytes (_TAPE) for (B, T), in the order they are carved, as the walks' own carver notes
 *     them: offsets[i] = where region i starts, bytes[i] = the size asked for (before the rounding up to 256).  The first `cap`
 *     regions are written (cap = 0: none, the arrays may be null), *n = the number of regions.  The layout's total size is the last
 *     region's offset + its size rounded up to 256 + the gap.
 *   ddimx_debug_op_layout: the same for ddimx_op_workspace_bytes(dtype, B, C, H, W) (which = DDIMX_OP_LAYOUT_RESBLOCK; Cbig unused),
 *     ddimx_resblock_bwd_workspace_bytes(dtype, B, C, H, W) (_RESBLOCK_BWD; Cbig unused) and
 *     ddimx_downup_bwd_workspace_bytes(dtype, C, Cbig, B, H, W) (_DOWNUP_BWD; C, H, W: the small side). */
#define DDIMX_LAYOUT_WORKSPACE 0
#define DDIMX_LAYOUT_TRAIN_WORKSPACE 1
#define DDIMX_LAYOUT_TAPE 2
#define DDIMX_OP_LAYOUT_RESBLOCK 0
#define DDIMX_OP_LAYOUT_RESBLOCK_BWD 1
#define DDIMX_OP_LAYOUT_DOWNUP_BWD 2
int ddimx_debug_set_carve_gap(long long bytes);
int ddimx_debug_layout(ddimx_handle h, int which, int B, int T, long long* offsets, long long* bytes, int cap, int* n);
int ddimx_debug_op_layout(int which, int dtype, int B, int C, int Cbig, int H, int W, long long* offsets, long long* bytes, int cap,
                          int* n);

/* Residual_Block.forward (models/diffusion.py:42-56) on NHWC x -> y (may alias x).  gn*_ are fp32
 * [C]; w0/w1 packed by ddimx_pack_conv; temb [B][temb_stride] fp32 (already offset to this block). */
int ddimx_resblock_fwd(int dtype, int C, const void* x, void* y, const float* temb, int temb_stride,
                       const float* gn0_w, const float* gn0_b, const void* w0, const float* gn1_w,
                       const float* gn1_b, const void* w1, const float* bias1, const float* gn2_w, void* workspace,
                       int B, int H, int W, void* stream);
/* ---- training (autograd of the same reference code: runners/diffusion.py:150 `loss.backward()`) ----
 * Residual_Block forward that keeps what its backward needs: u1 = conv.0(...) + temb and u2 = conv.1(...) + bias
 * (PRE-activation, NHWC [B][H][W][C] in the activation dtype) and tape_small (ddimx_rb_tape_floats(B, C) floats:
 * folded GroupNorm scale/shift and (mean, rstd) of the three norms).  Same result as ddimx_resblock_fwd. */
long long ddimx_rb_tape_floats(int B, int C);
int ddimx_resblock_fwd_train(int dtype, int C, const void* x, void* y, const float* temb, int temb_stride,
                             const float* gn0_w, const float* gn0_b, const void* w0, const float* gn1_w,
                             const float* gn1_b, const void* w1, const float* bias1, const float* gn2_w, void* u1,
                             void* u2, float* tape_small, void* workspace, int B, int H, int W, void* stream);
/* data-gradient packing of a 3x3 Conv2d.weight [O][I][3][3]: dst[tap][I][O] = w[.., 8 - tap] (activation dtype) */
int ddimx_pack_conv_dgrad(int dtype, const float* w, void* dst, int O, int I, void* stream);
/* Backward of Residual_Block (models/diffusion.py:42-56): dy -> dx and the gradients of its 8 parameters (fp32, the
 * parameters' own shapes, WRITTEN not accumulated) and of its timestep-embedding chunk d_temb [B][d_temb_stride]
 * (nullable).  workspace: ddimx_resblock_bwd_workspace_bytes(). */
long long ddimx_resblock_bwd_workspace_bytes(int dtype, int B, int C, int H, int W);
int ddimx_resblock_bwd(int dtype, int C, const void* x, const void* u1, const void* u2, const float* tape_small,
                       const void* dy, void* dx, const float* gn0_w, const float* gn1_w, const float* gn2_w,
                       const void* w0_dgrad, const void* w1_dgrad, float* d_gn0_w, float* d_gn0_b, float* d_w0,
                       float* d_gn1_w, float* d_gn1_b, float* d_w1, float* d_bias1, float* d_gn2_w, float* d_temb,
                       int d_temb_stride, void* workspace, int B, int H, int W, void* stream);
/* One fused 3x3 convolution of a Residual_Block (models/diffusion.py:28-40,46-53): the GroupNorm
 * affine (xf = 1) or affine + SiLU (xf = 2) folded as per-(sample, channel) scale/shift [B][C] is applied
 * to the input while it is staged; epilogue adds bias [C] and chan_add [B][chan_add_stride] (either may
 * be null), applies SiLU when act = 1, and writes per-channel (sum, sumsq) partials to stats (nullable;
 * ddimx_conv3x3_stats_floats() floats).  x, y: NHWC [B][H][W][C]. */
int ddimx_conv3x3_fwd(int dtype, int C, const void* x, const void* w, const float* bias, const float* chan_add,
                      int chan_add_stride, const float* in_scale, const float* in_shift, int xf, int act, void* y,
                      float* stats, int B, int H, int W, void* stream);
/* The same with the launch plan's flags: plan_flags = DDIMX_PLAN_BATCH (below) picks the tile variant from the real batch B, as
 * the training walk does (ddimx_conv3x3_fwd = plan_flags 0: from the sample's size alone); ddimx_debug_conv_plan with the same
 * flag predicts the launch.  act = 2 (training forward): y holds the pre-activation and stats are those of SiLU(y as stored).
 * Any other bit of plan_flags is refused: nothing is launched. */
int ddimx_conv3x3_fwd_ex(int dtype, int C, const void* x, const void* w, const float* bias, const float* chan_add,
                         int chan_add_stride, const float* in_scale, const float* in_shift, int xf, int act, void* y,
                         float* stats, int plan_flags, int B, int H, int W, void* stream);
long long ddimx_conv3x3_stats_floats(int dtype, int C, int B, int H, int W);
/* The same convolution through the register-streamed-weights kernel (csrc/conv_wreg.h; bf16, C in {64, 96, 128, 192, 256}, whole
 * tiles): w_frag = the weights in MFMA fragment order, ddimx_pack_conv_frag(w [O][I][3][3] fp32 -> 9*O*I bf16).  This is what
 * ddimx_unet_fwd launches for the Residual_Block convs (models/diffusion.py:46-53) of those widths; fails if the shape is not
 * eligible (ddimx_conv3x3_fwd is the general entry). */
int ddimx_pack_conv_frag(const float* w, void* dst, int O, int I, void* stream);
/* Diagnostic builds (-DDDIMX_STAMP) only: ddimx_conv3x3_wreg_fwd writes its per-wave phase stamps here (null: off). */
int ddimx_debug_set_stamps(unsigned long long* stamps);
/* The same for any tap count (KK = KH * KW; Downsample: 16), and Downsample.forward (models/diffusion.py:70-78) through the
 * register-streamed kernel: x [B][H][W][Cin] bf16 -> y [B][H/2][W/2][Cout], w_frag = ddimx_pack_conv_frag_k(w [Cout][Cin][4][4], 16);
 * stats: per-channel (sum, sumsq) partials of y (sized for one partial per 32 output pixels), nullable. */
int ddimx_pack_conv_frag_k(const float* w, void* dst, int O, int I, int KK, void* stream);
int ddimx_downsample_wreg_fwd(int Cin, int Cout, const void* x, const void* w_frag, const float* bias, void* y, float* stats, int B,
                              int H, int W, void* stream);
/* Upsample.forward + the skip addition (models/diffusion.py:59-67,284) through the register-streamed kernel: w_frag = both
 * row-parity classes of the sub-pixel form (ddimx_pack_convT) re-ordered by ddimx_pack_frag_from_taps(class a of the convT
 * packing, 6 taps, NOUT = 2 * Cout, Cin) one after the other; bias2, skip, y, stats as ddimx_upsample_add_fwd.
 * Of the 3 column taps of the sub-pixel form each output-column parity has two; the third -- dx = 2 for the virtual channels
 * vc < Cout, dx = 0 for vc >= Cout -- is zero by construction in ddimx_pack_convT's output.  The kernel does not read those
 * entries of w_frag (they keep their place in the layout): whatever they hold has no effect, and a non-finite input does not
 * reach an output through a tap the transposed convolution does not have.  Cout must be a multiple of 32. */
int ddimx_pack_frag_from_taps(const void* taps, void* dst, int ntaps, int NOUT, int CIN, void* stream);
int ddimx_upsample_add_wreg_fwd(int Cin, int Cout, const void* x, const void* w_frag, const float* bias2, const void* skip, void* y,
                                float* stats, int B, int H, int W, void* stream);
/* Both convs of Residual_Block (models/diffusion.py:46-53: conv(SiLU(GN(x))) + temb -> SiLU, conv(GN(h)) + bias -> SiLU) through
 * the software-pipelined kernel (csrc/conv_pipe.h: weights resident in registers, the next tile's halo transform and the previous
 * block's epilogue issued in the MFMA gaps of the same wave; bf16, C = 32 / 64, H and W whole numbers of its tiles) -- what
 * ddimx_unet_fwd launches for those widths.  xf = 1 (affine input) or 2 (affine + SiLU); the output activation is SiLU.
 * group_stats: [B][workgroups per sample][32] floats = 8 groups x (sum, sum of squares) of the fp32 values before the bf16
 * rounding + zero padding (gn_fused.h), ddimx_conv3x3_pipe_stats_floats floats (-1: shape not eligible); nullable. */
int ddimx_conv3x3_pipe_fwd(int C, const void* x, const void* w_frag, const float* bias, const float* chan_add, int chan_add_stride,
                           const float* in_scale, const float* in_shift, int xf, void* y, float* group_stats, int B, int H, int W,
                           void* stream);
long long ddimx_conv3x3_pipe_stats_floats(int C, int B, int H, int W);
/* Launch plan of one convolution, for tests: which kernel family and tiling the call described by `flags` gets.  Host only (no HIP
 * call): the same conv_plan / conv_rounds the launches run.  mode: 0 = 3x3 conv, 1 = Downsample (k4 s2), 2 = Upsample (sub-pixel);
 * H, W: the input's size.  flags: DDIMX_PLAN_* below (xf, act and kernel preference as fields).  out[12] = {family (DDIMX_FAMILY_*),
 * tile variant, tiles_x, tiles_y, tiles_per_wg, wgs_per_sample, conv_rounds (how many times over the launch fills the chip), tile
 * height, tile width, threads per workgroup, output-grid height, output-grid width}.  Fails where the call would fail. */
#define DDIMX_PLAN_WFRAG 1     /* fragment-order weights present */
#define DDIMX_PLAN_SKIP 2      /* skip tensor (Upsample + add) */
#define DDIMX_PLAN_STATS 4     /* statistics output present */
#define DDIMX_PLAN_GROUPS 8    /* ... in group format (gn_fused.h) */
#define DDIMX_PLAN_BATCH 16    /* training: the tile variant follows the real batch */
#define DDIMX_PLAN_BWD 32      /* GroupNorm-backward statistics epilogue (aux operand, bwd_mode) */
#define DDIMX_PLAN_XF(xf) ((xf) << 8)
#define DDIMX_PLAN_ACT(act) ((act) << 12)
#define DDIMX_PLAN_PREF(p) ((p) << 16) /* 0: the walk's choice, 1: never the pipelined kernel, 2: only it */
#define DDIMX_PLAN_XF_OF(f) (((f) >> 8) & 3)
#define DDIMX_PLAN_ACT_OF(f) (((f) >> 12) & 3)
#define DDIMX_PLAN_PREF_OF(f) (((f) >> 16) & 3)
#define DDIMX_FAMILY_RING 0    /* conv_mfma_kernel: weights through an LDS ring */
#define DDIMX_FAMILY_WREG 1    /* conv_wreg.h: weights streamed into registers */
#define DDIMX_FAMILY_PIPE 2    /* conv_pipe.h: software-pipelined, weights resident */
int ddimx_debug_conv_plan(int dtype, int mode, int cin, int cout, int B, int H, int W, int flags, int* out);
/* Plan of one weight gradient (host only): ci = channels of the halo operand, co = of the output gradient, Hd x Wd = the output
 * gradient's size.  out[8] = {tiles_x, tiles_y, nsplit (partial slabs), tiles per workgroup, reduce kernel (0: 4 threads per output,
 * 1: 16 threads per output, 2: 16 threads per output quad), tile height, tile width, taps}. */
int ddimx_debug_wgrad_plan(int dtype, int mode, int ci, int co, int B, int Hd, int Wd, int* out);
/* GroupNorm plan of one Residual_Block of the inference walk (host only, the same rule as the launches): for each GroupNorm input --
 * conv 0, conv 1, the residual tail -- whether the consumer finishes it in-kernel (1) or a gn_finalize_groups launch does (0).
 * x_nparts: statistics partials per sample of the block's input.  out[9] = {conv0: partials in, fused, partials out, conv1: the
 * same, resid: the same}. */
int ddimx_debug_gn_plan(int dtype, int C, int B, int H, int W, int x_nparts, int* out);
/* Size in floats of the per-channel statistics partials that Downsample (mode 1) / Upsample (mode 2) of Cin -> Cout on a
 * [B][H][W][Cin] input can write (every kernel form, the largest): the `stats` buffer of ddimx_downsample_wreg_fwd /
 * ddimx_upsample_add_wreg_fwd. */
long long ddimx_conv_stats_floats(int dtype, int mode, int cin, int cout, int B, int H, int W);
/* Weight gradient of one 3x3 conv of Residual_Block (models/diffusion.py:46-53) as ddimx_resblock_bwd computes it: a [B][H][W][C]
 * the conv's input before its input transform xf (0 none, 1 affine, 2 affine + SiLU, 3 SiLU + affine; a_scale / a_shift [B][C]),
 * du [B][H][W][C] the gradient of its output; d_w [C][C][3][3] fp32 is WRITTEN.  partial: ddimx_conv3x3_wgrad_partial_floats() floats. */
long long ddimx_conv3x3_wgrad_partial_floats(int dtype, int C, int B, int H, int W);
int ddimx_conv3x3_wgrad(int dtype, int C, const void* a, const void* du, const float* a_scale, const float* a_shift, int xf,
                        float* partial, float* d_w, int B, int H, int W, void* stream);
int ddimx_conv3x3_wreg_fwd(int C, const void* x, const void* w, const void* w_frag, const float* bias, const float* chan_add,
                           int chan_add_stride, const float* in_scale, const float* in_shift, int xf, int act, void* y,
                           float* stats, int B, int H, int W, void* stream);
/* Diagnostic only: as ddimx_conv3x3_fwd (xf = 2, act = 1); in a -DDDIMX_STAMP build of the library the kernel
 * also writes per-wave per-phase cycle sums to stamps[waves][12] (tools/conv_stamps.py). */
int ddimx_debug_conv3x3_stamps(int dtype, int C, const void* x, const void* w, const float* chan_add,
                                const float* in_scale, const float* in_shift, void* y, float* stats,
                                unsigned long long* stamps, int B, int H, int W, void* stream);
/* y = x + (h * scale + shift): tail of Residual_Block (models/diffusion.py:54-56), NHWC, stats nullable */
int ddimx_resid_gn_fwd(int dtype, int C, const void* x, const void* h, const float* scale, const float* shift, void* y,
                       float* stats, int B, int H, int W, void* stream);
/* Downsample.forward (models/diffusion.py:70-78): [B][H][W][Cin] -> [B][H/2][W/2][Cout] */
int ddimx_downsample_fwd(int dtype, int Cin, int Cout, const void* x, const void* w, const float* bias, void* y,
                         int B, int H, int W, void* stream);
/* Upsample.forward + the skip add that follows it (models/diffusion.py:59-67,284):
 * [B][H][W][Cin] -> [B][2H][2W][Cout] + skip.  bias2 is the bias repeated twice ([2*Cout]). */
int ddimx_upsample_add_fwd(int dtype, int Cin, int Cout, const void* x, const void* w, const float* bias2,
                           const void* skip, void* y, int B, int H, int W, void* stream);
/* BetaEmbedding.forward (models/diffusion.py:110-120): t [B] -> out [B][E]; h1/h2 [B][512] scratch */
int ddimx_temb_fwd(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1,
                   const float* b1, const float* w2, const float* b2, float* h1, float* h2, float* out, int B,
                   int pos_ch, int emb_ch, int E, void* stream);

/* Input convolution, `down_modules[0]` = Conv2d(C_io -> ch[0], k3, p1) (models/diffusion.py:189-198,255-256):
 * x [B][Cin][H][W] fp32 (the reference's NCHW boundary) -> y [B][H][W][C0] NHWC in `dtype`; also writes the GroupNorm
 * statistics partials of y into `stats` (ddimx_conv_in_stats_floats() floats).  w [C0][Cin][3][3] fp32 as stored.
 * Refused before any launch (here and in every edge export below: a dtype other than DDIMX_F32 / DDIMX_BF16; B, H, W, Cin or C0
 * below 1; H or W above 2^31 - 257; 4e18 or more elements): C0 not (4 fp32 | 8 bf16) times a power of two up to 64; B > 65535
 * (B is the grid's y); (9 Cin + 8) C0 floats above 64 KiB of LDS; H W above 2^31 - 1024 (the kernel's int pixel index runs to the
 * end of the last 1024-pixel part), for C0 = 32, Cin = 2 above 2^30 (its int offset of a tap in the second input plane reaches
 * 2 H W - 1). */
long long ddimx_conv_in_stats_floats(int B, int C0, int H, int W);
int ddimx_conv_in_fwd(int dtype, const float* x, const float* w, const float* bias, void* y, float* stats, int B, int Cin,
                      int C0, int H, int W, void* stream);
/* Output convolution, `up_modules[-1]` = Conv2d(ch[0] -> C_io, k3, p1) applied to `x + hidden[0]`
 * (models/diffusion.py:199-208,283-292): a, b NHWC [B][H][W][C0] in `dtype` (summed on the fly) -> eps [B][Cout][H][W] fp32.
 * w_packed: [9][Cout][C0] fp32 = ddimx_pack_conv(DDIMX_F32, w, ..).
 * Refused: C0 not a multiple of 8; Cout > 4; a 10 x 34 tile of C0 + 1 floats above 64 KiB of LDS (C0 > 40);
 * B ceil(H / 8) ceil(W / 32) above 2^31 - 1 (the tile index, sample included, is the grid's x and an int in the kernel). */
int ddimx_conv_out_fwd(int dtype, const void* a, const void* b, const float* w_packed, const float* bias, float* eps, int B,
                       int C0, int Cout, int H, int W, void* stream);
/* Launch plan of one edge-convolution launcher, for tests (host only; the launchers run exactly this plan).  op: DDIMX_EDGE_* below;
 * C0 the wide channel count, Cio the narrow one; groups: group-format statistics (the input conv only).  out[12] = {variant (0: the
 * kernel for any width, 1: the one for C0 = 32, Cio = 2), grid x, grid y, threads per block, dynamic LDS bytes, the most trips any
 * block makes of its outer loop (pixel slots of a part, grid strides, tiles per block, chunks of a strip), tiles / strips / parts
 * of one sample across, down, partial slabs of the weight gradient, blocks of its reduce, 8-deep trips and single trips of the
 * reduce's thread quarter that starts at slab 0}.  Fails where the launcher refuses, with the launcher's reason. */
#define DDIMX_EDGE_CONV_IN 0           /* ddimx_conv_in_fwd, ddimx_conv_in_fwd_groups */
#define DDIMX_EDGE_CONV_OUT 1          /* ddimx_conv_out_fwd */
#define DDIMX_EDGE_CONV_OUT_BWD_DATA 2 /* d_sum of ddimx_conv_out_bwd */
#define DDIMX_EDGE_CONV_IN_BWD_DATA 3  /* ddimx_conv_in_bwd_data */
#define DDIMX_EDGE_WGRAD 4             /* d_w, d_b of ddimx_conv_in_bwd and ddimx_conv_out_bwd */
int ddimx_debug_edge_plan(int op, int dtype, int B, int C0, int Cio, int H, int W, int groups, int* out);
/* Transformer_Module.forward (models/diffusion.py:148-167: TransformerEmbedding :131-145, FNetEncoder x num_hidden_layers
 * transformers modeling_fnet.py:138-279, compute_out), eval mode.  x: the bottleneck activation NHWC
 * [B][S][Fr][C_last] in act_dtype viewed as tokens [B*S][width]; out: fp32 [B*S][width], both in the library's token
 * order f*C_last + c (the reference's is c*Fr + f: models/diffusion.py:273-278).  workspace: ddimx_workspace_bytes(B, T). */
int ddimx_fnet_fwd(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                   const void* x, float* out, int B, int T, void* stream);

/* Transformer_Module alone in TRAINING mode (dropout after the projection and after every FNet FFN, tape kept) and its
 * backward -- the `_bwd` twin of ddimx_fnet_fwd (models/diffusion.py:148-167; autograd through TransformerEmbedding :131-145,
 * FNetEncoder modeling_fnet.py:138-279 and compute_out).  workspace / tape: the whole-network layouts for the same (B, T),
 * ddimx_train_workspace_bytes / ddimx_train_tape_bytes; the launches are the ones ddimx_unet_fwd_train / ddimx_unet_bwd issue for
 * the bottleneck.  x: tokens as for ddimx_fnet_fwd; out / d_out / d_x: fp32 [B*S][width] in the library's token order.
 * ddimx_fnet_bwd WRITES every transformer.* gradient at its ddimx_grad_offset() of `grads` (ddimx_grad_floats() floats; the other
 * entries are left untouched) and the gradient w.r.t. the tokens into d_x. */
int ddimx_fnet_fwd_train(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                         void* tape, long long tape_bytes, const void* x, float* out, int B, int T, float dropout_p,
                         unsigned long long seed, void* stream);
int ddimx_fnet_bwd(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                   long long workspace_bytes, const void* tape, long long tape_bytes, const void* x, const float* d_out, float* d_x,
                   float* grads, int B, int T, float dropout_p, unsigned long long seed, void* stream);

/* ---- backward twins of the per-op forwards (autograd of the reference modules; gradients are WRITTEN, fp32, in the
 * parameter's own layout).  The whole-network ddimx_unet_bwd issues exactly these launches. -------------------------------
 * Downsample (models/diffusion.py:70-78): x [B][H][W][Cin] the forward input, dy [B][H/2][W/2][Cout]; w_dgrad = the SAME weight
 * tensor packed with ddimx_pack_convT(dtype, w, .., I = Cout, O = Cin) (the data gradient of a stride-2 conv is the sub-pixel
 * transposed conv); dx = dx_add (nullable, same shape) + d(input).  workspace: ddimx_downup_bwd_workspace_bytes(dtype, Cout, Cin,
 * B, H/2, W/2) bytes. */
long long ddimx_downup_bwd_workspace_bytes(int dtype, int Csmall, int Cbig, int B, int Hsmall, int Wsmall);
int ddimx_downsample_bwd(int dtype, int Cin, int Cout, const void* x, const void* dy, const void* w_dgrad, const void* dx_add, void* dx,
                         float* d_w, float* d_b, void* workspace, int B, int H, int W, void* stream);
/* Upsample + skip add (models/diffusion.py:59-67,284): x [B][H][W][Cin] the forward input, dy [B][2H][2W][Cout] (also the
 * gradient of the skip tensor, unchanged); w_dgrad = the ConvTranspose2d weight packed with ddimx_pack_conv(dtype, w, .., O = Cin,
 * I = Cout, 4, 4).  d_w in the ConvTranspose2d layout [Cin][Cout][4][4].  workspace: (dtype, Cin, Cout, B, H, W). */
int ddimx_upsample_add_bwd(int dtype, int Cin, int Cout, const void* x, const void* dy, const void* w_dgrad, void* dx, float* d_w,
                           float* d_b, void* workspace, int B, int H, int W, void* stream);
/* Edge convolutions (models/diffusion.py:189-208).  conv_in: dy NHWC gradient of its output, x the NCHW fp32 network input.
 * conv_out: d_sum = gradient w.r.t. (a + b) NHWC (it is the gradient of both summands); weight / bias gradients from a + b.
 * partial: ddimx_edge_bwd_workspace_floats() floats (-1: a shape the weight gradient refuses).
 * The weight gradient refuses (besides what every edge export refuses, ddimx_conv_in_fwd): Cio > 4; for widths other than C0 = 32,
 * Cio = 2: C0 > 64 (a thread holds at most two of the 9 C0 items) or 256 (C0 + 1) + 324 Cio floats above 64 KiB of LDS (C0 > 60
 * at Cio = 2); more than 2^31 - 1025 blocks' worth of tiles (16 x 16) or strips (128 rows x 32 fp32 | 64 bf16 columns) over the
 * batch: the tile counter is an int that runs one grid past the last tile.
 * ddimx_conv_out_bwd refuses what ddimx_conv_out_fwd refuses, and B > 65535 (B is the grid's y of the data gradient). */
long long ddimx_edge_bwd_workspace_floats(int dtype, int B, int C0, int Cio, int H, int W);
int ddimx_conv_in_bwd(int dtype, const void* dy, const float* x, float* partial, float* d_w, float* d_b, int B, int Cin, int C0, int H,
                      int W, void* stream);
/* conv_in's data gradient (the gradient w.r.t. the network input, as ddimx_unet_bwd_ex computes it): dy NHWC [B][H][W][C0] the
 * gradient of its output, w_packed = ddimx_pack_conv_dgrad(DDIMX_F32, down_modules.0.weight, .., O = C0, I = Cin) ([9][Cin][C0],
 * transposed and flipped), d_x NCHW fp32 [B][Cin][H][W], WRITTEN.
 * Refused: Cin > 4; C0 not a multiple of (4 fp32 | 8 bf16); for C0 = 32, Cin = 2 B ceil(H / 8) ceil(W / 32) above 2^31 - 1 (the
 * int tile index), otherwise B > 65535 (the grid's y; pixel indices are 64-bit there). */
int ddimx_conv_in_bwd_data(int dtype, const void* dy, const float* w_packed, float* d_x, int B, int Cin, int C0, int H, int W,
                           void* stream);
int ddimx_conv_out_bwd(int dtype, const float* d_eps, const void* a, const void* b, const float* w_packed, void* d_sum, float* partial,
                       float* d_w, float* d_b, int B, int C0, int Cout, int H, int W, void* stream);
/* BetaEmbedding (models/diffusion.py:110-120), training: the forward keeps the two pre-activations ([B][emb_ch] each), the backward
 * returns every weight / bias gradient (d_h2, d_h1: [B][emb_ch] scratch). */
int ddimx_temb_fwd_train(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1, const float* b1,
                         const float* w2, const float* b2, float* h1_pre, float* h2_pre, float* out, int B, int pos_ch, int emb_ch, int E,
                         void* stream);
int ddimx_temb_bwd(const float* d_out, const float* te, const int64_t* t, const float* w1, const float* w2, const float* h1_pre,
                   const float* h2_pre, float* d_h2, float* d_h1, float* d_w0, float* d_b0, float* d_w1, float* d_b1, float* d_w2,
                   float* d_b2, int B, int pos_ch, int emb_ch, int E, void* stream);
/* The four kernels of that MLP and the table lookup of eval mode one launch at a time, for tests/test_gpu_temb_step_pack.py
 * (models/diffusion.py:110-120; the calls above issue exactly these launchers).  fp32; idx / t are int64 device arrays.
 *   ddimx_temb_gather: out[b] = table[t[b]], rows of E floats (E % 4 == 0), what ddimx_unet_fwd runs when tables->temb_table is given.
 *   ddimx_linear_rows: y[b][n] = g(sum_k f(x[row(b)][k]) W[n][k] + bias[n]); row(b) = idx[b] (idx nullable: b), f = SiLU when in_silu,
 *     g = SiLU when act_silu.  K % 4 == 0.
 *   ddimx_linear_bwd_w: dW[n][k] = sum_b dy[b][n] f(x[row(b)][k]), db[n] = sum_b dy[b][n]; f = SiLU when x_silu.
 *   ddimx_linear_bwd_x: dx[b][k] = (sum_n dy[b][n] W[n][k]) SiLU'(xpre[b][k]).
 * Arguments are validated before the launch: nulls (idx excepted), positive shapes, the batch / N where it is a grid dimension
 * (<= 65535), E % 4, K % 4. */
int ddimx_temb_gather(const float* table, const int64_t* t, float* out, int B, int E, void* stream);
int ddimx_linear_rows(const float* x, const int64_t* idx, const float* W, const float* bias, float* y, int B, int N, int K,
                      int act_silu, int in_silu, void* stream);
int ddimx_linear_bwd_w(const float* dy, const float* x, const int64_t* idx, float* dW, float* db, int B, int N, int K, int x_silu,
                       void* stream);
int ddimx_linear_bwd_x(const float* dy, const float* W, const float* xpre, float* dx, int B, int N, int K, void* stream);

/* ---- sampler (functions/denoising.py:10-52) ------------------------------------------------------- */
/* coef [n_iter][6] fp32 rows (t, sqrt(1-at), sqrt(at), sqrt(at_next), c2, c1); step: device int counter.
 * step_begin fills t[B] with the current timestep; ddim_update performs lines :27 and :41-43 in one pass,
 * writing the x0 prediction to x0 and x_{t-1} in place; step_end advances the counter. */
/* FNet Fourier mixing with its residual, transformers modeling_fnet.py:138-166 (`fftn(x, dim=(1, 2)).real`) + :182:
 * z[b] = Re(FFT2(x[b])) + x[b] over fp32 [B][S][hid]; dft_hidden / dft_seq as in ddimx_tables.  fused = 1: one launch
 * (when ddimx_fnet_mix_supported(S, hid)); fused = 0: two exact-fp32 GEMMs through ut [B][2*hid][S] and the split-K
 * scratch partial [8*B*2*hid*S floats].  The operator is symmetric, so it is also its own backward. */
int ddimx_fnet_mix_supported(int S, int hid);
int ddimx_fnet_mix(const float* dft_hidden, const float* dft_seq, const float* x, float* z, float* ut, float* partial, int B,
                   int S, int hid, int fused, void* stream);
/* ---- the kernels of the FNet bottleneck one by one (tests/test_gpu_fnet_kernels.py).  Each call enqueues the launches the
 * Transformer_Module walks issue for that step, on `stream`; nothing is allocated.  All tensors fp32 unless said otherwise. ----
 * ddimx_gemm_nt: the dense layers and the DFT-as-GEMM factors, nn.Linear of models/diffusion.py:128,156 and of transformers
 * modeling_fnet.py:138-279 (FNetIntermediate.dense, FNetOutput.dense), and the gradients autograd forms for them:
 *   C[z][M][N] (+)= A[z][M][K] * B[z][N][K]^T (+ bias[N]) (gelu_new when act = 1, transformers activations.py:59-66) (+ resid, laid
 *   out as C), z < batch with element strides sA / sB / sC, row strides lda / ldb / ldc.  bf16 = 1 rounds the operands to bf16
 *   (nearest even) and accumulates in fp32.  splitk > 1 splits K over that many workgroups per tile through `partial`
 *   (batch * splitk * M * N floats; null: no split) and a second kernel sums the slices in a fixed order and applies the epilogue.
 * ddimx_gemm_pick_splitk: the split the library itself uses for a GEMM whose ONE sample has rows_per_sample rows (host only,
 *   1 .. 8).
 * ddimx_gemm_ln: FNetOutput.forward (modeling_fnet.py:138-279: dense, LayerNorm(hidden + input)),
 *   out[M][N] = LayerNorm(A * B^T + bias + resid) * gamma + beta in two
 *   launches: the GEMM into `partial` (always; splitk * M * N floats) and a reduce fused with the row norm.  N <= 2048, batch <= 1,
 *   resid rows ldc apart; C, accumulate and act are not used. */
int ddimx_gemm_nt(const float* A, const float* B, float* C, const float* bias, const float* resid, float* partial, int M, int N, int K,
                  int lda, int ldb, int ldc, long long sA, long long sB, long long sC, int batch, int splitk, int accumulate, int act,
                  int bf16, void* stream);
int ddimx_gemm_pick_splitk(int rows_per_sample, int N, int K, int bf16);
int ddimx_gemm_ln(const float* A, const float* B, float* C, const float* bias, const float* resid, float* partial, int M, int N, int K,
                  int lda, int ldb, int ldc, long long sA, long long sB, long long sC, int batch, int splitk, int accumulate, int act,
                  int bf16, const float* gamma, const float* beta, float eps, float* out, void* stream);
/* nn.LayerNorm over rows of N <= 2048 (models/diffusion.py:140-142 with the positional rows `add`, modeling_fnet.py:182 and
 * FNetOutput.LayerNorm):
 *   y[m] = LN(x[m] + add[m % add_rows]) * gamma + beta; x in x_dtype (DDIMX_F32 / DDIMX_BF16), add nullable.
 * ddimx_layernorm (eval): chunk_rows > 0 writes y as [m / chunk_rows][n / 4][32][4] (32 * N floats per sample of chunk_rows <= 32
 *   rows, the other rows untouched), the operand layout of the fused dense kernels.
 * ddimx_ln_train: x is first multiplied by the dropout mask of (p, seed + *seed_ctr, mask_stream) over element index m * N + n
 *   (models/diffusion.py:144, FNetOutput.dropout; seed_ctr nullable, device); sum_out (nullable) keeps the pre-norm rows,
 *   stat [M][2] = (mean, rstd).
 * ddimx_ln_bwd: autograd of the same norm.  x / add: the forward's inputs AFTER dropout (sum_out, or x + add), stat from the
 *   forward; dx [M][N], and dgamma / dbeta [N] when non-null (null: `partial` keeps per-block sums only).  partial:
 *   ddimx_ln_bwd_partial_floats(M, N) floats. */
int ddimx_layernorm(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma, const float* beta, float eps, float* y,
                    int M, int N, int chunk_rows, void* stream);
int ddimx_ln_train(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma, const float* beta, float eps, float* y,
                   float* sum_out, float* stat, int M, int N, float p, unsigned long long seed, unsigned mask_stream,
                   const unsigned long long* seed_ctr, void* stream);
long long ddimx_ln_bwd_partial_floats(int M, int N);
int ddimx_ln_bwd(int x_dtype, const float* dy, const void* x, const float* add, int add_rows, const float* stat, const float* gamma,
                 float* dx, float* partial, float* dgamma, float* dbeta, int M, int N, void* stream);
/* gelu_new (transformers activations.py:59-66; FNetIntermediate.intermediate_act_fn) over n elements -- mode 0: dst = gelu_new(src); mode 1:
 * dst = src * gelu_new'(aux), its autograd. */
int ddimx_gelu(const float* src, const float* aux, float* dst, long long n, int mode, void* stream);
/* dst[C][R] = f(src[R][C])^T, f = identity or (act_gelu) gelu_new: the operands of the weight gradients autograd forms for
 * nn.Linear (dW = dy^T x) laid out for ddimx_gemm_nt. */
int ddimx_transpose(const float* src, float* dst, int R, int C, int act_gelu, void* stream);
/* dst[c] = sum_b src[b * stride + c], b < B, c < C, summed in fp64 and rounded once: nn.Linear's bias gradient. */
int ddimx_colsum(const float* src, int B, long long stride, int C, float* dst, void* stream);
/* nn.Dropout(p) (models/diffusion.py:129,144; FNetOutput.dropout): dst[i] = src[i] * keep(i) / (1 - p), in place allowed.
 * keep is a pure function of (seed + *seed_ctr, mask_stream, i), so that the backward regenerates the forward's mask. */
int ddimx_dropout_apply(const float* src, float* dst, long long n, float p, unsigned long long seed, unsigned mask_stream,
                        const unsigned long long* seed_ctr, void* stream);
/* ---- the fused dense path of the FNet inference walk at S <= 32 tokens per sample (modeling_fnet.py:138-279 restated), one launcher
 * at a time, for tests/test_gpu_fnet_dense.py.  Layouts (32 row slots per sample, rows >= S never written and never used):
 *   fragment order   bf16 [n / 32][k / 16][lane = 32 h + n % 32][8], k = 16 g + 8 h + i; fp32 [n / 32][k / 8][lane][4], k = 8 g + 4 h + i
 *   chunk-major      fp32 [b][k / 4][32][4], bf16 [b][k / 8][32][8]
 *   row statistics   [b][part / 2][32][(sum, centred sum of squares) x 2], parts of equal size
 * ddimx_fnet_fold: Wf = W[N][K] diag(gamma) (gamma null: W) in fragment order, fp32 or (wf_bf16) rounded to bf16;
 *   bf[n] = bias[n] + sum_k W[n][k] beta[k] (beta null: bf not written).  N % 32 == 0, K % 16 == 0.
 * ddimx_fnet_table: the hidden-DFT table in fp32 fragment order, row 2j = cos(2 pi j h / H) gamma[h], row 2j + 1 = sin(..) gamma[h]
 *   (gamma null: 1); bc[j] = sum_h cos(2 pi j h / H) beta[h] (beta null: bc not written).  H % 32 == 0.
 * ddimx_fnet_dense: out[b][t][n] = act(sum_k W[n][k] xf(X[b][t][k]) + bias[n]) (+ LN(R)[b][t][n] rgamma[n] + rbeta[n]); W in
 *   fragment order (bf16 when bf16 = 1); X row-major fp32 [B*S][K] or chunk-major (x_chunk) fp32 / (x_bf16) bf16; xstats non-null:
 *   xf(x) = (x - mean_row) rstd_row from xnp parts of xn elements; out row-major fp32 [B*S][N] or chunk-major (out_chunk) fp32 /
 *   (out_bf16) bf16; act 1 = gelu_new; R chunk-major fp32 with statistics rstats (rnp parts of rn elements); ostats nullable: the
 *   statistics of the fp32 output in N / 32 parts of 32.  Combinations the kernels do not have return an error before any launch;
 *   ddimx_fnet_dense_supported is the shape part of that rule (host only).
 * ddimx_fnet_mix2: zc = Re(FFT2(X)) + X chunk-major with its statistics zstats (hid / 16 parts of 16), X = V (vstats null) or
 *   LN(V) gamma + beta from vstats (16 parts of hid / 16); V chunk-major fp32; tab from ddimx_fnet_table(gamma), bc from
 *   ddimx_fnet_table(beta); dft_seq [S][2S] = [cos | -sin].  hid = 512, S in {8, 16, 24, 32}. */
int ddimx_fnet_fold(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, int wf_bf16, float* bf, int N,
                    int K, void* stream);
int ddimx_fnet_table(const float* gamma, const float* beta, float* tab, float* bc, int H, void* stream);
int ddimx_fnet_dense_supported(int S, int K, int N);
int ddimx_fnet_dense(const void* W, const float* bias, const void* X, const float* xstats, int xnp, int xn, void* out, int x_chunk,
                     int x_bf16, int out_chunk, int out_bf16, int act, const float* R, const float* rstats, const float* rgamma,
                     const float* rbeta, int rnp, int rn, float* ostats, float eps, int S, int K, int N, int B, int bf16, void* stream);
int ddimx_fnet_mix2(const float* tab, const float* dft_seq, const float* V, const float* vstats, const float* gamma, const float* beta,
                    const float* bc, float* zc, float* zstats, float eps, int S, int hid, int B, void* stream);
/* ---- the GroupNorm family of Residual_Block (models/diffusion.py:42-56) one launch at a time, for tests/test_gpu_gn_kernels.py.
 * Activations are NHWC [B][H][W][C] in `dtype`; everything else is fp32.  "parts" = workgroups per sample of the element-wise
 * passes (out[8] of ddimx_debug_gn_plan).  Channel-format statistics: [B][parts][C][2] (sum, sumsq); group format (groups = 1):
 * [B][parts][32], the first 16 floats = [8][2], the rest written as zero. */
int ddimx_tensor_stats(int dtype, const void* x, float* stats, int B, int H, int W, int C, int groups, void* stream);
/* statistics [B][nparts][Cs][2] (slab channel vc is channel vc % C) -> scale = rstd * gamma, shift = beta - mean * scale, [B][C] each;
 * count = elements per (sample, group); beta and mr_out ([B][8][2] = mean, rstd) nullable */
int ddimx_gn_finalize(const float* stats, int nparts, int Cs, int C, double count, const float* gamma, const float* beta, float eps,
                      float* scale, float* shift, float* mr_out, int B, void* stream);
/* the same from group-format statistics with the reduction order of a consumer of `nthreads` threads (64 .. 1024, multiple of 64) */
int ddimx_gn_finalize_groups(const float* gstats, int np, const float* gamma, const float* beta, double count, float eps, int C,
                             float* scale, float* shift, int B, int nthreads, void* stream);
/* block size and 16-byte pieces per thread of the element-wise passes (host only) */
int ddimx_resid_threads(int dtype, int C);
int ddimx_resid_iters(int dtype, int C, int H, int W);
/* the residual pass in all its forms -- h_mode 0: y = x + h * scale + shift, 1: y = x + h (h fp32), 2: y = x + SiLU(h) * scale + shift.
 * gn_stats non-null (h_mode 0 or 2, gn_np <= 256): scale / shift come from these group-format statistics of h, gamma, beta (nullable),
 * count and eps inside the kernel.  stats nullable; groups selects its format. */
int ddimx_resid_ex(int dtype, int C, const void* x, const void* h, int h_mode, const float* scale, const float* shift,
                   const float* gn_stats, int gn_np, const float* gamma, const float* beta, double count, float eps, void* y, float* stats,
                   int groups, int B, int H, int W, void* stream);
/* GroupNorm backward.  stats [B][parts][C][2] = (P, Q): mode 0 (norm fed by SiLU(u)) P = sum g, Q = sum g * SiLU(u); mode 1 (norm
 * followed by SiLU, u = its input) g' = g * SiLU'(scale * u + shift), P = sum g', Q = sum g' * u. */
int ddimx_gn_bwd_stats(int dtype, int mode, const void* g, const void* u, const float* scale, const float* shift, float* stats, int B,
                       int H, int W, int C, void* stream);
/* (P, Q) slabs, gamma [C], mean_rstd [B][8][2] -> coef [B][3][C] (ca, cb, cc of d input = ca g' + cb v + cc) and dgb [B][2][C]
 * (per-sample dgamma, dbeta terms) */
int ddimx_gn_bwd_finalize(const float* stats, int nparts, int C, double count, const float* gamma, const float* mean_rstd, float* coef,
                          float* dgb, int B, void* stream);
/* mode 0: out = (ca g + cb SiLU(u) + cc) SiLU'(u), sums (nullable) [B][parts][C] of out as stored; mode 1: out = gy + ca g' + cb u + cc
 * (+ extra, nullable), and with nu / nstats (both or neither) the mode-0 statistics of (out, nu) into nstats */
int ddimx_gn_bwd_apply(int dtype, int mode, const void* g, const void* u, const void* gy, const void* extra, const float* coef,
                       const float* scale, const float* shift, void* out, float* sums, const void* nu, float* nstats, int B, int H, int W,
                       int C, void* stream);
/* dst[b * dst_stride + c] = sum over p < nparts of src[((b * nparts + p) * C + c) * src_step] */
int ddimx_partsum(const float* src, int B, int nparts, int C, float* dst, long long dst_stride, int src_step, void* stream);
/* `count` such sums (src_step 1) / column sums (as ddimx_colsum) in one launch; the arrays are host arrays of `count` entries */
int ddimx_partsum_multi(const float* const* src, float* const* dst, const long long* dst_stride, const int* nparts, const int* C,
                        const int* B, int count, void* stream);
int ddimx_colsum_multi(const float* const* src, float* const* dst, const long long* stride, const int* B, const int* C, int count,
                       void* stream);
/* One data-gradient 3x3 conv of ddimx_resblock_bwd with the GroupNorm-backward statistics of its output dg taken in its epilogue:
 * bwd_mode 1 = mode 0 above against aux, 2 = mode 1 above against aux, aux_scale, aux_shift.  stats holds [B][*nparts][C][2] on
 * return (sized for `parts` slabs); *nparts = 0, and nothing launched, where the block would run the statistics pass on its own. */
int ddimx_conv3x3_dgrad_stats(int dtype, int C, const void* du, const void* w_dgrad, const void* aux, const float* aux_scale,
                              const float* aux_shift, int bwd_mode, void* dg, float* stats, int* nparts, int B, int H, int W,
                              void* stream);
/* ddimx_conv_in_fwd with group-format statistics, as the inference walk runs it: [B][parts][32], parts as for the channel format.
 * Refuses what ddimx_conv_in_fwd refuses, and C0 not a multiple of the 8 groups. */
int ddimx_conv_in_fwd_groups(int dtype, const float* x, const float* w, const float* bias, void* y, float* group_stats, int B, int Cin,
                             int C0, int H, int W, void* stream);
int ddimx_step_begin(const float* coef, const int* step, int64_t* t, int B, void* stream);
/* as ddimx_step_begin for coefficient tables with another row stride (ddpm_steps: 7) */
int ddimx_step_begin_ex(const float* coef, int row_stride, const int* step, int64_t* t, int B, void* stream);
int ddimx_ddim_update(float* xt, const float* et, const float* noise, float* x0, const float* coef, const int* step,
                      long long n, void* stream);
/* ddpm_steps update (functions/denoising.py:72-90): coef [n_iter][7] fp32 rows (t, (1/at).sqrt(), (1/at-1).sqrt(),
 * atm1.sqrt()*beta_t, (1-beta_t).sqrt()*(1-atm1), 1-at, mask*exp(0.5*log(beta_t))); x0 = clamp(x0 pred), xn = sample */
int ddimx_ddpm_update(const float* x, const float* et, const float* noise, float* x0, float* xn, const float* coef,
                      const int* step, long long n, void* stream);
int ddimx_step_end(int* step, void* stream);
/* Masked inpainting (ddim_audio_amd.inpaint_steps; the reference has no counterpart -- it is DPS, Chung et al. 2023, Algorithm 1,
 * per sample, with an element-wise mask operator) over NCHW fp32 [B][per_sample] tensors, in place on xt like ddim_update.
 * coef [n_iter][DDIMX_INPAINT_STRIDE] fp32 rows (t, s1 = sqrt(1-at), s2 = sqrt(at), s3 = sqrt(at_next), c2, c1, k1, k2, zeta):
 * columns 0-5 are ddim_update's, k1 = -2 s1/s2, k2 = 2/s2 and zeta the guidance scale of the row's step (schedule.
 * inpaint_coefficients); ddimx_step_begin_ex(coef, DDIMX_INPAINT_STRIDE, ...) fills t.  mask: fp32 in [0, 1], 1 = known;
 * y: the known content (0 where mask = 0).  Both kernels run a (blocks, B) grid: one fp32 partial of the squared residual per
 * (sample, block), reduced by every update block in one fixed order -- no atomics, bitwise reproducible.
 *   ddimx_inpaint_partials_floats: size of `partials` for (B, per_sample); -1 if per_sample is not a positive multiple of 4.
 *   ddimx_inpaint_residual (guided step, between the tape-keeping forward and ddimx_unet_bwd_ex(DDIMX_BWD_DATA_ONLY)):
 *     x0 = (xt - s1 eps) / s2 (ddim_update's rounding), r = mask (x0 - y), seed = k1 mask r (the backward's d_eps),
 *     partials = per-block sums of r^2.
 *   ddimx_inpaint_update: u = s3 x0 + c2 eps (+ c1 noise; noise nullable), ddim_update's operation order;
 *     DDIMX_INPAINT_GUIDED: x0 is read (the residual's), u -= zeta / sqrt(L_b) (k2 mask r + d_x) with L_b = the sample's sum of
 *       r^2 -- the gradient of L_b w.r.t. xt when d_x = J_eps^T seed; skipped when L_b = 0 or zeta = 0; without it, x0 is
 *       computed and written (a superset of ddim_update);
 *     DDIMX_INPAINT_REPLACE: k = s3 y + c2 eps (+ c1 noise), xt = mask k + (1 - mask) u: exactly u where mask = 0, k where 1;
 *     else xt = u.  y / mask are needed by either flag, d_x / partials by GUIDED.
 * Arguments are validated before the launch: nulls, 1 <= B <= 65535, per_sample % 4, flags against the buffers given. */
#define DDIMX_INPAINT_STRIDE 9
#define DDIMX_INPAINT_REPLACE 1
#define DDIMX_INPAINT_GUIDED 2
long long ddimx_inpaint_partials_floats(int B, long long per_sample);
int ddimx_inpaint_residual(const float* xt, const float* eps, const float* y, const float* mask, float* x0, float* seed,
                           float* partials, const float* coef, const int* step, int B, long long per_sample, void* stream);
int ddimx_inpaint_update(float* xt, const float* eps, const float* noise, float* x0, const float* y, const float* mask,
                         const float* d_x, const float* partials, const float* coef, const int* step, int B, long long per_sample,
                         int flags, void* stream);
/* Multistep ODE sampler (ddim_audio_amd.dpm_solver_steps; the reference has no counterpart -- it is DPM-Solver++ multistep in
 * data-prediction form, Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models",
 * orders 1-3) over fp32 tensors of n elements (n a positive multiple of 4), in place on xt like ddim_update.
 * coef [n_iter][DDIMX_SOLVER_STRIDE] fp32 rows (t, s1 = sqrt(1-at), s2 = sqrt(at), s3 = sqrt(at_next), c2, c1 = 0, w1, w2):
 * columns 0-5 are ddim_update's (eta = 0), w1 / w2 weight the differences of the last three x0 predictions (schedule.
 * dpm_coefficients; the order of an iteration lives in its row); ddimx_step_begin_ex(coef, DDIMX_SOLVER_STRIDE, ...) fills t.
 *   m0 = (xt - s1 eps) / s2, u = s3 m0 + c2 eps          (ddim_update's operations and rounding)
 *   u += w1 (m0 - m1)   when w1 != 0;   u += w2 (m1 - m2)   when w2 != 0     (one fma each, in this order)
 *   xt <- u, x0 <- m0, hist <- m1
 * with m1 = x0 on entry (the previous iteration's prediction) and m2 = hist on entry.  A row with w1 = w2 = 0 gives ddim_update's
 * bits whatever x0 / hist hold (they are uninitialised at the first iteration).  hist may be null when every row has w2 = 0
 * (orders 1 and 2): then no second history term is applied or kept.  No atomics: a sample's result does not depend on the batch.
 * Arguments are validated before the launch: nulls (hist excepted), n. */
#define DDIMX_SOLVER_STRIDE 8
int ddimx_multistep_update(float* xt, const float* eps, float* x0, float* hist, const float* coef, const int* step, long long n,
                           void* stream);
/* DDIM inversion with fixed-point refinement (ddim_audio_amd.invert_steps; the reference has no counterpart) over fp32
 * [B][per_sample] tensors, in place on xt.  The table has one row per NETWORK EVALUATION, in execution order (levels upwards,
 * `iters` rows per level): coef [rows][DDIMX_INVERT_STRIDE] fp32 (t, s1 = sqrt(1-a_i), s2 = sqrt(a_i), p = sqrt(a_i / a_j),
 * q = s1 - p sqrt(1-a_j), first) with i the level being solved for and j the level below it (a_j = 1, the data, under the first);
 * `first` is 1 on the first row of a level (schedule.invert_coefficients); ddimx_step_begin_ex(coef, DDIMX_INVERT_STRIDE, ...)
 * fills t.  With x_old = xt on entry and eps the network's output AT x_old, the row of step[0]:
 *   base <- x_old when `first` is set (the buffer's earlier content is never read then), else base is read;
 *   x0 = (x_old - s1 eps) / s2              (ddim_update's operations and rounding)
 *   xt <- p base + q eps                    (one product, one fma)
 *   log[step[0]][b] = |x_new - x_old|_2 / |x_new|_2 per sample (0 when the denominator is 0): the residual of the fixed-point
 *     iteration x = p base + q eps(x, t), whose solution is the point ddim_update maps to base.
 * The two sums are accumulated in double, per block into `partials` and then in one fixed order by a second small launch of the
 * same call: no atomics, bitwise reproducible; xt and x0 never depend on them, nor on the batch.  log is [rows][B] fp32; a counter
 * outside 0 .. rows - 1 makes the call a no-op on the device (nothing beyond the table or the log is touched).
 *   ddimx_invert_partials_doubles: size of `partials` in doubles for (B, per_sample) -- also enough for ddimx_slerp with P = B
 *     pairs; -1 if B is outside 1..65535 or per_sample is not a positive multiple of 4.
 * Spherical interpolation (the reference's `slerp`, runners/diffusion.py:427-432, per pair and on the device): z1, z2 [P][per_sample],
 * weights [M] fp32, out [P][M][per_sample]:
 *   cos(theta) = <z1_p, z2_p> / sqrt(|z1_p|^2 |z2_p|^2) over the whole sample (sums in double, fixed order; clamped to [-1, 1]),
 *   a_m = sin((1 - w_m) theta) / sin(theta), b_m = sin(w_m theta) / sin(theta) in double, each rounded once to fp32,
 *   out[p][m] = fma(b_m, z2_p, a_m * z1_p).
 * Where sin(theta) = 0 or an input is all zero (the reference's formula gives NaN) the straight line a_m = 1 - w_m, b_m = w_m.
 * w = 0 returns z1 and w = 1 returns z2 exactly.  Arguments are validated before the launch: nulls, 1 <= B or P <= 65535,
 * per_sample % 4, rows >= 1, M >= 1. */
#define DDIMX_INVERT_STRIDE 6
long long ddimx_invert_partials_doubles(int B, long long per_sample);
int ddimx_invert_update(float* xt, const float* eps, float* base, float* x0, double* partials, float* log, int rows,
                        const float* coef, const int* step, int B, long long per_sample, void* stream);
int ddimx_slerp(const float* z1, const float* z2, const float* weights, int M, float* out, double* partials, int P,
                long long per_sample, void* stream);
/* Seeded device noise (ddim_audio_amd.NoiseStream; stream definition, version 1): fills out[B][per_sample] from a counter-based
 * generator, so the value of element i of global sample s at draw k depends on (seed, s, k, i) only -- not on B, the shard, the
 * grid or the number of GPUs -- and the launch can be captured in a hipGraph.
 *   words   = Philox4x32-10 (Salmon et al., SC'11), key = (seed & 0xffffffff, seed >> 32),
 *             counter = (q, first_sample + b, draw, tag): q = i / 4 the group of four consecutive elements of the sample,
 *             draw = draw_base + (step ? step[0] : 0) with step (device int, nullable) read when the launch RUNS,
 *             tag = purpose (0: the noise a sampler step adds, 1: the initial x_T);
 *   normals = for the word pairs (w0, w1), (w2, w3): u = ((wa >> 8) + 1) 2^-24, v = (wb >> 8) 2^-23, r = sqrtf(-2 logf(u)),
 *             r cospi(v), r sinpi(v), fp32, every operation rounded on its own; element 4 q + j gets output j.
 *             |z| <= sqrt(48 ln 2) = 5.77: the tails are cut there (about 8e-9 per element).
 * kind DDIMX_NOISE_NORMALS writes fp32 normals, DDIMX_NOISE_WORDS the raw words as uint32.  The words are the contract, bit for
 * bit; the normals follow the device's logf / sincospif to their last bit (within 8 * 2^-24 * r of the exact values).
 * Arguments are validated before the launch: out, 1 <= B <= 65535, per_sample a positive multiple of 4 with at most 2^32 groups,
 * first_sample + B <= 2^32, kind. */
#define DDIMX_NOISE_NORMALS 0
#define DDIMX_NOISE_WORDS 1
int ddimx_noise_fill(void* out, int B, long long per_sample, unsigned long long seed, unsigned first_sample, const int* step,
                     unsigned draw_base, unsigned tag, int kind, void* stream);
/* Windowed long-form sampling (ddim_audio_amd.windowed_steps; the reference has no counterpart): one canvas [N][C][L][F] fp32 is
 * denoised through W = (L - T) / H + 1 overlapping windows of the network's length T, hop H (1 <= H <= T): window j of canvas
 * sample n is sample n W + j of the window batch [N W][C][T][F] and covers the canvas rows [j H, j H + T).
 *   ddimx_window_gather: win[n W + j][c][tau][:] = canvas[n][c][j H + tau][:], in 16-byte pieces (F % 4 == 0).
 *   ddimx_window_update: one DDIM update of the canvas, in place like ddim_update, from the window batch's noise predictions `eps`.
 *     The plan (schedule.window_plan) gives per canvas row l the first covering window jfirst[l], the number of covering windows
 *     cnt[l] in 1 .. K, K = ceil(T / H) <= DDIMX_WINDOW_MAX_COVER, and their normalised weights wt[k][l] ([K][L] fp32, k in
 *     ascending window order, summing to 1 over k < cnt; nullable when K = 1):
 *       e  = eps of window jfirst                                                          if cnt == 1 (no multiply),
 *       e  = fma(wt[cnt-1], eps[jfirst+cnt-1], ... fma(wt[1], eps[jfirst+1], wt[0] * eps[jfirst]))      otherwise,
 *       x0 = (x - s1 e) / s2, x = s3 x0 + c2 e (+ c1 noise; noise nullable, canvas-shaped): ddim_update's rounding and coefficient
 *     rows (coef [n_iter][6], the row of step[0]).  With H = T it is ddim_update bit for bit.  Window and row indices formed from
 *     the plan are clamped into the batch before any load.
 * Arguments are validated before the launch: nulls, N W in 1..65535, C, F % 4, 1 <= H <= T, L = T + (W - 1) H, K, and fewer than
 * 2^31 groups of four elements per canvas sample.  Neither result depends on N. */
#define DDIMX_WINDOW_MAX_COVER 8
int ddimx_window_gather(const float* canvas, float* win, int N, int W, int C, int L, int T, int H, int F, void* stream);
int ddimx_window_update(float* x, const float* eps, const float* noise, float* x0, const int* jfirst, const int* cnt, const float* wt,
                        const float* coef, const int* step, int N, int W, int C, int L, int T, int H, int F, void* stream);
/* Sampler pool (ddim_audio_amd.SamplerPool; the reference has no counterpart): the three launches that frame the forward of a batch
 * of n_slots samples [n_slots][per_sample] fp32 when every sample follows its own schedule from its own position -- continuous
 * batching.  They take the places of ddimx_step_begin_ex, ddimx_ddim_update / ddimx_multistep_update and ddimx_step_end.
 *   arena [n_slots][max_steps][DDIMX_POOL_STRIDE] fp32: slot b's coefficient rows (t, s1, s2, s3, c2, c1, w1, w2) in execution
 *     order -- schedule.dpm_coefficients as it stands, or schedule.ddim_coefficients (any eta) with w1 = w2 = 0;
 *   slots [n_slots][DDIMX_POOL_SLOT_WORDS] int32: pos, len, seed_lo, seed_hi, sample, draw_base, and two reserved words (the four
 *     noise words are unsigned values stored bit for bit).
 * Both are read when the launch RUNS.  Slot b is active iff 0 <= pos < len <= max_steps; an idle slot's xt, x0 and hist are neither
 * read nor written, and its arena rows are not read.
 *   ddimx_pool_begin:  t[b] = the t of row pos of slot b, 0 for an idle slot.
 *   ddimx_pool_update: for every active slot, on row pos, with m1 = x0[b] and m2 = hist[b] on entry:
 *       m0 = (xt - s1 eps) / s2, u = s3 m0 + c2 eps              (ddim_update's operations and rounding)
 *       u += w1 (m0 - m1) when w1 != 0;  u += w2 (m1 - m2) when w2 != 0    (multistep_update's, one fma each, in this order)
 *       u += c1 z when c1 != 0                                   (ddim_update's noise term, fma(z, c1, u))
 *       xt <- u, x0 <- m0, hist <- m1
 *     where z is the normal ddimx_noise_fill writes for (seed = seed_hi << 32 | seed_lo, sample, draw = draw_base + pos, tag 0)
 *     at that element, drawn inside the kernel: no noise buffer.  A row gives, bit for bit, what ddimx_ddim_update (after
 *     ddimx_noise_fill when c1 != 0) or ddimx_multistep_update gives for it; a sample's result depends on its own slot only.
 *   ddimx_pool_end:    pos += 1 for every active slot.
 * Arguments are validated before the launch: nulls, 1 <= n_slots <= 65535, max_steps >= 1, per_sample a positive multiple of 4 with
 * at most 2^32 groups. */
#define DDIMX_POOL_STRIDE 8
#define DDIMX_POOL_SLOT_WORDS 8
int ddimx_pool_begin(const float* arena, const int* slots, int64_t* t, int n_slots, int max_steps, void* stream);
int ddimx_pool_update(float* xt, const float* eps, float* x0, float* hist, const float* arena, const int* slots, int n_slots,
                      int max_steps, long long per_sample, void* stream);
int ddimx_pool_end(int* slots, int n_slots, int max_steps, void* stream);

/* ---- v-prediction (ddim_audio_amd/sampler.py, losses.py; Salimans & Ho 2022) ------------------------------------------
 * A network of model.type "v" predicts v = sqrt(a_t) e - sqrt(1 - a_t) x0; with s1 = sqrt(1 - a_t), s2 = sqrt(a_t) that is
 * x0 = s2 x - s1 v and e = s1 x + s2 v.
 *   ddimx_v_to_eps: eps[b] = fma(v[b], s2, x[b] * s1) per element -- two roundings, the product first -- with (s1, s2) = row t[b] of
 *     vtab, fp32 [n_table][2] (schedule.v_table).  x, v, eps are fp32 [B][per_sample]; eps may be v (in place).  t is the int64
 *     [B] timestep tensor the network was given, read when the launch RUNS, so one captured launch between the forward and the
 *     update kernel serves every sampler step.  A t[b] outside 0 .. n_table - 1 leaves eps[b] untouched and reads no row.  A
 *     sample's result does not depend on B.
 *   ddimx_qsample_v: x = x0 sqrt(a) + e sqrt(1 - a), bit for bit ddimx_qsample's, and the training target
 *     v = e sqrt(a) - x0 sqrt(1 - a) (each product and the difference rounded once), a = alphas[t[b]], from one read of x0 and e.
 * Arguments are validated before the launch: nulls, 1 <= B <= 65535, per_sample a positive multiple of 4, n_table >= 1. */
int ddimx_v_to_eps(const float* x, const float* v, float* eps, const float* vtab, int n_table, const int64_t* t, int B,
                   long long per_sample, void* stream);
int ddimx_qsample_v(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, float* v, int B,
                    long long per_sample, void* stream);

/* ---- training-step pieces (functions/losses.py:4-18, models/ema.py:16-23) ----------------------------
 * Arguments are validated before the launch: nulls, 1 <= B <= 65535 (the batch is a grid dimension), per_sample positive (these
 * kernels are scalar: any length).  A timestep lives in device memory and cannot be range-checked on the host: every t[b] must lie
 * in 0 .. (length of alphas) - 1, or ddimx_qsample reads outside alphas.
 * x[b] = x0[b] sqrt(a) + e[b] sqrt(1 - a), a = alphas[t[b]]: both products and the sum rounded separately */
int ddimx_qsample(const float* x0, const float* e, const float* alphas, const int64_t* t, float* x, int B,
                  long long per_sample, void* stream);
/* loss[0..B-1] = per-sample sum of squared error, loss[B] = batch mean; partial: [B*64] scratch */
int ddimx_sqerr_loss(const float* e, const float* out, float* partial, float* loss, int B, long long per_sample,
                     void* stream);
int ddimx_ema_block_elems(void);
/* shadow = c_param * param + c_shadow * shadow for a list of tensors in one launch (pointer tables on device; the two products and
 * the sum are rounded separately).  The reference evaluates (1.0 - mu) * p + mu * shadow with mu a Python double, so its two fp32
 * coefficients are c_param = fp32(1.0 - mu) and c_shadow = fp32(mu): pass those and the shadows carry the reference's bits.
 * Block tables: entry k is workgroup k, which updates elements blk_off[k] .. blk_off[k] + ddimx_ema_block_elems() - 1 (clipped to
 * sizes[...]) of tensor blk_tensor[k].  Validated before the launch: nulls, nblocks >= 0; nblocks = 0 launches nothing. */
int ddimx_ema_update_multi_coef(const long long* shadow_ptrs, const long long* param_ptrs, const long long* sizes,
                                const int* blk_tensor, const long long* blk_off, int nblocks, float c_param, float c_shadow,
                                void* stream);
/* the same with c_shadow = mu and c_param = fp32(1 - mu) formed from the fp32 mu: for mu = 0.9999 that is 1.00016594e-4, not the
 * reference's 1e-4, and about a fifth of the shadows differ from the reference in the last bit.  Kept for existing callers. */
int ddimx_ema_update_multi(const long long* shadow_ptrs, const long long* param_ptrs, const long long* sizes,
                           const int* blk_tensor, const long long* blk_off, int nblocks, float mu, void* stream);

/* ---- optimizer tail of train_step (runners/diffusion.py:155-173; functions/__init__.py:5-23) ------------------
 * Multi-tensor launches over device pointer tables (block tables as for ddimx_ema_update_multi).
 * grad_norm: out[0] = global L2 norm of all gradients, out[1] = min(1, max_norm/(norm+1e-6)) -- the coefficient of
 * torch.nn.utils.clip_grad_norm_ -- kept on the device (no host sync); partial: [nblocks] scratch.
 * adam: g *= clip[1] (if clip != null), then torch.optim.Adam (decoupled = 0) / AdamW (decoupled = 1), amsgrad off;
 * decoupled = 2: AdaBelief as published (Zhuang et al. 2020; decoupled decay, no rectification) -- the reference's default
 * optimizer (functions/__init__.py:24-42) comes from an un-vendored submodule, so this mode has no reference pin.
 * Arguments are validated before the launch: nulls (clip alone may be null), nblocks >= 0, step >= 1, decoupled in 0..2.  With
 * nblocks = 0 nothing is launched and nothing is written, out of ddimx_grad_norm_multi included. */
int ddimx_grad_norm_multi(const long long* grad_ptrs, const long long* sizes, const int* blk_tensor,
                          const long long* blk_off, int nblocks, float max_norm, float* partial, float* out, void* stream);
/* every tensor *= coef[0] (device scalar): the in-place scaling of clip_grad_norm_ */
int ddimx_scale_multi(const long long* ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                      int nblocks, const float* coef, void* stream);
int ddimx_adam_multi(const long long* param_ptrs, const long long* grad_ptrs, const long long* m_ptrs,
                     const long long* v_ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                     int nblocks, const float* clip, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int step, int decoupled, void* stream);
/* The same with the per-step scalars in device memory, dyn = {lr, 1 - beta1^step, sqrt(1 - beta2^step)} (fp32), read when
 * the kernel RUNS: a training step captured once into a hipGraph is replayed with new values written to dyn between replays
 * (LambdaLR, functions/__init__.py:53-60, and the bias corrections change every step). */
int ddimx_adam_multi_dyn(const long long* param_ptrs, const long long* grad_ptrs, const long long* m_ptrs,
                         const long long* v_ptrs, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                         int nblocks, const float* clip, const float* dyn, float beta1, float beta2, float eps,
                         float weight_decay, int decoupled, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDIMX_H */
