// Building blocks of the network walks: Residual_Block forward and backward (with the side-stream weight-gradient scheduler),
// timestep embedding, the FNet bottleneck in its inference and training forms, Down / Upsample backward.
#include "host.h"

// Residual_Block (models/diffusion.py:42-56), called by name (RBCall, host.h).  The stats of x must already be in `stats`
// ([B][x_nparts][x_Cs][2]).  On return, if want_stats, `stats` holds those of y (*y_nparts, Cs = C).
// tape != null: training forward -- the convs store their PRE-activation outputs (u1 = conv0 + temb, u2 = conv1 + bias)
// in the tape and the consumers apply SiLU while loading; the result is the same function of the same inputs.
// stats2 != null (inference walk, no tape): launch-free GroupNorm (gn_fused.h).  All partials are in group format
// ([B][np][8][2], x_Cs unused), every consumer finishes its input's normalisation itself, and the two buffers alternate
// because a kernel now reads its input's partials while it writes its output's: x in `stats` -> conv0 -> `stats2` ->
// conv1 -> `stats` -> resid -> `stats2` = those of y (the caller swaps).  Samples with more than kGnFuseMaxParts partials
// (long spectrograms, shallow levels) take one gn_finalize_groups launch instead, per GroupNorm.
// The two convs of Residual_Block on the launch-free inference path (group-format statistics; GroupNorm input set by the caller):
// which = 0: conv(SiLU(GN0(x))) + temb, which = 1: conv(GN1(h)) + bias, both with a SiLU output.
ConvCall rb_conv_call(int dtype, int C, int which, const void* in, const void* w, const void* wf, const float* bias,
                      const float* temb, int temb_stride, float* scale, float* shift, void* out, float* stats, int B, int H, int W) {
    ConvCall q = conv3_call(dtype, C, in, w, out, B, H, W);
    if (which) {
        q.bias = bias;
    } else {
        q.chan_add = temb;
        q.chan_add_stride = temb_stride;
    }
    q.in_scale = scale;
    q.in_shift = shift;
    q.xf = which ? XF_AFFINE : XF_AFFINE_SILU;
    q.act = 1;
    q.stats = stats;
    q.groups = true;
    q.wf = wf;
    return q;
}

// Statistics floats a Residual_Block level can need: its convs' partials and the residual pass's, one per-channel slab each --
// group_floor (the launch-free path, gn_fused.h): or one kGnSlab-float group slab where that is more
static inline size_t slab_floats(int C, bool group_floor) { return (size_t)(group_floor && C * 2 < kGnSlab ? kGnSlab : C * 2); }
size_t rb_stats_floats(int dtype, int B, int C, int H, int W, bool group_floor) {
    // (a conv's group slabs never exceed its per-channel ones)
    return std::max(conv_stats_floats(dtype, CONV3, C, C, B, H, W), (size_t)B * resid_nparts(dtype, H * W, C) * slab_floats(C, group_floor));
}
// ... and a whole forward walk at (B, T): the input conv, every level's blocks, the Downsample into it and the Upsample out of it.
// Every term is B x (a per-sample slab count).
size_t walk_stats_floats(const ddimx_ctx* c, int B, int T, bool group_floor) {
    const ddimx_config& f = c->cfg;
    size_t mx = (size_t)B * conv_in_nparts(T, f.f_size) * slab_floats(f.ch[0], group_floor);
    for (int l = 0; l < c->L; ++l) {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        mx = std::max(mx, rb_stats_floats(c->dtype, B, C, H, W, group_floor));
        if (l > 0) mx = std::max({mx, conv_stats_floats(c->dtype, DOWN4, f.ch[l - 1], C, B, H, W), conv_stats_floats(c->dtype, UP4, C, f.ch[l - 1], B, H, W)});
    }
    return mx;
}

int run_resblock(const RBCall& q, int* y_nparts) {
    const int dtype = q.dtype, C = q.C, B = q.B, H = q.H, W = q.W;
    const RBPtrs& p = q.p;
    const RBTape* const tape = q.tape;
    float *const stats = q.stats, *const stats2 = q.stats2, *const scale = q.scale, *const shift = q.shift;
    void *h1 = q.h1, *h2 = q.h2;
    hipStream_t const s = q.s;
    const double cnt = (double)H * W * (C / kGroups);
    const float eps = 1e-6f;
    int np = 0, cs = 0;
    if (stats2) {
        if (tape) return fail("run_resblock: the launch-free GroupNorm path keeps no tape");
        // GroupNorm input of one consumer: finished inside the consumer, or -- scale / shift from one launch -- when the sample
        // has too many partials, or when the consumer launch fills the chip so many times over that its per-workgroup prologue
        // (about a microsecond per round) costs more than the launch it saves (large batches).  Either way the numbers are the
        // same bit for bit: gn_finalize_groups runs the consumer's own reduction with the consumer's block size.
        auto gn_of = [&](const float* st, int n, const float* gamma, const float* beta, GnIn* g, bool* fused, int rounds,
                         int max_rounds, int nthreads) -> int {
            *g = GnIn{st, gamma, beta, 1.0 / cnt, eps, n};
            *fused = gn_fuse(n, rounds, max_rounds);
            if (!*fused) HIPCHK(gn_finalize_groups_launch(*g, C, scale, shift, B, nthreads, s));
            return 0;
        };
        GnIn g; bool fu;
        // (each conv is planned exactly as run_conv will plan it -- kernel family, block size -- BEFORE its GroupNorm input is
        // decided: the finalize launch must reduce with the block size of the kernel that would otherwise do it in its prologue)
        ConvCall k1 = rb_conv_call(dtype, C, 0, q.x, p.w0, p.w0f, nullptr, q.temb, q.temb_stride, scale, shift, h1, stats2, B, H, W);
        ConvPlan pl;
        CHK(conv_plan(k1, &pl));
        CHK(gn_of(stats, q.x_nparts, p.g0, p.b0, &g, &fu, conv_rounds(pl, B), kGnFuseConvRounds, pl.g.nthreads));
        if (fu) k1.gn = g;
        CHK(run_conv(k1, s, &np, &cs));
        ConvCall k2 = rb_conv_call(dtype, C, 1, h1, p.w1, p.w1f, p.bias1, nullptr, 0, scale, shift, h2, stats, B, H, W);
        CHK(conv_plan(k2, &pl));
        CHK(gn_of(stats2, np, p.g1, p.b1, &g, &fu, conv_rounds(pl, B), kGnFuseConvRounds, pl.g.nthreads));
        if (fu) k2.gn = g;
        CHK(run_conv(k2, s, &np, &cs));
        const int rparts = resid_nparts(dtype, H * W, C);
        CHK(gn_of(stats, np, p.g2, nullptr, &g, &fu, resid_rounds(dtype, C, B, H, W), kGnFuseResidRounds, resid_threads(dtype, C)));
        HIPCHK(resid_launch(dtype, q.x, h2, 0, scale, shift, q.y, q.want_stats ? stats2 : nullptr, B, H * W, C, s, fu ? &g : nullptr, 1));
        if (y_nparts) *y_nparts = rparts;
        return 0;
    }
    float *sc0 = scale, *sh0 = shift, *sc1 = scale, *sh1 = shift, *sc2 = scale, *sh2 = shift;
    float *mr0 = nullptr, *mr1 = nullptr, *mr2 = nullptr;
    if (tape) {
        sc0 = tape->sc(0, B, C); sh0 = tape->sh(0, B, C); sc1 = tape->sc(1, B, C); sh1 = tape->sh(1, B, C);
        sc2 = tape->sc(2, B, C); sh2 = tape->sh(2, B, C);
        mr0 = tape->mr(0, B, C); mr1 = tape->mr(1, B, C); mr2 = tape->mr(2, B, C);
        h1 = tape->u1; h2 = tape->u2;
    }
    const int act = tape ? 2 : 1;
    HIPCHK(gn_finalize_launch(stats, q.x_nparts, q.x_Cs, C, cnt, p.g0, p.b0, eps, sc0, sh0, B, s, mr0));
    ConvCall k1 = conv3_call(dtype, C, q.x, p.w0, h1, B, H, W);
    k1.chan_add = q.temb; k1.chan_add_stride = q.temb_stride;
    k1.in_scale = sc0; k1.in_shift = sh0; k1.xf = XF_AFFINE_SILU; k1.act = act;
    k1.stats = stats;
    CHK(run_conv(k1, s, &np, &cs));
    HIPCHK(gn_finalize_launch(stats, np, cs, C, cnt, p.g1, p.b1, eps, sc1, sh1, B, s, mr1));
    ConvCall k2 = conv3_call(dtype, C, h1, p.w1, h2, B, H, W);
    k2.bias = p.bias1;
    k2.in_scale = sc1; k2.in_shift = sh1; k2.xf = tape ? XF_SILU_AFFINE : XF_AFFINE; k2.act = act;
    k2.stats = stats;
    CHK(run_conv(k2, s, &np, &cs));
    HIPCHK(gn_finalize_launch(stats, np, cs, C, cnt, p.g2, nullptr, eps, sc2, sh2, B, s, mr2));
    HIPCHK(resid_launch(dtype, q.x, h2, tape ? 2 : 0, sc2, sh2, q.y, q.want_stats ? stats : nullptr, B, H * W, C, s));
    if (y_nparts) *y_nparts = resid_nparts(dtype, H * W, C);
    return 0;
}

static int push_colsum(const RBBwdWs& w, const float* src, int B, long long stride, int C, float* dst, hipStream_t s) {
    if (w.data_only) return 0;
    if (!w.defer) { HIPCHK(colsum_launch(src, B, stride, C, dst, s)); return 0; }
    ColsumBatch& q = *w.defer;
    q.src[q.count] = src; q.dst[q.count] = dst; q.stride[q.count] = stride; q.B[q.count] = B; q.C[q.count] = C;
    ++q.count;  // the caller flushes before the slots are reused (capacity is checked there)
    return 0;
}

// The data-gradient convs take the GroupNorm-backward partial sums of their own output in their epilogue (ConvCfg::BWD:
// one more read of u1 / x there instead of a pass over dg and u1 / x); the slab count is then the conv's, not resid's.
// Sets d up for it and returns the slab count in *nparts, or leaves d alone and returns 0 there: the statistics pass then runs
// on its own.  np_resid: slabs per sample `stats` is sized for (resid's partition).
int dgrad_fused_stats(ConvCall& d, const void* aux, const float* asc, const float* ash, int mode, float* stats, int np_resid,
                      int* nparts) {
    ConvPlan pl;
    CHK(conv_plan(d, &pl));
    *nparts = pl.wgs_per_sample * pl.g.classes;
    if (*nparts > np_resid) { *nparts = 0; return 0; }  // (slabs are sized for resid's partition)
    d.aux = aux; d.aux_scale = asc; d.aux_shift = ash; d.bwd_mode = mode; d.stats = stats;
    return 0;
}

// Backward of Residual_Block (autograd of models/diffusion.py:42-56).  dy -> dx (+ extra if given); parameter
// gradients are WRITTEN (not accumulated).  wd0 / wd1: data-gradient packings of conv.0 / conv.1.
int run_resblock_bwd(int dtype, int C, const void* x, const RBTape& tp, const void* dy, const void* extra, void* dx,
                     const float* gam0, const float* gam1, const float* gam2, const void* wd0, const void* wd1,
                     const RBGrads& gr, const RBBwdWs& w, int B, int H, int W, hipStream_t s, WgSide* sd, bool stats_ready,
                     const void* next_u2) {
    const int HW = H * W;
    const double cnt = (double)HW * (C / kGroups);
    const int np = resid_nparts(dtype, HW, C);
    const bool side = sd && sd->on();
    void* const* hold = side ? sd->hold : nullptr;         // this block's weight gradients wait for the bottleneck
    const int par = side && !hold ? (sd->blk++ & 1) : 0;
    void* const du2 = hold ? hold[0] : (side ? sd->du[2 * par] : w.du);      // gradient of conv.1's output / of conv.0's output
    void* const du1 = hold ? hold[1] : (side ? sd->du[2 * par + 1] : w.du);
    hipStream_t const sw = side ? sd->st : s;              // the weight gradients' stream
    float* const wpart = side ? sd->partial : w.partial;
    const bool early = side && sd->early_block && !hold;
    const void* const u1 = tp.u1;
    const float *const sc1 = tp.sc(1, B, C), *const sh1 = tp.sh(1, B, C), *const sc0 = tp.sc(0, B, C), *const sh0 = tp.sh(0, B, C);
    float *const gw1 = gr.w1, *const gw0 = gr.w0;
    auto wgrad1 = [=]() { return run_wgrad(dtype, CONV3, C, C, u1, du2, sc1, sh1, XF_SILU_AFFINE, wpart, gw1, B, H, W, sw); };
    auto wgrad0 = [=]() { return run_wgrad(dtype, CONV3, C, C, x, du1, sc0, sh0, XF_AFFINE_SILU, wpart, gw0, B, H, W, sw); };
    float* const slot0 = w.slots ? w.slots : w.dgb;  // [B][2][C] each; with deferral every use keeps its own slot
    const size_t slot_f = (size_t)B * 2 * C;
    float* const dgb2 = slot0;
    float* const sumb = w.slots ? slot0 + slot_f : w.dgb;
    float* const dgb1 = w.slots ? slot0 + 2 * slot_f : w.dgb;
    float* const dgb0 = w.slots ? slot0 + 3 * slot_f : w.dgb;
    // ---- GN2 (fed by SiLU(u2), weight only) and the SiLU in front of it: du2
    // (stats_ready: the kernel that produced dy -- the previous block's last apply pass -- has left these slabs in w.stats)
    if (!stats_ready) HIPCHK(gn_bwd_stats_launch(dtype, 0, dy, tp.u2, nullptr, nullptr, w.stats, B, HW, C, s));
    HIPCHK(gn_bwd_finalize_launch(w.stats, np, C, cnt, gam2, tp.mr(2, B, C), w.coef, dgb2, B, s));
    CHK(push_colsum(w, dgb2, B, 2 * C, C, gr.g2, s));
    if (side && !hold) CHK(sd->claim(par, s));
    // (the per-sample channel sums of du2 / du1 feed conv.1.bias and the timestep embedding only: not taken in data-only mode)
    float* const sums_a = w.data_only ? nullptr : (w.pdefer ? w.sums2 : w.sums);
    float* const sums_b = w.data_only ? nullptr : (w.pdefer ? w.sums2 + w.sums_f : w.sums);
    auto psum = [&](const float* src, float* dst, long long stride) -> int {
        if (w.data_only) return 0;
        if (!w.pdefer) { HIPCHK(partsum_launch(src, B, np, C, dst, stride, s)); return 0; }
        PartsumBatch& q = *w.pdefer;
        if (q.count >= PartsumBatch::kMax) return fail("partsum queue overflow");
        q.src[q.count] = src; q.dst[q.count] = dst; q.dst_stride[q.count] = stride; q.nparts[q.count] = np; q.C[q.count] = C; q.B[q.count] = B;
        ++q.count;
        return 0;
    };
    HIPCHK(gn_bwd_apply_launch(dtype, 0, dy, tp.u2, nullptr, nullptr, w.coef, nullptr, nullptr, du2, sums_a, B, HW, C, s));
    CHK(psum(sums_a, sumb, C));                                     // per-sample channel sums of du2
    CHK(push_colsum(w, sumb, B, C, C, gr.bias1, s));                // conv.1.bias
    // ---- conv.1: weight gradient against GN1(SiLU(u1)), data gradient -> dg
    if (early) CHK(sd->fork(s));
    if (!w.data_only && (!side || early)) CHK(wgrad1());
    ConvCall d1 = conv3_call(dtype, C, du2, wd1, w.dg, B, H, W);
    int np1 = 0;
    CHK(dgrad_fused_stats(d1, tp.u1, nullptr, nullptr, 1, w.stats, np, &np1));
    CHK(run_conv(d1, s, nullptr, nullptr));
    // ---- GN1 (fed by SiLU(u1)) and the SiLU in front of it: du1
    if (!np1) { HIPCHK(gn_bwd_stats_launch(dtype, 0, w.dg, tp.u1, nullptr, nullptr, w.stats, B, HW, C, s)); np1 = np; }
    HIPCHK(gn_bwd_finalize_launch(w.stats, np1, C, cnt, gam1, tp.mr(1, B, C), w.coef, dgb1, B, s));
    CHK(push_colsum(w, dgb1, B, 2 * C, C, gr.g1, s));
    CHK(push_colsum(w, dgb1 + C, B, 2 * C, C, gr.b1, s));
    HIPCHK(gn_bwd_apply_launch(dtype, 0, w.dg, tp.u1, nullptr, nullptr, w.coef, nullptr, nullptr, du1, sums_b, B, HW, C, s));
    if (gr.dtemb) CHK(psum(sums_b, gr.dtemb, gr.dtemb_stride));     // timestep-embedding chunk
    // ---- conv.0: weight gradient against SiLU(GN0(x)), data gradient -> dg
    if (early) CHK(sd->fork(s));
    if (!w.data_only && (!side || early)) CHK(wgrad0());
    ConvCall d0 = conv3_call(dtype, C, du1, wd0, w.dg, B, H, W);
    int np0 = 0;
    CHK(dgrad_fused_stats(d0, x, tp.sc(0, B, C), tp.sh(0, B, C), 2, w.stats, np, &np0));
    CHK(run_conv(d0, s, nullptr, nullptr));
    if (hold) {
        sd->held.push_back(wgrad1);
        sd->held.push_back(wgrad0);
    } else if (side && !early) {  // both weight gradients behind the last data-gradient conv: beside the HBM-bound passes that follow
        CHK(sd->fork(s));
        CHK(wgrad1());
        CHK(wgrad0());
    }
    if (side && !hold) CHK(sd->release(par));
    // ---- SiLU behind GN0, GN0 itself, and the identity path
    if (!np0) { HIPCHK(gn_bwd_stats_launch(dtype, 1, w.dg, x, tp.sc(0, B, C), tp.sh(0, B, C), w.stats, B, HW, C, s)); np0 = np; }
    HIPCHK(gn_bwd_finalize_launch(w.stats, np0, C, cnt, gam0, tp.mr(0, B, C), w.coef, dgb0, B, s));
    CHK(push_colsum(w, dgb0, B, 2 * C, C, gr.g0, s));
    CHK(push_colsum(w, dgb0 + C, B, 2 * C, C, gr.b0, s));
    // next_u2: dx is the dy of a block of the same shape whose saved u2 this is -- its first statistics pass rides this kernel
    HIPCHK(gn_bwd_apply_launch(dtype, 1, w.dg, x, dy, extra, w.coef, tp.sc(0, B, C), tp.sh(0, B, C), dx, nullptr, B, HW, C, s,
                               next_u2, next_u2 ? w.stats : nullptr));
    return 0;
}

RBPtrs rb_ptrs(const ddimx_ctx* c, const void* packed, const RBW& r) {
    RBPtrs p;
    p.g0 = pf(c, packed, r.g0); p.b0 = pf(c, packed, r.b0); p.g1 = pf(c, packed, r.g1); p.b1 = pf(c, packed, r.b1);
    p.g2 = pf(c, packed, r.g2); p.bias1 = pf(c, packed, r.bias1);
    p.w0 = pv(c, packed, r.w0); p.w1 = pv(c, packed, r.w1);
    p.w0f = frag_of(c, packed, r.w0);  // (a block has both copies or neither)
    p.w1f = frag_of(c, packed, r.w1);
    return p;
}

int run_temb(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1,
             const float* b1, const float* w2, const float* b2, float* h1, float* h2, float* out, int B,
             int pos_ch, int emb_ch, int E, hipStream_t s) {
    HIPCHK(linear_rows_launch(te, t, w0, b0, h1, B, emb_ch, pos_ch, 1, s));
    HIPCHK(linear_rows_launch(h1, nullptr, w1, b1, h2, B, emb_ch, emb_ch, 1, s));
    HIPCHK(linear_rows_launch(h2, nullptr, w2, b2, out, B, E, emb_ch, 0, s));
    return 0;
}
// ... in training: the pre-activations are kept (models/diffusion.py:110-120) and the consumers apply SiLU while loading
int run_temb_train(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1, const float* b1,
                   const float* w2, const float* b2, float* h1_pre, float* h2_pre, float* out, int B, int pos_ch, int emb_ch, int E,
                   hipStream_t s) {
    HIPCHK(linear_rows_launch(te, t, w0, b0, h1_pre, B, emb_ch, pos_ch, 0, s));
    HIPCHK(linear_rows_launch(h1_pre, nullptr, w1, b1, h2_pre, B, emb_ch, emb_ch, 0, s, 1));
    HIPCHK(linear_rows_launch(h2_pre, nullptr, w2, b2, out, B, E, emb_ch, 0, s, 1));
    return 0;
}
// ... and its backward: d_out [B][E] -> the three layers' weight / bias gradients (d_h2, d_h1: scratch [B][emb_ch])
int run_temb_bwd(const float* d_out, const float* te, const int64_t* t, const float* w1, const float* w2, const float* h1_pre,
                 const float* h2_pre, float* d_h2, float* d_h1, float* d_w0, float* d_b0, float* d_w1, float* d_b1, float* d_w2,
                 float* d_b2, int B, int pos_ch, int emb_ch, int E, hipStream_t s) {
    HIPCHK(linear_bwd_w_launch(d_out, h2_pre, nullptr, d_w2, d_b2, B, E, emb_ch, 1, s));
    HIPCHK(linear_bwd_x_launch(d_out, w2, h2_pre, d_h2, B, E, emb_ch, s));
    HIPCHK(linear_bwd_w_launch(d_h2, h1_pre, nullptr, d_w1, d_b1, B, emb_ch, emb_ch, 1, s));
    HIPCHK(linear_bwd_x_launch(d_h2, w1, h1_pre, d_h1, B, emb_ch, emb_ch, s));
    HIPCHK(linear_bwd_w_launch(d_h1, te, t, d_w0, d_b0, B, emb_ch, pos_ch, 0, s));
    return 0;
}

// ---- the FNet bottleneck: its GEMM call, its split-K scratch, the Fourier mixing, then the inference and training forms
// A GEMM (gemm_nt, gemm.h) over `partial`, its split-K chosen from ONE sample's rows (0: M itself -- batched GEMMs, the backward's)
static GemmArgs gemm_split(GemmArgs g, float* partial, int rows_per_sample) {
    g.partial = partial;
    g.splitk = sample_splitk(rows_per_sample > 0 ? rows_per_sample : g.M, g.N, g.K, g.bf16);
    return g;
}
int run_gemm(const GemmArgs& g, float* partial, int rows_per_sample, hipStream_t s) {
    HIPCHK(gemm_launch(gemm_split(g, partial, rows_per_sample), s));
    return 0;
}
// Floats of split-K scratch the GEMMs of this file can need at B samples of S tokens: the forward's six shapes (run_fnet,
// fnet_fwd_train_part, fourier_mix), `backward`: and fnet_bwd_part's four weight gradients, which contract over the tokens (its data
// gradients have the forward's shapes).  Sized for the cap; the forward's shapes all have B in their row or batch count (shards).
size_t fnet_partial_floats(const ddimx_ctx* c, int B, int S, bool backward) {
    const int M = B * S, hid = c->cfg.fnet_hidden, inter = c->cfg.fnet_inter, width = c->width;
    const int shp[10][3] = {{M, hid, 1}, {2 * hid, S, B}, {S, hid, B}, {M, inter, 1}, {M, hid, 1}, {M, width, 1},  // {M, N, batch}
                            {width, hid, 1}, {hid, inter, 1}, {inter, hid, 1}, {hid, width, 1}};
    size_t mx = 0;
    for (int i = 0; i < (backward ? 10 : 6); ++i) mx = std::max(mx, (size_t)kMaxSplitK * shp[i][2] * shp[i][0] * shp[i][1]);
    return mx;
}
// Z[b] = Re(FFT2(X[b])) + X[b] over [B][S][hid] token matrices (linear and symmetric: also its own backward).  fused: one launch
// (fnet_mix_supported), else two GEMMs on the exact fp32 MFMA through Ut [B][2 hid][S] and the split-K scratch
int fourier_mix(const float* dft_hidden, const float* dft_seq, const float* X, float* Z, float* Ut, float* partial, int B, int S, int hid,
                bool fused, hipStream_t s) {
    if (fused) {
        HIPCHK(fnet_mix_launch(dft_hidden, dft_seq, X, Z, B, S, hid, s));
        return 0;
    }
    // Ut[b] = D_H * X[b]^T -> [2*hid][S]; D_H rows interleaved (2k: cos_k, 2k+1: sin_k), so that row pair k of
    // Ut[b] is one contiguous K-vector [cos-part(S) | sin-part(S)] for the sequence transform
    GemmArgs g = gemm_nt(dft_hidden, X, Ut, 2 * hid, S, hid);
    g.batch = B; g.sB = (long long)S * hid; g.sC = (long long)2 * hid * S;
    CHK(run_gemm(g, partial, 0, s));
    // Z[b] = [C_S | -S_S] * Ut[b]^T + X[b]   (Re(FFT2) + residual) in one GEMM with K = 2S
    g = gemm_nt(dft_seq, Ut, Z, S, hid, 2 * S);
    g.resid = X; g.batch = B; g.sB = (long long)2 * hid * S; g.sC = (long long)S * hid;
    return run_gemm(g, partial, 0, s);
}

// Transformer_Module (models/diffusion.py:131-167 + transformers modeling_fnet.py:138-279), eval mode.
// x: NHWC bottleneck activation viewed as tokens [B*S][width]; writes O [B*S][width] fp32.
// Dense-weight GEMMs use bf16 MFMA in bf16 mode; the DFT factors always run on the exact fp32 MFMA.
int run_fnet(const ddimx_ctx* c, const void* packed, const ddimx_tables* tb, const FnetWs& w, const void* x, int B, int S, hipStream_t s) {
    const ddimx_config& f = c->cfg;
    const int hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width, M = B * S;
    const float eps = f.fnet_ln_eps;
    const int bf = c->fnet_bf16;
    const bool dense = c->fx_on && c->fx_packed == packed && fnet_mix_supported(S, hid) &&
                       fnet_dense_supported(S, hid, inter) && fnet_dense_supported(S, inter, hid) && fnet_dense_supported(S, width, hid) &&
                       fnet_dense_supported(S, hid, width);
    HIPCHK(layernorm_launch(c->dtype, x, tb->posenc, S, pf(c, packed, c->ln0_w), pf(c, packed, c->ln0_b), eps, w.ln0, M,
                            width, s, dense ? S : 0));
    if (dense) {
        // Three launches per layer instead of six (fnet_dense.hip): the Fourier mixing normalises its input rows on the fly (the
        // previous layer's output LayerNorm: statistics from that layer's last kernel, gamma folded into a per-layer DFT table)
        // and emits the row statistics of its output; the first FFN matrix normalises its operand from them (gamma / beta folded
        // into the packed weights) and applies bias + gelu_new; the second adds bias and the recomputed LayerNorm(Z) residual
        // and emits the statistics of ITS output; compute_out absorbs the last output LayerNorm the same way.
        const char* pk = (const char*)packed;
        const int npz = hid / 16, npv = hid / 32;
        FnetDenseArgs d;
        memset(&d, 0, sizeof(d));
        d.eps = eps; d.S = S;
        d.W = pk + c->fx_proj; d.bias = pf(c, packed, c->proj_b); d.X = w.ln0; d.x_chunk = 1; d.out = w.vc; d.out_chunk = 1; d.K = width; d.N = hid;
        HIPCHK(fnet_dense_launch(d, B, bf, s));
        for (int i = 0; i < f.fnet_layers; ++i) {
            const ddimx_ctx::FL& L = c->fl[i];
            const ddimx_ctx::FX& X = c->fx[i];
            FnetMixArgs m;
            memset(&m, 0, sizeof(m));
            m.tab = (const float*)(pk + X.tab); m.dft_seq = tb->dft_seq; m.V = w.vc; m.zc = w.zc; m.zstats = w.pz; m.eps = eps; m.S = S; m.hid = hid;
            if (i > 0) {
                m.vstats = w.pv; m.gamma = pf(c, packed, c->fl[i - 1].ln2_w); m.beta = pf(c, packed, c->fl[i - 1].ln2_b);
                m.bc = (const float*)(pk + X.bc);
            }
            HIPCHK(fnet_mix2_launch(m, B, s));
            memset(&d, 0, sizeof(d));
            d.eps = eps; d.S = S;
            d.W = pk + X.w1f; d.bias = (const float*)(pk + X.b1f); d.X = w.zc; d.x_chunk = 1; d.xstats = w.pz; d.xnp = npz; d.xn = 16;
            d.out = w.hc; d.out_chunk = 1; d.out_bf16 = bf; d.act = 1; d.K = hid; d.N = inter;
            HIPCHK(fnet_dense_launch(d, B, bf, s));
            memset(&d, 0, sizeof(d));
            d.eps = eps; d.S = S;
            d.W = pk + X.w2c; d.bias = pf(c, packed, L.b2); d.X = w.hc; d.x_chunk = 1; d.x_bf16 = bf; d.K = inter; d.N = hid;
            d.out = w.vc; d.out_chunk = 1; d.ostats = w.pv;
            d.R = w.zc; d.rstats = w.pz; d.rgamma = pf(c, packed, L.ln1_w); d.rbeta = pf(c, packed, L.ln1_b); d.rnp = npz; d.rn = 16;
            HIPCHK(fnet_dense_launch(d, B, bf, s));
        }
        memset(&d, 0, sizeof(d));
        d.eps = eps; d.S = S;
        d.W = pk + c->fx_coutf; d.bias = (const float*)(pk + c->fx_coutb); d.X = w.vc; d.x_chunk = 1; d.xstats = w.pv; d.xnp = npv; d.xn = 32;
        d.out = w.O; d.K = hid; d.N = width;
        HIPCHK(fnet_dense_launch(d, B, bf, s));
        return 0;
    }
    // a dense-weight layer over the tokens: C = A W^T + bias (act 1: gelu_new), split from one sample's S rows
    auto linear = [&](const float* A, int wi, int bi, float* C, int N, int K, int act) -> int {
        GemmArgs g = gemm_nt(A, pf(c, packed, wi), C, M, N, K);
        g.bias = pf(c, packed, bi); g.act = act; g.bf16 = bf;
        return run_gemm(g, w.gpart, S, s);
    };
    CHK(linear(w.ln0, c->proj_w, c->proj_b, w.X, hid, width, 0));
    float* cur = w.X;
    float* other = w.Y;
    for (int i = 0; i < f.fnet_layers; ++i) {
        const ddimx_ctx::FL& L = c->fl[i];
        CHK(fourier_mix(tb->dft_hidden, tb->dft_seq, cur, w.Z, w.Ut, w.gpart, B, S, hid, fnet_mix_supported(S, hid), s));
        HIPCHK(layernorm_launch(DT_F32, w.Z, nullptr, 1, pf(c, packed, L.ln1_w), pf(c, packed, L.ln1_b), eps, other, M, hid, s));
        // FFN; the second GEMM's split-K reduce also applies bias, residual and output.LayerNorm
        CHK(linear(other, L.w1, L.b1, w.Hb, inter, hid, 1));
        GemmArgs g = gemm_nt(w.Hb, pf(c, packed, L.w2), w.Z, M, hid, inter);
        g.bias = pf(c, packed, L.b2); g.resid = other; g.bf16 = bf;
        HIPCHK(gemm_ln_launch(gemm_split(g, w.gpart, S), pf(c, packed, L.ln2_w), pf(c, packed, L.ln2_b), eps, cur, s));
    }
    return linear(cur, c->cout_w, c->cout_b, w.O, width, hid, 0);
}

// Transformer_Module in training mode (models/diffusion.py:148-167 with the FNet layers of modeling_fnet.py:138-279): tokens
// `x` (NHWC bottleneck activation = [B*S][width] rows) -> w.O [B*S][width] fp32, keeping the tape rows the backward needs.
int fnet_fwd_train_part(const ddimx_ctx* c, const void* packed, const ddimx_tables* tables, const TrainWs& w, const TrainTape& tp,
                        const void* x, int B, int S, float dropout_p, unsigned long long seed, hipStream_t s) {
    const ddimx_config& f = c->cfg;
    const int dt = c->dtype;
    const int hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width, M = B * S;
    const float eps_ln = f.fnet_ln_eps;
    const int bf = c->fnet_bf16;
    HIPCHK(ln_train_launch(dt, x, tables->posenc, S, pf(c, packed, c->ln0_w), pf(c, packed, c->ln0_b), eps_ln, tp.ln0, nullptr,
                           tp.ln0_stat, M, width, 0.f, seed, 0, s, c->dropout_ctr));
    // a dense-weight layer over the tokens: C = A W^T + bias, split from one sample's S rows
    auto linear = [&](const float* A, int wi, int bi, float* C, int N, int K) -> int {
        GemmArgs g = gemm_nt(A, pf(c, packed, wi), C, M, N, K);
        g.bias = pf(c, packed, bi); g.bf16 = bf;
        return run_gemm(g, w.gpart, S, s);
    };
    CHK(linear(tp.ln0, c->proj_w, c->proj_b, tp.X0, hid, width));
    if (dropout_p > 0.f) HIPCHK(dropout_apply_launch(tp.X0, tp.X0, (long long)M * hid, dropout_p, seed, 0, s, c->dropout_ctr));
    const float* xc = tp.X0;
    for (int i = 0; i < f.fnet_layers; ++i) {
        const ddimx_ctx::FL& Lw = c->fl[i];
        const TrainTape::FLT& q = tp.fl[i];
        CHK(fourier_mix(tables->dft_hidden, tables->dft_seq, xc, q.Z, w.Ut, w.gpart, B, S, hid, fnet_mix_supported(S, hid), s));
        HIPCHK(ln_train_launch(DT_F32, q.Z, nullptr, 1, pf(c, packed, Lw.ln1_w), pf(c, packed, Lw.ln1_b), eps_ln, q.Y1, nullptr,
                               q.zstat, M, hid, 0.f, seed, 0, s, c->dropout_ctr));
        CHK(linear(q.Y1, Lw.w1, Lw.b1, q.pre, inter, hid));
        HIPCHK(gelu_launch(q.pre, nullptr, w.Hb, (long long)M * inter, 0, s));
        CHK(linear(w.Hb, Lw.w2, Lw.b2, w.dXa, hid, inter));
        HIPCHK(ln_train_launch(DT_F32, w.dXa, q.Y1, M, pf(c, packed, Lw.ln2_w), pf(c, packed, Lw.ln2_b), eps_ln, q.Xout, q.s,
                               q.sstat, M, hid, dropout_p, seed, (unsigned)(i + 1), s, c->dropout_ctr));
        xc = q.Xout;
    }
    return linear(xc, c->cout_w, c->cout_b, w.O, width, hid);
}

// Backward of the Transformer_Module: w.dO [B*S][width] fp32 (gradient of its output) -> every transformer.* parameter gradient
// (written at its plan offset of `grads`) and w.dTok [B*S][width] fp32 (gradient of its input tokens `x`).  data_only: w.dTok alone
// (`grads` is not touched: no bias / LayerNorm sums, no weight GEMM).
int fnet_bwd_part(const ddimx_ctx* c, const void* packed, const char* pb, const BwdPack& bp, const ddimx_tables* tables,
                  const TrainWs& w, const TrainTape& tp, const void* Dlast, float* grads, int B, int S, float dropout_p,
                  unsigned long long seed, hipStream_t s, bool data_only) {
    const ddimx_config& f = c->cfg;
    const int dt = c->dtype;
    const int hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width, M = B * S;
    const int bf = c->fnet_bf16;
    const int C5 = f.ch[c->L - 1], Fr = c->Fr;
    auto G = [&](int i) -> float* { return data_only ? nullptr : grads + c->grad_off[i]; };
    // C [m][n] = A [m][k] Bm[n][k]^T (+ resid), split from the whole m: the data gradients over the tokens, the weight gradients across them
    auto gemm = [&](const float* A, const float* Bm, float* C, int m, int n, int k, const float* resid = nullptr) -> int {
        GemmArgs g = gemm_nt(A, Bm, C, m, n, k);
        g.resid = resid; g.bf16 = bf;
        return run_gemm(g, w.gpart, 0, s);
    };
    {   // compute_out: O = Xlast Wc^T + bc   (parameters live in the token-order permutation; gradients are un-permuted)
        if (!data_only) {
            const float* Xlast = f.fnet_layers ? tp.fl[f.fnet_layers - 1].Xout : tp.X0;
            HIPCHK(colsum_launch(w.dO, M, width, width, w.pgrad, s));
            HIPCHK(pack_perm_cols_launch(w.pgrad, G(c->cout_b), 1, Fr, C5, s));
            HIPCHK(transpose_launch(w.dO, w.T1, M, width, 0, s));
            HIPCHK(transpose_launch(Xlast, w.T2, M, hid, 0, s));
            CHK(gemm(w.T1, w.T2, w.pgrad, width, hid, M));
            HIPCHK(pack_perm_rows_launch(w.pgrad, G(c->cout_w), Fr, C5, hid, s));
        }
        CHK(gemm(w.dO, (const float*)(pb + bp.coutT), w.dXa, M, hid, width));
    }
    for (int i = f.fnet_layers - 1; i >= 0; --i) {
        const ddimx_ctx::FL& Lw = c->fl[i];
        const TrainTape::FLT& q = tp.fl[i];
        // output.LayerNorm(s), s = Y1 + dropout(FFN)
        HIPCHK(ln_bwd_launch(DT_F32, w.dXa, q.s, nullptr, 1, q.sstat, pf(c, packed, Lw.ln2_w), w.dXb, w.lnpart, G(Lw.ln2_w), G(Lw.ln2_b),
                             M, hid, s));
        const float* dO2 = w.dXb;
        if (dropout_p > 0.f) {
            HIPCHK(dropout_apply_launch(w.dXb, w.dZ, (long long)M * hid, dropout_p, seed, (unsigned)(i + 1), s, c->dropout_ctr));
            dO2 = w.dZ;
        }
        if (!data_only) {
            HIPCHK(colsum_launch(dO2, M, hid, hid, G(Lw.b2), s));
            HIPCHK(transpose_launch(dO2, w.T1, M, hid, 0, s));
            HIPCHK(transpose_launch(q.pre, w.T2, M, inter, 1, s));                               // gelu(pre)^T
            CHK(gemm(w.T1, w.T2, G(Lw.w2), hid, inter, M));         // dW2 [hid][inter]
        }
        CHK(gemm(dO2, (const float*)(pb + bp.w2T[i]), w.dH, M, inter, hid));
        HIPCHK(gelu_launch(w.dH, q.pre, w.dH, (long long)M * inter, 1, s));                      // d(pre)
        if (!data_only) {
            HIPCHK(colsum_launch(w.dH, M, inter, inter, G(Lw.b1), s));
            HIPCHK(transpose_launch(w.dH, w.T1, M, inter, 0, s));
            HIPCHK(transpose_launch(q.Y1, w.T2, M, hid, 0, s));
            CHK(gemm(w.T1, w.T2, G(Lw.w1), inter, hid, M));         // dW1 [inter][hid]
        }
        CHK(gemm(w.dH, (const float*)(pb + bp.w1T[i]), w.dXa, M, hid, inter, w.dXb));  // dY1 = ds + dpre W1
        // fourier.output.LayerNorm(Z), Z = X + Re(FFT2(X))
        HIPCHK(ln_bwd_launch(DT_F32, w.dXa, q.Z, nullptr, 1, q.zstat, pf(c, packed, Lw.ln1_w), w.dXb, w.lnpart, G(Lw.ln1_w), G(Lw.ln1_b),
                             M, hid, s));
        CHK(fourier_mix(tables->dft_hidden, tables->dft_seq, w.dXb, w.dXa, w.Ut, w.gpart, B, S, hid, fnet_mix_supported(S, hid), s));
    }
    {   // embedding: X0 = dropout(LN0(tok + posenc) Wp^T + bp)
        if (dropout_p > 0.f) HIPCHK(dropout_apply_launch(w.dXa, w.dXa, (long long)M * hid, dropout_p, seed, 0, s, c->dropout_ctr));
        if (!data_only) {
            HIPCHK(colsum_launch(w.dXa, M, hid, hid, G(c->proj_b), s));
            HIPCHK(transpose_launch(w.dXa, w.T1, M, hid, 0, s));
            HIPCHK(transpose_launch(tp.ln0, w.T2, M, width, 0, s));
            CHK(gemm(w.T1, w.T2, w.pgrad, hid, width, M));
            HIPCHK(pack_perm_cols_launch(w.pgrad, G(c->proj_w), hid, Fr, C5, s));
        }
        CHK(gemm(w.dXa, (const float*)(pb + bp.projT), w.dO, M, width, hid));
        HIPCHK(ln_bwd_launch(dt, w.dO, Dlast, tables->posenc, S, tp.ln0_stat, pf(c, packed, c->ln0_w), w.dTok, w.lnpart,
                             data_only ? nullptr : w.pgrad, data_only ? nullptr : w.pgrad + width, M, width, s));
        if (!data_only) {
            HIPCHK(pack_perm_cols_launch(w.pgrad, G(c->ln0_w), 1, Fr, C5, s));
            HIPCHK(pack_perm_cols_launch(w.pgrad + width, G(c->ln0_b), 1, Fr, C5, s));
        }
    }
    return 0;
}

// per-channel sums of an NHWC tensor over (batch, pixels) -> dst[C]   (bias gradients of Downsample / Upsample)
// stats: statistics slabs of x's partition, dgb: [B][C] per-sample sums
static int channel_sums(int dt, const void* x, float* stats, float* dgb, float* dst, int B, int HW, int C, hipStream_t s) {
    HIPCHK(tensor_stats_launch(dt, x, stats, B, HW, C, s));
    HIPCHK(partsum_launch(stats, B, resid_nparts(dt, HW, C), C, dgb, C, s, 2));
    HIPCHK(colsum_launch(dgb, B, C, C, dst, s));
    return 0;
}

// The data-gradient convs below choose their tile variant from the real batch (ConvCall::batch_plan): the whole-network backward
// runs them inside a BatchPlanScope, the per-op exports outside one.
int run_downsample_bwd(int dtype, int cbig, int csmall, const void* x, const void* dy, const void* w_dgrad, const void* dx_add, void* dx,
                       float* d_w, float* d_b, const DuBwdWs& w, int B, int Hs, int Ws, hipStream_t s, WgSide* sd, bool data_only) {
    const bool side = sd && sd->on();
    if (!data_only) {
        if (side) CHK(sd->fork(s));  // (the caller writes x and dy no more)
        CHK(run_wgrad(dtype, DOWN4, cbig, csmall, x, dy, nullptr, nullptr, XF_NONE, side ? sd->partial : w.partial, d_w, B, Hs, Ws,
                      side ? sd->st : s));
        CHK(channel_sums(dtype, dy, w.stats, w.dgb, d_b, B, Hs * Ws, csmall, s));
    }
    // d(input) of Conv2d(k4 s2 p1) = ConvTranspose2d with the same weights
    ConvCall u = up4_call(dtype, csmall, cbig, dy, w_dgrad, dx_add, dx, B, Hs, Ws);
    u.batch_plan = true;
    return run_conv(u, s, nullptr, nullptr);
}
int run_upsample_bwd(int dtype, int csmall, int cbig, const void* x, const void* dy, const void* w_dgrad, void* dx, float* d_w,
                     float* d_b, const DuBwdWs& w, int B, int Hs, int Ws, hipStream_t s, WgSide* sd, bool data_only) {
    const bool side = sd && sd->on();
    if (!data_only) {
        if (side) CHK(sd->fork(s));  // (the caller writes x and dy no more)
        // ConvTranspose2d weight [csmall][cbig][4][4]: its gradient is the stride-2 weight gradient with the roles of input and output
        // swapped (the big tensor dy plays the halo operand, the small tensor x the output gradient)
        CHK(run_wgrad(dtype, DOWN4, cbig, csmall, dy, x, nullptr, nullptr, XF_NONE, side ? sd->partial : w.partial, d_w, B, Hs, Ws,
                      side ? sd->st : s));
        CHK(channel_sums(dtype, dy, w.stats, w.dgb, d_b, B, 4 * Hs * Ws, cbig, s));
    }
    // d(input) of ConvTranspose2d(k4 s2 p1) = Conv2d with the same weights
    ConvCall d = down4_call(dtype, cbig, csmall, dy, w_dgrad, dx, B, 2 * Hs, 2 * Ws);
    d.batch_plan = true;
    return run_conv(d, s, nullptr, nullptr);
}

