// Building blocks of the network walks: Residual_Block forward and backward (with the side-stream weight-gradient scheduler),
// timestep embedding, the FNet bottleneck in its inference and training forms, Down / Upsample backward.
#include "host.h"

// Residual_Block (models/diffusion.py:42-56).  The stats of x must already be in `stats`
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

int run_resblock(int dtype, int C, const void* x, void* y, const float* temb, int temb_stride, const RBPtrs& p,
                 void* h1, void* h2, float* stats, float* scale, float* shift, int x_nparts, int x_Cs,
                 bool want_stats, int* y_nparts, int B, int H, int W, hipStream_t s, const RBTape* tape, float* stats2) {
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
        ConvCall k1 = rb_conv_call(dtype, C, 0, x, p.w0, p.w0f, nullptr, temb, temb_stride, scale, shift, h1, stats2, B, H, W);
        ConvPlan pl;
        CHK(conv_plan(k1, &pl));
        CHK(gn_of(stats, x_nparts, p.g0, p.b0, &g, &fu, conv_rounds(pl, B), kGnFuseConvRounds, pl.g.nthreads));
        if (fu) k1.gn = g;
        CHK(run_conv(k1, s, &np, &cs));
        ConvCall k2 = rb_conv_call(dtype, C, 1, h1, p.w1, p.w1f, p.bias1, nullptr, 0, scale, shift, h2, stats, B, H, W);
        CHK(conv_plan(k2, &pl));
        CHK(gn_of(stats2, np, p.g1, p.b1, &g, &fu, conv_rounds(pl, B), kGnFuseConvRounds, pl.g.nthreads));
        if (fu) k2.gn = g;
        CHK(run_conv(k2, s, &np, &cs));
        const int rparts = resid_nparts(dtype, H * W, C);
        CHK(gn_of(stats, np, p.g2, nullptr, &g, &fu, resid_rounds(dtype, C, B, H, W), kGnFuseResidRounds, resid_threads(dtype, C)));
        HIPCHK(resid_launch(dtype, x, h2, 0, scale, shift, y, want_stats ? stats2 : nullptr, B, H * W, C, s, fu ? &g : nullptr, 1));
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
    HIPCHK(gn_finalize_launch(stats, x_nparts, x_Cs, C, cnt, p.g0, p.b0, eps, sc0, sh0, B, s, mr0));
    ConvCall k1 = conv3_call(dtype, C, x, p.w0, h1, B, H, W);
    k1.chan_add = temb; k1.chan_add_stride = temb_stride;
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
    HIPCHK(resid_launch(dtype, x, h2, tape ? 2 : 0, sc2, sh2, y, want_stats ? stats : nullptr, B, H * W, C, s));
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

// Transformer_Module (models/diffusion.py:131-167 + transformers modeling_fnet.py:138-279), eval mode.
// x: NHWC bottleneck activation viewed as tokens [B*S][width]; writes O [B*S][width] fp32.
// Dense-weight GEMMs use bf16 MFMA in bf16 mode; the DFT factors always run on the exact fp32 MFMA.
static int fnet_gemm(const Ws& w, hipStream_t s, const float* A, const float* Bm, float* C, int M, int N, int K, int lda,
                     int ldb, int ldc, const float* bias, const float* resid, int act, int accumulate, int bf16,
                     int batch = 1, long long sA = 0, long long sB = 0, long long sC = 0, int srows = 0) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = Bm; g.C = C; g.bias = bias; g.resid = resid; g.partial = w.gpart;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.sA = sA; g.sB = sB; g.sC = sC; g.batch = batch; g.accumulate = accumulate; g.act = act; g.bf16 = bf16;
    g.splitk = sample_splitk(srows > 0 ? srows : M, N, K, bf16);  // srows: rows of ONE sample (M itself for batched GEMMs)
    HIPCHK(gemm_launch(g, s));
    return 0;
}

int run_fnet(const ddimx_ctx* c, const void* packed, const ddimx_tables* tb, const Ws& w, const void* x, int B, int S, hipStream_t s) {
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
    CHK(fnet_gemm(w, s, w.ln0, pf(c, packed, c->proj_w), w.X, M, hid, width, width, width, hid, pf(c, packed, c->proj_b),
                  nullptr, 0, 0, bf, 1, 0, 0, 0, S));
    float* cur = w.X;
    float* other = w.Y;
    for (int i = 0; i < f.fnet_layers; ++i) {
        const ddimx_ctx::FL& L = c->fl[i];
        // Ut[b] = D_H * X[b]^T -> [2*hid][S]; D_H rows interleaved (2k: cos_k, 2k+1: sin_k), so that row pair k of
        // Ut[b] is one contiguous K-vector [cos-part(S) | sin-part(S)] for the sequence transform
        if (fnet_mix_supported(S, hid)) {
            HIPCHK(fnet_mix_launch(tb->dft_hidden, tb->dft_seq, cur, w.Z, B, S, hid, s));
        } else {
        CHK(fnet_gemm(w, s, tb->dft_hidden, cur, w.Ut, 2 * hid, S, hid, hid, hid, S, nullptr, nullptr, 0, 0, 0, B, 0,
                      (long long)S * hid, (long long)2 * hid * S));
        // Z[b] = [C_S | -S_S] * Ut[b]^T + X[b]   (Re(FFT2) + residual) in one GEMM with K = 2S
        CHK(fnet_gemm(w, s, tb->dft_seq, w.Ut, w.Z, S, hid, 2 * S, 2 * S, 2 * S, hid, nullptr, cur, 0, 0, 0, B, 0,
                      (long long)2 * hid * S, (long long)S * hid));
        }
        HIPCHK(layernorm_launch(DT_F32, w.Z, nullptr, 1, pf(c, packed, L.ln1_w), pf(c, packed, L.ln1_b), eps, other, M, hid, s));
        // FFN; the second GEMM's split-K reduce also applies bias, residual and output.LayerNorm
        CHK(fnet_gemm(w, s, other, pf(c, packed, L.w1), w.Hb, M, inter, hid, hid, hid, inter, pf(c, packed, L.b1), nullptr, 1, 0, bf, 1, 0, 0, 0, S));
        {
            GemmArgs g;
            memset(&g, 0, sizeof(g));
            g.A = w.Hb; g.B = pf(c, packed, L.w2); g.C = w.Z; g.bias = pf(c, packed, L.b2); g.resid = other; g.partial = w.gpart;
            g.M = M; g.N = hid; g.K = inter; g.lda = inter; g.ldb = inter; g.ldc = hid; g.batch = 1; g.bf16 = bf;
            g.splitk = sample_splitk(S, hid, inter, bf);
            HIPCHK(gemm_ln_launch(g, pf(c, packed, L.ln2_w), pf(c, packed, L.ln2_b), eps, cur, s));
        }
    }
    CHK(fnet_gemm(w, s, cur, pf(c, packed, c->cout_w), w.O, M, width, hid, hid, hid, width, pf(c, packed, c->cout_b), nullptr,
                  0, 0, bf, 1, 0, 0, 0, S));
    return 0;
}

// GEMM helper over the training scratch (same call shape as fnet_gemm)
static int tgemm(const TrainWs& w, hipStream_t s, const float* A, const float* Bm, float* C, int M, int N, int K, const float* bias,
                 const float* resid, int bf16, int batch = 1, long long sA = 0, long long sB = 0, long long sC = 0, int lda = -1,
                 int ldb = -1, int srows = 0) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = Bm; g.C = C; g.bias = bias; g.resid = resid; g.partial = w.gpart;
    g.M = M; g.N = N; g.K = K; g.lda = lda < 0 ? K : lda; g.ldb = ldb < 0 ? K : ldb; g.ldc = N;
    g.sA = sA; g.sB = sB; g.sC = sC; g.batch = batch; g.bf16 = bf16;
    g.splitk = sample_splitk(srows > 0 ? srows : M, N, K, bf16);
    HIPCHK(gemm_launch(g, s));
    return 0;
}
// Re(FFT2(X)) + X over [B][S][hid] token matrices (linear and symmetric: also its own backward)
static int fourier_mix(const ddimx_ctx* c, const ddimx_tables* tb, const TrainWs& w, const float* X, float* Z, int B, int S,
                       hipStream_t s) {
    const int hid = c->cfg.fnet_hidden;
    if (fnet_mix_supported(S, hid)) {
        HIPCHK(fnet_mix_launch(tb->dft_hidden, tb->dft_seq, X, Z, B, S, hid, s));
        return 0;
    }
    CHK(tgemm(w, s, tb->dft_hidden, X, w.Ut, 2 * hid, S, hid, nullptr, nullptr, 0, B, 0, (long long)S * hid, (long long)2 * hid * S));
    CHK(tgemm(w, s, tb->dft_seq, w.Ut, Z, S, hid, 2 * S, nullptr, X, 0, B, 0, (long long)2 * hid * S, (long long)S * hid));
    return 0;
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
    CHK(tgemm(w, s, tp.ln0, pf(c, packed, c->proj_w), tp.X0, M, hid, width, pf(c, packed, c->proj_b), nullptr, bf, 1, 0, 0, 0, -1, -1, S));
    if (dropout_p > 0.f) HIPCHK(dropout_apply_launch(tp.X0, tp.X0, (long long)M * hid, dropout_p, seed, 0, s, c->dropout_ctr));
    const float* xc = tp.X0;
    for (int i = 0; i < f.fnet_layers; ++i) {
        const ddimx_ctx::FL& Lw = c->fl[i];
        const TrainTape::FLT& q = tp.fl[i];
        CHK(fourier_mix(c, tables, w, xc, q.Z, B, S, s));
        HIPCHK(ln_train_launch(DT_F32, q.Z, nullptr, 1, pf(c, packed, Lw.ln1_w), pf(c, packed, Lw.ln1_b), eps_ln, q.Y1, nullptr,
                               q.zstat, M, hid, 0.f, seed, 0, s, c->dropout_ctr));
        CHK(tgemm(w, s, q.Y1, pf(c, packed, Lw.w1), q.pre, M, inter, hid, pf(c, packed, Lw.b1), nullptr, bf, 1, 0, 0, 0, -1, -1, S));
        HIPCHK(gelu_launch(q.pre, nullptr, w.Hb, (long long)M * inter, 0, s));
        CHK(tgemm(w, s, w.Hb, pf(c, packed, Lw.w2), w.dXa, M, hid, inter, pf(c, packed, Lw.b2), nullptr, bf, 1, 0, 0, 0, -1, -1, S));
        HIPCHK(ln_train_launch(DT_F32, w.dXa, q.Y1, M, pf(c, packed, Lw.ln2_w), pf(c, packed, Lw.ln2_b), eps_ln, q.Xout, q.s,
                               q.sstat, M, hid, dropout_p, seed, (unsigned)(i + 1), s, c->dropout_ctr));
        xc = q.Xout;
    }
    CHK(tgemm(w, s, xc, pf(c, packed, c->cout_w), w.O, M, width, hid, pf(c, packed, c->cout_b), nullptr, bf, 1, 0, 0, 0, -1, -1, S));
    return 0;
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
    {   // compute_out: O = Xlast Wc^T + bc   (parameters live in the token-order permutation; gradients are un-permuted)
        if (!data_only) {
            const float* Xlast = f.fnet_layers ? tp.fl[f.fnet_layers - 1].Xout : tp.X0;
            HIPCHK(colsum_launch(w.dO, M, width, width, w.pgrad, s));
            HIPCHK(pack_perm_cols_launch(w.pgrad, G(c->cout_b), 1, Fr, C5, s));
            HIPCHK(transpose_launch(w.dO, w.T1, M, width, 0, s));
            HIPCHK(transpose_launch(Xlast, w.T2, M, hid, 0, s));
            CHK(tgemm(w, s, w.T1, w.T2, w.pgrad, width, hid, M, nullptr, nullptr, bf));
            HIPCHK(pack_perm_rows_launch(w.pgrad, G(c->cout_w), Fr, C5, hid, s));
        }
        CHK(tgemm(w, s, w.dO, (const float*)(pb + bp.coutT), w.dXa, M, hid, width, nullptr, nullptr, bf));
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
            CHK(tgemm(w, s, w.T1, w.T2, G(Lw.w2), hid, inter, M, nullptr, nullptr, bf));         // dW2 [hid][inter]
        }
        CHK(tgemm(w, s, dO2, (const float*)(pb + bp.w2T[i]), w.dH, M, inter, hid, nullptr, nullptr, bf));
        HIPCHK(gelu_launch(w.dH, q.pre, w.dH, (long long)M * inter, 1, s));                      // d(pre)
        if (!data_only) {
            HIPCHK(colsum_launch(w.dH, M, inter, inter, G(Lw.b1), s));
            HIPCHK(transpose_launch(w.dH, w.T1, M, inter, 0, s));
            HIPCHK(transpose_launch(q.Y1, w.T2, M, hid, 0, s));
            CHK(tgemm(w, s, w.T1, w.T2, G(Lw.w1), inter, hid, M, nullptr, nullptr, bf));         // dW1 [inter][hid]
        }
        CHK(tgemm(w, s, w.dH, (const float*)(pb + bp.w1T[i]), w.dXa, M, hid, inter, nullptr, w.dXb, bf));  // dY1 = ds + dpre W1
        // fourier.output.LayerNorm(Z), Z = X + Re(FFT2(X))
        HIPCHK(ln_bwd_launch(DT_F32, w.dXa, q.Z, nullptr, 1, q.zstat, pf(c, packed, Lw.ln1_w), w.dXb, w.lnpart, G(Lw.ln1_w), G(Lw.ln1_b),
                             M, hid, s));
        CHK(fourier_mix(c, tables, w, w.dXb, w.dXa, B, S, s));
    }
    {   // embedding: X0 = dropout(LN0(tok + posenc) Wp^T + bp)
        if (dropout_p > 0.f) HIPCHK(dropout_apply_launch(w.dXa, w.dXa, (long long)M * hid, dropout_p, seed, 0, s, c->dropout_ctr));
        if (!data_only) {
            HIPCHK(colsum_launch(w.dXa, M, hid, hid, G(c->proj_b), s));
            HIPCHK(transpose_launch(w.dXa, w.T1, M, hid, 0, s));
            HIPCHK(transpose_launch(tp.ln0, w.T2, M, width, 0, s));
            CHK(tgemm(w, s, w.T1, w.T2, w.pgrad, hid, width, M, nullptr, nullptr, bf));
            HIPCHK(pack_perm_cols_launch(w.pgrad, G(c->proj_w), hid, Fr, C5, s));
        }
        CHK(tgemm(w, s, w.dXa, (const float*)(pb + bp.projT), w.dO, M, width, hid, nullptr, nullptr, bf));
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

