// ======================================================================================================
// Training: forward that keeps a tape, and the whole-network backward.
// (reference: functions/losses.py:12-18 builds the graph, runners/diffusion.py:150 `loss.backward()` walks it)
// ======================================================================================================
#include "host.h"

void carve_tape(const ddimx_ctx* c, char* base, int B, int T, TrainTape* t) {
    const ddimx_config& f = c->cfg;
    const int L = c->L;
    const size_t es = esz(c->dtype);
    Carver cv{base, 0};
    t->temb_h1 = (float*)cv.take((size_t)B * 512 * 4);
    t->temb_h2 = (float*)cv.take((size_t)B * 512 * 4);
    t->temb = (float*)cv.take((size_t)B * c->E * 4);
    t->A = cv.take((size_t)B * T * f.f_size * f.ch[0] * es);
    t->dn_in.assign(L, nullptr); t->up_in.assign(L, nullptr);
    t->dn_rb.assign(L, {}); t->up_rb.assign(L, {}); t->dn_y.assign(L, {}); t->up_y.assign(L, {});
    for (int l = 0; l < L; ++l) {
        const size_t act = (size_t)B * (T >> l) * (f.f_size >> l) * f.ch[l] * es;
        t->dn_in[l] = l == 0 ? t->A : cv.take(act);
        t->up_in[l] = cv.take(act);
        for (int pass = 0; pass < 2; ++pass)
            for (int r = 0; r < f.res[l]; ++r) {
                RBTape rb;
                rb.u1 = cv.take(act); rb.u2 = cv.take(act);
                rb.small = (float*)cv.take(rb_tape_small_floats(B, f.ch[l]) * 4);
                (pass ? t->up_rb : t->dn_rb)[l].push_back(rb);
                (pass ? t->up_y : t->dn_y)[l].push_back(cv.take(act));
            }
    }
    const int S = T >> (L - 1);
    const size_t M = (size_t)B * S, hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width;
    t->ln0 = (float*)cv.take(M * width * 4);
    t->ln0_stat = (float*)cv.take(M * 2 * 4);
    t->X0 = (float*)cv.take(M * hid * 4);
    t->fl.clear();
    for (int i = 0; i < f.fnet_layers; ++i) {
        TrainTape::FLT q;
        q.Z = (float*)cv.take(M * hid * 4); q.zstat = (float*)cv.take(M * 2 * 4);
        q.Y1 = (float*)cv.take(M * hid * 4); q.pre = (float*)cv.take(M * inter * 4);
        q.s = (float*)cv.take(M * hid * 4); q.sstat = (float*)cv.take(M * 2 * 4);
        q.Xout = (float*)cv.take(M * hid * 4);
        t->fl.push_back(q);
    }
    t->total = cv.off;
}

// Residual blocks whose deferred batch sums fit one ColsumBatch (7 entries each)
constexpr int kDeferBlocks = ColsumBatch::kMax / 7;
void carve_train_ws(const ddimx_ctx* c, char* base, int B, int T, TrainWs* w) {
    const ddimx_config& f = c->cfg;
    const int L = c->L, dt = c->dtype;
    const size_t es = esz(dt);
    Carver cv{base, 0};
    const size_t stats_f = walk_stats_floats(c, B, T, false);  // per-channel slabs: the forward's, which cover the backward's (resid's partition)
    size_t hmax = 0, part_f = 0, sums_f = 0;
    int cmax = 0;
    w->Ga.assign(L, nullptr); w->Gb.assign(L, nullptr); w->GS.assign(L, nullptr);
    for (int l = 0; l < L; ++l) {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        const size_t act = (size_t)B * H * W * C * es;
        w->Ga[l] = cv.take(act); w->Gb[l] = cv.take(act); w->GS[l] = cv.take(act);
        if (act > hmax) hmax = act;
        if (C > cmax) cmax = C;
        sums_f = std::max(sums_f, rb_bwd_stats_floats(dt, B, H * W, C) / 2);  // per-sample channel sums: one float per statistics pair
        part_f = std::max(part_f, wgrad_partial_floats(dt, CONV3, C, C, B, H, W));
        if (l > 0) part_f = std::max(part_f, wgrad_partial_floats(dt, DOWN4, f.ch[l - 1], C, B, H, W));
    }
    part_f = std::max(part_f, edge_wgrad_partial_floats(dt, B, f.ch[0], f.in_channels, T, f.f_size));
    w->gA = cv.take((size_t)B * T * f.f_size * f.ch[0] * es);
    w->du = cv.take(hmax);
    w->dg = cv.take(hmax);
    for (int i = 0; i < 3; ++i) w->du_b[i] = cv.take(hmax);
    w->hold.assign(L, {});
    for (int l = 0; l < L - 1 && l < kWgradHoldLevels; ++l)
        for (int i = 0; i < 2 * f.res[l]; ++i) w->hold[l].push_back(cv.take((size_t)B * (T >> l) * (f.f_size >> l) * f.ch[l] * es));
    w->stats = (float*)cv.take(stats_f * 4);
    w->scale = (float*)cv.take((size_t)B * cmax * 4);
    w->shift = (float*)cv.take((size_t)B * cmax * 4);
    w->coef = (float*)cv.take((size_t)B * 3 * cmax * 4);
    w->dgb = (float*)cv.take((size_t)B * 2 * cmax * 4);
    w->slots = (float*)cv.take((size_t)kDeferBlocks * 4 * B * 2 * cmax * 4);
    w->sums = (float*)cv.take(sums_f * 4);
    w->sums_f = sums_f;
    w->sums_ring = (float*)cv.take((size_t)kDeferBlocks * 2 * sums_f * 4);
    w->partial = (float*)cv.take(part_f * 4);
    w->partial_b = (float*)cv.take(part_f * 4);
    w->dtemb = (float*)cv.take((size_t)B * c->E * 4);
    w->dh2 = (float*)cv.take((size_t)B * 512 * 4);
    w->dh1 = (float*)cv.take((size_t)B * 512 * 4);
    const int S = T >> (L - 1);
    const size_t M = (size_t)B * S, hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width;
    const size_t big = inter > width ? inter : width;
    w->Ut = (float*)cv.take((size_t)B * 2 * hid * S * 4);
    w->Hb = (float*)cv.take(M * inter * 4);
    w->O = (float*)cv.take(M * width * 4);
    w->dO = (float*)cv.take(M * width * 4);
    w->dXa = (float*)cv.take(M * hid * 4);
    w->dXb = (float*)cv.take(M * hid * 4);
    w->dZ = (float*)cv.take(M * hid * 4);
    w->dH = (float*)cv.take(M * inter * 4);
    w->T1 = (float*)cv.take(M * big * 4);
    w->T2 = (float*)cv.take(M * big * 4);
    w->lnpart = (float*)cv.take((size_t)ln_bwd_nblocks((int)M) * 2 * big * 4);
    w->dTok = (float*)cv.take(M * width * 4);
    w->pgrad = (float*)cv.take(hid * width * 4);
    w->gpart = (float*)cv.take(fnet_partial_floats(c, B, S, true) * 4);  // split-K partial tiles of the FNet GEMMs, forward and backward
    w->total = cv.off;
}

extern "C" {

long long ddimx_train_tape_bytes(ddimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    TrainTape t;
    carve_tape(h, nullptr, B, T, &t);
    return (long long)t.total;
}
long long ddimx_train_workspace_bytes(ddimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    TrainWs w;
    carve_train_ws(h, nullptr, B, T, &w);
    return (long long)w.total;
}

int ddimx_unet_fwd_train(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace,
                         long long workspace_bytes, void* tape, long long tape_bytes, const float* x, const int64_t* t, float* eps,
                         int B, int T, float dropout_p, unsigned long long seed, void* stream) {
    if (!h || !packed || !tables || !workspace || !tape || !x || !t || !eps) return fail("ddimx_unet_fwd_train: null argument");
    const ddimx_ctx* c = h;
    CHK(check_shape(c, B, T, &dropout_p));
    for (int l = 0; l < c->L; ++l) if (c->cfg.res[l] < 1) return fail("training needs at least one residual block per level");
    BatchPlanScope plan_scope;
    TrainWs w;
    CHK(carve_checked("ddimx_unet_fwd_train", carve_train_ws, c, workspace, workspace_bytes, B, T, &w));
    TrainTape tp;
    CHK(carve_checked("ddimx_unet_fwd_train", carve_tape, c, tape, tape_bytes, B, T, &tp));
    FwdWalk k;  // the one-lane walk over the tape's sites, per-channel statistics in one buffer
    k.at = &tp; k.tape = &tp; k.tws = &w; k.dropout_p = dropout_p; k.seed = seed;
    k.stats = w.stats; k.scale = w.scale; k.shift = w.shift;
    k.s = (hipStream_t)stream;
    return unet_fwd_walk(c, packed, tables, x, t, eps, B, T, k);
}

// Backward of the whole network: d_eps [B][cio][T][F] fp32 -> every parameter gradient, WRITTEN into `grads`
// (fp32, ddimx_grad_floats() floats; parameter i at ddimx_grad_offset(i) in its own shape; the temb.te buffer's slot is
// left untouched).  x, t: the forward's inputs.  The gradient w.r.t. x: ddimx_unet_bwd_ex.
int ddimx_unet_bwd(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                   long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                   const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed, void* stream) {
    return ddimx_unet_bwd_staged(h, packed, packed_bwd, tables, workspace, workspace_bytes, tape, tape_bytes, x, t, d_eps, grads, B, T,
                                 dropout_p, seed, nullptr, 0, stream);
}

int ddimx_unet_bwd_staged(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                          long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                          const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed,
                          void* const* bucket_events, int n_events, void* stream) {
    return ddimx_unet_bwd_forked(h, packed, packed_bwd, tables, workspace, workspace_bytes, tape, tape_bytes, x, t, d_eps, grads, B, T,
                                 dropout_p, seed, bucket_events, n_events, stream, nullptr, nullptr, 0);
}

// Events ddimx_unet_bwd_forked needs for its weight-gradient branch: per Residual_Block two forks and two buffer releases, one fork
// per Downsample / Upsample weight and for the output conv's, the fork in front of bucket 0's event, the final join.
int ddimx_bwd_side_events(ddimx_handle h) {
    if (!h) return 0;
    int blocks = 0;
    for (int l = 0; l < h->L; ++l) blocks += 2 * h->cfg.res[l];
    return 4 * blocks + 2 * (h->L - 1) + 3;
}

// The backward with its weight gradients on `side_stream` (WgSide above; results are bit-identical to the one-stream call: same
// kernels, same partitions, same order of additions).  The branch is joined into `stream` before the call returns; bucket 0's event
// is recorded on the side stream (behind the up path's last weight gradient AND the chain's batch sums), the other two on `stream`.
// side_stream null (or the same as `stream`): one stream.
int ddimx_unet_bwd_forked(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                          long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                          const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed,
                          void* const* bucket_events, int n_events, void* stream, void* side_stream, void* const* side_events,
                          int n_side_events) {
    return ddimx_unet_bwd_ex(h, packed, packed_bwd, tables, workspace, workspace_bytes, tape, tape_bytes, x, t, d_eps, grads, B, T,
                             dropout_p, seed, bucket_events, n_events, stream, side_stream, side_events, n_side_events, nullptr, 0);
}

// The backward with the gradient w.r.t. the network input (d_x, nullable: one launch behind the chain, the input conv's data
// gradient) and, with DDIMX_BWD_DATA_ONLY, without any parameter gradient: the data-gradient chain alone.  Data-only mode skips every
// launch whose result reaches only a parameter slot -- weight gradients (Residual_Block convs, Down / Upsample, the edge convs), bias
// and GroupNorm / LayerNorm batch sums, the per-sample sums of du2 / du1 (conv.1.bias, timestep embedding), the FNet weight GEMMs,
// the timestep-embedding MLP -- and needs no side stream; every launch it does issue is the full backward's own, with the same
// operands, so d_x is bit-identical to a full backward's.
int ddimx_unet_bwd_ex(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                      long long workspace_bytes, const void* tape, long long tape_bytes, const float* x, const int64_t* t,
                      const float* d_eps, float* grads, int B, int T, float dropout_p, unsigned long long seed,
                      void* const* bucket_events, int n_events, void* stream, void* side_stream, void* const* side_events,
                      int n_side_events, float* d_x, int flags) {
    // (everything is validated before the first launch: no error path leaves a forked branch unjoined)
    if (flags & ~DDIMX_BWD_DATA_ONLY) return fail("ddimx_unet_bwd_ex: unknown flags 0x%x", (unsigned)flags);
    const bool data_only = (flags & DDIMX_BWD_DATA_ONLY) != 0;
    if (!h || !packed || !packed_bwd || !tables || !workspace || !tape || !x || !t || !d_eps || (!grads && !data_only))
        return fail("ddimx_unet_bwd: null argument");
    if (data_only && (n_events != 0 || bucket_events))
        return fail("ddimx_unet_bwd_ex: the data-only backward has no gradient buckets (pass 0 events)");
    if (data_only && !d_x) return fail("ddimx_unet_bwd_ex: the data-only backward needs d_x (it computes nothing else)");
    if (n_events != 0 && (n_events != 3 || !bucket_events)) return fail("ddimx_unet_bwd_staged: pass 0 or 3 bucket events");
    if (!data_only && side_stream && (!side_events || n_side_events < ddimx_bwd_side_events(h)))
        return fail("ddimx_unet_bwd_forked: %d side events, the plan needs %d", n_side_events, ddimx_bwd_side_events(h));
    const ddimx_ctx* c = h;
    const ddimx_config& f = c->cfg;
    const int L = c->L, dt = c->dtype;
    CHK(check_shape(c, B, T, &dropout_p));
    for (int l = 0; l < L; ++l) if (f.res[l] < 1) return fail("training needs at least one residual block per level");
    BatchPlanScope plan_scope;
    TrainWs w;
    CHK(carve_checked("ddimx_unet_bwd", carve_train_ws, c, workspace, workspace_bytes, B, T, &w));
    TrainTape tp;
    CHK(carve_checked("ddimx_unet_bwd", carve_tape, c, tape, tape_bytes, B, T, &tp));
    BwdPack bp;
    plan_bwd_pack(c, &bp);
    const char* pb = (const char*)packed_bwd;
    hipStream_t s = (hipStream_t)stream;
    auto G = [&](int i) -> float* { return data_only ? nullptr : grads + c->grad_off[i]; };
    RBBwdWs rw = {w.du, w.dg, w.stats, w.coef, w.dgb, w.sums, w.partial};
    rw.data_only = data_only;
    WgSide sd;
    if (!data_only && side_stream && side_stream != stream) {
        sd.st = (hipStream_t)side_stream; sd.ev = side_events; sd.n = n_side_events;
        sd.partial = w.partial_b; sd.du[0] = w.du; sd.du[1] = w.du_b[0]; sd.du[2] = w.du_b[1]; sd.du[3] = w.du_b[2];
    }
    hipStream_t const sw = sd.on() ? sd.st : s;            // the weight gradients' stream ...
    float* const wpart = sd.on() ? sd.partial : w.partial;  // ... and slab buffer
    const DuBwdWs du_ws = {w.partial, w.stats, w.dgb, 0};    // scratch of the Down / Upsample backward
    ColsumBatch defer;
    defer.count = 0;
    rw.defer = &defer;
    PartsumBatch pdefer;
    pdefer.count = 0;
    rw.pdefer = &pdefer;
    rw.sums_f = w.sums_f;
    auto flush_sums = [&]() -> int {  // the queued per-sample sums first: some of the batch sums read them
        HIPCHK(partsum_multi_launch(pdefer, s));
        pdefer.count = 0;
        HIPCHK(colsum_multi_launch(defer, s));
        defer.count = 0;
        return 0;
    };
    int deferred_blocks = 0;
    int cmax = 0;
    for (int l = 0; l < L; ++l) if (f.ch[l] > cmax) cmax = f.ch[l];
    auto next_slots = [&]() -> int {  // hands the next block its slots; flushes the batch when the arena is full
        if (deferred_blocks == kDeferBlocks) {
            CHK(flush_sums());
            deferred_blocks = 0;
        }
        rw.slots = w.slots + (size_t)deferred_blocks * 4 * B * 2 * cmax;
        rw.sums2 = w.sums_ring + (size_t)deferred_blocks * 2 * w.sums_f;
        ++deferred_blocks;
        return 0;
    };
    auto rb_grads = [&](const RBW& r, float* dtemb) {
        if (data_only) return RBGrads{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c->E};
        RBGrads g = {G(r.g0), G(r.b0), G(r.g1), G(r.b1), G(r.g2), G(r.w0), G(r.w1), G(r.bias1), dtemb, c->E};
        return g;
    };

    // ---- output conv (models/diffusion.py:283-292): gradient of `x + hidden[0]`, weight / bias gradients
    HIPCHK(conv_out_bwd_data_launch(dt, d_eps, pf(c, packed, c->out_w), w.gA, B, f.ch[0], f.in_channels, T, f.f_size, s));
    if (!data_only) {
        if (sd.on()) CHK(sd.fork(s));
        HIPCHK(edge_wgrad_launch(dt, 1, tp.up_y[0].back(), tp.A, d_eps, wpart, G(c->out_w), G(c->out_b), B, f.ch[0], f.in_channels,
                                 T, f.f_size, sw));
    }
    // ---- up path, last level first executed = level 0 ... L-1
    const void* gy = w.gA;
    bool have_stats = false;  // w.stats holds the first statistics pass of the block about to run
    int bi = (int)c->emb_off_up.size();  // Residual_Blocks in the forward's execution order: walked backwards
    for (int l = 0; l < L; ++l) {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        for (int r = f.res[l] - 1; r >= 0; --r) {
            const void* xin = r ? tp.up_y[l][r - 1] : tp.up_in[l];
            void* dx = r == 0 ? w.GS[l] : (gy == w.Gb[l] ? w.Ga[l] : w.Gb[l]);
            const RBW& rbw = c->up_rb[l][r];
            --bi;
            CHK(next_slots());
            sd.hold = sd.on() && !w.hold[l].empty() ? &w.hold[l][2 * r] : nullptr;
            // (block r - 1 of the level takes dx as its dy: its first statistics pass rides this block's last kernel)
            const void* nu2 = r > 0 ? tp.up_rb[l][r - 1].u2 : nullptr;
            CHK(run_resblock_bwd(dt, C, xin, tp.up_rb[l][r], gy, nullptr, dx, pf(c, packed, rbw.g0), pf(c, packed, rbw.g1),
                                 pf(c, packed, rbw.g2), pb + bp.up_wd0[l][r], pb + bp.up_wd1[l][r],
                                 rb_grads(rbw, w.dtemb + c->emb_off_up[bi]), rw, B, H, W, s, &sd, have_stats, nu2));
            have_stats = nu2 != nullptr;
            gy = dx;
        }
        sd.hold = nullptr;
        // now GS[l] = d(up_in[l]) = gradient of the skip D_l as well
        if (l < L - 1) {
            // up_in[l] = ConvTranspose2d(up_y[l+1].back()) + D_l   (GS[l] is not written again in this call)
            CHK(run_upsample_bwd(dt, f.ch[l + 1], C, tp.up_y[l + 1].back(), w.GS[l], pb + bp.up_dg[l + 1], w.Ga[l + 1], G(c->up_w[l + 1]),
                                 G(c->up_b[l + 1]), du_ws, B, H / 2, W / 2, s, &sd, data_only));
            gy = w.Ga[l + 1];
        }
    }
    if (n_events) {  // bucket 0: every up_modules.* gradient is final once the deferred batch sums are flushed
        CHK(flush_sums());
        deferred_blocks = 0;
    }
    if (sd.on()) CHK(sd.flush_held(s));  // the held weight gradients of the up path: now, under the bottleneck's launch-bound kernels
    if (n_events) {
        if (sd.on()) CHK(sd.fork(s));  // the chain does not wait for the branch here: the event goes behind both on the branch's stream
        HIPCHK(hipEventRecord((hipEvent_t)bucket_events[0], sw));
    }
    // ---- bottleneck: up_in[L-1] = D_{L-1} + O
    const int S = T >> (L - 1), CL = f.ch[L - 1];
    const int width = c->width, M = B * S, Fr = c->Fr;
    const void* Dlast = tp.dn_y[L - 1].back();
    HIPCHK(cast_f32_launch(dt, w.GS[L - 1], w.dO, (long long)M * width, s));
    CHK(fnet_bwd_part(c, packed, pb, bp, tables, w, tp, Dlast, grads, B, S, dropout_p, seed, s, data_only));
    if (n_events) HIPCHK(hipEventRecord((hipEvent_t)bucket_events[1], s));  // bucket 1: transformer.* gradients are final
    // d(D_{L-1}) = skip gradient + gradient through the bottleneck
    HIPCHK(resid_launch(dt, w.GS[L - 1], w.dTok, 1, nullptr, nullptr, w.Ga[L - 1], nullptr, B, S * Fr, CL, s));
    gy = w.Ga[L - 1];
    // ---- down path
    bi = (int)c->emb_off_down.size();
    for (int l = L - 1; l >= 0; --l) {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        for (int r = f.res[l] - 1; r >= 0; --r) {
            const void* xin = r ? tp.dn_y[l][r - 1] : tp.dn_in[l];
            void* dx = gy == w.Gb[l] ? w.Ga[l] : w.Gb[l];
            const RBW& rbw = c->down_rb[l][r];
            --bi;
            CHK(next_slots());
            const void* nu2 = r > 0 ? tp.dn_rb[l][r - 1].u2 : nullptr;
            // the walk's last block forks its weight gradients as soon as their `du` exists: nothing follows that they could run beside,
            // so they start under the block's own data-gradient convs (48.05 vs 48.20 ms per step, profiles/r04/wgside/last_block_early_ab.txt)
            sd.early_block = l == 0 && r == 0;
            CHK(run_resblock_bwd(dt, C, xin, tp.dn_rb[l][r], gy, (l == 0 && r == 0) ? w.gA : nullptr, dx, pf(c, packed, rbw.g0),
                                 pf(c, packed, rbw.g1), pf(c, packed, rbw.g2), pb + bp.dn_wd0[l][r], pb + bp.dn_wd1[l][r],
                                 rb_grads(rbw, w.dtemb + c->emb_off_down[bi]), rw, B, H, W, s, &sd, have_stats, nu2));
            have_stats = nu2 != nullptr;
            gy = dx;
        }
        if (l > 0) {
            // dn_in[l] = Conv2d(D_{l-1}, k4 s2 p1)   (level l's gradient buffers are not written again in this call)
            CHK(run_downsample_bwd(dt, f.ch[l - 1], C, tp.dn_y[l - 1].back(), gy, pb + bp.down_dg[l], w.GS[l - 1], w.Ga[l - 1],
                                   G(c->down_w[l]), G(c->down_b[l]), du_ws, B, H, W, s, &sd, data_only));
            gy = w.Ga[l - 1];
        }
    }
    CHK(flush_sums());
    // ---- input conv (models/diffusion.py:255-256): gy = d(hidden[0]) including the skip into the output conv
    if (d_x)  // d(x): the only thing x feeds is this conv
        HIPCHK(conv_in_bwd_data_launch(dt, gy, (const float*)(pb + bp.in_dg), d_x, B, f.ch[0], f.in_channels, T, f.f_size, s));
    if (!data_only) {
        HIPCHK(edge_wgrad_launch(dt, 0, gy, nullptr, x, w.partial, G(c->in_w), G(c->in_b), B, f.ch[0], f.in_channels, T, f.f_size, s));
        // ---- timestep-embedding MLP
        CHK(run_temb_bwd(w.dtemb, pf(c, packed, c->te), t, pf(c, packed, c->tw[1]), pf(c, packed, c->tw[2]), tp.temb_h1, tp.temb_h2,
                         w.dh2, w.dh1, G(c->tw[0]), G(c->tb[0]), G(c->tw[1]), G(c->tb[1]), G(c->tw[2]), G(c->tb[2]), B, 128, 512, c->E, s));
    }
    if (sd.on()) CHK(sd.join(s));
    if (n_events) HIPCHK(hipEventRecord((hipEvent_t)bucket_events[2], s));  // bucket 2: temb.* and down_modules.*
    return 0;
}

static int sqerr_bwd_args(const char* who, const float* e, const float* out, const float* g, const float* d_out, int B, long long per_sample) {
    if (!e || !out || !g || !d_out) return fail("%s: null argument", who);
    CHK(batch_range(who, B));
    if (per_sample <= 0) return fail("%s: per_sample = %lld must be positive", who, per_sample);
    return 0;
}
int ddimx_sqerr_loss_bwd(const float* e, const float* out, const float* g_per_sample, float* d_out, int B, long long per_sample,
                         void* stream) {
    CHK(sqerr_bwd_args("ddimx_sqerr_loss_bwd", e, out, g_per_sample, d_out, B, per_sample));
    HIPCHK(sqerr_bwd_launch(e, out, g_per_sample, d_out, B, per_sample, (hipStream_t)stream));
    return 0;
}
int ddimx_sqerr_loss_bwd_mean(const float* e, const float* out, const float* g, float* d_out, int B, long long per_sample, void* stream) {
    CHK(sqerr_bwd_args("ddimx_sqerr_loss_bwd_mean", e, out, g, d_out, B, per_sample));
    HIPCHK(sqerr_bwd_launch(e, out, g, d_out, B, per_sample, (hipStream_t)stream, 1));
    return 0;
}

// ---- backward twins of the per-op forwards (the whole-network backward runs exactly these launches) ---------------------
// Transformer_Module alone, training mode + its backward (the `_bwd` twin of ddimx_fnet_fwd).  Both use the whole-network
// scratch / tape layouts (ddimx_train_workspace_bytes, ddimx_train_tape_bytes for the same B, T) and run exactly the launches
// ddimx_unet_fwd_train / ddimx_unet_bwd issue for the bottleneck.
int ddimx_fnet_fwd_train(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                         void* tape, long long tape_bytes, const void* x, float* out, int B, int T, float dropout_p,
                         unsigned long long seed, void* stream) {
    if (!h || !packed || !tables || !workspace || !tape || !x || !out) return fail("ddimx_fnet_fwd_train: null argument");
    const ddimx_ctx* c = h;
    const int L = c->L;
    CHK(check_shape(c, B, T, &dropout_p));
    TrainWs w;
    CHK(carve_checked("ddimx_fnet_fwd_train", carve_train_ws, c, workspace, workspace_bytes, B, T, &w));
    TrainTape tp;
    CHK(carve_checked("ddimx_fnet_fwd_train", carve_tape, c, tape, tape_bytes, B, T, &tp));
    hipStream_t s = (hipStream_t)stream;
    const int S = T >> (L - 1);
    CHK(fnet_fwd_train_part(c, packed, tables, w, tp, x, B, S, dropout_p, seed, s));
    HIPCHK(hipMemcpyAsync(out, w.O, (size_t)B * S * c->width * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}
int ddimx_fnet_bwd(ddimx_handle h, const void* packed, const void* packed_bwd, const ddimx_tables* tables, void* workspace,
                   long long workspace_bytes, const void* tape, long long tape_bytes, const void* x, const float* d_out, float* d_x,
                   float* grads, int B, int T, float dropout_p, unsigned long long seed, void* stream) {
    if (!h || !packed || !packed_bwd || !tables || !workspace || !tape || !x || !d_out || !d_x || !grads)
        return fail("ddimx_fnet_bwd: null argument");
    const ddimx_ctx* c = h;
    const int L = c->L;
    CHK(check_shape(c, B, T, &dropout_p));
    TrainWs w;
    CHK(carve_checked("ddimx_fnet_bwd", carve_train_ws, c, workspace, workspace_bytes, B, T, &w));
    TrainTape tp;
    CHK(carve_checked("ddimx_fnet_bwd", carve_tape, c, tape, tape_bytes, B, T, &tp));
    BwdPack bp;
    plan_bwd_pack(c, &bp);
    hipStream_t s = (hipStream_t)stream;
    const int S = T >> (L - 1);
    const size_t bytes = (size_t)B * S * c->width * 4;
    HIPCHK(hipMemcpyAsync(w.dO, d_out, bytes, hipMemcpyDeviceToDevice, s));
    CHK(fnet_bwd_part(c, packed, (const char*)packed_bwd, bp, tables, w, tp, x, grads, B, S, dropout_p, seed, s));
    HIPCHK(hipMemcpyAsync(d_x, w.dTok, bytes, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // extern "C"
