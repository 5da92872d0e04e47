// Inference: workspace layout and the network walk of Model.forward (reference models/diffusion.py:237-294).
#include "host.h"

void carve(const ddimx_ctx* c, char* base, int B, int T, Ws* w) {
    const ddimx_config& f = c->cfg;
    const int L = c->L;
    const size_t es = esz(c->dtype);
    Carver cv{base, 0};
    w->temb_h1 = (float*)cv.take((size_t)B * 512 * 4);
    w->temb_h2 = (float*)cv.take((size_t)B * 512 * 4);
    w->temb = (float*)cv.take((size_t)B * c->E * 4);
    const size_t lvl0 = (size_t)B * T * f.f_size * f.ch[0] * es;
    w->A = cv.take(lvl0);
    w->xd.resize(L); w->xu.resize(L);
    // per-channel slabs (training) and one 128-byte group slab per partial (inference, gn_fused.h): size for the larger
    size_t stats_f = (size_t)B * conv_in_nparts(T, f.f_size) * (f.ch[0] * 2 > kGnSlab ? f.ch[0] * 2 : kGnSlab);
    size_t hmax = 0;
    int cmax = 0;
    for (int l = 0; l < L; ++l) {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        const size_t bytes = (size_t)B * H * W * C * es;
        w->xd[l] = cv.take(bytes);
        w->xu[l] = cv.take(bytes);
        if (bytes > hmax) hmax = bytes;
        if (C > cmax) cmax = C;
        size_t s = conv_stats_floats(c->dtype, CONV3, C, C, B, H, W);
        if (s > stats_f) stats_f = s;
        s = (size_t)B * resid_nparts(c->dtype, H * W, C) * (C * 2 > kGnSlab ? C * 2 : kGnSlab);
        if (s > stats_f) stats_f = s;
        if (l > 0) {
            s = conv_stats_floats(c->dtype, DOWN4, f.ch[l - 1], C, B, H, W);
            if (s > stats_f) stats_f = s;
            s = conv_stats_floats(c->dtype, UP4, C, f.ch[l - 1], B, H, W);
            if (s > stats_f) stats_f = s;
        }
    }
    w->h1 = cv.take(hmax);
    w->h2 = cv.take(hmax);
    w->stats_per_sample = stats_f / B;  // every term above is B x (per-sample slab)
    w->h_per_sample = hmax / B;
    w->cmax = cmax;
    w->stats = (float*)cv.take(stats_f * 4);
    w->stats2 = (float*)cv.take(stats_f * 4);  // (a conv's group slabs, 128 B per >= 32-channel workgroup, never exceed its per-channel ones)
    w->scale = (float*)cv.take((size_t)B * cmax * 4);
    w->shift = (float*)cv.take((size_t)B * cmax * 4);
    const int S = T >> (L - 1);
    const size_t M = (size_t)B * S;
    const int hid = f.fnet_hidden, inter = f.fnet_inter;
    w->ln0 = (float*)cv.take((size_t)B * (S > 32 ? S : 32) * c->width * 4);  // (chunk-major for the dense FNet path: 32 rows per sample)
    w->X = (float*)cv.take(M * hid * 4);
    w->Ut = (float*)cv.take((size_t)B * 2 * hid * S * 4);
    w->Z = (float*)cv.take(M * hid * 4);
    w->Y = (float*)cv.take(M * hid * 4);
    w->Hb = (float*)cv.take(M * inter * 4);
    w->O = (float*)cv.take(M * c->width * 4);
    w->pz = (float*)cv.take((size_t)B * (hid / 16) * 64 * 4);  // (blocks of 32 rows per sample whatever S)
    w->pv = (float*)cv.take((size_t)B * (hid / 32) * 64 * 4);
    w->zc = (float*)cv.take((size_t)B * 32 * hid * 4);
    w->hc = (float*)cv.take((size_t)B * 32 * inter * 4);
    w->vc = (float*)cv.take((size_t)B * 32 * hid * 4);
    {   // split-K partial tiles of the skinny FNet GEMMs
        const int bf = c->fnet_bf16;
        const int shp[6][5] = {{(int)M, hid, c->width, 1, bf}, {2 * hid, S, hid, B, 0}, {S, hid, S, B, 0},
                               {(int)M, inter, hid, 1, bf}, {(int)M, hid, inter, 1, bf}, {(int)M, c->width, hid, 1, bf}};
        size_t mx = 0;
        for (auto& q : shp) {
            const size_t n = (size_t)kMaxSplitK * q[3] * q[0] * q[1];  // the split depends on the per-sample shape only; size for the cap
            if (n > mx) mx = n;
        }
        w->gpart_per_sample = mx / B;  // every shape above has B in its row or batch count
        w->gpart = (float*)cv.take(mx * 4);
    }
    w->total = cv.off;
}

extern "C" {

long long ddimx_workspace_bytes(ddimx_handle h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    Ws w;
    carve(h, nullptr, B, T, &w);
    return (long long)w.total;
}

int ddimx_unet_fwd(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace,
                   long long workspace_bytes, const float* x, const int64_t* t, float* eps, int B, int T, void* stream) {
    return ddimx_unet_fwd_forked(h, packed, tables, workspace, workspace_bytes, x, t, eps, B, T, stream, nullptr, nullptr, 0, 0);
}

// Model.forward with part of the network run as TWO batch shards on two streams.  Every op is per sample and its launch plan
// depends on the sample's size only, so an op over samples [0, B) equals the same op over [0, B/2) and [B/2, B): results are
// bit-identical whatever the mask.  fork_mask bit l: the ops whose OUTPUT lives on level l (its Residual_Blocks, the Downsample
// into it, the Upsample into it, the edge convs for level 0) run as two shards, shard 0 on `stream`, shard 1 on `aux_stream`;
// bit 16: the FNet bottleneck.  Consecutive sharded ops stay forked (the shards drift apart freely); the streams are joined
// in front of the next unsharded op.  Where it pays is measured, not assumed: the full-chip, HBM-bound levels
// and the FNet gain from a second stream covering launch gaps and GroupNorm finalisation; the latency-bound deep levels lose.
int ddimx_unet_fwd_forked(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                          const float* x, const int64_t* t, float* eps, int B, int T, void* stream, void* aux_stream,
                          void* const* events, int n_events, unsigned fork_mask) {
    if (!h || !packed || !tables || !workspace || !x || !t || !eps) return fail("ddimx_unet_fwd: null argument");
    const ddimx_ctx* c = h;
    const ddimx_config& f = c->cfg;
    const int L = c->L;
    CHK(check_shape(c, B, T));
    Ws w;
    CHK(carve_checked("ddimx_unet_fwd", carve, c, workspace, workspace_bytes, B, T, &w));
    hipStream_t s = (hipStream_t)stream, sa = (hipStream_t)aux_stream;
    if (!sa || !events || n_events < 2 || B < 2) fork_mask = 0;
    fork_mask &= 0xFFFFFu;
    int ev_used = 0;  // every fork and every join records an event of its own: nothing is re-recorded inside one capture
    const int dt = c->dtype;
    const size_t es = esz(dt);
    const int bh = B / 2;  // shard 0 = samples [0, bh), shard 1 = [bh, B)
    bool forked = false;
    // fork / join in front of an op, as its shardedness requires
    auto sync_for = [&](bool sharded) -> int {
        if (sharded == forked) return 0;
        if (ev_used >= n_events) return fail("ddimx_unet_fwd_forked: %d events are not enough for this fork mask", n_events);
        hipEvent_t ev = (hipEvent_t)events[ev_used++];
        if (sharded) {
            HIPCHK(hipEventRecord(ev, s));
            HIPCHK(hipStreamWaitEvent(sa, ev, 0));
        } else {
            HIPCHK(hipEventRecord(ev, sa));
            HIPCHK(hipStreamWaitEvent(s, ev, 0));
        }
        forked = sharded;
        return 0;
    };
    auto lvl_on = [&](int l) { return (fork_mask >> l) & 1u; };
    auto act_bytes = [&](int l) { return (size_t)(T >> l) * (f.f_size >> l) * f.ch[l] * es; };  // one sample's activation on level l
    struct Lane { int b0, n; hipStream_t st; };
    // runs `op(lane)` once over the whole batch or once per shard
    auto for_lanes = [&](bool sharded, auto&& op) -> int {
        CHK(sync_for(sharded));
        if (!sharded) return op(Lane{0, B, s});
        CHK(op(Lane{bh, B - bh, sa}));
        CHK(op(Lane{0, bh, s}));
        return 0;
    };
    auto at = [&](const void* p, size_t per_sample, int b0) { return (void*)((char*)const_cast<void*>(p) + per_sample * b0); };
    // scratch shared by all levels (h1 / h2, statistics, scale / shift): a shard's share starts at b0 x (the most one sample
    // can need on ANY level) -- the two shards drift apart and may be on different levels at the same time
    // statistics partials (group format, gn_fused.h): buffer `cur` holds those of the tensor the next GroupNorm reads
    int cur = 0;
    auto stats_of = [&](const Lane& ln, int which) { return (which ? w.stats2 : w.stats) + w.stats_per_sample * ln.b0; };
    auto scale_of = [&](const Lane& ln) { return w.scale + (size_t)w.cmax * ln.b0; };
    auto shift_of = [&](const Lane& ln) { return w.shift + (size_t)w.cmax * ln.b0; };

    if (tables->temb_table) {
        HIPCHK(temb_gather_launch(tables->temb_table, t, w.temb, B, c->E, s));
    } else {
        CHK(run_temb(pf(c, packed, c->te), t, pf(c, packed, c->tw[0]), pf(c, packed, c->tb[0]), pf(c, packed, c->tw[1]),
                     pf(c, packed, c->tb[1]), pf(c, packed, c->tw[2]), pf(c, packed, c->tb[2]), w.temb_h1, w.temb_h2, w.temb,
                     B, 128, 512, c->E, s));
    }
    auto resblock = [&](int l, const void* in, void* out, const float* temb_chunk, const RBW& rbw, int np, int cs, bool want_stats,
                        int* ynp) -> int {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        return for_lanes(lvl_on(l), [&](const Lane& ln) -> int {
            return run_resblock(dt, C, at(in, act_bytes(l), ln.b0), at(out, act_bytes(l), ln.b0), temb_chunk + (size_t)c->E * ln.b0, c->E,
                                rb_ptrs(c, packed, rbw), at(w.h1, w.h_per_sample, ln.b0), at(w.h2, w.h_per_sample, ln.b0), stats_of(ln, cur),
                                scale_of(ln), shift_of(ln), np, cs, want_stats, ynp, ln.n, H, W, ln.st, nullptr, stats_of(ln, cur ^ 1));
        });
    };

    cur = 0;
    // ---- down path (models/diffusion.py:252-264) ----
    const size_t in_per = (size_t)f.in_channels * T * f.f_size;  // fp32 NCHW elements per sample at the network boundary
    CHK(for_lanes(lvl_on(0), [&](const Lane& ln) -> int {
        HIPCHK(conv_in_launch(dt, x + in_per * ln.b0, pf(c, packed, c->in_w), pf(c, packed, c->in_b), at(w.A, act_bytes(0), ln.b0),
                              stats_of(ln, 0), ln.n, f.in_channels, f.ch[0], T, f.f_size, ln.st, 1));
        return 0;
    }));
    int np = conv_in_nparts(T, f.f_size), cs = f.ch[0];
    const void* xcur = w.A;
    int bi = 0;
    for (int l = 0; l < L; ++l) {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        if (l > 0) {
            CHK(for_lanes(lvl_on(l), [&](const Lane& ln) -> int {
                ConvCall d = down4_call(dt, f.ch[l - 1], C, at(xcur, act_bytes(l - 1), ln.b0), pv(c, packed, c->down_w[l]),
                                        at(w.xd[l], act_bytes(l), ln.b0), ln.n, H * 2, W * 2);
                d.bias = pf(c, packed, c->down_b[l]);
                d.stats = stats_of(ln, 0);
                d.groups = true;
                d.wf = frag_of(c, packed, c->down_w[l]);
                return run_conv(d, ln.st, &np, &cs);
            }));
            cur = 0;
            xcur = w.xd[l];
        }
        for (int r = 0; r < f.res[l]; ++r, ++bi) {
            const bool last = (r == f.res[l] - 1);
            int ynp = 0;
            CHK(resblock(l, xcur, w.xd[l], w.temb + c->emb_off_down[bi], c->down_rb[l][r], np, cs, !last, &ynp));
            xcur = w.xd[l];
            cur ^= 1;
            np = ynp; cs = C;
        }
        if (f.res[l] == 0 && l == 0) return fail("level 0 needs at least one residual block");
    }
    // ---- bottleneck (models/diffusion.py:267-279) + first skip add (:284) ----
    const int S = T >> (L - 1), CL = f.ch[L - 1];
    CHK(for_lanes((fork_mask >> 16) & 1u, [&](const Lane& ln) -> int {
        Ws v = w;  // this shard's rows of every token matrix, its share of the split-K scratch
        const size_t rows = (size_t)ln.b0 * S;
        v.ln0 = w.ln0 + (size_t)ln.b0 * (S > 32 ? S : 32) * c->width; v.X = w.X + rows * f.fnet_hidden; v.Z = w.Z + rows * f.fnet_hidden;
        v.Y = w.Y + rows * f.fnet_hidden; v.Hb = w.Hb + rows * f.fnet_inter; v.O = w.O + rows * c->width;
        v.Ut = w.Ut + (size_t)ln.b0 * 2 * f.fnet_hidden * S;
        v.pz = w.pz + (size_t)ln.b0 * (f.fnet_hidden / 16) * 64; v.pv = w.pv + (size_t)ln.b0 * (f.fnet_hidden / 32) * 64;
        v.zc = w.zc + (size_t)ln.b0 * 32 * f.fnet_hidden; v.hc = w.hc + (size_t)ln.b0 * 32 * f.fnet_inter;
        v.vc = w.vc + (size_t)ln.b0 * 32 * f.fnet_hidden;
        v.gpart = w.gpart + w.gpart_per_sample * ln.b0;
        return run_fnet(c, packed, tables, v, at(w.xd[L - 1], act_bytes(L - 1), ln.b0), ln.n, S, ln.st);
    }));
    CHK(for_lanes(lvl_on(L - 1), [&](const Lane& ln) -> int {
        HIPCHK(resid_launch(dt, at(w.xd[L - 1], act_bytes(L - 1), ln.b0), w.O + (size_t)ln.b0 * S * c->width, 1, nullptr, nullptr,
                            at(w.xu[L - 1], act_bytes(L - 1), ln.b0), stats_of(ln, 0), ln.n, S * c->Fr, CL, ln.st, nullptr, 1));
        return 0;
    }));
    cur = 0;
    np = resid_nparts(dt, S * c->Fr, CL); cs = CL;
    // ---- up path (models/diffusion.py:281-292) ----
    bi = 0;
    for (int l = L - 1; l >= 0; --l) {
        const int H = T >> l, W = f.f_size >> l, C = f.ch[l];
        for (int r = 0; r < f.res[l]; ++r, ++bi) {
            const bool last = (r == f.res[l] - 1);
            int ynp = 0;
            CHK(resblock(l, w.xu[l], w.xu[l], w.temb + c->emb_off_up[bi], c->up_rb[l][r], np, cs, !last, &ynp));
            cur ^= 1;
            np = ynp; cs = C;
        }
        if (l > 0) {
            CHK(for_lanes(lvl_on(l - 1), [&](const Lane& ln) -> int {
                ConvCall u = up4_call(dt, C, f.ch[l - 1], at(w.xu[l], act_bytes(l), ln.b0), pv(c, packed, c->up_w[l]),
                                      at(w.xd[l - 1], act_bytes(l - 1), ln.b0), at(w.xu[l - 1], act_bytes(l - 1), ln.b0), ln.n, H, W);
                u.bias = pf(c, packed, c->up_b[l]);
                u.stats = stats_of(ln, 0);
                u.groups = true;
                u.wf = frag_of(c, packed, c->up_w[l]);
                return run_conv(u, ln.st, &np, &cs);
            }));
            cur = 0;
        }
    }
    CHK(for_lanes(lvl_on(0), [&](const Lane& ln) -> int {
        HIPCHK(conv_out_launch(dt, at(w.xu[0], act_bytes(0), ln.b0), at(w.A, act_bytes(0), ln.b0), pf(c, packed, c->out_w),
                               pf(c, packed, c->out_b), eps + in_per * ln.b0, ln.n, f.ch[0], f.in_channels, T, f.f_size, ln.st));
        return 0;
    }));
    CHK(sync_for(false));  // leave with everything joined into `stream`
    return 0;
}

int ddimx_fnet_fwd(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                   const void* x, float* out, int B, int T, void* stream) {
    if (!h || !packed || !tables || !workspace || !x || !out) return fail("ddimx_fnet_fwd: null argument");
    const ddimx_ctx* c = h;
    const int L = c->L;
    CHK(check_shape(c, B, T));
    Ws w;
    CHK(carve_checked("ddimx_fnet_fwd", carve, c, workspace, workspace_bytes, B, T, &w));
    hipStream_t s = (hipStream_t)stream;
    const int S = T >> (L - 1);
    CHK(run_fnet(c, packed, tables, w, x, B, S, s));
    HIPCHK(hipMemcpyAsync(out, w.O, (size_t)B * S * c->width * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // extern "C"
