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
    w->A = cv.take((size_t)B * T * f.f_size * f.ch[0] * es);
    w->dn_in.resize(L); w->up_in.resize(L); w->dn_y.resize(L); w->up_y.resize(L);
    // per-channel slabs and one 128-byte group slab per partial (gn_fused.h): sized for the larger
    const size_t stats_f = walk_stats_floats(c, B, T, true);
    size_t hmax = 0;
    int cmax = 0;
    for (int l = 0; l < L; ++l) {
        const size_t bytes = (size_t)B * (T >> l) * (f.f_size >> l) * f.ch[l] * es;
        void *const xd = cv.take(bytes), *const xu = cv.take(bytes);  // the level's down and up stream: its blocks run in place
        w->dn_in[l] = l ? xd : w->A;
        w->up_in[l] = xu;
        w->dn_y[l].assign(f.res[l], xd);
        w->up_y[l].assign(f.res[l], xu);
        if (bytes > hmax) hmax = bytes;
        if (f.ch[l] > cmax) cmax = f.ch[l];
    }
    w->h1 = cv.take(hmax);
    w->h2 = cv.take(hmax);
    w->stats_per_sample = stats_f / B;
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
    const size_t gpart_f = fnet_partial_floats(c, B, S, false);  // split-K partial tiles of the skinny FNet GEMMs
    w->gpart_per_sample = gpart_f / B;
    w->gpart = (float*)cv.take(gpart_f * 4);
    w->total = cv.off;
}

// Events a forked forward records: one per change of shardedness along the walk -- the input conv and level 0, every deeper level,
// the bottleneck, the levels back up to the output conv -- and the final join.
static int fwd_events_needed(int L, unsigned fork_mask) {
    int n = 0;
    bool forked = false;
    auto op = [&](unsigned sharded) { n += (sharded != 0) != forked; forked = sharded != 0; };
    for (int l = 0; l < L; ++l) op((fork_mask >> l) & 1u);
    op((fork_mask >> 16) & 1u);
    for (int l = L - 1; l >= 0; --l) op((fork_mask >> l) & 1u);
    op(0);
    return n;
}

// An early return of a forked walk first joins the aux stream back into `s`, with the event the next join would have recorded (a
// capture both streams belong to stays valid).  Best effort: the caller gets the error that ended the walk.
struct JoinGuard {
    const bool& forked; hipStream_t s, sa; void* const* events; const int& used; int n;
    ~JoinGuard() {
        hipEvent_t ev = forked && used < n ? (hipEvent_t)events[used] : nullptr;
        if (ev && hipEventRecord(ev, sa) == hipSuccess) (void)hipStreamWaitEvent(s, ev, 0);
    }
};

// Model.forward (reference models/diffusion.py:237-294) with part of the network run as TWO batch shards on two streams.  Every op
// is per sample and its launch plan depends on the sample's size only, so an op over samples [0, B) equals the same op over [0, B/2)
// and [B/2, B): results are bit-identical whatever the mask.  fork_mask bit l: the ops whose OUTPUT lives on level l (its
// Residual_Blocks, the Downsample into it, the Upsample into it, the edge convs for level 0) run as two shards, shard 0 on `s`,
// shard 1 on `sa`; bit 16: the FNet bottleneck.  Consecutive sharded ops stay forked (the shards drift apart freely); the streams
// are joined in front of the next unsharded op.  Where it pays is measured, not assumed: the full-chip, HBM-bound
// levels and the FNet gain from a second stream covering launch gaps and GroupNorm finalisation; the latency-bound deep levels lose.
// The training forward is the one-lane walk (fork_mask 0) over the tape's sites.
int unet_fwd_walk(const ddimx_ctx* c, const void* packed, const ddimx_tables* tables, const float* x, const int64_t* t, float* eps, int B,
                  int T, const FwdWalk& k) {
    const ddimx_config& f = c->cfg;
    const WalkSites& at = *k.at;
    const int L = c->L, dt = c->dtype;
    const size_t es = esz(dt);
    const bool groups = k.stats2 != nullptr;
    hipStream_t const s = k.s, sa = k.sa;
    const int bh = B / 2;  // shard 0 = samples [0, bh), shard 1 = [bh, B)
    int ev_used = 0;       // every fork and every join records an event of its own: nothing is re-recorded inside one capture
    bool forked = false;
    JoinGuard guard{forked, s, sa, k.events, ev_used, k.n_events};
    // fork / join in front of an op, as its shardedness requires
    auto sync_for = [&](bool sharded) -> int {
        if (sharded == forked) return 0;
        if (ev_used >= k.n_events) return fail("ddimx_unet_fwd_forked: %d events are not enough for this fork mask", k.n_events);
        hipEvent_t ev = (hipEvent_t)k.events[ev_used++];
        HIPCHK(hipEventRecord(ev, sharded ? s : sa));  // fork: the aux stream goes on behind `s`; join: `s` behind the aux stream
        HIPCHK(hipStreamWaitEvent(sharded ? sa : s, ev, 0));
        forked = sharded;
        return 0;
    };
    auto lvl_on = [&](int l) { return (k.fork_mask >> l) & 1u; };
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
    auto lane_of = [&](const void* p, size_t per_sample, int b0) { return (void*)((char*)const_cast<void*>(p) + per_sample * b0); };
    // scratch shared by all levels (h1 / h2, statistics, scale / shift): a shard's share starts at b0 x (the most one sample
    // can need on ANY level) -- the two shards drift apart and may be on different levels at the same time
    // statistics partials: buffer `cur` holds those of the tensor the next GroupNorm reads (group format: the two alternate)
    float* const stats[2] = {k.stats, groups ? k.stats2 : k.stats};
    int cur = 0;
    auto stats_of = [&](const Lane& ln, int which) { return stats[which] + k.stats_per_sample * ln.b0; };

    if (!k.tape && tables->temb_table)
        HIPCHK(temb_gather_launch(tables->temb_table, t, at.temb, B, c->E, s));
    else
        CHK((k.tape ? run_temb_train : run_temb)(pf(c, packed, c->te), t, pf(c, packed, c->tw[0]), pf(c, packed, c->tb[0]),
                                                 pf(c, packed, c->tw[1]), pf(c, packed, c->tb[1]), pf(c, packed, c->tw[2]),
                                                 pf(c, packed, c->tb[2]), at.temb_h1, at.temb_h2, at.temb, B, 128, 512, c->E, s));
    int np = 0, cs = 0;  // the partition of the statistics in buffer `cur`
    // one Residual_Block of level l, in -> out; leaves np / cs / cur those of `out`
    auto resblock = [&](int l, const void* in, void* out, int emb_off, const RBW& rbw, const RBTape* tape, bool want_stats) -> int {
        const int C = f.ch[l];
        int ynp = 0;
        CHK(for_lanes(lvl_on(l), [&](const Lane& ln) -> int {
            RBCall q = rb_call(dt, C, lane_of(in, act_bytes(l), ln.b0), lane_of(out, act_bytes(l), ln.b0), ln.n, T >> l, f.f_size >> l,
                               rb_ptrs(c, packed, rbw), ln.st);
            q.temb = at.temb + emb_off + (size_t)c->E * ln.b0; q.temb_stride = c->E;
            q.h1 = lane_of(k.h1, k.h_per_sample, ln.b0); q.h2 = lane_of(k.h2, k.h_per_sample, ln.b0);
            q.stats = stats_of(ln, cur); q.stats2 = groups ? stats_of(ln, cur ^ 1) : nullptr;
            q.scale = k.scale + (size_t)k.cmax * ln.b0; q.shift = k.shift + (size_t)k.cmax * ln.b0;
            q.x_nparts = np; q.x_Cs = cs; q.want_stats = want_stats; q.tape = tape;
            return run_resblock(q, &ynp);
        }));
        cur ^= 1;
        np = ynp; cs = C;
        return 0;
    };
    // a Down / Upsample conv between levels, as the lane's ConvCall; leaves np / cs / cur those of its output
    auto resample = [&](int l_out, auto&& call, int w_idx, int b_idx) -> int {
        CHK(for_lanes(lvl_on(l_out), [&](const Lane& ln) -> int {
            ConvCall q = call(ln);
            q.bias = pf(c, packed, b_idx);
            q.stats = stats_of(ln, 0);
            q.groups = groups;
            if (groups) q.wf = frag_of(c, packed, w_idx);
            return run_conv(q, ln.st, &np, &cs);
        }));
        cur = 0;
        return 0;
    };

    // ---- down path (models/diffusion.py:252-264) ----
    const size_t in_per = (size_t)f.in_channels * T * f.f_size;  // fp32 NCHW elements per sample at the network boundary
    CHK(for_lanes(lvl_on(0), [&](const Lane& ln) -> int {
        HIPCHK(conv_in_launch(dt, x + in_per * ln.b0, pf(c, packed, c->in_w), pf(c, packed, c->in_b), lane_of(at.A, act_bytes(0), ln.b0),
                              stats_of(ln, 0), ln.n, f.in_channels, f.ch[0], T, f.f_size, ln.st, groups));
        return 0;
    }));
    np = conv_in_nparts(T, f.f_size); cs = f.ch[0];
    const void* skip[DDIMX_MAX_LEVELS];  // each level's down-path output: the Upsample's additive skip, the bottleneck's input
    const void* xcur = at.A;
    int bi = 0;  // Residual_Blocks in execution order (the timestep embedding's chunks)
    for (int l = 0; l < L; ++l) {
        if (l > 0) {
            CHK(resample(l, [&](const Lane& ln) {
                return down4_call(dt, f.ch[l - 1], f.ch[l], lane_of(xcur, act_bytes(l - 1), ln.b0), pv(c, packed, c->down_w[l]),
                                  lane_of(at.dn_in[l], act_bytes(l), ln.b0), ln.n, T >> (l - 1), f.f_size >> (l - 1));
            }, c->down_w[l], c->down_b[l]));
            xcur = at.dn_in[l];
        }
        for (int r = 0; r < f.res[l]; ++r, ++bi) {
            CHK(resblock(l, xcur, at.dn_y[l][r], c->emb_off_down[bi], c->down_rb[l][r], k.tape ? &k.tape->dn_rb[l][r] : nullptr,
                         r != f.res[l] - 1));
            xcur = at.dn_y[l][r];
        }
        skip[l] = xcur;
    }
    // ---- bottleneck (models/diffusion.py:267-279; training mode: dropout after the projection and after each FFN) + first skip add (:284) ----
    const int S = T >> (L - 1), CL = f.ch[L - 1];
    const float* O = nullptr;
    if (k.tape) {
        CHK(fnet_fwd_train_part(c, packed, tables, *k.tws, *k.tape, xcur, B, S, k.dropout_p, k.seed, s));
        O = k.tws->O;
    } else {
        const FnetWs& w = *k.ws;
        O = w.O;
        CHK(for_lanes((k.fork_mask >> 16) & 1u, [&](const Lane& ln) -> int {
            FnetWs v;  // this shard's rows of every token matrix, its share of the split-K scratch
            const size_t b0 = ln.b0, rows = b0 * S, hid = f.fnet_hidden, inter = f.fnet_inter;
            v.ln0 = w.ln0 + b0 * (S > 32 ? S : 32) * c->width; v.X = w.X + rows * hid; v.Z = w.Z + rows * hid; v.Y = w.Y + rows * hid;
            v.Hb = w.Hb + rows * inter; v.O = w.O + rows * c->width; v.Ut = w.Ut + b0 * 2 * hid * S;
            v.pz = w.pz + b0 * (hid / 16) * 64; v.pv = w.pv + b0 * (hid / 32) * 64;
            v.zc = w.zc + b0 * 32 * hid; v.hc = w.hc + b0 * 32 * inter; v.vc = w.vc + b0 * 32 * hid;
            v.gpart = w.gpart + k.ws->gpart_per_sample * b0;
            return run_fnet(c, packed, tables, v, lane_of(xcur, act_bytes(L - 1), ln.b0), ln.n, S, ln.st);
        }));
    }
    CHK(for_lanes(lvl_on(L - 1), [&](const Lane& ln) -> int {
        HIPCHK(resid_launch(dt, lane_of(xcur, act_bytes(L - 1), ln.b0), O + (size_t)ln.b0 * S * c->width, 1, nullptr, nullptr,
                            lane_of(at.up_in[L - 1], act_bytes(L - 1), ln.b0), stats_of(ln, 0), ln.n, S * c->Fr, CL, ln.st, nullptr, groups));
        return 0;
    }));
    cur = 0;
    np = resid_nparts(dt, S * c->Fr, CL); cs = CL;
    // ---- up path (models/diffusion.py:281-292) ----
    bi = 0;
    for (int l = L - 1; l >= 0; --l) {
        xcur = at.up_in[l];
        for (int r = 0; r < f.res[l]; ++r, ++bi) {
            CHK(resblock(l, xcur, at.up_y[l][r], c->emb_off_up[bi], c->up_rb[l][r], k.tape ? &k.tape->up_rb[l][r] : nullptr,
                         r != f.res[l] - 1));
            xcur = at.up_y[l][r];
        }
        if (l > 0)
            CHK(resample(l - 1, [&](const Lane& ln) {
                return up4_call(dt, f.ch[l], f.ch[l - 1], lane_of(xcur, act_bytes(l), ln.b0), pv(c, packed, c->up_w[l]),
                                lane_of(skip[l - 1], act_bytes(l - 1), ln.b0), lane_of(at.up_in[l - 1], act_bytes(l - 1), ln.b0), ln.n,
                                T >> l, f.f_size >> l);
            }, c->up_w[l], c->up_b[l]));
    }
    CHK(for_lanes(lvl_on(0), [&](const Lane& ln) -> int {
        HIPCHK(conv_out_launch(dt, lane_of(xcur, act_bytes(0), ln.b0), lane_of(at.A, act_bytes(0), ln.b0), pf(c, packed, c->out_w),
                               pf(c, packed, c->out_b), eps + in_per * ln.b0, ln.n, f.ch[0], f.in_channels, T, f.f_size, ln.st));
        return 0;
    }));
    return sync_for(false);  // leave with everything joined into `stream`
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

// unet_fwd_walk over the inference workspace.  Everything is validated before the first launch: no refusal leaves work enqueued.
int ddimx_unet_fwd_forked(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                          const float* x, const int64_t* t, float* eps, int B, int T, void* stream, void* aux_stream,
                          void* const* events, int n_events, unsigned fork_mask) {
    if (!h || !packed || !tables || !workspace || !x || !t || !eps) return fail("ddimx_unet_fwd: null argument");
    const ddimx_ctx* c = h;
    CHK(check_shape(c, B, T));
    Ws w;
    CHK(carve_checked("ddimx_unet_fwd", carve, c, workspace, workspace_bytes, B, T, &w));
    if (c->cfg.res[0] < 1) return fail("level 0 needs at least one residual block");
    if (!aux_stream || !events || n_events < 2 || B < 2) fork_mask = 0;
    fork_mask &= 0xFFFFFu;
    if (fwd_events_needed(c->L, fork_mask) > n_events)
        return fail("ddimx_unet_fwd_forked: %d events are not enough for this fork mask", n_events);
    FwdWalk k;
    k.at = &w; k.ws = &w;
    k.h1 = w.h1; k.h2 = w.h2; k.stats = w.stats; k.stats2 = w.stats2; k.scale = w.scale; k.shift = w.shift;
    k.stats_per_sample = w.stats_per_sample; k.h_per_sample = w.h_per_sample; k.cmax = w.cmax;
    k.s = (hipStream_t)stream; k.sa = (hipStream_t)aux_stream; k.events = events; k.n_events = n_events; k.fork_mask = fork_mask;
    return unet_fwd_walk(c, packed, tables, x, t, eps, B, T, k);
}

int ddimx_fnet_fwd(ddimx_handle h, const void* packed, const ddimx_tables* tables, void* workspace, long long workspace_bytes,
                   const void* x, float* out, int B, int T, void* stream) {
    if (!h || !packed || !tables || !workspace || !x || !out) return fail("ddimx_fnet_fwd: null argument");
    const ddimx_ctx* c = h;
    CHK(check_shape(c, B, T));
    Ws w;
    CHK(carve_checked("ddimx_fnet_fwd", carve, c, workspace, workspace_bytes, B, T, &w));
    hipStream_t s = (hipStream_t)stream;
    const int S = T >> (c->L - 1);
    CHK(run_fnet(c, packed, tables, w, x, B, S, s));
    HIPCHK(hipMemcpyAsync(out, w.O, (size_t)B * S * c->width * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // extern "C"
