// Per-op entry points: single ops of the network as the bit-exact tests and the tuning tools call them.
#include "host.h"

extern "C" {

// ---- per-op entry points ---------------------------------------------------------------------------
int ddimx_to_nhwc(int dtype, const float* nchw, void* nhwc, int B, int C, int H, int W, void* stream) {
    HIPCHK(to_nhwc_launch(dtype, nchw, nhwc, B, C, H * W, (hipStream_t)stream));
    return 0;
}
int ddimx_from_nhwc(int dtype, const void* nhwc, float* nchw, int B, int C, int H, int W, void* stream) {
    HIPCHK(from_nhwc_launch(dtype, nhwc, nchw, B, C, H * W, (hipStream_t)stream));
    return 0;
}
int ddimx_pack_conv(int dtype, const float* w, void* dst, int O, int I, int KH, int KW, void* stream) {
    HIPCHK(pack_conv_launch(dtype, w, dst, O, I, KH, KW, (hipStream_t)stream));
    return 0;
}
int ddimx_pack_convT(int dtype, const float* w, void* dst, int I, int O, void* stream) {
    HIPCHK(pack_convT_launch(dtype, w, dst, I, O, (hipStream_t)stream));
    return 0;
}
// ---- the packing kernels of ddimx_pack_weights / ddimx_pack_weights_bwd one by one (plan.cpp issues exactly these launchers) ----
int ddimx_pack_perm_cols(const float* src, float* dst, int rows, int C, int Fr, void* stream) {
    if (!src || !dst) return fail("ddimx_pack_perm_cols: null argument");
    if (rows < 1 || C < 1 || Fr < 1 || (long long)C * Fr > 0x7fffffffll) return fail("ddimx_pack_perm_cols: bad shape rows=%d C=%d Fr=%d", rows, C, Fr);
    HIPCHK(pack_perm_cols_launch(src, dst, rows, C, Fr, (hipStream_t)stream));
    return 0;
}
int ddimx_pack_perm_rows(const float* src, float* dst, int C, int Fr, int K, void* stream) {
    if (!src || !dst) return fail("ddimx_pack_perm_rows: null argument");
    if (C < 1 || Fr < 1 || K < 1 || (long long)C * Fr > 0x7fffffffll) return fail("ddimx_pack_perm_rows: bad shape C=%d Fr=%d K=%d", C, Fr, K);
    HIPCHK(pack_perm_rows_launch(src, dst, C, Fr, K, (hipStream_t)stream));
    return 0;
}
int ddimx_pack_copy_multi(const float* const* srcs, float* const* dsts, const long long* ns, int count, void* stream) {
    if (!srcs || !dsts || !ns) return fail("ddimx_pack_copy_multi: null argument");
    if (count < 1) return fail("ddimx_pack_copy_multi: %d entries", count);
    for (int i = 0; i < count; ++i)
        if (!srcs[i] || !dsts[i] || ns[i] < 1) return fail("ddimx_pack_copy_multi: bad entry %d", i);
    hipStream_t s = (hipStream_t)stream;
    PackCopyBatch batch;
    batch.count = 0;
    for (int i = 0; i < count; ++i) HIPCHK(batch.push(srcs[i], dsts[i], ns[i], s));
    HIPCHK(pack_copy_multi_launch(batch, s));
    return 0;
}
int ddimx_pack_conv_multi(const float* const* srcs, void* const* dsts, const int* O, const int* I, const int* KK, const int* mode,
                          const int* dtype, int count, void* stream) {
    if (!srcs || !dsts || !O || !I || !KK || !mode || !dtype) return fail("ddimx_pack_conv_multi: null argument");
    if (count < 1) return fail("ddimx_pack_conv_multi: %d entries", count);
    for (int i = 0; i < count; ++i) {
        const bool shape = O[i] >= 1 && I[i] >= 1 && KK[i] >= 1 && (long long)KK[i] * O[i] * I[i] <= 0x7fffffffll;
        if (!srcs[i] || !dsts[i] || !shape || mode[i] < 0 || mode[i] > 1 || (mode[i] == 1 && KK[i] != 9) ||
            (dtype[i] != DT_F32 && dtype[i] != DT_BF16))
            return fail("ddimx_pack_conv_multi: bad entry %d", i);
    }
    hipStream_t s = (hipStream_t)stream;
    PackConvBatch convs;
    convs.count = 0;
    for (int i = 0; i < count; ++i) HIPCHK(convs.push(srcs[i], dsts[i], O[i], I[i], KK[i], mode[i], dtype[i], s));
    HIPCHK(pack_conv_multi_launch(convs, s));
    return 0;
}
static_assert(PK_COPY == DDIMX_PACK_COPY && PK_CONV == DDIMX_PACK_CONV && PK_CONVT == DDIMX_PACK_CONVT && PK_BIAS2 == DDIMX_PACK_BIAS2 &&
                  PK_PERM_COLS == DDIMX_PACK_PERM_COLS && PK_PERM_ROWS == DDIMX_PACK_PERM_ROWS && PK_CONV_F32 == DDIMX_PACK_CONV_F32,
              "the pack kinds of include/ddimx.h are the plan's");
int ddimx_debug_param_pack(ddimx_handle h, int i, int* kind, long long* offset, long long* bytes, int* dims) {
    if (!h || i < 0 || i >= (int)h->specs.size()) return fail("ddimx_debug_param_pack: index %d out of range", i);
    const ParamSpec& p = h->specs[i];
    if (kind) *kind = p.kind;
    if (offset) *offset = (long long)p.off;
    if (bytes) *bytes = (long long)p.bytes;
    if (dims) { dims[0] = p.d0; dims[1] = p.d1; dims[2] = p.d2; dims[3] = p.d3; }
    return 0;
}

}  // extern "C"

// ---- the carvers' test hooks (host.h: Carver) ----
static size_t g_carve_gap = 0;
static thread_local CarveLog* g_carve_log = nullptr;
size_t carve_gap() { return g_carve_gap; }
void carve_note(size_t off, size_t bytes) {
    CarveLog* q = g_carve_log;
    if (!q) return;
    if (q->n < q->cap) { q->off[q->n] = (long long)off; q->bytes[q->n] = (long long)bytes; }
    ++q->n;
}
// runs `carver` with the recorder on: the first `cap` regions into offsets / bytes, the number of regions into *n
template <class F>
static int record_layout(const char* who, long long* offsets, long long* bytes, int cap, int* n, F&& carver) {
    if (!n || cap < 0 || (cap > 0 && (!offsets || !bytes))) return fail("%s: null argument", who);
    CarveLog q = {offsets, bytes, cap, 0};
    g_carve_log = &q;
    carver();
    g_carve_log = nullptr;
    *n = q.n;
    return 0;
}

extern "C" {

int ddimx_debug_set_carve_gap(long long bytes) {
    if (bytes < 0 || bytes % 256) return fail("ddimx_debug_set_carve_gap: %lld is not a non-negative multiple of 256", bytes);
    g_carve_gap = (size_t)bytes;
    return 0;
}
int ddimx_debug_layout(ddimx_handle h, int which, int B, int T, long long* offsets, long long* bytes, int cap, int* n) {
    if (!h) return fail("ddimx_debug_layout: null argument");
    if (which < DDIMX_LAYOUT_WORKSPACE || which > DDIMX_LAYOUT_TAPE) return fail("ddimx_debug_layout: which = %d", which);
    if (check_shape(h, B, T)) return fail("ddimx_debug_layout: B = %d, T = %d is no shape of this network", B, T);
    return record_layout("ddimx_debug_layout", offsets, bytes, cap, n, [&] {
        Ws w; TrainWs tw; TrainTape tp;
        if (which == DDIMX_LAYOUT_WORKSPACE) carve(h, nullptr, B, T, &w);
        else if (which == DDIMX_LAYOUT_TRAIN_WORKSPACE) carve_train_ws(h, nullptr, B, T, &tw);
        else carve_tape(h, nullptr, B, T, &tp);
    });
}

struct OpWs { void *h1, *h2; float *stats, *stats2, *scale, *shift; size_t total; };
static void carve_op(char* base, int dtype, int B, int C, int H, int W, OpWs* o) {
    Carver cv{base, 0};
    const size_t act = (size_t)B * H * W * C * esz(dtype);
    o->h1 = cv.take(act);
    o->h2 = cv.take(act);
    const size_t sf = rb_stats_floats(dtype, B, C, H, W, true);
    o->stats = (float*)cv.take(sf * 4);
    o->stats2 = (float*)cv.take(sf * 4);
    o->scale = (float*)cv.take((size_t)B * C * 4);
    o->shift = (float*)cv.take((size_t)B * C * 4);
    o->total = cv.off;
}
long long ddimx_op_workspace_bytes(int dtype, int B, int C, int H, int W) {
    OpWs o;
    carve_op(nullptr, dtype, B, C, H, W, &o);
    return (long long)o.total;
}

int ddimx_resblock_fwd(int dtype, int C, const void* x, void* y, const float* temb, int temb_stride, const float* gn0_w,
                       const float* gn0_b, const void* w0, const float* gn1_w, const float* gn1_b, const void* w1,
                       const float* bias1, const float* gn2_w, void* workspace, int B, int H, int W, void* stream) {
    if (!x || !y || !workspace) return fail("ddimx_resblock_fwd: null argument");
    hipStream_t s = (hipStream_t)stream;
    OpWs o;
    carve_op((char*)workspace, dtype, B, C, H, W, &o);
    HIPCHK(tensor_stats_launch(dtype, x, o.stats, B, H * W, C, s, 1));
    RBCall q = rb_call(dtype, C, x, y, B, H, W, RBPtrs{gn0_w, gn0_b, gn1_w, gn1_b, gn2_w, bias1, w0, w1}, s);
    q.temb = temb; q.temb_stride = temb_stride; q.x_nparts = resid_nparts(dtype, H * W, C); q.x_Cs = C;
    q.h1 = o.h1; q.h2 = o.h2; q.stats = o.stats; q.stats2 = o.stats2; q.scale = o.scale; q.shift = o.shift;
    return run_resblock(q, nullptr);
}
// ---- training: Residual_Block forward that keeps its tape, and its backward --------------------------
long long ddimx_rb_tape_floats(int B, int C) { return (long long)rb_tape_small_floats(B, C); }
int ddimx_pack_conv_dgrad(int dtype, const float* w, void* dst, int O, int I, void* stream) {
    HIPCHK(pack_conv_dgrad_launch(dtype, w, dst, O, I, (hipStream_t)stream));
    return 0;
}
int ddimx_resblock_fwd_train(int dtype, int C, const void* x, void* y, const float* temb, int temb_stride, const float* gn0_w,
                             const float* gn0_b, const void* w0, const float* gn1_w, const float* gn1_b, const void* w1,
                             const float* bias1, const float* gn2_w, void* u1, void* u2, float* tape_small, void* workspace,
                             int B, int H, int W, void* stream) {
    if (!x || !y || !workspace || !u1 || !u2 || !tape_small) return fail("ddimx_resblock_fwd_train: null argument");
    hipStream_t s = (hipStream_t)stream;
    OpWs o;
    carve_op((char*)workspace, dtype, B, C, H, W, &o);
    HIPCHK(tensor_stats_launch(dtype, x, o.stats, B, H * W, C, s));
    RBTape tp = {u1, u2, tape_small};
    RBCall q = rb_call(dtype, C, x, y, B, H, W, RBPtrs{gn0_w, gn0_b, gn1_w, gn1_b, gn2_w, bias1, w0, w1}, s);
    q.temb = temb; q.temb_stride = temb_stride; q.x_nparts = resid_nparts(dtype, H * W, C); q.x_Cs = C;
    q.stats = o.stats; q.scale = o.scale; q.shift = o.shift; q.tape = &tp;
    return run_resblock(q, nullptr);
}
static void carve_rb_bwd(char* base, int dtype, int B, int C, int H, int W, RBBwdWs* w, size_t* total) {
    Carver cv{base, 0};
    const size_t act = (size_t)B * H * W * C * esz(dtype);
    w->du = cv.take(act);
    w->dg = cv.take(act);
    w->stats = (float*)cv.take(rb_bwd_stats_floats(dtype, B, H * W, C) * 4);
    w->coef = (float*)cv.take((size_t)B * 3 * C * 4);
    w->dgb = (float*)cv.take((size_t)B * 2 * C * 4);
    w->sums = (float*)cv.take((size_t)B * resid_nparts(dtype, H * W, C) * C * 4);
    w->partial = (float*)cv.take(wgrad_partial_floats(dtype, CONV3, C, C, B, H, W) * 4);
    *total = cv.off;
}
long long ddimx_resblock_bwd_workspace_bytes(int dtype, int B, int C, int H, int W) {
    RBBwdWs w;
    size_t total;
    carve_rb_bwd(nullptr, dtype, B, C, H, W, &w, &total);
    return (long long)total;
}
int ddimx_resblock_bwd(int dtype, int C, const void* x, const void* u1, const void* u2, const float* tape_small,
                       const void* dy, void* dx, const float* gn0_w, const float* gn1_w, const float* gn2_w,
                       const void* w0_dgrad, const void* w1_dgrad, float* d_gn0_w, float* d_gn0_b, float* d_w0,
                       float* d_gn1_w, float* d_gn1_b, float* d_w1, float* d_bias1, float* d_gn2_w, float* d_temb,
                       int d_temb_stride, void* workspace, int B, int H, int W, void* stream) {
    if (!x || !u1 || !u2 || !tape_small || !dy || !dx || !workspace) return fail("ddimx_resblock_bwd: null argument");
    RBBwdWs w;
    size_t total;
    carve_rb_bwd((char*)workspace, dtype, B, C, H, W, &w, &total);
    RBTape tp = {const_cast<void*>(u1), const_cast<void*>(u2), const_cast<float*>(tape_small)};
    RBGrads gr = {d_gn0_w, d_gn0_b, d_gn1_w, d_gn1_b, d_gn2_w, d_w0, d_w1, d_bias1, d_temb, d_temb_stride};
    return run_resblock_bwd(dtype, C, x, tp, dy, nullptr, dx, gn0_w, gn1_w, gn2_w, w0_dgrad, w1_dgrad, gr, w, B, H, W,
                            (hipStream_t)stream);
}
int ddimx_conv3x3_fwd_ex(int dtype, int C, const void* x, const void* w, const float* bias, const float* chan_add,
                         int chan_add_stride, const float* in_scale, const float* in_shift, int xf, int act, void* y,
                         float* stats, int plan_flags, int B, int H, int W, void* stream) {
    if (plan_flags & ~DDIMX_PLAN_BATCH)
        return fail("ddimx_conv3x3_fwd_ex: plan_flags 0x%x (only DDIMX_PLAN_BATCH is honoured)", plan_flags);
    ConvCall k = conv3_call(dtype, C, x, w, y, B, H, W);
    k.bias = bias; k.chan_add = chan_add; k.chan_add_stride = chan_add_stride;
    k.in_scale = in_scale; k.in_shift = in_shift; k.xf = xf; k.act = act;
    k.stats = stats;
    k.batch_plan = (plan_flags & DDIMX_PLAN_BATCH) != 0;
    return run_conv(k, (hipStream_t)stream, nullptr, nullptr);
}
int ddimx_conv3x3_fwd(int dtype, int C, const void* x, const void* w, const float* bias, const float* chan_add,
                      int chan_add_stride, const float* in_scale, const float* in_shift, int xf, int act, void* y,
                      float* stats, int B, int H, int W, void* stream) {
    return ddimx_conv3x3_fwd_ex(dtype, C, x, w, bias, chan_add, chan_add_stride, in_scale, in_shift, xf, act, y, stats, 0, B, H, W,
                                stream);
}
static unsigned long long* g_debug_stamps = nullptr;
int ddimx_debug_set_stamps(unsigned long long* stamps) { g_debug_stamps = stamps; return 0; }  // diagnostic builds: next conv launches stamp here
int ddimx_pack_conv_frag(const float* w, void* dst, int O, int I, void* stream) {
    if (!w || !dst) return fail("ddimx_pack_conv_frag: null argument");
    HIPCHK(pack_conv_frag_launch(w, dst, O, I, 9, (hipStream_t)stream));
    return 0;
}
int ddimx_pack_conv_frag_k(const float* w, void* dst, int O, int I, int KK, void* stream) {
    if (!w || !dst) return fail("ddimx_pack_conv_frag_k: null argument");
    HIPCHK(pack_conv_frag_launch(w, dst, O, I, KK, (hipStream_t)stream));
    return 0;
}
int ddimx_downsample_wreg_fwd(int Cin, int Cout, const void* x, const void* w_frag, const float* bias, void* y, float* stats, int B,
                              int H, int W, void* stream) {
    ConvCall d = down4_call(DT_BF16, Cin, Cout, x, w_frag, y, B, H, W);
    d.bias = bias;
    d.stats = stats;
    d.wf = w_frag;
    ConvPlan pl;
    CHK(conv_plan(d, &pl));
    if (!pl.wreg) return fail("ddimx_downsample_wreg_fwd: %d->%d %dx%d is not eligible for the register-streamed kernel", Cin, Cout, H, W);
    return run_conv(d, (hipStream_t)stream, nullptr, nullptr);
}
int ddimx_pack_frag_from_taps(const void* taps, void* dst, int ntaps, int NOUT, int CIN, void* stream) {
    if (!taps || !dst) return fail("ddimx_pack_frag_from_taps: null argument");
    HIPCHK(pack_frag_from_taps_launch(taps, dst, ntaps, NOUT, CIN, (hipStream_t)stream));
    return 0;
}
int ddimx_upsample_add_wreg_fwd(int Cin, int Cout, const void* x, const void* w_frag, const float* bias2, const void* skip, void* y,
                                float* stats, int B, int H, int W, void* stream) {
    ConvCall u = up4_call(DT_BF16, Cin, Cout, x, w_frag, skip, y, B, H, W);
    u.bias = bias2;
    u.stats = stats;
    u.wf = w_frag;
    ConvPlan pl;
    CHK(conv_plan(u, &pl));
    if (!pl.wreg) return fail("ddimx_upsample_add_wreg_fwd: %d->%d %dx%d is not eligible for the register-streamed kernel", Cin, Cout, H, W);
    return run_conv(u, (hipStream_t)stream, nullptr, nullptr);
}
int ddimx_conv3x3_pipe_fwd(int C, const void* x, const void* w_frag, const float* bias, const float* chan_add, int chan_add_stride,
                           const float* in_scale, const float* in_shift, int xf, void* y, float* group_stats, int B, int H, int W,
                           void* stream) {
    ConvCall k = conv3_call(DT_BF16, C, x, nullptr, y, B, H, W);
    k.bias = bias; k.chan_add = chan_add; k.chan_add_stride = chan_add_stride;
    k.in_scale = in_scale; k.in_shift = in_shift; k.xf = xf; k.act = 1;
    k.stats = group_stats;
    k.wf = w_frag;
    k.groups = true;
    k.kernel_pref = 2;
    k.stamps = g_debug_stamps;
    return run_conv(k, (hipStream_t)stream, nullptr, nullptr);
}
long long ddimx_conv3x3_pipe_stats_floats(int C, int B, int H, int W) {
    ConvCall k = conv3_call(DT_BF16, C, nullptr, nullptr, nullptr, B, H, W);
    k.xf = XF_AFFINE; k.act = 1;
    k.wf = &k;  // (any non-null value: only the plan is asked for)
    k.groups = true;
    k.kernel_pref = 2;
    ConvPlan pl;
    if (conv_plan(k, &pl)) return -1;
    return (long long)B * pl.wgs_per_sample * kGnSlab;
}
long long ddimx_conv_stats_floats(int dtype, int mode, int cin, int cout, int B, int H, int W) {
    const int sxy = mode == DOWN4 ? 2 : 1;
    return (long long)conv_stats_floats(dtype, mode, cin, cout, B, H / sxy, W / sxy);
}
long long ddimx_conv3x3_wgrad_partial_floats(int dtype, int C, int B, int H, int W) {
    return (long long)wgrad_partial_floats(dtype, CONV3, C, C, B, H, W);
}
int ddimx_conv3x3_wgrad(int dtype, int C, const void* a, const void* du, const float* a_scale, const float* a_shift, int xf,
                        float* partial, float* d_w, int B, int H, int W, void* stream) {
    if (!a || !du || !partial || !d_w) return fail("ddimx_conv3x3_wgrad: null argument");
    if (xf != XF_NONE && (!a_scale || !a_shift)) return fail("ddimx_conv3x3_wgrad: xf = %d without scale / shift", xf);
    return run_wgrad(dtype, CONV3, C, C, a, du, a_scale, a_shift, xf, partial, d_w, B, H, W, (hipStream_t)stream);
}
int ddimx_conv3x3_wreg_fwd(int C, const void* x, const void* w, const void* w_frag, const float* bias, const float* chan_add,
                           int chan_add_stride, const float* in_scale, const float* in_shift, int xf, int act, void* y, float* stats,
                           int B, int H, int W, void* stream) {
    ConvCall k = conv3_call(DT_BF16, C, x, w, y, B, H, W);
    k.bias = bias; k.chan_add = chan_add; k.chan_add_stride = chan_add_stride;
    k.in_scale = in_scale; k.in_shift = in_shift; k.xf = xf; k.act = act;
    k.stats = stats;
    k.wf = w_frag;
    k.kernel_pref = 1;
    k.stamps = g_debug_stamps;
    ConvPlan pl;
    CHK(conv_plan(k, &pl));
    if (!pl.wreg) return fail("ddimx_conv3x3_wreg_fwd: C=%d %dx%d xf=%d is not eligible for the register-streamed kernel", C, H, W, xf);
    return run_conv(k, (hipStream_t)stream, nullptr, nullptr);
}
int ddimx_debug_conv3x3_stamps(int dtype, int C, const void* x, const void* w, const float* chan_add, const float* in_scale,
                                const float* in_shift, void* y, float* stats, unsigned long long* stamps, int B, int H, int W,
                                void* stream) {
    // DDIMX_STAMP_XF=1 (diagnostic runs): stamp the block's second conv (affine input) instead of its first
    static const int xf = getenv("DDIMX_STAMP_XF") ? atoi(getenv("DDIMX_STAMP_XF")) : XF_AFFINE_SILU;
    ConvCall k = conv3_call(dtype, C, x, w, y, B, H, W);
    k.chan_add = chan_add; k.chan_add_stride = C;
    k.in_scale = in_scale; k.in_shift = in_shift; k.xf = xf; k.act = 1;
    k.stats = stats;
    k.stamps = stamps;
    return run_conv(k, (hipStream_t)stream, nullptr, nullptr);
}
long long ddimx_conv3x3_stats_floats(int dtype, int C, int B, int H, int W) {
    return (long long)conv_stats_floats(dtype, CONV3, C, C, B, H, W);
}
int ddimx_resid_gn_fwd(int dtype, int C, const void* x, const void* h, const float* scale, const float* shift, void* y,
                       float* stats, int B, int H, int W, void* stream) {
    HIPCHK(resid_launch(dtype, x, h, 0, scale, shift, y, stats, B, H * W, C, (hipStream_t)stream));
    return 0;
}
int ddimx_downsample_fwd(int dtype, int Cin, int Cout, const void* x, const void* w, const float* bias, void* y, int B,
                         int H, int W, void* stream) {
    ConvCall d = down4_call(dtype, Cin, Cout, x, w, y, B, H, W);
    d.bias = bias;
    return run_conv(d, (hipStream_t)stream, nullptr, nullptr);
}
int ddimx_upsample_add_fwd(int dtype, int Cin, int Cout, const void* x, const void* w, const float* bias2,
                           const void* skip, void* y, int B, int H, int W, void* stream) {
    ConvCall u = up4_call(dtype, Cin, Cout, x, w, skip, y, B, H, W);
    u.bias = bias2;
    return run_conv(u, (hipStream_t)stream, nullptr, nullptr);
}
// ---- edge convolutions and the FNet bottleneck as single ops (the whole-network call runs exactly these) ----------
long long ddimx_conv_in_stats_floats(int B, int C0, int H, int W) { return (long long)B * conv_in_nparts(H, W) * C0 * 2; }
// One refusal for the edge exports: the launcher's own plan (edge_conv.h), before anything is launched.
#define EDGE_CHK(who, op, dtype, B, C0, Cio, H, W, groups)                                              \
    do {                                                                                                \
        EdgePlan plan_;                                                                                 \
        if (const char* why_ = edge_plan(op, dtype, B, C0, Cio, H, W, groups, &plan_)) return fail(who ": %s", why_); \
    } while (0)
int ddimx_conv_in_fwd(int dtype, const float* x, const float* w, const float* bias, void* y, float* stats, int B, int Cin, int C0,
                      int H, int W, void* stream) {
    if (!x || !w || !bias || !y || !stats) return fail("ddimx_conv_in_fwd: null argument");
    EDGE_CHK("ddimx_conv_in_fwd", EDGE_CONV_IN, dtype, B, C0, Cin, H, W, 0);
    HIPCHK(conv_in_launch(dtype, x, w, bias, y, stats, B, Cin, C0, H, W, (hipStream_t)stream));
    return 0;
}
int ddimx_conv_out_fwd(int dtype, const void* a, const void* b, const float* w_packed, const float* bias, float* eps, int B, int C0,
                       int Cout, int H, int W, void* stream) {
    if (!a || !b || !w_packed || !bias || !eps) return fail("ddimx_conv_out_fwd: null argument");
    EDGE_CHK("ddimx_conv_out_fwd", EDGE_CONV_OUT, dtype, B, C0, Cout, H, W, 0);
    HIPCHK(conv_out_launch(dtype, a, b, w_packed, bias, eps, B, C0, Cout, H, W, (hipStream_t)stream));
    return 0;
}
int ddimx_debug_edge_plan(int op, int dtype, int B, int C0, int Cio, int H, int W, int groups, int* out) {
    if (!out) return fail("ddimx_debug_edge_plan: null argument");
    EdgePlan p;
    if (const char* why = edge_plan(op, dtype, B, C0, Cio, H, W, groups, &p)) return fail("ddimx_debug_edge_plan: %s", why);
    const int v[12] = {p.variant, (int)p.grid_x, (int)p.grid_y, p.threads, p.lds, p.trips, p.tiles_x, p.tiles_y, p.partial_blocks,
                       p.reduce_blocks, p.reduce_unrolled, p.reduce_tail};
    memcpy(out, v, sizeof(v));
    return 0;
}

static void carve_du_bwd(char* base, int dtype, int Cs, int Cb, int B, int Hs, int Ws, DuBwdWs* o) {
    // Cs/Hs/Ws: the SMALL (low-resolution) side, Cb the big side's channels; the bias gradient sums run over whichever side
    // carries the bias (Downsample: small side, Upsample: big side), so size for the larger of the two
    Carver cv{base, 0};
    o->partial = (float*)cv.take(wgrad_partial_floats(dtype, DOWN4, Cb, Cs, B, Hs, Ws) * 4);
    const size_t s_small = (size_t)B * resid_nparts(dtype, Hs * Ws, Cs) * Cs * 2;
    const size_t s_big = (size_t)B * resid_nparts(dtype, 4 * Hs * Ws, Cb) * Cb * 2;
    o->stats = (float*)cv.take((s_small > s_big ? s_small : s_big) * 4);
    o->dgb = (float*)cv.take((size_t)B * (Cs > Cb ? Cs : Cb) * 4);
    o->total = cv.off;
}
long long ddimx_downup_bwd_workspace_bytes(int dtype, int Csmall, int Cbig, int B, int Hsmall, int Wsmall) {
    DuBwdWs o;
    carve_du_bwd(nullptr, dtype, Csmall, Cbig, B, Hsmall, Wsmall, &o);
    return (long long)o.total;
}
int ddimx_debug_op_layout(int which, int dtype, int B, int C, int Cbig, int H, int W, long long* offsets, long long* bytes, int cap, int* n) {
    if (which < DDIMX_OP_LAYOUT_RESBLOCK || which > DDIMX_OP_LAYOUT_DOWNUP_BWD) return fail("ddimx_debug_op_layout: which = %d", which);
    return record_layout("ddimx_debug_op_layout", offsets, bytes, cap, n, [&] {
        OpWs o; RBBwdWs rw; DuBwdWs du; size_t total;
        if (which == DDIMX_OP_LAYOUT_RESBLOCK) carve_op(nullptr, dtype, B, C, H, W, &o);
        else if (which == DDIMX_OP_LAYOUT_RESBLOCK_BWD) carve_rb_bwd(nullptr, dtype, B, C, H, W, &rw, &total);
        else carve_du_bwd(nullptr, dtype, C, Cbig, B, H, W, &du);
    });
}
int ddimx_downsample_bwd(int dtype, int Cin, int Cout, const void* x, const void* dy, const void* w_dgrad, const void* dx_add, void* dx,
                         float* d_w, float* d_b, void* workspace, int B, int H, int W, void* stream) {
    if (!x || !dy || !w_dgrad || !dx || !d_w || !d_b || !workspace) return fail("ddimx_downsample_bwd: null argument");
    if ((H | W) & 1) return fail("ddimx_downsample_bwd: H, W must be even (got %d x %d)", H, W);
    DuBwdWs o;
    carve_du_bwd((char*)workspace, dtype, Cout, Cin, B, H / 2, W / 2, &o);
    return run_downsample_bwd(dtype, Cin, Cout, x, dy, w_dgrad, dx_add, dx, d_w, d_b, o, B, H / 2, W / 2, (hipStream_t)stream);
}
int ddimx_upsample_add_bwd(int dtype, int Cin, int Cout, const void* x, const void* dy, const void* w_dgrad, void* dx, float* d_w,
                           float* d_b, void* workspace, int B, int H, int W, void* stream) {
    if (!x || !dy || !w_dgrad || !dx || !d_w || !d_b || !workspace) return fail("ddimx_upsample_add_bwd: null argument");
    DuBwdWs o;
    carve_du_bwd((char*)workspace, dtype, Cin, Cout, B, H, W, &o);
    return run_upsample_bwd(dtype, Cin, Cout, x, dy, w_dgrad, dx, d_w, d_b, o, B, H, W, (hipStream_t)stream);
}
long long ddimx_edge_bwd_workspace_floats(int dtype, int B, int C0, int Cio, int H, int W) {
    EdgePlan p;
    if (const char* why = edge_plan(EDGE_WGRAD, dtype, B, C0, Cio, H, W, 0, &p)) {
        fail("ddimx_edge_bwd_workspace_floats: %s", why);
        return -1;
    }
    return (long long)edge_wgrad_partial_floats(dtype, B, C0, Cio, H, W);
}
int ddimx_conv_in_bwd(int dtype, const void* dy, const float* x, float* partial, float* d_w, float* d_b, int B, int Cin, int C0, int H,
                      int W, void* stream) {
    if (!dy || !x || !partial || !d_w || !d_b) return fail("ddimx_conv_in_bwd: null argument");
    EDGE_CHK("ddimx_conv_in_bwd", EDGE_WGRAD, dtype, B, C0, Cin, H, W, 0);
    HIPCHK(edge_wgrad_launch(dtype, 0, dy, nullptr, x, partial, d_w, d_b, B, C0, Cin, H, W, (hipStream_t)stream));
    return 0;
}
int ddimx_conv_in_bwd_data(int dtype, const void* dy, const float* w_packed, float* d_x, int B, int Cin, int C0, int H, int W,
                           void* stream) {
    if (!dy || !w_packed || !d_x) return fail("ddimx_conv_in_bwd_data: null argument");
    EDGE_CHK("ddimx_conv_in_bwd_data", EDGE_CONV_IN_BWD_DATA, dtype, B, C0, Cin, H, W, 0);
    HIPCHK(conv_in_bwd_data_launch(dtype, dy, w_packed, d_x, B, C0, Cin, H, W, (hipStream_t)stream));
    return 0;
}
int ddimx_conv_out_bwd(int dtype, const float* d_eps, const void* a, const void* b, const float* w_packed, void* d_sum, float* partial,
                       float* d_w, float* d_b, int B, int C0, int Cout, int H, int W, void* stream) {
    if (!d_eps || !a || !b || !w_packed || !d_sum || !partial || !d_w || !d_b) return fail("ddimx_conv_out_bwd: null argument");
    // the forward whose gradients these are, then the two launchers: all three before the first launch
    EDGE_CHK("ddimx_conv_out_bwd", EDGE_CONV_OUT, dtype, B, C0, Cout, H, W, 0);
    EDGE_CHK("ddimx_conv_out_bwd", EDGE_CONV_OUT_BWD_DATA, dtype, B, C0, Cout, H, W, 0);
    EDGE_CHK("ddimx_conv_out_bwd", EDGE_WGRAD, dtype, B, C0, Cout, H, W, 0);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(conv_out_bwd_data_launch(dtype, d_eps, w_packed, d_sum, B, C0, Cout, H, W, s));
    HIPCHK(edge_wgrad_launch(dtype, 1, a, b, d_eps, partial, d_w, d_b, B, C0, Cout, H, W, s));
    return 0;
}
int ddimx_temb_fwd_train(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1, const float* b1,
                         const float* w2, const float* b2, float* h1_pre, float* h2_pre, float* out, int B, int pos_ch, int emb_ch, int E,
                         void* stream) {
    return run_temb_train(te, t, w0, b0, w1, b1, w2, b2, h1_pre, h2_pre, out, B, pos_ch, emb_ch, E, (hipStream_t)stream);
}
int ddimx_temb_bwd(const float* d_out, const float* te, const int64_t* t, const float* w1, const float* w2, const float* h1_pre,
                   const float* h2_pre, float* d_h2, float* d_h1, float* d_w0, float* d_b0, float* d_w1, float* d_b1, float* d_w2,
                   float* d_b2, int B, int pos_ch, int emb_ch, int E, void* stream) {
    return run_temb_bwd(d_out, te, t, w1, w2, h1_pre, h2_pre, d_h2, d_h1, d_w0, d_b0, d_w1, d_b1, d_w2, d_b2, B, pos_ch, emb_ch, E,
                        (hipStream_t)stream);
}
// ---- the kernels of the timestep-embedding MLP one by one (run_temb / run_temb_train / run_temb_bwd issue exactly these launchers) ----
int ddimx_temb_gather(const float* table, const int64_t* t, float* out, int B, int E, void* stream) {
    if (!table || !t || !out) return fail("ddimx_temb_gather: null argument");
    if (B < 1 || B > 65535 || E < 1 || E % 4) return fail("ddimx_temb_gather: bad shape B=%d E=%d", B, E);
    HIPCHK(temb_gather_launch(table, t, out, B, E, (hipStream_t)stream));
    return 0;
}
int ddimx_linear_rows(const float* x, const int64_t* idx, const float* W, const float* bias, float* y, int B, int N, int K,
                      int act_silu, int in_silu, void* stream) {
    if (!x || !W || !bias || !y) return fail("ddimx_linear_rows: null argument");
    if (B < 1 || N < 1 || K < 1 || K % 4) return fail("ddimx_linear_rows: bad shape B=%d N=%d K=%d", B, N, K);
    HIPCHK(linear_rows_launch(x, idx, W, bias, y, B, N, K, act_silu, (hipStream_t)stream, in_silu));
    return 0;
}
int ddimx_linear_bwd_w(const float* dy, const float* x, const int64_t* idx, float* dW, float* db, int B, int N, int K, int x_silu,
                       void* stream) {
    if (!dy || !x || !dW || !db) return fail("ddimx_linear_bwd_w: null argument");
    if (B < 1 || N < 1 || N > 65535 || K < 1) return fail("ddimx_linear_bwd_w: bad shape B=%d N=%d K=%d", B, N, K);
    HIPCHK(linear_bwd_w_launch(dy, x, idx, dW, db, B, N, K, x_silu, (hipStream_t)stream));
    return 0;
}
int ddimx_linear_bwd_x(const float* dy, const float* W, const float* xpre, float* dx, int B, int N, int K, void* stream) {
    if (!dy || !W || !xpre || !dx) return fail("ddimx_linear_bwd_x: null argument");
    if (B < 1 || B > 65535 || N < 1 || K < 1) return fail("ddimx_linear_bwd_x: bad shape B=%d N=%d K=%d", B, N, K);
    HIPCHK(linear_bwd_x_launch(dy, W, xpre, dx, B, N, K, (hipStream_t)stream));
    return 0;
}

int ddimx_temb_fwd(const float* te, const int64_t* t, const float* w0, const float* b0, const float* w1, const float* b1,
                   const float* w2, const float* b2, float* h1, float* h2, float* out, int B, int pos_ch, int emb_ch, int E,
                   void* stream) {
    return run_temb(te, t, w0, b0, w1, b1, w2, b2, h1, h2, out, B, pos_ch, emb_ch, E, (hipStream_t)stream);
}

// Z[b] = Re(FFT2(X[b])) + X[b] over [B][S][hid] fp32 token matrices (the FNet mixing + residual; also its own backward).
// fused = 1: the single-launch kernel (needs ddimx_fnet_mix_supported); 0: two GEMMs through `ut` ([B][2*hid][S]) and
// `partial` (split-K scratch, 8*B*2*hid*S floats).
int ddimx_fnet_mix_supported(int S, int hid) { return fnet_mix_supported(S, hid) ? 1 : 0; }
int ddimx_fnet_mix(const float* dft_hidden, const float* dft_seq, const float* x, float* z, float* ut, float* partial, int B, int S,
                   int hid, int fused, void* stream) {
    if (fused && !fnet_mix_supported(S, hid)) return fail("ddimx_fnet_mix: S=%d hid=%d not supported by the fused kernel", S, hid);
    return fourier_mix(dft_hidden, dft_seq, x, z, ut, partial, B, S, hid, fused != 0, (hipStream_t)stream);
}

// ---- the fused dense path of the inference walk (fnet_dense.hip; run_fnet at S <= 32) one launcher at a time ----
int ddimx_fnet_fold(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, int wf_bf16, float* bf, int N,
                    int K, void* stream) {
    if (!W || !Wf || (beta && (!bias || !bf))) return fail("ddimx_fnet_fold: null argument");
    if (N < 1 || K < 1) return fail("ddimx_fnet_fold: bad shape N=%d K=%d", N, K);
    HIPCHK(fnet_fold_launch(W, gamma, beta, bias, Wf, wf_bf16, bf, N, K, (hipStream_t)stream));
    return 0;
}
int ddimx_fnet_table(const float* gamma, const float* beta, float* tab, float* bc, int H, void* stream) {
    if (!tab || (beta && !bc)) return fail("ddimx_fnet_table: null argument");
    if (H < 1) return fail("ddimx_fnet_table: bad shape H=%d", H);
    HIPCHK(fnet_table_launch(gamma, beta, tab, bc, H, (hipStream_t)stream));
    return 0;
}
int ddimx_fnet_dense_supported(int S, int K, int N) { return fnet_dense_supported(S, K, N) ? 1 : 0; }
int ddimx_fnet_dense(const void* W, const float* bias, const void* X, const float* xstats, int xnp, int xn, void* out, int x_chunk,
                     int x_bf16, int out_chunk, int out_bf16, int act, const float* R, const float* rstats, const float* rgamma,
                     const float* rbeta, int rnp, int rn, float* ostats, float eps, int S, int K, int N, int B, int bf16, void* stream) {
    if (!W || !bias || !X || !out || (R && (!rstats || !rgamma || !rbeta))) return fail("ddimx_fnet_dense: null argument");
    if (B < 1 || (xstats && xnp < 0) || (R && rn < 1)) return fail("ddimx_fnet_dense: bad shape B=%d xnp=%d rn=%d", B, xnp, rn);
    FnetDenseArgs a;
    memset(&a, 0, sizeof(a));
    a.W = W; a.bias = bias; a.X = X; a.xstats = xstats; a.xnp = xnp; a.xn = xn; a.out = out;
    a.x_chunk = x_chunk; a.x_bf16 = x_bf16; a.out_chunk = out_chunk; a.out_bf16 = out_bf16; a.act = act;
    a.R = R; a.rstats = rstats; a.rgamma = rgamma; a.rbeta = rbeta; a.rnp = rnp; a.rn = rn;
    a.ostats = ostats; a.eps = eps; a.S = S; a.K = K; a.N = N;
    HIPCHK(fnet_dense_launch(a, B, bf16, (hipStream_t)stream));
    return 0;
}
int ddimx_fnet_mix2(const float* tab, const float* dft_seq, const float* V, const float* vstats, const float* gamma, const float* beta,
                    const float* bc, float* zc, float* zstats, float eps, int S, int hid, int B, void* stream) {
    if (!tab || !dft_seq || !V || !zc || !zstats || (vstats && (!gamma || !beta || !bc))) return fail("ddimx_fnet_mix2: null argument");
    if (B < 1) return fail("ddimx_fnet_mix2: bad shape B=%d", B);
    FnetMixArgs a;
    memset(&a, 0, sizeof(a));
    a.tab = tab; a.dft_seq = dft_seq; a.V = V; a.vstats = vstats; a.gamma = gamma; a.beta = beta; a.bc = bc; a.zc = zc; a.zstats = zstats;
    a.eps = eps; a.S = S; a.hid = hid;
    HIPCHK(fnet_mix2_launch(a, B, (hipStream_t)stream));
    return 0;
}

// ---- the FNet's GEMM, LayerNorm and elementwise training kernels one by one (the walks above issue exactly these launchers) ----
// the two GEMM exports take every field of GemmArgs, the split included, from their caller
static GemmArgs gemm_args(const float* A, const float* B, float* C, const float* bias, const float* resid, float* partial, int M, int N,
                          int K, int lda, int ldb, int ldc, long long sA, long long sB, long long sC, int batch, int splitk,
                          int accumulate, int act, int bf16) {
    GemmArgs g = gemm_nt(A, B, C, M, N, K);
    g.bias = bias; g.resid = resid; g.partial = partial; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.sA = sA; g.sB = sB; g.sC = sC; g.batch = batch; g.splitk = splitk; g.accumulate = accumulate; g.act = act; g.bf16 = bf16;
    return g;
}
int ddimx_gemm_nt(const float* A, const float* B, float* C, const float* bias, const float* resid, float* partial, int M, int N, int K,
                  int lda, int ldb, int ldc, long long sA, long long sB, long long sC, int batch, int splitk, int accumulate, int act,
                  int bf16, void* stream) {
    if (!A || !B || !C) return fail("ddimx_gemm_nt: null argument");
    if (M < 1 || N < 1 || K < 1 || lda < K || ldb < K || ldc < N) return fail("ddimx_gemm_nt: bad shape M=%d N=%d K=%d lda=%d ldb=%d ldc=%d", M, N, K, lda, ldb, ldc);
    HIPCHK(gemm_launch(gemm_args(A, B, C, bias, resid, partial, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, splitk, accumulate, act, bf16),
                       (hipStream_t)stream));
    return 0;
}
int ddimx_gemm_pick_splitk(int rows_per_sample, int N, int K, int bf16) { return sample_splitk(rows_per_sample, N, K, bf16); }
int ddimx_gemm_ln(const float* A, const float* B, float* C, const float* bias, const float* resid, float* partial, int M, int N, int K,
                  int lda, int ldb, int ldc, long long sA, long long sB, long long sC, int batch, int splitk, int accumulate, int act,
                  int bf16, const float* gamma, const float* beta, float eps, float* out, void* stream) {
    if (!A || !B || !gamma || !beta || !out) return fail("ddimx_gemm_ln: null argument");
    if (M < 1 || N < 1 || K < 1 || lda < K || ldb < K || ldc < N) return fail("ddimx_gemm_ln: bad shape M=%d N=%d K=%d lda=%d ldb=%d ldc=%d", M, N, K, lda, ldb, ldc);
    HIPCHK(gemm_ln_launch(gemm_args(A, B, C, bias, resid, partial, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, splitk, accumulate, act, bf16),
                          gamma, beta, eps, out, (hipStream_t)stream));
    return 0;
}
int ddimx_layernorm(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma, const float* beta, float eps, float* y,
                    int M, int N, int chunk_rows, void* stream) {
    if (!x || !gamma || !beta || !y) return fail("ddimx_layernorm: null argument");
    if (M < 1 || N < 1 || (add && add_rows < 1)) return fail("ddimx_layernorm: bad shape M=%d N=%d add_rows=%d", M, N, add_rows);
    HIPCHK(layernorm_launch(x_dtype, x, add, add_rows, gamma, beta, eps, y, M, N, (hipStream_t)stream, chunk_rows));
    return 0;
}
int ddimx_ln_train(int x_dtype, const void* x, const float* add, int add_rows, const float* gamma, const float* beta, float eps, float* y,
                   float* sum_out, float* stat, int M, int N, float p, unsigned long long seed, unsigned mask_stream,
                   const unsigned long long* seed_ctr, void* stream) {
    if (!x || !gamma || !beta || !y || !stat) return fail("ddimx_ln_train: null argument");
    if (M < 1 || N < 1 || (add && add_rows < 1) || !(p >= 0.f && p < 1.f)) return fail("ddimx_ln_train: bad shape M=%d N=%d add_rows=%d p=%g", M, N, add_rows, (double)p);
    HIPCHK(ln_train_launch(x_dtype, x, add, add_rows, gamma, beta, eps, y, sum_out, stat, M, N, p, seed, mask_stream, (hipStream_t)stream,
                           seed_ctr));
    return 0;
}
long long ddimx_ln_bwd_partial_floats(int M, int N) { return (long long)ln_bwd_nblocks(M) * 2 * N; }
int ddimx_ln_bwd(int x_dtype, const float* dy, const void* x, const float* add, int add_rows, const float* stat, const float* gamma,
                 float* dx, float* partial, float* dgamma, float* dbeta, int M, int N, void* stream) {
    if (!dy || !x || !stat || !gamma || !dx || !partial) return fail("ddimx_ln_bwd: null argument");
    if (M < 1 || N < 1 || (add && add_rows < 1)) return fail("ddimx_ln_bwd: bad shape M=%d N=%d add_rows=%d", M, N, add_rows);
    HIPCHK(ln_bwd_launch(x_dtype, dy, x, add, add_rows, stat, gamma, dx, partial, dgamma, dbeta, M, N, (hipStream_t)stream));
    return 0;
}
int ddimx_gelu(const float* src, const float* aux, float* dst, long long n, int mode, void* stream) {
    if (!src || !dst || (mode && !aux)) return fail("ddimx_gelu: null argument");
    if (n < 1) return fail("ddimx_gelu: n = %lld", n);
    HIPCHK(gelu_launch(src, aux, dst, n, mode, (hipStream_t)stream));
    return 0;
}
int ddimx_transpose(const float* src, float* dst, int R, int C, int act_gelu, void* stream) {
    if (!src || !dst) return fail("ddimx_transpose: null argument");
    if (R < 1 || C < 1) return fail("ddimx_transpose: bad shape %d x %d", R, C);
    HIPCHK(transpose_launch(src, dst, R, C, act_gelu, (hipStream_t)stream));
    return 0;
}
int ddimx_colsum(const float* src, int B, long long stride, int C, float* dst, void* stream) {
    if (!src || !dst) return fail("ddimx_colsum: null argument");
    if (B < 1 || C < 1 || stride < C) return fail("ddimx_colsum: bad shape B=%d C=%d stride=%lld", B, C, stride);
    HIPCHK(colsum_launch(src, B, stride, C, dst, (hipStream_t)stream));
    return 0;
}
int ddimx_dropout_apply(const float* src, float* dst, long long n, float p, unsigned long long seed, unsigned mask_stream,
                        const unsigned long long* seed_ctr, void* stream) {
    if (!src || !dst) return fail("ddimx_dropout_apply: null argument");
    if (n < 1 || !(p >= 0.f && p < 1.f)) return fail("ddimx_dropout_apply: n=%lld p=%g", n, (double)p);
    HIPCHK(dropout_apply_launch(src, dst, n, p, seed, mask_stream, (hipStream_t)stream, seed_ctr));
    return 0;
}

// ---- the GroupNorm family one by one: statistics, finalisation, the residual pass, the three backward passes, their reductions
// and the data-gradient conv's statistics epilogue (the blocks and walks above issue exactly these launchers) ----
static int gn_shape_ok(const char* who, int dtype, int B, int H, int W, int C) {
    if (dtype != DT_F32 && dtype != DT_BF16) return fail("%s: dtype %d", who, dtype);
    if (B < 1 || H < 1 || W < 1 || C < 1 || C % (dtype == DT_BF16 ? 8 : 4)) return fail("%s: bad shape B=%d H=%d W=%d C=%d", who, B, H, W, C);
    return 0;
}
int ddimx_tensor_stats(int dtype, const void* x, float* stats, int B, int H, int W, int C, int groups, void* stream) {
    if (!x || !stats) return fail("ddimx_tensor_stats: null argument");
    CHK(gn_shape_ok("ddimx_tensor_stats", dtype, B, H, W, C));
    HIPCHK(tensor_stats_launch(dtype, x, stats, B, H * W, C, (hipStream_t)stream, groups));
    return 0;
}
int ddimx_gn_finalize(const float* stats, int nparts, int Cs, int C, double count, const float* gamma, const float* beta, float eps,
                      float* scale, float* shift, float* mr_out, int B, void* stream) {
    if (!stats || !gamma || !scale || !shift) return fail("ddimx_gn_finalize: null argument");
    if (B < 1 || nparts < 1 || C < 1 || Cs < C || !(count > 0.0)) return fail("ddimx_gn_finalize: bad shape B=%d nparts=%d Cs=%d C=%d count=%g", B, nparts, Cs, C, count);
    HIPCHK(gn_finalize_launch(stats, nparts, Cs, C, count, gamma, beta, eps, scale, shift, B, (hipStream_t)stream, mr_out));
    return 0;
}
int ddimx_gn_finalize_groups(const float* gstats, int np, const float* gamma, const float* beta, double count, float eps, int C,
                             float* scale, float* shift, int B, int nthreads, void* stream) {
    if (!gstats || !gamma || !scale || !shift) return fail("ddimx_gn_finalize_groups: null argument");
    if (B < 1 || np < 1 || C < 1 || !(count > 0.0)) return fail("ddimx_gn_finalize_groups: bad shape B=%d np=%d C=%d count=%g", B, np, C, count);
    const GnIn g = {gstats, gamma, beta, 1.0 / count, eps, np};
    HIPCHK(gn_finalize_groups_launch(g, C, scale, shift, B, nthreads, (hipStream_t)stream));
    return 0;
}
int ddimx_resid_threads(int dtype, int C) { return resid_threads(dtype, C); }
int ddimx_resid_iters(int dtype, int C, int H, int W) { return resid_iters(dtype, H * W, C); }
int ddimx_resid_ex(int dtype, int C, const void* x, const void* h, int h_mode, const float* scale, const float* shift,
                   const float* gn_stats, int gn_np, const float* gamma, const float* beta, double count, float eps, void* y, float* stats,
                   int groups, int B, int H, int W, void* stream) {
    if (!x || !h || !y) return fail("ddimx_resid_ex: null argument");
    CHK(gn_shape_ok("ddimx_resid_ex", dtype, B, H, W, C));
    if (h_mode < 0 || h_mode > 2) return fail("ddimx_resid_ex: h_mode %d", h_mode);
    if (gn_stats && (!gamma || gn_np < 1 || !(count > 0.0))) return fail("ddimx_resid_ex: in-kernel GroupNorm without gamma / partials / count");
    if (!gn_stats && h_mode != 1 && (!scale || !shift)) return fail("ddimx_resid_ex: h_mode %d without scale / shift", h_mode);
    const GnIn g = {gn_stats, gamma, beta, gn_stats ? 1.0 / count : 0.0, eps, gn_np};
    HIPCHK(resid_launch(dtype, x, h, h_mode, scale, shift, y, stats, B, H * W, C, (hipStream_t)stream, gn_stats ? &g : nullptr, groups));
    return 0;
}
int ddimx_gn_bwd_stats(int dtype, int mode, const void* g, const void* u, const float* scale, const float* shift, float* stats, int B,
                       int H, int W, int C, void* stream) {
    if (!g || !u || !stats) return fail("ddimx_gn_bwd_stats: null argument");
    CHK(gn_shape_ok("ddimx_gn_bwd_stats", dtype, B, H, W, C));
    if (mode < 0 || mode > 1 || (mode == 1 && (!scale || !shift))) return fail("ddimx_gn_bwd_stats: mode %d (1 needs scale / shift)", mode);
    HIPCHK(gn_bwd_stats_launch(dtype, mode, g, u, scale, shift, stats, B, H * W, C, (hipStream_t)stream));
    return 0;
}
int ddimx_gn_bwd_finalize(const float* stats, int nparts, int C, double count, const float* gamma, const float* mean_rstd, float* coef,
                          float* dgb, int B, void* stream) {
    if (!stats || !gamma || !mean_rstd || !coef || !dgb) return fail("ddimx_gn_bwd_finalize: null argument");
    if (B < 1 || nparts < 1 || C < 1 || !(count > 0.0)) return fail("ddimx_gn_bwd_finalize: bad shape B=%d nparts=%d C=%d count=%g", B, nparts, C, count);
    HIPCHK(gn_bwd_finalize_launch(stats, nparts, C, count, gamma, mean_rstd, coef, dgb, B, (hipStream_t)stream));
    return 0;
}
int ddimx_gn_bwd_apply(int dtype, int mode, const void* g, const void* u, const void* gy, const void* extra, const float* coef,
                       const float* scale, const float* shift, void* out, float* sums, const void* nu, float* nstats, int B, int H, int W,
                       int C, void* stream) {
    if (!g || !u || !coef || !out) return fail("ddimx_gn_bwd_apply: null argument");
    CHK(gn_shape_ok("ddimx_gn_bwd_apply", dtype, B, H, W, C));
    if (mode < 0 || mode > 1 || (mode == 1 && (!gy || !scale || !shift))) return fail("ddimx_gn_bwd_apply: mode %d (1 needs gy, scale, shift)", mode);
    HIPCHK(gn_bwd_apply_launch(dtype, mode, g, u, gy, extra, coef, scale, shift, out, sums, B, H * W, C, (hipStream_t)stream, nu, nstats));
    return 0;
}
int ddimx_partsum(const float* src, int B, int nparts, int C, float* dst, long long dst_stride, int src_step, void* stream) {
    if (!src || !dst) return fail("ddimx_partsum: null argument");
    if (B < 1 || nparts < 1 || C < 1 || dst_stride < C || src_step < 1) return fail("ddimx_partsum: bad shape B=%d nparts=%d C=%d dst_stride=%lld src_step=%d", B, nparts, C, dst_stride, src_step);
    HIPCHK(partsum_launch(src, B, nparts, C, dst, dst_stride, (hipStream_t)stream, src_step));
    return 0;
}
int ddimx_partsum_multi(const float* const* src, float* const* dst, const long long* dst_stride, const int* nparts, const int* C,
                        const int* B, int count, void* stream) {
    if (!src || !dst || !dst_stride || !nparts || !C || !B) return fail("ddimx_partsum_multi: null argument");
    if (count < 1 || count > PartsumBatch::kMax) return fail("ddimx_partsum_multi: %d entries (1 .. %d)", count, PartsumBatch::kMax);
    PartsumBatch q;
    memset(&q, 0, sizeof(q));
    for (int i = 0; i < count; ++i) {
        if (!src[i] || !dst[i] || B[i] < 1 || nparts[i] < 1 || C[i] < 1 || dst_stride[i] < C[i]) return fail("ddimx_partsum_multi: bad entry %d", i);
        q.src[i] = src[i]; q.dst[i] = dst[i]; q.dst_stride[i] = dst_stride[i]; q.nparts[i] = nparts[i]; q.C[i] = C[i]; q.B[i] = B[i];
    }
    q.count = count;
    HIPCHK(partsum_multi_launch(q, (hipStream_t)stream));
    return 0;
}
int ddimx_colsum_multi(const float* const* src, float* const* dst, const long long* stride, const int* B, const int* C, int count,
                       void* stream) {
    if (!src || !dst || !stride || !B || !C) return fail("ddimx_colsum_multi: null argument");
    if (count < 1 || count > ColsumBatch::kMax) return fail("ddimx_colsum_multi: %d entries (1 .. %d)", count, ColsumBatch::kMax);
    ColsumBatch q;
    memset(&q, 0, sizeof(q));
    for (int i = 0; i < count; ++i) {
        if (!src[i] || !dst[i] || B[i] < 1 || C[i] < 1 || stride[i] < C[i]) return fail("ddimx_colsum_multi: bad entry %d", i);
        q.src[i] = src[i]; q.dst[i] = dst[i]; q.stride[i] = stride[i]; q.B[i] = B[i]; q.C[i] = C[i];
    }
    q.count = count;
    HIPCHK(colsum_multi_launch(q, (hipStream_t)stream));
    return 0;
}
int ddimx_conv3x3_dgrad_stats(int dtype, int C, const void* du, const void* w_dgrad, const void* aux, const float* aux_scale,
                              const float* aux_shift, int bwd_mode, void* dg, float* stats, int* nparts, int B, int H, int W,
                              void* stream) {
    if (!du || !w_dgrad || !aux || !dg || !stats || !nparts) return fail("ddimx_conv3x3_dgrad_stats: null argument");
    if (bwd_mode < 1 || bwd_mode > 2 || (bwd_mode == 2 && (!aux_scale || !aux_shift)))
        return fail("ddimx_conv3x3_dgrad_stats: bwd_mode %d (2 needs aux_scale / aux_shift)", bwd_mode);
    CHK(gn_shape_ok("ddimx_conv3x3_dgrad_stats", dtype, B, H, W, C));
    ConvCall d = conv3_call(dtype, C, du, w_dgrad, dg, B, H, W);  // as run_resblock_bwd builds d1 / d0
    CHK(dgrad_fused_stats(d, aux, aux_scale, aux_shift, bwd_mode, stats, resid_nparts(dtype, H * W, C), nparts));
    if (!*nparts) return 0;  // the block would run gn_bwd_stats on its own: nothing is launched here
    return run_conv(d, (hipStream_t)stream, nullptr, nullptr);
}
int ddimx_conv_in_fwd_groups(int dtype, const float* x, const float* w, const float* bias, void* y, float* group_stats, int B, int Cin,
                             int C0, int H, int W, void* stream) {
    if (!x || !w || !bias || !y || !group_stats) return fail("ddimx_conv_in_fwd_groups: null argument");
    EDGE_CHK("ddimx_conv_in_fwd_groups", EDGE_CONV_IN, dtype, B, C0, Cin, H, W, 1);
    HIPCHK(conv_in_launch(dtype, x, w, bias, y, group_stats, B, Cin, C0, H, W, (hipStream_t)stream, 1));
    return 0;
}

}  // extern "C"
