// Parameter plan, weight packing (forward, inference-only copies, backward) and the gradient layout.
#include "host.h"

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

// ------------------------------------------------------------------------------------------ plan
static int add_spec(ddimx_ctx* c, const std::string& name, int kind, int d0, int d1 = 1, int d2 = 1, int d3 = 1) {
    ParamSpec s;
    s.name = name; s.kind = kind; s.d0 = d0; s.d1 = d1; s.d2 = d2; s.d3 = d3;
    s.numel = (long long)d0 * d1 * d2 * d3;
    size_t bytes;
    const size_t es = esz(c->dtype);
    switch (kind) {
        case PK_CONV: bytes = (size_t)s.numel * es; break;
        case PK_CONVT: bytes = (size_t)2 * 6 * 2 * d1 * d0 * es; break;  // [I][O][4][4] -> [2][6][2*O][I]
        case PK_BIAS2: bytes = (size_t)2 * d0 * 4; break;
        default: bytes = (size_t)s.numel * 4;
    }
    s.off = c->packed_bytes;
    s.bytes = bytes;
    c->packed_bytes += al256(bytes);
    c->specs.push_back(s);
    return (int)c->specs.size() - 1;
}

// Does a Residual_Block of width C get its conv weights a second time in MFMA fragment order (eval mode, conv_wreg.h / conv_pipe.h)?
bool rb_frag_weights(int dtype, int C) {
    WregGeom wg;
    PipeGeom pg;
    return dtype == DT_BF16 && (wreg_geometry(CONV3, C, C, &wg) == hipSuccess || pipe_geometry(C, &pg) == hipSuccess);
}

static RBW add_rb(ddimx_ctx* c, const std::string& p, int C, int k) {
    RBW r;
    r.g0 = add_spec(c, p + "norm.0.weight", PK_COPY, C);
    r.b0 = add_spec(c, p + "norm.0.bias", PK_COPY, C);
    r.g1 = add_spec(c, p + "norm.1.weight", PK_COPY, C);
    r.b1 = add_spec(c, p + "norm.1.bias", PK_COPY, C);
    r.g2 = add_spec(c, p + "norm.2.weight", PK_COPY, C);
    r.w0 = add_spec(c, p + "conv.0.weight", PK_CONV, C, C, k, k);
    r.w1 = add_spec(c, p + "conv.1.weight", PK_CONV, C, C, k, k);
    r.bias1 = add_spec(c, p + "conv.1.bias", PK_COPY, C);
    if (k == 3 && rb_frag_weights(c->dtype, C)) {  // second copy in MFMA fragment order
        c->frag_off.resize(c->specs.size(), 0);
        for (int i : {r.w0, r.w1}) {
            c->frag_off[i] = c->packed_bytes;
            c->packed_bytes += al256((size_t)9 * C * C * 2);
        }
    }
    return r;
}

static int build_plan(ddimx_ctx* c) {
    const ddimx_config& f = c->cfg;
    const int L = f.n_levels;
    c->L = L;
    c->dtype = f.act_dtype;
    if (L < 1 || L > DDIMX_MAX_LEVELS) return fail("n_levels %d out of range", L);
    if (f.act_dtype != DDIMX_F32 && f.act_dtype != DDIMX_BF16) return fail("act_dtype %d not supported", f.act_dtype);
    if (f.fnet_dtype != DDIMX_F32 && f.fnet_dtype != DDIMX_BF16) return fail("fnet_dtype %d not supported", f.fnet_dtype);
    if (f.fnet_dtype == DDIMX_BF16 && f.act_dtype != DDIMX_BF16) return fail("fnet_dtype bf16 needs act_dtype bf16");
    c->fnet_bf16 = f.fnet_dtype == DDIMX_BF16;
    for (int l = 0; l < L; ++l) {
        if (f.krn[l] != 3) return fail("kernel size %d at level %d: only 3 is implemented", f.krn[l], l);
        if (f.ch[l] % 32) return fail("channel width %d at level %d must be a multiple of 32", f.ch[l], l);
        ConvGeom g;
        if (conv_geometry(c->dtype, CONV3, f.ch[l], f.ch[l], 0, &g) != hipSuccess)
            return fail("no 3x3 conv kernel instantiated for %d channels", f.ch[l]);
        if (l > 0) {
            if (conv_geometry(c->dtype, DOWN4, f.ch[l - 1], f.ch[l], 0, &g) != hipSuccess)
                return fail("no downsample kernel instantiated for %d->%d", f.ch[l - 1], f.ch[l]);
            if (conv_geometry(c->dtype, UP4, f.ch[l], f.ch[l - 1], 0, &g) != hipSuccess)
                return fail("no upsample kernel instantiated for %d->%d", f.ch[l], f.ch[l - 1]);
        }
    }
    if (f.f_size % (1 << (L - 1))) return fail("f_size %d not divisible by 2^(levels-1)", f.f_size);
    c->Fr = f.f_size >> (L - 1);
    c->width = f.ch[L - 1] * c->Fr;
    if (c->width > 2048) return fail("FNet token width %d > 2048 not supported by the LayerNorm kernel", c->width);
    if (f.fnet_hidden > 2048) return fail("fnet hidden %d > 2048", f.fnet_hidden);
    c->packed_bytes = 0;
    c->E = 0;
    for (int l = 0; l < L; ++l) c->E += 2 * f.res[l] * f.ch[l];

    c->te = add_spec(c, "temb.te", PK_COPY, f.n_timesteps, 128);
    const int tdim[3][2] = {{512, 128}, {512, 512}, {c->E, 512}};
    for (int i = 0; i < 3; ++i) {
        c->tw[i] = add_spec(c, "temb.weight." + std::to_string(i) + ".weight", PK_COPY, tdim[i][0], tdim[i][1]);
        c->tb[i] = add_spec(c, "temb.weight." + std::to_string(i) + ".bias", PK_COPY, tdim[i][0]);
    }
    c->in_w = add_spec(c, "down_modules.0.weight", PK_COPY, f.ch[0], f.in_channels, 3, 3);
    c->in_b = add_spec(c, "down_modules.0.bias", PK_COPY, f.ch[0]);
    c->down_rb.resize(L); c->up_rb.resize(L);
    c->down_w.assign(L, -1); c->down_b.assign(L, -1); c->up_w.assign(L, -1); c->up_b.assign(L, -1);
    for (int l = 0; l < L; ++l) {
        const std::string base = "down_modules." + std::to_string(l + 1) + ".";
        int j = 0;
        if (l > 0) {
            c->down_w[l] = add_spec(c, base + "0.conv.weight", PK_CONV, f.ch[l], f.ch[l - 1], 4, 4);
            {
                WregGeom wg;
                if (c->dtype == DT_BF16 && wreg_geometry(DOWN4, f.ch[l - 1], f.ch[l], &wg) == hipSuccess) {
                    c->frag_off.resize(c->specs.size(), 0);
                    c->frag_off[c->down_w[l]] = c->packed_bytes;
                    c->packed_bytes += al256((size_t)16 * f.ch[l] * f.ch[l - 1] * 2);
                }
            }
            c->down_b[l] = add_spec(c, base + "0.conv.bias", PK_COPY, f.ch[l]);
            j = 1;
        }
        for (int r = 0; r < f.res[l]; ++r) c->down_rb[l].push_back(add_rb(c, base + std::to_string(j + r) + ".", f.ch[l], 3));
    }
    for (int k = 0; k < L; ++k) {
        const int l = L - 1 - k;
        const std::string base = "up_modules." + std::to_string(k) + ".";
        for (int r = 0; r < f.res[l]; ++r) c->up_rb[l].push_back(add_rb(c, base + std::to_string(r) + ".", f.ch[l], 3));
        if (l > 0) {
            c->up_w[l] = add_spec(c, base + std::to_string(f.res[l]) + ".conv.weight", PK_CONVT, f.ch[l], f.ch[l - 1], 4, 4);
            {
                WregGeom wg;
                if (c->dtype == DT_BF16 && wreg_geometry(UP4, f.ch[l], 2 * f.ch[l - 1], &wg) == hipSuccess) {
                    c->frag_off.resize(c->specs.size(), 0);
                    c->frag_off[c->up_w[l]] = c->packed_bytes;
                    c->packed_bytes += al256((size_t)2 * 6 * 2 * f.ch[l - 1] * f.ch[l] * 2);
                }
            }
            c->up_b[l] = add_spec(c, base + std::to_string(f.res[l]) + ".conv.bias", PK_BIAS2, f.ch[l - 1]);
        }
    }
    c->out_w = add_spec(c, "up_modules." + std::to_string(L) + ".weight", PK_CONV_F32, f.in_channels, f.ch[0], 3, 3);
    c->out_b = add_spec(c, "up_modules." + std::to_string(L) + ".bias", PK_COPY, f.in_channels);
    const int hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width;
    c->ln0_w = add_spec(c, "transformer.embedding.LayerNorm.weight", PK_PERM_COLS, 1, width);
    c->ln0_b = add_spec(c, "transformer.embedding.LayerNorm.bias", PK_PERM_COLS, 1, width);
    c->proj_w = add_spec(c, "transformer.embedding.projection.weight", PK_PERM_COLS, hid, width);
    c->proj_b = add_spec(c, "transformer.embedding.projection.bias", PK_COPY, hid);
    for (int i = 0; i < f.fnet_layers; ++i) {
        const std::string p = "transformer.encoder.layer." + std::to_string(i) + ".";
        ddimx_ctx::FL fl;
        fl.ln1_w = add_spec(c, p + "fourier.output.LayerNorm.weight", PK_COPY, hid);
        fl.ln1_b = add_spec(c, p + "fourier.output.LayerNorm.bias", PK_COPY, hid);
        fl.w1 = add_spec(c, p + "intermediate.dense.weight", PK_COPY, inter, hid);
        fl.b1 = add_spec(c, p + "intermediate.dense.bias", PK_COPY, inter);
        fl.w2 = add_spec(c, p + "output.dense.weight", PK_COPY, hid, inter);
        fl.b2 = add_spec(c, p + "output.dense.bias", PK_COPY, hid);
        fl.ln2_w = add_spec(c, p + "output.LayerNorm.weight", PK_COPY, hid);
        fl.ln2_b = add_spec(c, p + "output.LayerNorm.bias", PK_COPY, hid);
        c->fl.push_back(fl);
    }
    c->cout_w = add_spec(c, "transformer.compute_out.weight", PK_PERM_ROWS, width, hid);
    c->cout_b = add_spec(c, "transformer.compute_out.bias", PK_PERM_COLS, 1, width);
    // exactly the shapes fnet_dense_launch instantiates: K = hid = 512 -> N = inter / width ("wide"), and K = inter / width -> N = hid
    // only as the "deep" form (K >= 4 N: inter, width >= 2048) -- smaller widths take the GEMM path instead of failing in the launcher
    c->fx_on = f.fnet_layers > 0 && hid == 512 && inter % 512 == 0 && width % 512 == 0 && inter >= 2048 && width >= 2048;
    if (c->fx_on) {
        const size_t wes = c->fnet_bf16 ? 2 : 4;
        auto take = [&](size_t bytes) { const size_t o = c->packed_bytes; c->packed_bytes += al256(bytes); return o; };
        for (int i = 0; i < f.fnet_layers; ++i) {
            ddimx_ctx::FX x;
            x.w1f = take((size_t)inter * hid * wes);
            x.b1f = take((size_t)inter * 4);
            x.w2c = take((size_t)hid * inter * wes);
            x.tab = take((size_t)2 * hid * hid * 4);
            x.bc = take((size_t)hid * 4);
            c->fx.push_back(x);
        }
        c->fx_proj = take((size_t)hid * width * wes);
        c->fx_coutf = take((size_t)width * hid * wes);
        c->fx_coutb = take((size_t)width * 4);
    }
    // timestep-embedding chunk offsets in execution order (models/diffusion.py:178-184,249-250)
    int off = 0;
    for (int l = 0; l < L; ++l)
        for (int r = 0; r < f.res[l]; ++r) { c->emb_off_down.push_back(off); off += f.ch[l]; }
    for (int l = L - 1; l >= 0; --l)
        for (int r = 0; r < f.res[l]; ++r) { c->emb_off_up.push_back(off); off += f.ch[l]; }
    // the flat gradient buffer: parameter i in its own shape at grad_off[i], every slot a multiple of 64 floats
    c->grad_total = 0;
    for (const ParamSpec& p : c->specs) {
        c->grad_off.push_back(c->grad_total);
        c->grad_total += (p.numel + 63) & ~63ll;
    }
    return 0;
}

void plan_bwd_pack(const ddimx_ctx* c, BwdPack* b) {
    const ddimx_config& f = c->cfg;
    const int L = c->L;
    const size_t es = esz(c->dtype);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    b->dn_wd0.assign(L, {}); b->dn_wd1.assign(L, {}); b->up_wd0.assign(L, {}); b->up_wd1.assign(L, {});
    b->down_dg.assign(L, 0); b->up_dg.assign(L, 0);
    for (int l = 0; l < L; ++l) {
        const size_t cc = (size_t)9 * f.ch[l] * f.ch[l] * es;
        for (int r = 0; r < f.res[l]; ++r) {
            b->dn_wd0[l].push_back(take(cc)); b->dn_wd1[l].push_back(take(cc));
            b->up_wd0[l].push_back(take(cc)); b->up_wd1[l].push_back(take(cc));
        }
        if (l > 0) {
            b->down_dg[l] = take((size_t)2 * 6 * 2 * f.ch[l - 1] * f.ch[l] * es);  // Conv2d weight read as ConvTranspose2d [I=C][O=Cprev]
            b->up_dg[l] = take((size_t)16 * f.ch[l] * f.ch[l - 1] * es);           // ConvTranspose2d weight read as Conv2d [O=C][I=Cprev]
        }
    }
    const size_t hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width;
    b->projT = take(width * hid * 4);
    b->coutT = take(hid * width * 4);
    for (int i = 0; i < f.fnet_layers; ++i) { b->w1T.push_back(take(hid * inter * 4)); b->w2T.push_back(take(inter * hid * 4)); }
    b->in_dg = take((size_t)9 * f.in_channels * f.ch[0] * 4);
    b->total = off;
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

int ddimx_abi_version(void) { return DDIMX_ABI_VERSION; }
const char* ddimx_last_error(void) { return g_err; }

int ddimx_create(const ddimx_config* cfg, ddimx_handle* out) {
    if (!cfg || !out) return fail("ddimx_create: null argument");
    ddimx_ctx* c = new ddimx_ctx();
    c->cfg = *cfg;
    if (build_plan(c)) { delete c; return 1; }
    *out = c;
    return 0;
}
int ddimx_destroy(ddimx_handle h) { delete h; return 0; }
int ddimx_set_dropout_counter(ddimx_handle h, const unsigned long long* counter) {
    if (!h) return fail("ddimx_set_dropout_counter: null handle");
    h->dropout_ctr = counter;
    return 0;
}
int ddimx_num_params(ddimx_handle h) { return h ? (int)h->specs.size() : 0; }
int ddimx_param_info(ddimx_handle h, int i, const char** name, long long* numel) {
    if (!h || i < 0 || i >= (int)h->specs.size()) return fail("ddimx_param_info: index %d out of range", i);
    if (name) *name = h->specs[i].name.c_str();
    if (numel) *numel = h->specs[i].numel;
    return 0;
}
long long ddimx_packed_bytes(ddimx_handle h) { return h ? (long long)h->packed_bytes : 0; }
long long ddimx_packed_bwd_bytes(ddimx_handle h) {
    if (!h) return 0;
    BwdPack b;
    plan_bwd_pack(h, &b);
    return (long long)b.total;
}
long long ddimx_grad_floats(ddimx_handle h) { return h ? h->grad_total : 0; }
long long ddimx_grad_offset(ddimx_handle h, int i) {
    if (!h || i < 0 || i >= (int)h->specs.size()) return -1;
    return h->grad_off[i];
}

// Gradient buckets in the order the backward completes them (reverse execution order of the forward): the flat gradient buffer
// is in plan order  temb | down_modules | up_modules | transformer, so the three buckets are contiguous ranges of it.
int ddimx_grad_buckets(ddimx_handle h, long long* ranges) {
    if (!h || !ranges) return fail("ddimx_grad_buckets: null argument");
    long long lo[3] = {-1, -1, -1}, hi[3] = {0, 0, 0};
    const long long n = h->grad_total;
    for (size_t i = 0; i < h->specs.size(); ++i) {
        const ParamSpec& p = h->specs[i];
        const int b = p.name.rfind("up_modules.", 0) == 0 ? 0 : (p.name.rfind("transformer.", 0) == 0 ? 1 : 2);
        if (lo[b] < 0) lo[b] = h->grad_off[i];
        hi[b] = i + 1 < h->specs.size() ? h->grad_off[i + 1] : n;
    }
    for (int b = 0; b < 3; ++b) { ranges[2 * b] = lo[b] < 0 ? 0 : lo[b]; ranges[2 * b + 1] = lo[b] < 0 ? 0 : hi[b]; }
    // a bucket must be one contiguous run of the plan: temb + down_modules come first, then up_modules, then transformer
    if (!(ranges[4] == 0 && ranges[5] == ranges[0] && ranges[1] == ranges[2] && ranges[3] == n)) return fail("ddimx_grad_buckets: plan order changed");
    return 0;
}

int ddimx_pack_weights(ddimx_handle h, const void* const* params, int n_params, void* packed, void* stream) {
    if (!h || !params || !packed) return fail("ddimx_pack_weights: null argument");
    if (n_params != (int)h->specs.size()) return fail("ddimx_pack_weights: got %d tensors, plan has %zu", n_params, h->specs.size());
    hipStream_t s = (hipStream_t)stream;
    if (h->fx_packed == packed) h->fx_packed = nullptr;  // the folded FNet copies of this buffer are stale from here on
    if (h->frag_packed == packed) h->frag_packed = nullptr;  // ... and so are the fragment-order conv copies
    const int C5 = h->cfg.ch[h->L - 1], Fr = h->Fr;
    PackCopyBatch batch;  // plain copies (norm weights, biases, dense matrices) go out in batches of kMax per launch
    batch.count = 0;
    PackConvBatch convs;  // ... and the conv weights likewise (64 per launch)
    convs.count = 0;
    for (int i = 0; i < n_params; ++i) {
        const ParamSpec& p = h->specs[i];
        const float* src = (const float*)params[i];
        void* dst = (char*)packed + p.off;
        if (!src) return fail("ddimx_pack_weights: parameter %d (%s) is null", i, p.name.c_str());
        switch (p.kind) {
            case PK_COPY: HIPCHK(batch.push(src, (float*)dst, p.numel, s)); break;
            case PK_CONV: HIPCHK(convs.push(src, dst, p.d0, p.d1, p.d2 * p.d3, 0, h->dtype, s)); break;
            case PK_CONV_F32: HIPCHK(convs.push(src, dst, p.d0, p.d1, p.d2 * p.d3, 0, DT_F32, s)); break;
            case PK_CONVT:
                HIPCHK(pack_convT_launch(h->dtype, src, dst, p.d0, p.d1, s));
                break;
            case PK_BIAS2:
                HIPCHK(batch.push(src, (float*)dst, p.d0, s));
                HIPCHK(batch.push(src, (float*)dst + p.d0, p.d0, s));
                break;
            case PK_PERM_COLS: HIPCHK(pack_perm_cols_launch(src, (float*)dst, p.d0, C5, Fr, s)); break;
            case PK_PERM_ROWS: HIPCHK(pack_perm_rows_launch(src, (float*)dst, C5, Fr, p.d1, s)); break;
            default: return fail("bad pack kind");
        }
    }
    HIPCHK(pack_copy_multi_launch(batch, s));
    HIPCHK(pack_conv_multi_launch(convs, s));
    return 0;
}

// The inference-only second copies of the FNet weights (fnet_dense.hip: fragment order, LayerNorm gamma / beta folded in, per-layer
// DFT tables), from the fp32 copies ddimx_pack_weights wrote into `packed` (stream order).  Separate because a training step
// re-packs after every optimizer step and never reads them (38 launches); the host calls it when it packs for eval mode.
// Without it the inference walk must not take the dense FNet path: `ready` is kept in the handle.
int ddimx_pack_fnet_inference(ddimx_handle h, void* packed, void* stream) {
    if (!h || !packed) return fail("ddimx_pack_fnet_inference: null argument");
    hipStream_t s = (hipStream_t)stream;
    h->fx_packed = nullptr;
    h->frag_packed = nullptr;
    // fragment-order copies of the conv weights (conv_wreg.h / conv_pipe.h: inference walk only -- a training step re-packs after every
    // optimizer step and never reads them: 79 launches per step), re-ordered from the tap-layout copies just packed
    for (size_t i = 0; i < h->frag_off.size() && i < h->specs.size(); ++i) {
        if (!h->frag_off[i]) continue;
        const ParamSpec& p = h->specs[i];
        const char* taps = (const char*)packed + p.off;
        if (p.kind == PK_CONV) {
            HIPCHK(pack_frag_from_taps_launch(taps, (char*)packed + h->frag_off[i], p.d2 * p.d3, p.d0, p.d1, s));
        } else if (p.kind == PK_CONVT) {  // both row-parity classes of the sub-pixel form
            const size_t cls_bytes = (size_t)6 * 2 * p.d1 * p.d0 * 2;
            for (int a = 0; a < 2; ++a)
                HIPCHK(pack_frag_from_taps_launch(taps + a * cls_bytes, (char*)packed + h->frag_off[i] + a * cls_bytes, 6, 2 * p.d1, p.d0, s));
        }
    }
    h->frag_packed = packed;
    if (h->fx_on) {
        const ddimx_ctx* c = h;
        const ddimx_config& f = c->cfg;
        const int hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width, bf = c->fnet_bf16;
        char* pk = (char*)packed;
        for (int i = 0; i < f.fnet_layers; ++i) {
            const ddimx_ctx::FL& L = c->fl[i];
            const ddimx_ctx::FX& x = c->fx[i];
            HIPCHK(fnet_fold_launch(pf(c, packed, L.w1), pf(c, packed, L.ln1_w), pf(c, packed, L.ln1_b), pf(c, packed, L.b1),
                                    pk + x.w1f, bf, (float*)(pk + x.b1f), inter, hid, s));
            HIPCHK(fnet_fold_launch(pf(c, packed, L.w2), nullptr, nullptr, nullptr, pk + x.w2c, bf, nullptr, hid, inter, s));
            if (i == 0)
                HIPCHK(fnet_table_launch(nullptr, nullptr, (float*)(pk + x.tab), nullptr, hid, s));
            else
                HIPCHK(fnet_table_launch(pf(c, packed, c->fl[i - 1].ln2_w), pf(c, packed, c->fl[i - 1].ln2_b), (float*)(pk + x.tab),
                                         (float*)(pk + x.bc), hid, s));
        }
        HIPCHK(fnet_fold_launch(pf(c, packed, c->proj_w), nullptr, nullptr, nullptr, pk + c->fx_proj, bf, nullptr, hid, width, s));
        const ddimx_ctx::FL& LL = c->fl[f.fnet_layers - 1];
        HIPCHK(fnet_fold_launch(pf(c, packed, c->cout_w), pf(c, packed, LL.ln2_w), pf(c, packed, LL.ln2_b), pf(c, packed, c->cout_b),
                                pk + c->fx_coutf, bf, (float*)(pk + c->fx_coutb), width, hid, s));
        h->fx_packed = packed;
    }
    return 0;
}

int ddimx_pack_weights_bwd(ddimx_handle h, const void* const* params, int n_params, const void* packed, void* packed_bwd,
                           void* stream) {
    if (!h || !params || !packed || !packed_bwd) return fail("ddimx_pack_weights_bwd: null argument");
    if (n_params != (int)h->specs.size()) return fail("ddimx_pack_weights_bwd: got %d tensors, plan has %zu", n_params, h->specs.size());
    const ddimx_ctx* c = h;
    const ddimx_config& f = c->cfg;
    hipStream_t s = (hipStream_t)stream;
    BwdPack b;
    plan_bwd_pack(c, &b);
    char* base = (char*)packed_bwd;
    const int dt = c->dtype;
    PackConvBatch convs;  // all conv packings of the backward in two launches (pack_conv_multi_kernel)
    convs.count = 0;
    for (int l = 0; l < c->L; ++l) {
        const int C = f.ch[l];
        for (int r = 0; r < f.res[l]; ++r) {
            HIPCHK(convs.push((const float*)params[c->down_rb[l][r].w0], base + b.dn_wd0[l][r], C, C, 9, 1, dt, s));
            HIPCHK(convs.push((const float*)params[c->down_rb[l][r].w1], base + b.dn_wd1[l][r], C, C, 9, 1, dt, s));
            HIPCHK(convs.push((const float*)params[c->up_rb[l][r].w0], base + b.up_wd0[l][r], C, C, 9, 1, dt, s));
            HIPCHK(convs.push((const float*)params[c->up_rb[l][r].w1], base + b.up_wd1[l][r], C, C, 9, 1, dt, s));
        }
        if (l > 0) {
            // d(input) of Conv2d(W [C][Cprev][4][4], s2 p1) = ConvTranspose2d with the same tensor read as [I = C][O = Cprev]
            HIPCHK(pack_convT_launch(dt, (const float*)params[c->down_w[l]], base + b.down_dg[l], C, f.ch[l - 1], s));
            // d(input) of ConvTranspose2d(W [C][Cprev][4][4]) = Conv2d with the same tensor read as [O = C][I = Cprev]
            HIPCHK(convs.push((const float*)params[c->up_w[l]], base + b.up_dg[l], C, f.ch[l - 1], 16, 0, dt, s));
        }
    }
    HIPCHK(pack_conv_multi_launch(convs, s));
    const int hid = f.fnet_hidden, inter = f.fnet_inter, width = c->width;
    HIPCHK(transpose_launch(pf(c, packed, c->proj_w), (float*)(base + b.projT), hid, width, 0, s));   // [hid][width] -> [width][hid]
    HIPCHK(transpose_launch(pf(c, packed, c->cout_w), (float*)(base + b.coutT), width, hid, 0, s));   // [width][hid] -> [hid][width]
    for (int i = 0; i < f.fnet_layers; ++i) {
        HIPCHK(transpose_launch(pf(c, packed, c->fl[i].w1), (float*)(base + b.w1T[i]), inter, hid, 0, s));
        HIPCHK(transpose_launch(pf(c, packed, c->fl[i].w2), (float*)(base + b.w2T[i]), hid, inter, 0, s));
    }
    // d(x) of Conv2d(in_channels -> ch0, k3 p1) = a 3x3 conv ch0 -> in_channels with the transposed, flipped weight (fp32: the
    // network boundary's gradient is fp32)
    HIPCHK(pack_conv_dgrad_launch(DT_F32, (const float*)params[c->in_w], base + b.in_dg, f.ch[0], f.in_channels, s));
    return 0;
}

}  // extern "C"
