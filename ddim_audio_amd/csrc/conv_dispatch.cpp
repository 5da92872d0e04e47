// Conv dispatch: which kernel family and tile plan a convolution (or a weight gradient) gets, and its launch.
#include "host.h"

namespace ddimx {
hipError_t conv_geometry_bf16_c3(int, int, int, int, ConvGeom*);
hipError_t conv_geometry_bf16_du(int, int, int, int, ConvGeom*);
hipError_t conv_geometry_f32_c3(int, int, int, int, ConvGeom*);
hipError_t conv_geometry_f32_du(int, int, int, int, ConvGeom*);
hipError_t conv_launch_bf16_c3(int, int, int, int, ConvArgs&, hipStream_t);
hipError_t conv_launch_bf16_du(int, int, int, int, ConvArgs&, hipStream_t);
hipError_t conv_launch_f32_c3(int, int, int, int, ConvArgs&, hipStream_t);
hipError_t conv_launch_f32_du(int, int, int, int, ConvArgs&, hipStream_t);
hipError_t conv_launch_bf16_c3b(int, int, int, int, ConvArgs&, hipStream_t);  // + GroupNorm-backward statistics epilogue
hipError_t conv_launch_f32_c3b(int, int, int, int, ConvArgs&, hipStream_t);

hipError_t conv_geometry(int dtype, int mode, int cin, int cout, int var, ConvGeom* g) {
    const int nout = mode == UP4 ? 2 * cout : cout;
    if (dtype == DT_BF16)
        return mode == CONV3 ? conv_geometry_bf16_c3(mode, cin, nout, var, g) : conv_geometry_bf16_du(mode, cin, nout, var, g);
    return mode == CONV3 ? conv_geometry_f32_c3(mode, cin, nout, var, g) : conv_geometry_f32_du(mode, cin, nout, var, g);
}
hipError_t conv_launch(int dtype, int mode, int cin, int cout, int var, ConvArgs& a, hipStream_t s) {
    const int nout = mode == UP4 ? 2 * cout : cout;
    if (a.bwd_mode) {
        if (mode != CONV3 || !a.aux || !a.stats) return hipErrorInvalidValue;
        return dtype == DT_BF16 ? conv_launch_bf16_c3b(mode, cin, nout, var, a, s) : conv_launch_f32_c3b(mode, cin, nout, var, a, s);
    }
    if (dtype == DT_BF16)
        return mode == CONV3 ? conv_launch_bf16_c3(mode, cin, nout, var, a, s) : conv_launch_bf16_du(mode, cin, nout, var, a, s);
    return mode == CONV3 ? conv_launch_f32_c3(mode, cin, nout, var, a, s) : conv_launch_f32_du(mode, cin, nout, var, a, s);
}
int conv_pick_variant(int dtype, int mode, int cin, int cout, int B, int Hv, int Wv) {
    ConvGeom g0, g1;
    if (conv_geometry(dtype, mode, cin, cout, 0, &g0) != hipSuccess) return 0;
    if (conv_geometry(dtype, mode, cin, cout, 1, &g1) != hipSuccess) return 0;
    // The choice depends on the SAMPLE's size only (never on B): a sample then runs through the same kernels, with the same
    // statistics partition, alone or in any batch / on any number of GPUs -> bit-identical results.  The threshold is the
    // one measured at the headline batch of 8 (the large tile wins from ~256 workgroups up, i.e. >= 25 tiles per sample).
    // (The training step passes its real batch: gradients depend on the whole batch anyway, and the large tile is faster
    // once B x tiles fills the GPU.  B <= 0 selects the batch-independent rule.)
    const long long per_sample = (long long)((Wv + g0.tw - 1) / g0.tw) * ((Hv + g0.th - 1) / g0.th) * g0.classes * (g0.nout / g0.nb);
    return per_sample * (B > 0 ? B : 8) < 200 ? 1 : 0;
}
}  // namespace ddimx

static thread_local bool g_batch_plan = false;
BatchPlanScope::BatchPlanScope() { g_batch_plan = true; }
BatchPlanScope::~BatchPlanScope() { g_batch_plan = false; }

static ConvCall conv_call(int dtype, int mode, int cin, int cout, const void* in, const void* w, void* out, int B, int H, int W) {
    ConvCall q;
    q.dtype = dtype; q.mode = mode; q.cin = cin; q.cout = cout; q.in = in; q.w = w; q.out = out; q.B = B; q.Hin = H; q.Win = W;
    return q;
}
ConvCall conv3_call(int dtype, int C, const void* in, const void* w, void* out, int B, int H, int W) {
    return conv_call(dtype, CONV3, C, C, in, w, out, B, H, W);
}
ConvCall down4_call(int dtype, int cin, int cout, const void* in, const void* w, void* out, int B, int H, int W) {
    return conv_call(dtype, DOWN4, cin, cout, in, w, out, B, H, W);
}
ConvCall up4_call(int dtype, int cin, int cout, const void* in, const void* w, const void* skip, void* out, int B, int H, int W) {
    ConvCall q = conv_call(dtype, UP4, cin, cout, in, w, out, B, H, W);
    q.skip = skip;
    return q;
}

size_t conv_stats_floats(int dtype, int mode, int cin, int cout, int B, int Hv, int Wv) {
    size_t mx = 0;
    for (int var = 0; var < 2; ++var) {
        ConvGeom g;
        if (conv_geometry(dtype, mode, cin, cout, var, &g) != hipSuccess) continue;
        const size_t n = (size_t)B * cdiv(Wv, g.tw) * cdiv(Hv, g.th) * g.classes * g.nout * 2;
        if (n > mx) mx = n;
    }
    if (mode == CONV3 && cin == cout && dtype == DT_BF16) {  // the specialised kernels partition a sample into their own tiles
        WregGeom wg;
        if (wreg_geometry(CONV3, cin, cout, &wg) == hipSuccess) {
            const size_t n = (size_t)B * cdiv(Wv, wg.tw) * cdiv(Hv, wg.th) * cout * 2;
            if (n > mx) mx = n;
        }
        PipeGeom pg;  // (one 32-float slab per workgroup of >= 1 tile)
        if (pipe_geometry(cin, &pg) == hipSuccess) {
            const size_t n = (size_t)B * cdiv(Wv, pg.tw) * cdiv(Hv, pg.th) * kGnSlab;
            if (n > mx) mx = n;
        }
    }
    if (mode != CONV3 && dtype == DT_BF16) {
        WregGeom wg;
        const int nout = mode == UP4 ? 2 * cout : cout, ncls = mode == UP4 ? 2 : 1;
        if (wreg_geometry(mode, cin, nout, &wg) == hipSuccess) {
            const size_t n = (size_t)B * cdiv(Wv, wg.tw) * cdiv(Hv, wg.th) * ncls * nout * 2;
            if (n > mx) mx = n;
        }
    }
    return mx;
}

// The software-pipelined kernel (conv_pipe.h) takes the Residual_Block convs of the inference walk at the widths it is instantiated
// for (C = 32, 64): bf16, GroupNorm-affine (+ SiLU) input, SiLU output, group-format statistics, fragment-order weights, whole
// tiles.  The choice depends on the sample's size only (never on the batch).
// The walk (kernel_pref 0) takes it at C = 32 only.  With the two batch shards in flight the C = 64 form (one four-wave workgroup per
// CU: 144 registers of weights per wave) runs its B = 4 launches on half the chip, 51-63 us against conv3_wreg_kernel's 43
// (profiles/r04/pipe_v2_forked_step_kernels.txt); alone on the chip it is level (58 / 65 vs 57 / 67 us at B = 8) and in the
// single-stream step it wins (+5.5 % with both levels on).  The per-op export (kernel_pref 2) takes any instantiated width.
static bool pipe_eligible(const ConvCall& q, PipeGeom* pg) {
    if (q.kernel_pref == 1 || (q.kernel_pref != 2 && q.cin != 32)) return false;
    if (!q.wf || q.dtype != DT_BF16 || q.mode != CONV3 || q.cin != q.cout || q.act != 1 || q.aux || q.bwd_mode || q.skip || q.batch_plan || g_batch_plan)
        return false;
    if (q.xf != XF_AFFINE && q.xf != XF_AFFINE_SILU) return false;
    if (q.stats && !q.groups) return false;
    if (pipe_geometry(q.cin, pg) != hipSuccess) return false;
    return q.Hin % pg->th == 0 && q.Win % pg->tw == 0;
}
// The register-streamed-weights kernel (conv_wreg.h) takes the 3x3 convs of the inference walk from C = 64 up when the caller has
// the fragment-order weights and the image is a whole number of its tiles (sample size only, never the batch).
static bool wreg_eligible(const ConvCall& q, WregGeom* wg) {
    if (!q.wf || q.dtype != DT_BF16 || q.act > 1 || q.aux || q.bwd_mode || q.batch_plan || g_batch_plan) return false;
    if (q.skip && q.mode != UP4) return false;
    if (q.mode == UP4 && q.cout % 32) return false;  // a wave's 32-cout block must lie in ONE column parity: it runs that parity's taps only
    if (q.xf != XF_NONE && q.xf != XF_AFFINE && q.xf != XF_AFFINE_SILU) return false;
    if (wreg_geometry(q.mode, q.cin, q.mode == UP4 ? 2 * q.cout : q.cout, wg) != hipSuccess) return false;
    const int sxy = q.mode == DOWN4 ? 2 : 1;
    return q.Hin % (wg->th * sxy) == 0 && q.Win % (wg->tw * sxy) == 0;
}
int conv_plan(const ConvCall& q, ConvPlan* p) {
    ConvGeom& g = p->g;
    p->wreg = false;
    p->pipe = false;
    PipeGeom pgm;
    if (pipe_eligible(q, &pgm)) {
        p->pipe = true;
        p->Hv = q.Hin; p->Wv = q.Win; p->var = 0;
        g.th = pgm.th; g.tw = pgm.tw; g.nb = g.nout = q.cout; g.classes = 1; g.lds_bytes = pgm.lds_bytes; g.nthreads = pgm.nthreads;
        p->tiles_x = q.Win / pgm.tw;
        p->tiles_y = q.Hin / pgm.th;
        const int tiles_s = p->tiles_x * p->tiles_y;
        // persistent workgroups of 8 tiles: C = 32 (8 x 32 tiles, two workgroups per CU): 128 workgroups per T = 1024 sample, a shard of
        // four samples = one round of 512; C = 64 (one workgroup per CU): 32 per sample.  Long samples keep the tile count per workgroup
        p->tiles_per_wg = tiles_s < 8 ? tiles_s : 8;
        p->wgs_per_sample = cdiv(tiles_s, p->tiles_per_wg);
        return 0;
    }
    if (q.kernel_pref == 2) return fail("conv %d->%d %dx%d xf=%d act=%d: not eligible for the software-pipelined kernel", q.cin, q.cout, q.Hin, q.Win, q.xf, q.act);
    WregGeom wgm;
    if (wreg_eligible(q, &wgm)) {
        p->wreg = true;
        const int sxy = q.mode == DOWN4 ? 2 : 1;
        p->Hv = q.Hin / sxy; p->Wv = q.Win / sxy; p->var = 0;
        g.th = wgm.th; g.tw = wgm.tw; g.nout = q.mode == UP4 ? 2 * q.cout : q.cout; g.nb = g.nout / wgm.nsplit; g.classes = q.mode == UP4 ? 2 : 1;
        g.lds_bytes = wgm.lds_bytes; g.nthreads = wgm.nthreads;
        p->tiles_x = p->Wv / wgm.tw;
        p->tiles_y = p->Hv / wgm.th;
        const int tiles_s = p->tiles_x * p->tiles_y;
        int wps = tiles_s < 128 ? tiles_s : 128;
        if (tiles_s / 4 > wps) wps = tiles_s / 4;
        // level 2 (C = 96, twelve-wave workgroups): two tiles per workgroup -- the 6.7 us prologue (GroupNorm partials, weight
        // warm-up, first halo) is paid once per 2 x 5 us of tile work instead of once per 5: +1.5-2 % sample-fwd/s at B = 8 with
        // the two shards in flight (same-box A/B, round 3; four tiles: -4 %; the same at C = 64 / 128: -1 / -2.5 %)
        if (q.mode == CONV3 && q.cin == 96 && tiles_s >= 4 && wps > tiles_s / 2) wps = tiles_s / 2;
        // Down / Upsample: at least two tiles per workgroup from 64 tiles per sample up (+0.5-1 %, round 3)
        if (q.mode != CONV3 && tiles_s >= 64 && cdiv(tiles_s, wps) < 2) wps = tiles_s / 2;
        p->tiles_per_wg = cdiv(tiles_s, wps);
        p->wgs_per_sample = cdiv(tiles_s, p->tiles_per_wg);
        return 0;
    }
    if (q.mode == DOWN4 && ((q.Hin | q.Win) & 1)) return fail("downsample needs even H, W (got %d x %d)", q.Hin, q.Win);
    p->Hv = q.mode == DOWN4 ? q.Hin / 2 : q.Hin;
    p->Wv = q.mode == DOWN4 ? q.Win / 2 : q.Win;
    p->var = conv_pick_variant(q.dtype, q.mode, q.cin, q.cout, (q.batch_plan || g_batch_plan) ? q.B : 0, p->Hv, p->Wv);
    if (conv_geometry(q.dtype, q.mode, q.cin, q.cout, p->var, &g) != hipSuccess)
        return fail("conv %d->%d mode %d dtype %d: no kernel", q.cin, q.cout, q.mode, q.dtype);
    p->tiles_x = cdiv(p->Wv, g.tw);
    p->tiles_y = cdiv(p->Hv, g.th);
    // persistent workgroups: each walks tiles_per_wg consecutive tiles of ONE sample.  The split depends only
    // on the sample's size, never on the batch, so a sample's statistics partials (and hence its result, bit
    // for bit) are the same alone, inside any batch, or on any number of GPUs.
    const int tiles_s = p->tiles_x * p->tiles_y;
    int wps = tiles_s < 128 ? tiles_s : 128;
    if (tiles_s / 4 > wps) wps = tiles_s / 4;  // long spectrograms (T >= 2048): at most 4 tiles per workgroup, so that a
                                               // single sample still fills the 256 CUs
    if (q.cin >= 64 && tiles_s >= 512 && wps < 256) wps = 256;  // streamed-weight levels of long samples: 2 tiles per workgroup
    // Down / Upsample with exactly one tile per workgroup (levels 1-2 at T = 1024): two tiles per workgroup halve the
    // per-workgroup costs (82 KB of weights, statistics tail): 114 -> 106 / 97 -> 88 / 61 -> 58 us at B = 8
    // (profiles/r02/downup_wps.txt); a single short sample pays about 12 us per launch for the emptier grid.
    if (q.mode != CONV3 && tiles_s == 128) wps = 64;
    p->tiles_per_wg = cdiv(tiles_s, wps);
    p->wgs_per_sample = cdiv(tiles_s, p->tiles_per_wg);
    return 0;
}
// how many times over the launch fills the chip (workgroup "rounds" per CU slot)
int conv_rounds(const ConvPlan& p, int B) {
    const long long wgs = (long long)p.wgs_per_sample * B * (p.g.nout / p.g.nb) * p.g.classes;
    int per_cu = (160 * 1024) / p.g.lds_bytes;
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 2048 / p.g.nthreads) per_cu = 2048 / p.g.nthreads;
    return (int)((wgs + (long long)kNumCUs * per_cu - 1) / ((long long)kNumCUs * per_cu));
}
// Is a GroupNorm input of the launch-free inference path finished inside its consumer (true) or by a gn_finalize_groups launch?
// n: statistics partials per sample; rounds: the consumer's conv_rounds (resid: resid_rounds).
bool gn_fuse(int n, int rounds, int max_rounds) { return n <= kGnFuseMaxParts && rounds <= max_rounds; }
int resid_rounds(int dtype, int C, int B, int H, int W) {
    return (int)(((long long)resid_nparts(dtype, H * W, C) * B + kNumCUs * 8 - 1) / (kNumCUs * 8));
}
// statistics partials per sample that a launch planned as `p` writes
int conv_nparts(const ConvPlan& p, bool groups) { return p.wgs_per_sample * p.g.classes * (groups ? p.g.nout / p.g.nb : 1); }
// launches one fused conv; returns the stats slab geometry (nparts, Cs) it produced
int run_conv(const ConvCall& q, hipStream_t s, int* nparts, int* Cs) {
    ConvPlan pl;
    CHK(conv_plan(q, &pl));
    const ConvGeom& g = pl.g;
    if (pl.wreg || pl.pipe) {
        WregArgs f;
        memset(&f, 0, sizeof(f));
        f.in = q.in; f.wf = q.wf; f.skip = q.skip; f.bias = q.bias; f.chan_add = q.chan_add; f.chan_add_stride = q.chan_add_stride;
        f.in_scale = q.in_scale; f.in_shift = q.in_shift; f.gn = q.gn; f.out = q.out; f.stats = q.stats;
        f.stats_groups_c = q.groups ? q.cout : 0; f.xf = q.xf; f.act = q.act; f.stamps = q.stamps;
#ifdef DDIMX_STAMP
        { static const int dbg = getenv("DDIMX_PIPE_DBG") ? atoi(getenv("DDIMX_PIPE_DBG")) : 0; f.dbg = dbg; }
#endif
        if (q.gn.stats && q.gn.np > kGnFuseMaxParts) return fail("conv: %d statistics partials per sample cannot be finished in-kernel", q.gn.np);
        if (q.xf != XF_NONE && !q.gn.stats && (!q.in_scale || !q.in_shift)) return fail("conv: affine input without scale / shift");
        f.B = q.B; f.H = q.Hin; f.W = q.Win;
        f.tiles_x = pl.tiles_x; f.tiles_y = pl.tiles_y; f.tiles_per_wg = pl.tiles_per_wg; f.wgs_per_sample = pl.wgs_per_sample;
        if (nparts) *nparts = conv_nparts(pl, q.groups);
        if (Cs) *Cs = g.nout;
        if (pl.pipe) HIPCHK(pipe_launch(q.cin, q.xf, f, s));
        else HIPCHK(wreg_launch(q.mode, q.cin, g.nout, f, s));
        return 0;
    }
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.in = q.in; a.w = q.w; a.bias = q.bias; a.chan_add = q.chan_add; a.chan_add_stride = q.chan_add_stride;
    a.in_scale = q.in_scale; a.in_shift = q.in_shift; a.xf = q.xf; a.act = q.act;
    a.skip = q.skip; a.out = q.out; a.stats = q.stats;
    a.gn = q.gn;
    a.aux = q.aux; a.aux_scale = q.aux_scale; a.aux_shift = q.aux_shift; a.bwd_mode = q.bwd_mode;
    a.stats_groups_c = q.groups ? q.cout : 0;
    if (q.gn.stats && q.gn.np > kGnFuseMaxParts) return fail("conv: %d statistics partials per sample cannot be finished in-kernel", q.gn.np);
    if (q.groups && q.cout % kGroups) return fail("conv: group-format statistics need cout %% 8 == 0");
    a.B = q.B; a.Hin = q.Hin; a.Win = q.Win;
    a.stamps = q.stamps;
    a.Hv = pl.Hv; a.Wv = pl.Wv;
    a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y;
    a.tiles_per_wg = pl.tiles_per_wg; a.wgs_per_sample = pl.wgs_per_sample;
    const int var = pl.var;
    if (nparts) *nparts = conv_nparts(pl, q.groups);
    if (Cs) *Cs = g.nout;
    HIPCHK(conv_launch(q.dtype, q.mode, q.cin, q.cout, var, a, s));
    return 0;
}

// ---- weight gradient of one convolution: MFMA partial slabs + fixed-order reduction into dst[co][ci][taps] ----
void wgrad_plan(const WgradGeom& g, int B, int Hd, int Wd, int* tiles_x, int* tiles_y, int* nsplit, int* per) {
    *tiles_x = cdiv(Wd, g.tw);
    *tiles_y = cdiv(Hd, g.th);
    const int total = B * *tiles_x * *tiles_y;
    // workgroups per launch: 2 per CU alone on the chip; 1.5 per CU where the launch shares the chip with the data-gradient chain (the
    // weight-gradient branch, WgSide: 49.1-49.4 vs 49.5-49.9 ms per step, profiles/r04/wgside/wgrad_split_ab.txt)
    int want = 384 / g.grid_y;
    if (want < 1) want = 1;
    if (want > total) want = total;
    *per = cdiv(total, want);
    *nsplit = cdiv(total, *per);
}
size_t wgrad_partial_floats(int dtype, int mode, int ci, int co, int B, int Hd, int Wd) {
    WgradGeom g;
    if (wgrad_geometry(dtype, mode, ci, co, &g) != hipSuccess) return 0;
    int tx, ty, ns, per;
    wgrad_plan(g, B, Hd, Wd, &tx, &ty, &ns, &per);
    return (size_t)ns * g.ntaps * co * ci;
}
// a: [B][Ha][Wa][ci] (halo operand, transformed by xf), du: [B][Hd][Wd][co]; dst fp32 [co][ci][taps]
int run_wgrad(int dtype, int mode, int ci, int co, const void* a_t, const void* du, const float* a_scale,
                     const float* a_shift, int xf, float* partial, float* dst, int B, int Hd, int Wd, hipStream_t s) {
    WgradGeom g;
    if (wgrad_geometry(dtype, mode, ci, co, &g) != hipSuccess)
        return fail("weight gradient %d x %d mode %d dtype %d: no kernel", ci, co, mode, dtype);
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.a = a_t; a.du = du; a.a_scale = a_scale; a.a_shift = a_shift; a.xf = xf; a.partial = partial;
    a.B = B; a.Hd = Hd; a.Wd = Wd;
    a.Ha = mode == DOWN4 ? 2 * Hd : Hd;
    a.Wa = mode == DOWN4 ? 2 * Wd : Wd;
    int ns;
    wgrad_plan(g, B, Hd, Wd, &a.tiles_x, &a.tiles_y, &ns, &a.tiles_per_wg);
    a.total_tiles = B * a.tiles_x * a.tiles_y;
    HIPCHK(wgrad_launch(dtype, mode, ci, co, a, ns, s));
    HIPCHK(wgrad_reduce_launch(partial, ns, g.ntaps, co, ci, dst, s));
    return 0;
}

extern "C" {

int ddimx_debug_conv_plan(int dtype, int mode, int cin, int cout, int B, int H, int W, int flags, int* out) {
    if (!out) return fail("ddimx_debug_conv_plan: null argument");
    static const char tag = 0;  // any non-null address: conv_plan only tests the pointers it is given for null
    const void* nz = &tag;
    ConvCall q = conv_call(dtype, mode, cin, cout, nz, nz, nullptr, B, H, W);
    q.xf = DDIMX_PLAN_XF_OF(flags);
    q.act = DDIMX_PLAN_ACT_OF(flags);
    q.skip = (flags & DDIMX_PLAN_SKIP) ? nz : nullptr;
    q.stats = (flags & DDIMX_PLAN_STATS) ? (float*)nz : nullptr;
    q.wf = (flags & DDIMX_PLAN_WFRAG) ? nz : nullptr;
    q.groups = (flags & DDIMX_PLAN_GROUPS) != 0;
    q.batch_plan = (flags & DDIMX_PLAN_BATCH) != 0;
    q.kernel_pref = DDIMX_PLAN_PREF_OF(flags);
    if (flags & DDIMX_PLAN_BWD) { q.aux = nz; q.bwd_mode = 1; }
    ConvPlan pl;
    CHK(conv_plan(q, &pl));
    const int v[12] = {pl.pipe ? DDIMX_FAMILY_PIPE : pl.wreg ? DDIMX_FAMILY_WREG : DDIMX_FAMILY_RING, pl.var, pl.tiles_x, pl.tiles_y,
                       pl.tiles_per_wg, pl.wgs_per_sample, conv_rounds(pl, B), pl.g.th, pl.g.tw, pl.g.nthreads, pl.Hv, pl.Wv};
    memcpy(out, v, sizeof(v));
    return 0;
}
int ddimx_debug_wgrad_plan(int dtype, int mode, int ci, int co, int B, int Hd, int Wd, int* out) {
    if (!out) return fail("ddimx_debug_wgrad_plan: null argument");
    WgradGeom g;
    if (wgrad_geometry(dtype, mode, ci, co, &g) != hipSuccess)
        return fail("weight gradient %d x %d mode %d dtype %d: no kernel", ci, co, mode, dtype);
    int tx, ty, ns, per;
    wgrad_plan(g, B, Hd, Wd, &tx, &ty, &ns, &per);
    const int v[8] = {tx, ty, ns, per, wgrad_reduce_kind(ns, g.ntaps, co, ci), g.th, g.tw, g.ntaps};
    memcpy(out, v, sizeof(v));
    return 0;
}
int ddimx_debug_gn_plan(int dtype, int C, int B, int H, int W, int x_nparts, int* out) {
    if (!out) return fail("ddimx_debug_gn_plan: null argument");
    static const char tag = 0;  // any non-null address: conv_plan only tests the pointers it is given for null
    void* nz = (void*)&tag;
    const void* wf = rb_frag_weights(dtype, C) ? nz : nullptr;  // the fragment copies the walk's packing has
    int v[9];
    int n_in = x_nparts;
    for (int k = 0; k < 2; ++k) {  // the two convs, built and planned as run_resblock builds and plans them
        const ConvCall q = rb_conv_call(dtype, C, k, nz, nz, wf, (const float*)nz, (const float*)nz, C, (float*)nz, (float*)nz, nz,
                                        (float*)nz, B, H, W);
        ConvPlan pl;
        CHK(conv_plan(q, &pl));
        const bool fused = gn_fuse(n_in, conv_rounds(pl, B), kGnFuseConvRounds);
        v[3 * k] = n_in;
        v[3 * k + 1] = fused ? 1 : 0;
        v[3 * k + 2] = n_in = conv_nparts(pl, q.groups);  // this conv's output partials = the next consumer's input partials
    }
    v[6] = n_in;
    v[7] = gn_fuse(n_in, resid_rounds(dtype, C, B, H, W), kGnFuseResidRounds) ? 1 : 0;
    v[8] = resid_nparts(dtype, H * W, C);
    memcpy(out, v, sizeof(v));
    return 0;
}

}  // extern "C"
