"""Time one Downsample or Upsample(+skip) launch of the inference walk (bf16, register-streamed weights; HIP events) and print the
launch plan beside it: downup_time.py {down|up} LEVEL B   (LEVEL = the smaller-resolution level, 1..5)."""
import ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddim_audio_amd import _lib
kind, lvl, B = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
lib = _lib.load()
dt, tdt = _lib.DDIMX_BF16, torch.bfloat16
CH = [32, 64, 96, 128, 192, 256]
cp, c = CH[lvl - 1], CH[lvl]
H, W = 1024 >> (lvl - 1), 256 >> (lvl - 1)
st = _lib.stream()
big = torch.randn(B, H, W, cp, device="cuda").to(tdt); small = torch.randn(B, H // 2, W // 2, c, device="cuda").to(tdt)
wd = torch.empty(16 * c * cp, dtype=tdt, device="cuda")
w32 = torch.randn(c, cp, 4, 4, device="cuda") * 0.02
_lib.check(lib.ddimx_pack_conv_frag_k(_lib.ptr(w32), _lib.ptr(wd), c, cp, 16, st))
wt = torch.randn(c, cp, 4, 4, device="cuda") * 0.02
wp = torch.empty(2 * 6 * 2 * cp * c, dtype=tdt, device="cuda"); wu = torch.empty_like(wp)
_lib.check(lib.ddimx_pack_convT(dt, _lib.ptr(wt), _lib.ptr(wp), c, cp, st))
per = 6 * 2 * cp * c
for a in range(2):
    _lib.check(lib.ddimx_pack_frag_from_taps(_lib.ptr(wp[a * per:]), _lib.ptr(wu[a * per:]), 6, 2 * cp, c, st))
bd = torch.zeros(c, device="cuda"); bu = torch.zeros(2 * cp, device="cuda")
yd, yu = torch.empty_like(small), torch.empty_like(big)
mode, flags = (1, _lib.DDIMX_PLAN_WFRAG | _lib.DDIMX_PLAN_STATS) if kind == "down" else (2, _lib.DDIMX_PLAN_WFRAG | _lib.DDIMX_PLAN_STATS | _lib.DDIMX_PLAN_SKIP)
cin, cout, Hi, Wi = (cp, c, H, W) if kind == "down" else (c, cp, H // 2, W // 2)
stats = torch.empty(int(lib.ddimx_conv_stats_floats(dt, mode, cin, cout, B, Hi, Wi)), device="cuda")
plan = (ctypes.c_int * 12)()
_lib.check(lib.ddimx_debug_conv_plan(dt, mode, cin, cout, B, Hi, Wi, flags, plan))
fam, _, tx, ty, tpw, wps, rounds, th, tw, nthr = list(plan)[:10]
def run(n):
    for _ in range(n):
        if kind == "down":
            _lib.check(lib.ddimx_downsample_wreg_fwd(cp, c, _lib.ptr(big), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(yd), _lib.ptr(stats), B, H, W, st))
        else:
            _lib.check(lib.ddimx_upsample_add_wreg_fwd(c, cp, _lib.ptr(small), _lib.ptr(wu), _lib.ptr(bu), _lib.ptr(big), _lib.ptr(yu), _lib.ptr(stats), B, H // 2, W // 2, st))
run(5); torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(); run(50); e1.record(); torch.cuda.synchronize()
print(kind, "level", lvl, "B", B, "us/launch %.1f" % (e0.elapsed_time(e1) * 1e3 / 50),
      f"| tile {th}x{tw}, {nthr} threads, {tx}x{ty} tiles per sample, {tpw} per workgroup, {wps} workgroups per sample and cout split, {rounds} round(s)")
