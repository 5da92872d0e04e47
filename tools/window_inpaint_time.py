"""Windowed inpainting timing on one MI355X: the audio config (bf16 activations), N W = 8 windows of T = 1024 at hop 512 on one canvas
of L = 4608, HIP events after warm-up (every round times each leg once, 10 replayed steps between two events, the order within a
round alternates, the spread of every leg over the rounds is reported).

In one process, ms per replayed sampler step over the same 20-entry log-SNR schedule of
  windowed_ddim      -- WindowStepper (windowed_steps, eta = 0): the yardstick of the replacement-only step;
  winp_replace_only  -- WindowInpaintStepper, guidance 0: gather, forward, one ddimxwi_update launch;
  inpaint_guided     -- InpaintStepper (inpaint_steps, guidance 0.3) at B = 8, T = 1024: the yardstick of the guided step;
  winp_guided        -- WindowInpaintStepper, guidance 0.3: gather, tape-keeping forward, ddimxwi_residual, data-only backward,
                        ddimxwi_update.
Then the kernels alone (50 calls captured into one graph, the replay between two events): us per call and the bytes they move as a
share of the 8 TB/s HBM peak, next to ddimx_inpaint_residual / ddimx_inpaint_update at B = 8.
With ``unchanged``: only windowed_ddim and inpaint_guided -- the two paths that existed before -- so no ddimxwi_ function is touched
and the same file can time another build of the library and of the package (``DDIMX_LIB``, or a copy of this file in another
checkout's tools/).
usage: python tools/window_inpaint_time.py [rounds=5] [unchanged]   (rounds = 0: the kernels alone)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.inpaint import InpaintStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, inpaint_coefficients, logsnr_seq, make_schedule, window_plan  # noqa: E402
from ddim_audio_amd.window import WindowStepper  # noqa: E402

T, H, F = 1024, 512, 256
N_TIMED = 10
N, W = 1, 8
ZETA = 0.3


def _known(shape):
    """A packet-loss mask (a quarter of the rows missing) and the known content, canvas- or batch-shaped."""
    y = torch.randn(shape, device="cuda")
    mask = torch.ones(shape, device="cuda")
    mask[:, :, shape[2] // 4: shape[2] // 2] = 0
    return y * mask, mask


def time_case(m, rounds, unchanged):
    length = T + (W - 1) * H
    alphas = make_schedule(m._full_config.diffusion)[1]
    seq = logsnr_seq(alphas, 20)
    xc, xb = torch.randn((N, 2, length, F), device="cuda"), torch.randn((N * W, 2, T, F), device="cuda")
    (yc, mc), (yb, mb) = _known(xc.shape), _known(xb.shape)
    guided, plain = inpaint_coefficients(seq, alphas, 0.0, ZETA), inpaint_coefficients(seq, alphas, 0.0, 0.0)
    with torch.no_grad():
        # the backward packing is allocated before any leg captures: allocating it later would make the graphs captured so far stale
        m.prepare(xc.device, T)
        m._ensure_packed_bwd(_lib.load(), xc.device)
        xs = [xc.clone(), xc.clone(), xb.clone(), xc.clone()]
        legs = {"windowed_ddim": timing.stepper_leg(WindowStepper(m, xs[0], ddim_coefficients(seq, alphas, 0.0), T, H, "tri"), xs[0], xc, N_TIMED),
                "inpaint_guided": timing.stepper_leg(InpaintStepper(m, xs[2], yb, mb, guided, True, True), xs[2], xb, N_TIMED)}
        if not unchanged:
            from ddim_audio_amd.window_inpaint import WindowInpaintStepper
            legs["winp_replace_only"] = timing.stepper_leg(WindowInpaintStepper(m, xs[1], yc, mc, plain, False, True, T, H, "tri"), xs[1], xc,
                                                           N_TIMED)
            legs["winp_guided"] = timing.stepper_leg(WindowInpaintStepper(m, xs[3], yc, mc, guided, True, True, T, H, "tri"), xs[3], xc,
                                                     N_TIMED)
    r, _ = timing.time_legs(legs, rounds)
    out = {"what": "ms per replayed sampler step", "N": N, "W": W, "T": T, "H": H, "L": length, "dtype": "bf16", "rounds": rounds,
           "lib": os.path.basename(os.path.dirname(os.path.dirname(_lib.LIB_PATH))) + "/" + os.path.basename(_lib.LIB_PATH), **r}
    if not unchanged:
        out["winp_replace_only_minus_windowed_ddim_ms"] = r["winp_replace_only"]["ms_per_step"] - r["windowed_ddim"]["ms_per_step"]
        out["winp_guided_minus_inpaint_guided_ms"] = r["winp_guided"]["ms_per_step"] - r["inpaint_guided"]["ms_per_step"]
    return out


def time_kernels():
    lib, P = _lib.load(), _lib.ptr
    length = T + (W - 1) * H
    canvas, x0, beps, nz = (torch.randn((N, 2, length, F), device="cuda") for _ in range(4))
    y, mask = _known(canvas.shape)
    eps, seed, dwin = (torch.randn((N * W, 2, T, F), device="cuda") for _ in range(3))
    p = window_plan(length, T, H, "tri")
    jf, cn, wt = (torch.from_numpy(v.copy()).cuda() for v in (p.jfirst, p.cnt, p.wt))
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.6, 0.4, 0.1, -1.5, 2.5, ZETA]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    geom = (N, W, 2, length, T, H, F)
    per = canvas[0].numel()
    parts = torch.zeros(int(lib.ddimxwi_partials_floats(N, per)), device="cuda")
    m_b, c_b = eps.numel() * 4, canvas.numel() * 4
    out = []

    def report(name, fn, nbytes, note):
        canvas.normal_()
        ms = timing.time_graph_replay(fn, reps=50, warm=3)
        out.append({**timing.bandwidth_record(name, ms, 1, nbytes, unit="us", N=N, W=W), "note": note})

    def residual():
        _lib.check(lib.ddimxwi_residual(P(canvas), P(eps), P(y), P(mask), P(x0), P(beps), P(seed), P(parts), P(jf), P(cn), P(wt), P(coef),
                                        P(ctr), *geom, _lib.stream()))

    def update(flags, e, noise=None):
        return lambda: _lib.check(lib.ddimxwi_update(P(canvas), P(e), P(noise), P(x0), P(y), P(mask), P(dwin), P(parts), P(jf), P(cn), P(wt),
                                                     P(coef), P(ctr), *geom, flags, _lib.stream()))

    report("ddimxwi_residual", residual, 2 * m_b + 5 * c_b, "eps read, seed written; x, y, mask read, x0 and the blend written")
    residual()
    report("ddimxwi_update guided + replace", update(3, beps), m_b + 6 * c_b, "d_win read; blend, x0, y, mask, x read; x written")
    report("ddimxwi_update replace only", update(1, eps), m_b + 5 * c_b, "eps read; x, y, mask read; x0 and x written")
    report("ddimxwi_update replace only, with noise", update(1, eps, nz), m_b + 6 * c_b, "+ the canvas-shaped noise read")
    # the yardsticks at B = N W, T: as many network elements
    xb, eb, sb, db, x0b = (torch.randn((N * W, 2, T, F), device="cuda") for _ in range(5))
    yb, mb = _known(xb.shape)
    pb = torch.zeros(int(lib.ddimx_inpaint_partials_floats(N * W, xb[0].numel())), device="cuda")
    report("ddimx_inpaint_residual at batch N W", lambda: _lib.check(lib.ddimx_inpaint_residual(
        P(xb), P(eb), P(yb), P(mb), P(x0b), P(sb), P(pb), P(coef), P(ctr), N * W, xb[0].numel(), _lib.stream())), 6 * m_b,
        "x, eps, y, mask read; x0 and seed written")
    report("ddimx_inpaint_update guided + replace at batch N W", lambda: _lib.check(lib.ddimx_inpaint_update(
        P(xb), P(eb), None, P(x0b), P(yb), P(mb), P(db), P(pb), P(coef), P(ctr), N * W, xb[0].numel(), 3, _lib.stream())), 6 * m_b,
        "eps, x0, y, mask, d_x read; x written")
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"rounds": 5}, flags=("unchanged",))
    timing.require_gpu()
    torch.manual_seed(0)
    if not a.unchanged:
        for rec in time_kernels():
            print(json.dumps(rec), flush=True)
    if a.rounds > 0:
        print(json.dumps(time_case(timing.audio_model(), a.rounds, a.unchanged)), flush=True)


if __name__ == "__main__":
    main()
