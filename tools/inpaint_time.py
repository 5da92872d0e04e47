"""Inpainting sampler timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Per batch size it times ms per sampler step of five variants over a 10-step schedule, one after the other in every round (the
same order each time, no untimed step in front of the window: the figures quoted from this tool were taken that way):
  generalized    -- (a) DDIMStepper, replayed (the plain sampler step);
  replace        -- (b) InpaintStepper, replacement only, replayed;
  guided         -- (c) InpaintStepper, guided (tape forward + residual + data-only backward + update), replayed;
  guided_eager   -- (d) the same launches without the graph;
  recipe         -- (e) INTEGRATION.md section E in a Python loop: eval-mode autograd forward / backward, the update in torch ops.
and then each new kernel alone (back-to-back launches between two events), with the bytes it must move over its time as a
share of the HBM peak.
usage: python tools/inpaint_time.py [T=1024] [rounds=5] [B ...=8 32]   (rounds = 0: the kernels alone)
"""
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402
from ddim_audio_amd import _lib  # noqa: E402
from ddim_audio_amd.inpaint import InpaintStepper  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, inpaint_coefficients, make_schedule  # noqa: E402

SEQ = list(range(0, 1000, 100))
ZETA = 0.3


@torch.enable_grad()
def _recipe_step(m, xt, y, mk, row):
    ti, s1, s2, s3, c2, _ = [float(v) for v in row[:6]]
    t = torch.full((xt.size(0),), int(ti), device=xt.device)
    x = xt.detach().requires_grad_(True)
    eps = m(x, t)
    x0 = (x - s1 * eps) / s2
    L = (mk * (x0 - y)).square().flatten(1).sum(1)
    (g,) = torch.autograd.grad(L.sum(), x)
    with torch.no_grad():
        eps, x0 = eps.detach(), x0.detach()
        u = s3 * x0 + c2 * eps - (ZETA / L.sqrt()).view(-1, 1, 1, 1) * g
        xt.copy_(mk * (s3 * y + c2 * eps) + (1 - mk) * u)


def time_steps(m, b, t_len, rounds):
    shape = (b, 2, t_len, 256)
    x_init = torch.randn(shape, device="cuda")
    y = torch.randn(shape, device="cuda")
    mk = torch.ones(b, 1, t_len, 1, device="cuda")
    mk[:, :, t_len // 4: t_len // 2] = 0
    mk = mk.expand(shape).contiguous()
    y = (y * mk).contiguous()
    alphas = make_schedule(m._full_config.diffusion)[1]
    c_plain = ddim_coefficients(SEQ, alphas, 0.0)
    c_repl = inpaint_coefficients(SEQ, alphas, 0.0, 0.0)
    c_guid = inpaint_coefficients(SEQ, alphas, 0.0, ZETA)
    xts = {k: x_init.clone() for k in ("generalized", "replace", "guided", "guided_eager", "recipe")}
    with torch.no_grad():
        steppers = {
            "generalized": DDIMStepper(m, xts["generalized"], c_plain),
            "replace": InpaintStepper(m, xts["replace"], y, mk, c_repl, False, True),
            "guided": InpaintStepper(m, xts["guided"], y, mk, c_guid, True, True),
            "guided_eager": InpaintStepper(m, xts["guided_eager"], y, mk, c_guid, True, True, use_graph=False),
        }
    legs = {k: timing.stepper_leg(st, xts[k], x_init, len(SEQ), untimed=0) for k, st in steppers.items()}
    assert len(c_guid) == len(SEQ)
    rows = itertools.cycle(c_guid)  # the recipe has no stepper: every round walks the table once
    legs["recipe"] = timing.Leg(lambda: xts["recipe"].copy_(x_init), lambda: _recipe_step(m, xts["recipe"], y, mk, next(rows)), len(SEQ), 0)
    m.requires_grad_(False)
    try:
        return timing.time_legs(legs, rounds, fixed_order=True, expect_captures=None)[0]
    finally:
        m.requires_grad_(True)


def time_kernels(b, t_len):
    lib = _lib.load()
    shape = (b, 2, t_len, 256)
    per = 2 * t_len * 256
    xt, eps, y, mk, dx = (torch.randn(shape, device="cuda") for _ in range(5))
    mk = (mk > 0).float()
    x0, seed = torch.empty_like(xt), torch.empty_like(xt)
    part = torch.empty(int(lib.ddimx_inpaint_partials_floats(b, per)), device="cuda")
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.9, 0.4, 0.0, -1.5, 2.5, 0.3]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    P, n = _lib.ptr, xt.numel() * 4
    out = []

    def report(name, fn, passes):
        out.append(timing.bandwidth_record(name, timing.time_launches(fn, reps=20, warm=3), passes, n, B=b, T=t_len))

    # x_t, eps, y, m read; x0, seed written
    report("ddimx_inpaint_residual", lambda: _lib.check(lib.ddimx_inpaint_residual(P(xt), P(eps), P(y), P(mk), P(x0), P(seed), P(part), P(coef),
                                                                                 P(ctr), b, per, _lib.stream())), 6)
    # guided: eps, x0, y, m, d_x read, x_t written; replace only: x_t, eps, y, m read, x0, x_t written
    for flags, name in ((3, "ddimx_inpaint_update guided+replace"), (1, "ddimx_inpaint_update replace")):
        report(name, lambda: _lib.check(lib.ddimx_inpaint_update(P(xt), P(eps), None, P(x0), P(y), P(mk), P(dx), P(part), P(coef), P(ctr), b,
                                                                 per, flags, _lib.stream())), 6)
    report("ddimx_ddim_update (for comparison)",
           lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef), P(ctr), xt.numel(), _lib.stream())), 4)
    return out


def main(argv=None):
    a = timing.parse_args(argv, {"T": 1024, "rounds": 5, "B": [8, 32]})
    torch.manual_seed(0)
    m = timing.audio_model()
    for b in a.B if a.rounds > 0 else []:
        r = time_steps(m, b, a.T, a.rounds)
        r["replace_over_generalized"] = r["replace"]["ms_per_step"] / r["generalized"]["ms_per_step"]
        print(json.dumps({"what": "ms per sampler step", "B": b, "T": a.T, "dtype": "bf16", "rounds": a.rounds, **r}), flush=True)
    for b in a.B:
        for rec in time_kernels(b, a.T):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
