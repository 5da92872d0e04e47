"""Inpainting sampler timing on one MI355X: the audio config (bf16 activations), [B, 2, T, 256], HIP events after warm-up.

Per batch size it times ms per sampler step of five variants over a 10-step schedule, alternating them round by round:
  generalized    -- (a) DDIMStepper, replayed (the plain sampler step);
  replace        -- (b) InpaintStepper, replacement only, replayed;
  guided         -- (c) InpaintStepper, guided (tape forward + residual + data-only backward + update), replayed;
  guided_eager   -- (d) the same launches without the graph;
  recipe         -- (e) INTEGRATION.md section E in a Python loop: eval-mode autograd forward / backward, the update in torch ops.
and then each new kernel alone (back-to-back launches between two events), with the bytes it must move over its time as a
share of the HBM peak.
usage: python tools/inpaint_time.py [T=1024] [rounds=5] [B ...=8 32]   (rounds = 0: the kernels alone)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddim_audio_amd as D  # noqa: E402
from ddim_audio_amd import _lib, configs, synth  # noqa: E402
from ddim_audio_amd.inpaint import InpaintStepper  # noqa: E402
from ddim_audio_amd.sampler import DDIMStepper  # noqa: E402
from ddim_audio_amd.schedule import ddim_coefficients, inpaint_coefficients, make_schedule  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X spec
SEQ = list(range(0, 1000, 100))
ZETA = 0.3


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
    m.requires_grad_(False)
    res = {k: [] for k in xts}
    try:
        for r in range(rounds + 2):  # two warm-up rounds (the first also captures every graph)
            for name in xts:
                xts[name].copy_(x_init)
                st = steppers.get(name)
                if st is not None:
                    st.rewind()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if st is not None:
                    with torch.no_grad():
                        for _ in SEQ:
                            st.step()
                else:
                    for row in c_guid:
                        _recipe_step(m, xts[name], y, mk, row)
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    res[name].append(e0.elapsed_time(e1) / len(SEQ))
    finally:
        for st in steppers.values():
            st.close()
        m.requires_grad_(True)
    return {k: {"ms_per_step": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in res.items()}


def _events(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_kernels(b, t_len, reps=20):
    lib = _lib.load()
    shape = (b, 2, t_len, 256)
    per = 2 * t_len * 256
    xt, eps, y, mk, dx = (torch.randn(shape, device="cuda") for _ in range(5))
    mk = (mk > 0).float()
    x0, seed = torch.empty_like(xt), torch.empty_like(xt)
    part = torch.empty(int(lib.ddimx_inpaint_partials_floats(b, per)), device="cuda")
    coef = torch.tensor([[500.0, 0.6, 0.8, 0.9, 0.4, 0.0, -1.5, 2.5, 0.3]], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    P = _lib.ptr
    out = []

    def report(name, ms, nbytes):
        out.append({"what": name, "B": b, "T": t_len, "ms": ms, "bytes": nbytes, "TB_per_s": nbytes / ms / 1e9,
                    "frac_of_8TBps": nbytes / HBM_PEAK / (ms * 1e-3)})

    n = xt.numel() * 4
    ms = _events(lambda: _lib.check(lib.ddimx_inpaint_residual(P(xt), P(eps), P(y), P(mk), P(x0), P(seed), P(part), P(coef), P(ctr),
                                                                b, per, _lib.stream())), reps)
    report("ddimx_inpaint_residual", ms, 6 * n)  # x_t, eps, y, m read; x0, seed written
    for flags, name, nb in ((3, "ddimx_inpaint_update guided+replace", 6 * n), (1, "ddimx_inpaint_update replace", 6 * n),
                            (0, "ddimx_ddim_update (for comparison)", 4 * n)):
        if flags == 0:
            fn = lambda: _lib.check(lib.ddimx_ddim_update(P(xt), P(eps), None, P(x0), P(coef), P(ctr), xt.numel(),  # noqa: E731
                                                          _lib.stream()))
        else:
            fn = lambda f=flags: _lib.check(lib.ddimx_inpaint_update(P(xt), P(eps), None, P(x0), P(y), P(mk), P(dx), P(part),  # noqa: E731
                                                                     P(coef), P(ctr), b, per, f, _lib.stream()))
        # guided: eps, x0, y, m, d_x read, x_t written; replace only: x_t, eps, y, m read, x0, x_t written
        report(name, _events(fn, reps), nb)
    return out


def main():
    t_len = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    bs = [int(a) for a in sys.argv[3:]] or [8, 32]
    torch.manual_seed(0)
    cfg = configs.dict2namespace(configs.audio_dict("torch.cuda.BFloat16Tensor"))
    m = D.Model(cfg)
    synth.fill_module(m, 0)
    m.eval()
    for b in bs if rounds > 0 else []:
        r = time_steps(m, b, t_len, rounds)
        r["replace_over_generalized"] = r["replace"]["ms_per_step"] / r["generalized"]["ms_per_step"]
        print(json.dumps({"what": "ms per sampler step", "B": b, "T": t_len, "dtype": "bf16", "rounds": rounds, **r}), flush=True)
    for b in bs:
        for rec in time_kernels(b, t_len):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
