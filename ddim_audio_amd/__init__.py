"""ddim_audio_amd -- MI355X-native DDIM denoising hot path behind the reference's Python API.

Public names mirror the reference's modules for this path (klae01/ddim-audio):
``Model`` (models/diffusion.py), ``generalized_steps`` (functions/denoising.py),
``noise_estimation_loss`` (functions/losses.py), ``EMAHelper`` (models/ema.py), plus the schedule
helpers of runners/diffusion.py.  All tensor arithmetic runs in ``libddimx.so`` (hand-written HIP for
gfx950, C ABI in ``include/ddimx.h``); nothing here falls back to CPU or eager PyTorch.
"""
from . import configs, schedule, synth  # noqa: F401  (pure host logic, importable without the library)


def __getattr__(name):
    if name == "Model":
        from .model import Model
        return Model
    if name in ("generalized_steps", "ddpm_steps"):
        from . import sampler
        return getattr(sampler, name)
    if name == "inpaint_steps":
        from .inpaint import inpaint_steps
        return inpaint_steps
    if name == "inpaint_solver_steps":
        from .inpaint_solver import inpaint_solver_steps
        return inpaint_solver_steps
    if name == "dpm_solver_steps":
        from .solver import dpm_solver_steps
        return dpm_solver_steps
    if name in ("windowed_steps", "windowed_solver_steps"):
        from . import window
        return getattr(window, name)
    if name == "windowed_inpaint_steps":
        from .window_inpaint import windowed_inpaint_steps
        return windowed_inpaint_steps
    if name == "windowed_inpaint_solver_steps":
        from .window_inpaint_solver import windowed_inpaint_solver_steps
        return windowed_inpaint_solver_steps
    if name in ("invert_steps", "slerp"):
        from . import invert
        return getattr(invert, name)
    if name == "SamplerPool":
        from .pool import SamplerPool
        return SamplerPool
    if name == "RestorePool":
        from .restore_pool import RestorePool
        return RestorePool
    if name in ("X0Clip", "X0Threshold"):
        return getattr(schedule, name)
    if name in ("NoiseStream", "BrownianStream"):
        from . import noise
        return getattr(noise, name)
    if name in ("distill_target", "distill_step"):
        from . import distill
        return getattr(distill, name)
    if name in ("consistency_target", "consistency_step", "consistency_steps", "consistency_loss", "ConsistencyStepper"):
        from . import consistency
        return getattr(consistency, name)
    if name in ("log_likelihood", "Likelihood", "LikelihoodStepper"):
        from . import likelihood
        return getattr(likelihood, name)
    if name in ("noise_estimation_loss", "v_prediction_loss", "target_loss", "loss_registry"):
        from . import losses
        return getattr(losses, name)
    if name == "EMAHelper":
        from .ema import EMAHelper
        return EMAHelper
    raise AttributeError(name)
