"""``generalized_steps`` -- the reference's DDIM / eta-generalised reverse loop on the HIP library.

Mirrors reference ``functions/denoising.py:10-52`` (same signature, same return value, same
in-place semantics: ``xs[0]`` is the caller's tensor and ``x`` is updated in place when it already
is a GPU float tensor).  Differences that are fixes, not behaviour changes:
the device follows the model / ``x`` instead of hard-coded ``torch.cuda.*Tensor`` strings; the
per-step scalars live in a device table indexed by a device step counter so the whole step
(timestep fill, U-Net, fused x0-prediction + x_{t-1} update) replays as one hipGraph; ``randn_like``
is only drawn when eta > 0.  All tensor arithmetic runs in libddimx kernels.
"""
import os

import numpy as np
import torch

from . import _lib
from .graphs import GraphOwner
from .schedule import X0Threshold, check_prediction, check_threshold, ddim_coefficients, ddpm_coefficients, threshold_rank, v_table


def _selected(select_index, index, n):
    return select_index is None or index in select_index or index - n in select_index


def _device(model, x):
    """The device a sampling run computes on: the model's if its parameters live on a GPU, else x's, else the current one."""
    if isinstance(model, torch.nn.Module):
        p = next(model.parameters(), None)
        if p is not None and p.is_cuda:
            return p.device
    return x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _check_noise(noise, noise_fn):
    """``noise`` is a ``noise.NoiseStream`` or None, and excludes ``noise_fn``."""
    if noise is None:
        return
    from .noise import NoiseStream
    if not isinstance(noise, NoiseStream):
        raise TypeError(f"noise must be a NoiseStream, got {type(noise).__name__}")
    if noise_fn is not None:
        raise ValueError("give either noise= (a NoiseStream, drawn on the device) or noise_fn= (a callable, eager steps), not both")


def _check_model(model, shape, t_len, batch="B", length="T", what="T", positive="positive "):
    """``x``'s channels and F against a ``ddim_audio_amd.Model``'s config, and ``t_len`` -- the length the network sees --
    against its down-sampling (the library sizes what it is handed from the config); any other callable has none to check."""
    if not hasattr(model, "forward_slot"):
        return
    mc = model.config
    if shape[1] != mc.channels or shape[3] != mc.f_size:
        raise ValueError(f"x of shape {shape} does not match the model: expected [{batch}, {mc.channels}, {length}, {mc.f_size}]")
    step = 1 << (len(mc.ch) - 1)
    if t_len % step:
        raise ValueError(f"{what} = {t_len} must be a {positive}multiple of {step} for this model")


def _check_sample(x, model):
    """The checks on ``x`` every sampler that hands it to the library makes before any device work; returns its shape."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("x must be a [B, C, T, F] tensor")
    shape = tuple(x.shape)
    if not 1 <= shape[0] <= 65535:
        raise ValueError(f"batch size {shape[0]} outside 1..65535")
    if x[0].numel() == 0 or x[0].numel() % 4:
        raise ValueError("the size of one sample (C * T * F) must be a positive multiple of 4 elements")
    _check_model(model, shape, shape[2])
    return shape


def _prediction(model, prediction):
    """What a sampler takes the network's output for: an explicit ``prediction`` wins, ``None`` means ``model.prediction`` if the
    model has one (a ``ddim_audio_amd.Model`` reads it from ``config.type``), else ``"eps"``; ValueError for anything but
    ``"eps"`` / ``"v"``.  Before any device work."""
    return check_prediction(getattr(model, "prediction", "eps") if prediction is None else prediction)


def _v_table(prediction, alpha):
    """The ``v_table=`` of a stepper: ``schedule.v_table(alpha)`` for ``"v"``, None (nothing allocated or launched) for ``"eps"``."""
    return v_table(alpha) if prediction == "v" else None


def _threshold(threshold, alpha):
    """The ``threshold=`` of a stepper: None (nothing allocated or launched), or the checked rule with the (s1, s2) table its
    kernels index by every sample's own ``t`` -- ``schedule.v_table(alpha)``, whose fp32 rows are columns 1-2 of every coefficient
    table.  ValueError for anything but None, an ``X0Clip`` or an ``X0Threshold``; before any device work."""
    return None if check_threshold(threshold) is None else (threshold, v_table(alpha))


def _check_eta(eta):
    eta = float(eta)
    if not np.isfinite(eta) or eta < 0:
        raise ValueError("eta must be finite and >= 0")
    return eta


def _as_state(x, device):
    """The run's x_t (reference :18, ``x.type("torch.cuda.FloatTensor")``): ``x`` itself, updated in place, when it already is a
    contiguous fp32 GPU tensor, else a copy on ``device``."""
    return x if (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()) else x.to(device, torch.float32).contiguous()


def _host_noise_fn(eta, noise, noise_fn):
    """The per-step host draw of a run, or None: none for eta = 0 or a device ``NoiseStream``; ``torch.randn_like`` (reference
    :42 draws it every step) unless the caller gave one."""
    if eta == 0.0 or noise is not None:
        return None
    return noise_fn if noise_fn is not None else torch.randn_like


def _run(stepper, x, select_index, per=1, finish=None):
    """Every step of ``stepper``, ``per`` of them to an iteration; returns (xs, x0_preds): ``x`` followed by CPU copies of
    x_{t-1}, and CPU copies of the x0 prediction, at the selected iterations.  ``finish(stepper)`` runs after the last step,
    while the stepper's buffers are still there."""
    xs, x0_preds, n_iter = [x], [], stepper.n_iter // per
    try:
        for index in range(n_iter):
            for _ in range(per):
                stepper.step()
            if _selected(select_index, index, n_iter):
                x0_preds.append(stepper.x0.to("cpu"))
                xs.append(stepper.xt.to("cpu"))
        if finish is not None:
            finish(stepper)
    finally:
        stepper.close()  # graph first, then the events / buffers it referenced
    return xs, x0_preds


class DDIMStepper(GraphOwner):
    """One sampling run's device state and its step function, and the skeleton of every other sampler's
    (``inpaint.InpaintStepper``, ``solver.MultistepStepper``, ``window.WindowStepper`` / ``WindowSolverStepper``,
    ``invert.InvertStepper``).

    ``step()`` = reference ``functions/denoising.py:22-43`` for one iteration: timestep fill, model
    forward, fused x0-prediction + x_{t-1} update, counter advance.  The scalars come from a device
    table indexed by a device counter, so after the first (eager) step the same launch sequence is
    captured once into a hipGraph and replayed for every later step.  (The two batch shards on two streams live inside the
    library call, ``ddimx_unet_fwd_forked``: the captured graph has two parallel branches.)

    A subclass changes the middle of the frame in ``_launch`` and nothing else: ``_update`` (its own update kernel on the same
    table row), ``_gather`` (work in front of the forward), ``_forward`` (another way to eps), ``_prepare`` (what that needs).
    ``pool.PoolStepper``, whose samples each have a table and a counter of their own, also replaces the two launches that
    open and close the frame (``_begin``, ``_end``).
    ``v_table`` (``schedule.v_table``, [n_table, 2] rows (s1, s2)): the network predicts v, and ``_launch`` turns its output into
    eps between ``_forward`` and ``_update`` -- one ``ddimx_v_to_eps`` launch on (``net_in``, ``t``) into ``eps``, inside the captured
    step.  With None nothing is allocated or launched and the frame is the eps one.
    ``threshold`` (``_threshold``: an ``X0Clip`` / ``X0Threshold`` and the same [n_table, 2] table): behind that conversion the x0
    prediction of (``net_in``, eps) is clipped or dynamically thresholded per sample and ``eps`` receives the eps of the result
    (``ddimxq_x0_quantile``'s four launches for the dynamic rule, then ``ddimxq_threshold_eps``), inside the captured step; the update
    kernel then runs on it unchanged, so ``x0`` holds the clipped prediction.  Another callable's output is read, never rewritten:
    the result lands in this object's ``eps``.  With None nothing is allocated or launched.
    ``net_in`` is the tensor the network sees -- ``xt`` unless the subclass passes another: ``t`` and ``eps`` are sized from it,
    the workspace is reserved for it and the capture's fork looks at its batch.

    Ownership (``graphs.GraphOwner``).  The captured graph holds raw pointers into the model's packed
    weights, embedding table, DFT / positional tables and workspaces, into this object's ``xt`` / ``x0`` / ``eps`` / ``t`` /
    ``coef`` / ``counter`` / ``noise_buf`` / ``scale`` / ``qwork`` (and a subclass's own buffers), and its capture recorded the fork / join events of
    its own ``ForkContext``.  A replay is refused -- the step falls back to eager launches and re-captures -- when the model has
    re-allocated any of those buffers since the capture (``Model._gen``) or left eval mode; a repack (new parameter values) is
    carried out in place before the replay.
    Nothing is allocated on a side stream or inside the capture: the workspace is reserved and every buffer allocated on the
    launch stream before.
    """

    def __init__(self, model, xt, coef64, use_graph=True, noise_fn=None, slot=0, fork=True, noise=None, net_in=None, v_table=None, threshold=None):
        super().__init__(model)
        _check_noise(noise, noise_fn)
        self.lib = _lib.load()
        self.xt = xt
        self.net_in = net_in = xt if net_in is None else net_in
        dev = xt.device
        self.coef = torch.from_numpy(np.ascontiguousarray(coef64, dtype=np.float32)).to(dev).contiguous()
        self.n_iter = self.coef.size(0)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t = torch.zeros(net_in.size(0), dtype=torch.int64, device=dev)
        self.x0 = torch.empty_like(xt)
        self.noise_fn = noise_fn
        self.use_graph = (use_graph and noise_fn is None and os.environ.get("DDIMX_GRAPH", "1") != "0"
                          and not torch.cuda.is_current_stream_capturing())
        self.done = 0
        self._capture_pending = self.use_graph
        self.native = hasattr(model, "forward_slot")  # ddim_audio_amd.Model; anything else is called as model(x, t)
        # workspace slot of the model this stepper computes in (steppers that run concurrently on different streams must not share
        # scratch memory) and whether its forward may fork into two batch shards itself
        self.slot, self.fork = slot, fork
        # the v -> eps table and its length; with one, eps is also where the conversion of any other callable's output lands
        self.vtab = None
        if v_table is not None:
            vt = np.ascontiguousarray(v_table, dtype=np.float32)
            if vt.ndim != 2 or vt.shape[0] < 1 or vt.shape[1] != 2:
                raise ValueError("v_table must be [n_table, 2] rows (s1, s2) (schedule.v_table)")
            self.vtab = torch.from_numpy(vt).to(dev).contiguous()
        # the x0 clip / threshold: its table (the v table's device copy if there is one: the same rows), the per-sample (s, r) rows --
        # written once here for a static clip, by the selection kernels every step for the dynamic rule -- and the zeroed histograms
        # of the selection, which every call leaves zeroed (ddimx_threshold.h)
        self.threshold = self.ttab = self.scale = self.qwork = None
        if threshold is not None:
            self.threshold, tt = threshold
            tin = self._threshold_in()
            b = tin.size(0)
            self.ttab = self.vtab if self.vtab is not None else torch.from_numpy(np.ascontiguousarray(tt, dtype=np.float32)).to(dev).contiguous()
            if isinstance(self.threshold, X0Threshold):
                self.rank = threshold_rank(self.threshold.ratio, tin[0].numel())
                self.scale = torch.zeros(b, 2, dtype=torch.float32, device=dev)
                self.qwork = torch.zeros(int(self.lib.ddimxq_quantile_work_bytes(b)), dtype=torch.uint8, device=dev)
            else:
                self.scale = torch.tensor([[self.threshold.limit, 1.0]] * b, dtype=torch.float32, device=dev)
        # the forward writes here: no allocation per step
        self.eps = torch.empty_like(net_in) if (self.native or self.vtab is not None or self.threshold is not None) else None
        # seeded device noise (noise.NoiseStream): the step fills this buffer itself, inside the captured graph too, with the device
        # counter as the draw index.  Owned here and allocated here, on the launch stream and outside any capture, like eps; a table
        # whose every c1 is 0 (eta = 0) needs none, and the step is launch for launch what it is without a stream.  Column 5 is c1
        # in the tables of the samplers that take ``noise=`` (DDIM, inpainting, windowed); the others never pass one, so what
        # their column 5 holds (the inversion's ``first`` flag) is not read here
        self.noise = noise
        self.noise_buf = torch.empty_like(xt) if noise is not None and bool((np.asarray(coef64)[:, 5] != 0).any()) else None

    def _threshold_in(self):
        """The tensor whose samples the threshold acts on, which sizes its per-sample rows, histograms and rank: what the network
        sees (the windowed solver, whose threshold acts on the canvas, answers ``xt``)."""
        return self.net_in

    def _draw(self, noise):
        """The noise tensor the update kernel reads: the stream's fill of ``noise_buf`` for this iteration, else ``noise``."""
        if self.noise_buf is None:
            return noise
        return self.noise.fill(self.noise_buf, self.counter)

    def _prepare(self):
        """On the launch stream: weight packing (a no-op unless a parameter changed), tables, the workspace."""
        if self.native:
            dev, t_len = self.net_in.device, self.net_in.size(2)
            self.model.prepare(dev, t_len)
            self.model.reserve(dev, self.net_in.size(0), t_len, self.slot)

    def _gather(self, st):
        """Launches between the timestep fill and the forward (the windowed sampler cuts ``net_in`` out of ``xt`` here)."""

    def _forward(self):
        """eps = eps_theta(net_in, t), contiguous fp32 and of ``net_in``'s shape."""
        x, t = self.net_in, self.t
        if self.native:
            # a graph stepper's EAGER launches (the sizing step in front of a capture, the fallback after its graph went stale) stay on
            # one stream: the two-shard fork is for the captured step (and for eager-only steppers) -- same bits either way, and no eager
            # two-stream launch right after an executable graph with parallel branches was destroyed
            fork = self.fork and (not self.use_graph or torch.cuda.is_current_stream_capturing())
            return self.model(x, t, _slot=self.slot, _fork=fork, _ctx=self._ctx, _out=self.eps)
        et = self.model(x, t)
        if et.shape != x.shape:  # the update kernel reads net_in's extent
            raise RuntimeError(f"model returned {tuple(et.shape)} for an input of {tuple(x.shape)}")
        if et.dtype != torch.float32 or not et.is_contiguous():
            et = et.float().contiguous()
        return et

    def _to_eps(self, out, st):
        """The eps of the network's output ``out``: ``out`` itself unless the network predicts v, then ``eps`` <- s1 net_in +
        s2 out with the row of every sample's own ``t`` (in place when ``out`` is ``eps``, a native model's); with a ``threshold``
        the eps of the clipped x0 prediction of that, into ``eps`` too."""
        out = self._v_eps(out, st)
        if self.threshold is not None:
            out = self._threshold_eps(self.net_in, out, self.eps, st)
        return out

    def _v_eps(self, out, st):
        """The v conversion of ``_to_eps`` alone."""
        x, eps = self.net_in, self.eps
        if self.vtab is not None:
            _lib.check(self.lib.ddimx_v_to_eps(_lib.ptr(x), _lib.ptr(out), _lib.ptr(eps), _lib.ptr(self.vtab), self.vtab.size(0),
                                               _lib.ptr(self.t), x.size(0), x[0].numel(), st))
            out = eps
        return out

    def _threshold_eps(self, x, out, eps, st):
        """``eps`` <- the eps of the clipped or thresholded x0 prediction of (``x``, ``out``), per sample of ``x`` with the row of
        its own ``t`` (the first ``x.size(0)`` entries); returns ``eps``."""
        tab, shape = (_lib.ptr(self.ttab), self.ttab.size(0), _lib.ptr(self.t)), (x.size(0), x[0].numel(), st)
        if self.qwork is not None:
            th = self.threshold
            _lib.check(self.lib.ddimxq_x0_quantile(_lib.ptr(x), _lib.ptr(out), *tab, self.rank, th.floor,
                                                   float("inf") if th.ceil is None else th.ceil, _lib.ptr(self.qwork),
                                                   _lib.ptr(self.scale), *shape))
        _lib.check(self.lib.ddimxq_threshold_eps(_lib.ptr(x), _lib.ptr(out), _lib.ptr(eps), _lib.ptr(self.scale), *tab, *shape))
        return eps

    def _update(self, et, noise, st):
        """x0 <- the prediction, xt <- x_{t-1}, from the table row of the device counter."""
        xt = self.xt
        _lib.check(self.lib.ddimx_ddim_update(_lib.ptr(xt), _lib.ptr(et), _lib.ptr(noise), _lib.ptr(self.x0), _lib.ptr(self.coef),
                                              _lib.ptr(self.counter), xt.numel(), st))

    def _begin(self, st):
        """Opens the frame: ``t`` <- the timestep of the counter's row; the row stride of the fill is the table's width."""
        t = self.t
        _lib.check(self.lib.ddimx_step_begin_ex(_lib.ptr(self.coef), self.coef.size(1), _lib.ptr(self.counter), _lib.ptr(t), t.numel(), st))

    def _end(self, st):
        """Closes the frame: the counter advances."""
        _lib.check(self.lib.ddimx_step_end(_lib.ptr(self.counter), st))

    def _launch(self, noise):
        """The frame of every sampler's step."""
        st = _lib.stream()
        self._begin(st)
        self._gather(st)
        et = self._to_eps(self._forward(), st)
        self._update(et, self._draw(noise), st)  # a NoiseStream fills the stepper's buffer here
        self._end(st)

    def _captured_refs(self):
        """The model's buffers the captured step points at (this object's own are alive while it is)."""
        return self.model.captured_refs() if self.native else None

    def rewind(self):
        """Restart the coefficient table (benchmark loops longer than the schedule)."""
        self.counter.zero_()

    def _stale(self):
        """Before a replay.  ``_prepare`` runs the model's own staleness test -- (data_ptr, version) of every parameter, the
        same key the eager forward uses -- so an optimizer step, ``load_state_dict`` (also the plain nn.Module one), an in-place
        ``p.copy_()``, an EMA swap-in or ``invalidate()`` repack the weights and the embedding table IN PLACE on the launch
        stream: the graph stays valid and the replay sees the new values.  (Host work of a replay loop that is otherwise idle:
        the GPU step takes milliseconds.)  The graph is stale only if a buffer it points at was re-allocated since the capture
        (``Model._gen``: .to() / .type(), another T, a larger batch) or the model left eval mode."""
        if not self.native:
            return False
        if self.model.training:
            return True
        self._prepare()
        return self._moved()

    def step(self):
        if self.graph is not None and self._stale():
            self._drop_graph()
            self._capture_pending = self.use_graph
        if self.graph is not None:
            self.graph.replay()
        else:
            self._prepare()
            self._launch(self.noise_fn(self.xt) if self.noise_fn is not None else None)
            if self._capture_pending and not (self.native and self.model.training):
                # this step ran eagerly (the first one also sized the model's workspaces); capture one generic step.  thread_local:
                # only THIS thread's calls are checked against the capture -- other threads of the process (a collective library's
                # proxy / watchdog threads, a data loader pinning memory) may allocate or free while we capture
                self._capture_pending = False
                m = self.model
                fork = self.native and self.fork and m.fork_mask and self.net_in.size(0) >= 4
                self._capture_graph(lambda: self._launch(None), self.xt.device, self._captured_refs,
                                    fork=m.new_fork_context if fork else None, error_mode="thread_local")
        self.done += 1


def generalized_steps(x, seq, model, alpha, select_index, **kwargs):
    """x [B,C,T,F]; seq: increasing timesteps; alpha: fp32 alphas-cumprod table; returns (xs, x0_preds)
    as lists of CPU tensors for the selected iterations (``select_index`` semantics of the reference:
    ``None`` = all, else iteration indices, negative allowed).  ``eta > 0``: the noise of every step is ``torch.randn_like`` from
    torch's generator and every step runs eagerly (the reference's behaviour), or ``noise_fn(x_t)`` if that keyword is given; with
    ``noise=`` a ``NoiseStream`` it is drawn inside the step from the seeded device stream, the step replays from one hipGraph,
    and a sample's result depends on (seed, global sample index) only.  ``noise`` and ``noise_fn`` together raise ValueError.
    ``prediction=``: ``"eps"`` or ``"v"``, what the network's output is (None: ``model.prediction`` if it has one, else
    ``"eps"``); for ``"v"`` every step converts it to eps in fp32 before the update (``ddimx_v_to_eps``).
    ``threshold=``: None, ``schedule.X0Clip`` or ``schedule.X0Threshold``: every step clips or dynamically thresholds its x0
    prediction, per sample, before the update (behind the v conversion), and ``x0_preds`` holds the clipped predictions; anything
    else raises ValueError before any device work."""
    noise, noise_fn = kwargs.get("noise"), kwargs.get("noise_fn")
    _check_noise(noise, noise_fn)
    prediction = _prediction(model, kwargs.get("prediction"))
    threshold = _threshold(kwargs.get("threshold"), alpha)
    _lib.load()
    eta = float(kwargs.get("eta", 0))
    seq = list(seq)
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        xt = _as_state(x, device)
        if xt.numel() % 4:
            raise RuntimeError("sample tensor size must be a multiple of 4 elements")
        coef = ddim_coefficients(seq, alpha, eta)
        stepper = DDIMStepper(model, xt, coef, use_graph=(len(seq) >= 4), noise_fn=_host_noise_fn(eta, noise, noise_fn), noise=noise,
                              v_table=_v_table(prediction, alpha), threshold=threshold)
        return _run(stepper, x, select_index)


def ddpm_steps(x, seq, model, b, select_index, **kwargs):
    """Ancestral sampler of the reference (``functions/denoising.py:55-92``): same signature and return value
    (every iteration appends the clamped x0 prediction and the new sample as CPU tensors; ``select_index`` must be
    None like upstream).  ``b`` is the fp32 beta table.  The per-step update is one libddimx pass
    (``ddimx_ddpm_update``); the noise is drawn with ``torch.randn_like`` like the reference (``noise_fn`` kwarg:
    test hook returning the noise tensor for iteration k), or, with ``noise=`` a ``NoiseStream``, filled from the seeded device
    stream into one reused buffer (draw index k).  The loop stays eager: it copies every iteration to the host.
    ``prediction=`` as in ``generalized_steps``; the v table is ``schedule.v_table`` of the fp32 cumulative product the
    coefficients use."""
    if select_index is not None:
        raise NotImplementedError("Specifying select_index is not implemented in ddpm_steps.")
    noise_fn, stream = kwargs.get("noise_fn"), kwargs.get("noise")
    _check_noise(stream, noise_fn)
    prediction = _prediction(model, kwargs.get("prediction"))
    lib = _lib.load()
    seq = list(seq)
    device = _device(model, x)
    with torch.no_grad(), torch.cuda.device(device):
        xs, x0_preds = [x], []
        cur = x.to(device, torch.float32).contiguous().clone()
        nxt, x0buf = torch.empty_like(cur), torch.empty_like(cur)
        coef = torch.from_numpy(ddpm_coefficients(seq, b)).to(device).contiguous()
        counter = torch.zeros(1, dtype=torch.int32, device=device)
        t = torch.zeros(cur.size(0), dtype=torch.int64, device=device)
        noise_buf = torch.empty_like(cur) if stream is not None else None
        vtab = ebuf = None
        if prediction == "v":
            acp = (1 - torch.cat([torch.zeros(1), torch.as_tensor(b).to("cpu", torch.float32)], dim=0)).cumprod(dim=0)  # ddpm_coefficients'
            vtab = torch.from_numpy(v_table(acp[1:]).astype(np.float32)).to(device).contiguous()
            ebuf = torch.empty_like(cur)
        for k in range(len(seq)):
            st = _lib.stream()
            _lib.check(lib.ddimx_step_begin_ex(_lib.ptr(coef), 7, _lib.ptr(counter), _lib.ptr(t), t.numel(), st))
            e = model(cur, t)
            if e.dtype != torch.float32 or not e.is_contiguous():
                e = e.float().contiguous()
            if vtab is not None:
                _lib.check(lib.ddimx_v_to_eps(_lib.ptr(cur), _lib.ptr(e), _lib.ptr(ebuf), _lib.ptr(vtab), vtab.size(0), _lib.ptr(t),
                                              cur.size(0), cur[0].numel(), st))
                e = ebuf
            if stream is not None:
                noise = stream.fill(noise_buf, None, k)
            else:
                noise = (noise_fn(k, cur) if noise_fn is not None else torch.randn_like(cur)).to(device, torch.float32).contiguous()
            _lib.check(lib.ddimx_ddpm_update(_lib.ptr(cur), _lib.ptr(e), _lib.ptr(noise), _lib.ptr(x0buf), _lib.ptr(nxt),
                                             _lib.ptr(coef), _lib.ptr(counter), cur.numel(), st))
            _lib.check(lib.ddimx_step_end(_lib.ptr(counter), st))
            x0_preds.append(x0buf.to("cpu"))
            xs.append(nxt.to("cpu"))
            cur, nxt = nxt, cur
    return xs, x0_preds
