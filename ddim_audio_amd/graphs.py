"""The owner of a captured hipGraph: whoever captures a graph owns everything the capture references."""
import torch


class GraphOwner:
    """Base of every object that captures a graph and replays it: ``sampler.DDIMStepper`` (with it every sampler's stepper) and
    ``train.GraphedTrainStep``.  The subclass decides when to capture, replay or fall back to eager launches; this class
    holds the graph and what it points at.

    The graph holds raw pointers into device buffers -- the model's (``Model.captured_refs``), the subclass's own, any other
    the captured code reads -- and, if its capture forked onto a second stream, the fork / join events and the stream of a
    ``ForkContext``.  That context is made for the capture, eagerly, before it starts, and never shared (``_ctx``); the buffers
    are listed next to the graph (``_refs``), so they live as long as it does whatever happens to the model; ``close`` and
    ``__del__`` synchronise, destroy the graph, synchronise again, and only then release them.  ``_gen`` is the model's buffer
    generation at capture (``Model._gen``): once it has moved (``_moved``) a replay would run on pointers of an earlier
    generation, and the subclass captures again instead."""

    def __init__(self, model):
        self.graph = None  # first attribute: close() / __del__ must find it whatever else failed
        self._ctx = self._refs = self._gen = self._device = None
        self.captures = 0
        self.model = model

    def _capture_graph(self, fn, device, refs, fork=None, stream=None, error_mode="global"):
        """Capture ``fn()`` into this owner's graph on ``stream`` (None: torch's capture stream) and return what it returned.
        ``fork(device)``, if given, makes the capture's own ForkContext before the capture starts (``fn`` hands ``self._ctx``
        on); ``refs()`` is called after it and lists every buffer the graph points at."""
        self._ctx = fork(device) if fork is not None else None
        self._device = device
        torch.cuda.synchronize(device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream, capture_error_mode=error_mode):
            out = fn()
        self.graph = g
        self.captures += 1
        self._refs, self._gen = refs(), getattr(self.model, "_gen", None)
        return out

    def _moved(self):
        """Whether the model re-allocated a buffer the graph points at since the capture."""
        return getattr(self.model, "_gen", None) != self._gen

    def _drop_graph(self):
        """Destroy the graph, THEN release what its capture referenced (events, buffers)."""
        g, self.graph = self.graph, None
        if g is not None:
            torch.cuda.synchronize(self._device)  # no replay in flight when the executable graph goes away
            del g
            torch.cuda.synchronize(self._device)  # ... and the runtime has finished with it before its events / buffers go
        self._ctx = self._refs = None

    def close(self):
        """Back to eager launches: the graph goes first, then what it referenced."""
        self._drop_graph()

    def __del__(self):
        # an owner that is simply dropped may still have its last replay in flight: the same order as close(), with the same
        # synchronisation (an executable graph destroyed under a running replay, then the events and buffers it references
        # freed, is a use-after-free inside the runtime's completion thread)
        try:
            self._drop_graph()
        except Exception:
            try:
                g, self.graph = self.graph, None
                del g                          # hipGraphExecDestroy first ...
                self._ctx = self._refs = None  # ... then the events its capture recorded and the buffers it points at
            except Exception:
                pass
