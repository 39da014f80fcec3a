"""Eval-mode forwards by HIP-graph replay: `GraphedForward`, the mechanism behind `train.hip_graph_val` of the harness.

An eager MHCT block issues about 250 launches through Python and ctypes, so an eval forward is bounded by the host, not by
its kernels.  Every libcloudct launch goes to torch's current stream and reads nothing on the host, so a whole forward
captures into one graph; a replay then costs one launch.

What a graph is keyed by, and why:
* the inputs' shapes and dtypes — a graph's kernels, grids and workspaces are those of one shape;
* the address of every parameter and buffer of the model (and the frozen-norm marks) — the graph reads the weights and the
  running statistics WHERE THEY LIVE, so an optimizer step, a training step or a `load_state_dict` between two calls needs no
  re-capture and the next replay sees the new values; a model whose tensors were replaced (`model.to`, `convert_sync_batchnorm`,
  an assignment to `.data`) has other addresses, gets a new graph, and never replays stale ones;
* `precision.code()`, `precision.conv_code()` and `is_deterministic()` — the modes select kernels when a launch is issued,
  that is at capture, so a change of mode between two calls captures anew.
"""
import torch

from . import determinism, precision

__all__ = ["GraphedForward", "eval_forward", "is_capture_error"]


def is_capture_error(ex):
    """Is this RuntimeError HIP refusing or invalidating a stream capture (as opposed to an error of the captured code)?"""
    msg = str(ex).lower()
    return any(k in msg for k in ("capture", "hipgraph", "cudagraph", "graph", "operation not permitted when stream is capturing",
                                  "streamcapture"))


def eval_forward(model, cfg, clone_outputs=False, verbose=True):
    """What an --eval loop calls in place of `model`: `model` itself, or — where `train.hip_graph_val` of `cfg` is set and the
    model lives on the GPU — a GraphedForward over it that falls back to eager forwards when HIP refuses the capture."""
    if not bool(cfg.get("train", {}).get("hip_graph_val", False)) or not any(p.is_cuda for p in model.parameters()):
        return model
    return GraphedForward(model, clone_outputs=clone_outputs, fallback=True, verbose=verbose)


def _flatten(out, leaves):
    """The structure of `out` with every tensor replaced by its index in `leaves` (which it is appended to)."""
    if isinstance(out, torch.Tensor):
        leaves.append(out)
        return ("t", len(leaves) - 1)
    if isinstance(out, (tuple, list)):
        return ("s", type(out), [_flatten(o, leaves) for o in out])
    return ("v", out)                         # (a model's plain numbers, e.g. the lattice sizes the blocks report)


def _rebuild(spec, leaves):
    if spec[0] == "t":
        return leaves[spec[1]]
    if spec[0] == "s":
        return spec[1](_rebuild(s, leaves) for s in spec[2])
    return spec[1]


class GraphedForward:
    """`GraphedForward(model)(*tensors)` is `model(*tensors)` in the model's eval mode under `torch.no_grad()`, by replay of one
    HIP graph per key (the module's docstring says what the key holds).

    The first call with a key runs `warmup` eager forwards on a side stream of this object (lazy attributes, library choices
    and the per-stream workspaces of the ops are created there, outside the capture), captures one forward on that stream
    over static copies of the inputs, and replays it; later calls copy the inputs into the static buffers, replay, and return
    the static outputs: tensors, or tuples / lists of tensors as the zoo's models return them (anything else in the output is
    returned as the capture saw it).

    THE OUTPUTS ARE OVERWRITTEN BY THE NEXT CALL WITH THE SAME KEY.  Consume them before that call, clone what must live
    longer, or build the wrapper with `clone_outputs=True`, which returns copies.

    A model in training mode is refused with a RuntimeError: its running statistics would move with every replay, the
    warm-ups included (training by replay is `harness.Trainer.fit(hip_graph=True)`).  CPU tensors are refused as the ops
    refuse them.  `fn`: the callable that is run instead of `model` itself (the harness passes a validation step: forward
    plus loss terms); `model` then only names the parameters the graph reads.  `fallback=True` (the harness and the --eval
    loops): a capture that HIP refuses (`is_capture_error`) is reported once (`verbose`) and this and every later call run
    `fn` eagerly (`eager` is then True); without it the error is raised.  `reset()` drops the graphs; `graphs_captured`
    counts the captures since construction."""

    def __init__(self, model, warmup=2, clone_outputs=False, fn=None, fallback=False, verbose=True):
        self.model, self.fn = model, (model if fn is None else fn)
        self.warmup, self.clone_outputs = int(warmup), bool(clone_outputs)
        self.fallback, self.verbose, self.eager = bool(fallback), bool(verbose), False
        self.graphs_captured = 0
        self._graphs, self._stream = {}, None

    def reset(self):
        """Drop every captured graph (and its static buffers); the next call of any key captures again."""
        self._graphs = {}

    def _state_key(self):
        ptrs = []
        for m in self.model.modules():
            if m.training:
                raise RuntimeError("GraphedForward replays an eval-mode forward: a model in training mode would update its running "
                                   "statistics on every replay (the warm-ups included); call model.eval() first, and use "
                                   "Trainer.fit(hip_graph=True) to train by graph replay")
            for t in m._parameters.values():
                if t is not None:
                    ptrs.append(t.data_ptr())
            for t in m._buffers.values():
                if t is not None:
                    ptrs.append(t.data_ptr())
            if m.__dict__.get("_ct_frozen", False):
                ptrs.append(-1)
        return tuple(ptrs)

    def key(self, *tensors):
        """The key of a call with `tensors` (raises what `__call__` would raise for them)."""
        for t in tensors:
            if not isinstance(t, torch.Tensor):
                raise TypeError("GraphedForward takes tensors, got %s" % type(t).__name__)
            if not t.is_cuda:
                raise RuntimeError("cloud_transformers_amd ops need tensors on a HIP device (MI355X); "
                                   "got a %s tensor and there is no CPU fallback" % t.device.type)
        return (tuple((tuple(t.shape), t.dtype) for t in tensors), self._state_key(),
                precision.code(), precision.conv_code(), bool(determinism.is_deterministic()))

    def _capture(self, tensors):
        device = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(device), torch.no_grad():
            if self._stream is None or self._stream.device != device:
                self._stream = torch.cuda.Stream(device=device)
            side, cur = self._stream, torch.cuda.current_stream(device)
            static = [t.clone() for t in tensors]
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(self.warmup):
                    self.fn(*static)
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            # (captured on the stream the warm-up ran on: the per-stream workspaces and tickets of the raster ops were created
            #  by the warm-up, outside the capture and outside the graph's private pool)
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                out = self.fn(*static)
        leaves = []
        spec = _flatten(out, leaves)
        self.graphs_captured += 1
        return graph, static, spec, leaves

    def _eager(self, tensors):
        with torch.no_grad():
            return self.fn(*tensors)

    def __call__(self, *tensors):
        key = self.key(*tensors)
        if self.eager:
            return self._eager(tensors)
        rec = self._graphs.get(key)
        if rec is None:
            # graphs over addresses the model no longer has can never be replayed again: their pools go first
            self._graphs = {k: v for k, v in self._graphs.items() if k[1] == key[1]}
            try:
                rec = self._capture(tensors)
            except RuntimeError as ex:
                # only what a refused CAPTURE raises; a genuine error of the model or the loss is not swallowed
                if not (self.fallback and is_capture_error(ex)):
                    raise
                torch.cuda.synchronize()
                if self.verbose:
                    print("GraphedForward: HIP-graph capture failed (%s); continuing with eager forwards" % (ex,), flush=True)
                self.eager = True
                return self._eager(tensors)
            self._graphs[key] = rec
        graph, static, spec, leaves = rec
        with torch.no_grad():
            for dst, src in zip(static, tensors):
                dst.copy_(src, non_blocking=True)
        graph.replay()
        return _rebuild(spec, [t.clone() for t in leaves] if self.clone_outputs else leaves)
