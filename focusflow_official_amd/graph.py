"""hipGraph capture of the FF-RAFT forward (inference).

One forward is ~700 small launches (8.8 ms of host time); at small batch the GPU finishes sooner than
the host can issue them.  Every libfocusflow_hip entry point only enqueues work on the current stream
(no allocation, no synchronisation), so the whole step is capturable: torch.cuda.CUDAGraph is a
hipGraph on ROCm and its graph-aware allocator provides the intermediate buffers.  CapturedStep is the
capture-and-replay procedure itself (warm-up, capture, the range guard around a replay); GraphedForward
is the model's forward under it, and frames.FrameSequence puts a whole video step under it."""
import contextlib

import torch

from . import ops


def require_mask_reader(model):
    """keypoints= makes sense only for a model whose forward reads mask1: FF_RAFT_FUSION with a fusion branch."""
    if getattr(model, "mask_modal", None) is None:
        raise ValueError(f"keypoints= given to {type(model).__name__}, which reads no key-point mask here: plain RAFT (use_fusion=None) "
                         "takes no mask, and models other than FF_RAFT_FUSION are not supported by these session classes "
                         "(give FF-PWC the detector's mask like any other mask)")


class CapturedStep:
    """`step()` - work that only enqueues on the current stream - as one hipGraph, with the always-on range guard of ops around it.
    The one capture-and-replay procedure of GraphedForward and frames.FrameSequence.

    capture(step, put_back): `warmup` steps on a side stream (they pack weights, set kernel attributes, decide the routes - exact
    context convolutions or not - and warm the allocator) with no capture words set; `put_back()` there, which undoes what the
    warm-up changed (a caller that has to save state for it does so before it calls capture); ops.guard_check(sync=True); then
    the capture under ops.guard_capture: the probes of a captured forward go to a static pair of words (zeroed by a captured
    fill).  One pair per entry of `labels`: the step's first forward fills the first, and a step with further forwards runs the
    k-th of them inside `with self.guard(k):`.
    replay(): ops.guard_check (raises if an earlier replay left the split formats' range), the replay, and every pair copied to
    the host under its label for the asynchronous look at the next call (ops.guard_queue, with `owner` = the RAFT module and the
    owner's `_exact_ctx` as it stood at capture: a graph captured on the split route is refused on context features beyond the
    range at EVERY replay, also after the first refusal armed the flag - capturing again is the caller's business).  -> out
    It keeps neither `step` nor `put_back`: they are its user's methods or closures, and a reference back would leave the
    hipGraph to the garbage collector, which may run inside somebody's capture, where a graph cannot be destroyed."""

    def __init__(self, device, labels, owner):
        self.device, self.labels, self.owner = device, labels, owner
        self.graph = self.out = None
        self._words, self._capturing, self._exact_ctx = [None] * len(labels), False, False

    def guard(self, k):
        """Around the k-th further forward of the step: its own pair of words while THIS step is being captured; otherwise (a
        warm-up step, an eager session) the thread's capture words stay as they are."""
        return ops.guard_capture(self._words[k]) if self._capturing else contextlib.nullcontext()

    def capture(self, step, put_back, warmup=3):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                step()
            put_back()
        torch.cuda.current_stream().wait_stream(side)
        ops.guard_check(sync=True)
        if ops.RANGE_GUARD:
            self._words = [torch.zeros(2, dtype=torch.int32, device=self.device) for _ in self.labels]
        # the route the graph holds: the owner's flag as the warm-up left it (SepConvGRU.prepare runs at capture time); every
        # replay is judged by it, whatever the flag says by then
        self._exact_ctx = bool(getattr(self.owner, "_exact_ctx", False))
        self.graph, self._capturing = torch.cuda.CUDAGraph(), True
        try:
            with ops.guard_capture(self._words[0]), torch.cuda.graph(self.graph), torch.no_grad():
                self.out = step()
        finally:
            self._capturing = False
        return self.out

    def replay(self):
        ops.guard_check()
        self.graph.replay()
        for words, label in zip(self._words, self.labels):
            if words is not None:
                ops.guard_queue(words, label, self.owner, exact_ctx=self._exact_ctx)
        return self.out


class GraphedForward:
    """Capture `model(image1, image2, mask1, mask2, raft_iters, test_mode=True)` for fixed shapes.

    Call it with new inputs of the same shape: they are copied into the captured input buffers, the
    graph is replayed and the (static) output tensors are returned — valid until the next call.

    flow_init=True: the capture passes the static (B,2,H/8,W/8) buffer `self.flow_init` to the model as its flow_init
    (raft.py:211-212).  It starts at zero, which is bit-identical to no flow_init (x + 0.0f); `__call__(..., flow_init=t)`
    copies t into it and `reset()` zeroes it.
    warm_start=True (implies flow_init): ops.forward_interpolate(flow_low, out=self.flow_init) is captured behind the
    forward on the main stream, so every replay leaves the next replay's initialisation in place without the host seeing
    it - consecutive pairs of a video; `reset()` at a sequence boundary.
    keypoints=det (keypoints.GoodFeatures): det(static image1, out=self.mask1) is captured in front of the model, so every
    replay computes the key-point mask of the frame it was given; example_inputs[2] may then be None, and `__call__` takes
    None for mask1 and refuses a tensor there (either the graph detects or the caller supplies)."""

    def __init__(self, model, example_inputs, raft_iters=12, warmup=3, flow_init=False, warm_start=False, keypoints=None):
        if model.training:
            raise ValueError("capture the eval-mode forward (training mutates BatchNorm buffers and the tape)")
        self.model, self.iters = model, raft_iters
        self.static_in = [t.clone() if t is not None else None for t in example_inputs]    # (plain RAFT: masks may be None)
        self.keypoints = keypoints
        if keypoints is not None:
            require_mask_reader(model)
            b, _, h, w = self.static_in[0].shape
            self.static_in[2] = torch.zeros((b, 1, h, w), dtype=torch.float32, device=self.static_in[0].device)
        self.warm_start = bool(warm_start)
        self.flow_init = None
        if flow_init or warm_start:
            b, _, h, w = self.static_in[0].shape
            self.flow_init = torch.zeros((b, 2, h // 8, w // 8), dtype=torch.float32, device=self.static_in[0].device)

        def step():
            if keypoints is not None:
                keypoints(self.static_in[0], out=self.static_in[2])
            if self.flow_init is None:      # (the call as it always was)
                return model(*self.static_in, raft_iters=raft_iters, test_mode=True)
            out = model(*self.static_in, raft_iters=raft_iters, flow_init=self.flow_init, test_mode=True)
            if self.warm_start:
                ops.forward_interpolate(out[0], out=self.flow_init)
            return out

        # (put back after the warm-up: the forwards of a warm start left their own initialisation in flow_init)
        self._captured = CapturedStep(self.static_in[0].device, ("GraphedForward replay",), getattr(model, "flow_net", None))
        self.out = self._captured.capture(step, self.reset, warmup)

    @property
    def graph(self):
        """The captured torch.cuda.CUDAGraph."""
        return self._captured.graph

    @property
    def mask1(self):
        """The static mask1 buffer: with keypoints=, the mask of the last replay's image1."""
        return self.static_in[2]

    def __call__(self, *inputs, flow_init=None):
        if self.keypoints is not None and len(inputs) > 2 and inputs[2] is not None:
            raise ValueError("this graph detects mask1 itself (keypoints=...): pass None for mask1, or capture without a detector and supply it")
        for k, (dst, src) in enumerate(zip(self.static_in, inputs)):
            if self.keypoints is not None and k == 2:
                continue
            if dst is not None and dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
        if flow_init is not None:
            if self.flow_init is None:
                raise ValueError("this graph was captured without a flow_init input: GraphedForward(..., flow_init=True)")
            if flow_init.data_ptr() != self.flow_init.data_ptr():
                self.flow_init.copy_(flow_init)
        return self._captured.replay()

    def reset(self):
        """Back to a cold start: zero the flow_init buffer (a sequence boundary)."""
        if self.flow_init is not None:
            self.flow_init.zero_()

    def check_range(self):
        """Wait for the replays issued so far and raise if one of them left the fp16-split formats' range (ops: the always-on guard)."""
        ops.guard_check(sync=True)
