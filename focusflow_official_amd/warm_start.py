"""Warm-start inference over the consecutive frame pairs of a video.

The reference ships `forward_interpolate` (core/utils/utils.py:26-54) and the model's `flow_init` argument
(raft.py:211-212) for RAFT's warm-start loop: the 1/8-resolution flow of one pair, pushed along itself, initialises the
next pair.  `forward_interpolate` here is that function on the device (csrc/warm_start.hip; `utils.forward_interpolate`
stays the reference's host version), `FlowSequence` is the loop:

    seq = FlowSequence(model)                      # one per B sequences that advance in lock-step
    for image1, image2 in pairs:                   # padded by the caller (utils.InputPadder)
        flow_low, flow_up = seq(image1, image2)    # masks as the model takes them; seq.reset() at a sequence boundary

FF-RAFT reads a key-point mask of image1; FlowSequence(model, keypoints=keypoints.GoodFeatures()) detects it on the device
in front of every forward (inside the graph), so that `seq(image1, image2)` is all a video needs.
"""
import torch

from . import ops
from .graph import GraphedForward, require_mask_reader

forward_interpolate = ops.forward_interpolate


class FlowSequence:
    """`model(image1, image2, mask1, mask2, raft_iters, flow_init, test_mode=True)` over consecutive pairs, each pair
    initialised from the previous pair's flow (warm_start=False: every pair starts cold).

    graph=True: one hipGraph replay per pair (graph.GraphedForward with warm_start: the interpolation is part of the
    graph and nothing passes through the host); it is captured on the first call and again whenever the input shapes
    change, which also starts a new sequence.  The tensors returned are the graph's static outputs: valid until the
    next call.  graph=False: the same operations issued one by one.

    keypoints=det (keypoints.GoodFeatures): mask1 of every pair is det(image1), computed in front of the forward (graph=True:
    inside the graph); `seq.mask1` is the last one.  mask1 must then stay None; a caller's mask2 passes through untouched
    (`point` mode ignores it)."""

    def __init__(self, model, raft_iters=12, warm_start=True, graph=True, keypoints=None):
        self.model, self.iters, self.warm_start, self.graph = model, raft_iters, bool(warm_start), bool(graph)
        self.keypoints = keypoints
        if keypoints is not None:
            require_mask_reader(model)
        self._require_eval()
        self._mask1 = None          # graph=False: the last detected mask
        self._graphed, self._key = None, None
        self._flow_init = None      # graph=False: the next pair's initialisation

    def _require_eval(self):
        if self.model.training:
            raise ValueError("FlowSequence runs the eval-mode forward: call model.eval() first")

    @property
    def flow_init(self):
        """What the next pair starts from: a (B,2,H/8,W/8) device tensor (graph=True: the graph's own buffer), or None
        before the first pair of a shape / after reset() without a graph."""
        return self._flow_init if not self.graph else (self._graphed.flow_init if self._graphed is not None else None)

    @property
    def mask1(self):
        """keypoints=: the mask detected for the last pair's image1 (graph=True: the graph's own buffer); None before."""
        if self.keypoints is None:
            return None
        return self._mask1 if not self.graph else (self._graphed.mask1 if self._graphed is not None else None)

    def reset(self):
        """A sequence boundary: the next pair starts cold."""
        self._flow_init = None
        if self._graphed is not None:
            self._graphed.reset()

    def __call__(self, image1, image2, mask1=None, mask2=None):
        self._require_eval()
        if self.keypoints is not None and mask1 is not None:
            raise ValueError("this session detects mask1 itself (keypoints=...): pass None for mask1")
        inputs = (image1, image2, mask1, mask2)
        if not self.graph:
            with torch.no_grad():
                if self.keypoints is not None:
                    self._mask1 = self.keypoints(image1)
                    inputs = (image1, image2, self._mask1, mask2)
                flow_low, flow_up = self.model(*inputs, raft_iters=self.iters, flow_init=self._flow_init, test_mode=True)
                if self.warm_start:
                    self._flow_init = ops.forward_interpolate(flow_low)
            return flow_low, flow_up
        key = tuple(None if t is None else (tuple(t.shape), t.dtype, t.device) for t in inputs)
        if key != self._key:
            self._graphed = None      # (the old graph's buffers go before the new ones come)
            self._graphed = GraphedForward(self.model, inputs, raft_iters=self.iters, warm_start=self.warm_start, keypoints=self.keypoints)
            self._key = key
        return self._graphed(*inputs)
