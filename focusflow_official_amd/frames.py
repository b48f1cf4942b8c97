"""Video sessions at the application's boundary: raw uint8 frames in, key-point matches and flow images out.

`warm_start.FlowSequence` takes padded fp32 image pairs and returns the dense padded field.  A video application has
neither: a decoder hands it one uint8 HWC frame at a time, whose height is usually no multiple of 8 (540, 1080), and a
tracking or visual-odometry consumer wants the matches (x, y) -> (x + u, y + v) of the frame's key points.
`FrameSequence` is the loop over frames (csrc/frame_io.hip does the conversions on the device):

    seq = FrameSequence(model, raft_iters=12, keypoints=GoodFeatures())     # one per B videos that advance in lock-step
    for frame in video:                      # uint8 (B,H,W,3) / (H,W,3): torch CPU (pinned or not), torch GPU, or numpy
        res = seq.push(frame)                # None for the first frame of a sequence; afterwards flow(previous -> this)
        res.flow_low, res.flow_up            # flow_up: the (B,2,H,W) unpadded view of the padded output (a slice)
        res.matches, res.valid, res.count    # (B,N,4) fp32 [x, y, x + u, y + v], (B,N) uint8, (B) int32: the key points of
                                             # the previous frame and where they went
    seq.reset()                              # a sequence boundary: the next push returns None, the next pair starts cold

With tracks (tracks.TrackTable, csrc/tracks.hip) the session follows its key points over the frames and gives each a persistent id:

    seq = FrameSequence(model, raft_iters=12, keypoints=GoodFeatures(), tracks=True)     # or tracks=N slots
    res = seq.push(frame)
    res.matches, res.valid                   # per SLOT: (B,N,4) [x, y, x', y'] at sub-pixel positions, (B,N) uint8
    res.tracks.ids, res.tracks.age           # (B,N) int64 / int32 of those rows (-1 / 0: a dead slot); res.tracks.born (B) int32
    res.count                                # (B) int32: the live tracks this pair started with
    seq.tracks                               # the table after the advance: where the tracks are in the newest frame

With fb=True (or fb=FBCheck(alpha, beta, iters, warm)) the step also computes the BACKWARD flow of the pair and holds the
forward flow to it (csrc/fb_check.hip): a point whose round trip does not end where it began is occluded or sits on a bad vector.

    seq = FrameSequence(model, raft_iters=12, keypoints=GoodFeatures(), tracks=True, fb=True)
    res = seq.push(frame)
    res.fb.flow_bw, res.fb.err2, res.fb.occluded    # (B,2,H,W) flow(this -> previous); (B,1,H,W) fp32 squared round-trip error in
                                                    # px^2 (+inf: the target left the frame); (B,1,H,W) uint8 occlusion map
    res.fb.point_err2, res.fb.status         # per row of res.matches: (B,N) fp32, (B,N) uint8 (0 no row, 1 consistent, 2 the target
                                             # left the frame, 3 inconsistent); res.valid is 1 only where the status is 1, and
                                             # with tracks the slots of status 3 have died: the next replenish refills them

With epipolar=True (or epipolar=geometry.Epipolar(threshold, hypotheses, min_inliers, min_ratio, cull, seed)) the step ends with the
epipolar check (csrc/epipolar.hip): a RANSAC fundamental matrix over the rows that are still valid, so behind fb= over the
round-trip-consistent ones.

    seq = FrameSequence(model, raft_iters=12, keypoints=GoodFeatures(), tracks=True, fb=True, epipolar=True)
    res = seq.push(frame)
    res.epi.F, res.epi.ok                    # (B,3,3) fp32 in pixel coordinates of the frame, x'^t F x = 0; (B) uint8: a verdict
    res.epi.status, res.epi.dist2            # per row of res.matches: (B,N) uint8 (0 no row, 1 inlier, 2 not a candidate, 3
                                             # outlier, 4 no verdict), (B,N) fp32 Sampson distance in px^2; where there is a
                                             # verdict res.valid is cleared for the outliers, and with tracks their slots have died
    res.epi.inliers, res.epi.candidates      # (B) int32

With homography=True (or homography=geometry.Homography(...)) the step asks, behind fb= and before epipolar=, whether ONE
homography explains the pair - a planar scene, a camera that only rotates - (csrc/homography.hip), holds the epipolar check back
where it does (F is under-determined there), and with Homography.dense writes the residual of the flow against the map:

    seq = FrameSequence(model, raft_iters=12, keypoints=GoodFeatures(), tracks=True, epipolar=True, homography=True)
    res.hom.H, res.hom.ok, res.hom.planar    # (B,3,3) fp32 in pixel coordinates, (x', y', 1) ~ H (x, y, 1); (B) uint8; (B) uint8
    res.hom.status, res.hom.dist2            # per row of res.matches, as res.epi's; the squared transfer error in px^2
    res.hom.residual                         # dense=True: (B,H,W) fp32 px^2, -1 without a verdict; else None

With render=True (or render=Render(max_flow, clip_flow, order, layout, occluded, backward)) the step also paints the flow
(csrc/flow_viz.hip: the Middlebury colour wheel of the reference's flow_viz.py): bytes in, bytes out, 3 B per pixel ready for an
encoder or a window instead of the 8 B of the field and a numpy pass over them.

    seq = FrameSequence(model, raft_iters=12, fb=True, render=Render(max_flow=24.0, occluded=(255, 0, 255)))
    res.view.image                           # uint8 (B,H,W,3) / (B,3,H,W), in the layout and channel order of the session's
                                             # frames unless Render says otherwise; occluded pixels (res.fb.occluded) painted
    res.view.rad_max                         # (B) fp32: the maximum magnitude each frame was scaled by; None with max_flow
    res.view.image_bw                        # backward=True: the image of res.fb.flow_bw; else None
"""
from operator import itemgetter
from typing import NamedTuple, Optional

import torch

from . import ops
from .geometry import EpiResult, EpipolarCheck, HomResult, HomographyCheck, as_config, as_epipolar, as_homography
from .graph import CapturedStep
from .model import FF_RAFT_FUSION
from .tracks import MAX_SLOTS, TrackResult, TrackTable


class FBCheck(NamedTuple):
    """The forward-backward check of a session (FrameSequence(fb=...)).  A point is inconsistent where the squared round-trip
    error exceeds alpha (|forward|^2 + |backward|^2) + beta (px^2); the defaults are the occlusion criterion of UnFlow (Meister
    et al. 2018).  iters: the update iterations of the backward flow (None: the session's raft_iters); warm: start the backward
    flow from the negated forward_interpolate of the forward flow instead of from zero."""
    alpha: float = 0.01
    beta: float = 0.5
    iters: Optional[int] = None
    warm: bool = True

    def validated(self):
        """-> self, or a ValueError that names `fb` and the field."""
        if not (self.alpha >= 0 and self.beta >= 0):
            raise ValueError(f"fb: alpha={self.alpha}, beta={self.beta}: both >= 0 (and no NaN)")
        if self.iters is not None and int(self.iters) < 1:
            raise ValueError(f"fb: iters={self.iters}: None (the session's raft_iters) or at least 1")
        return self


def as_fb(fb) -> Optional[FBCheck]:
    """None / False -> None, True -> the defaults, an FBCheck -> itself, checked; anything else is a ValueError."""
    return as_config("fb", fb, FBCheck)


class FBResult(NamedTuple):
    """What a pair adds to a FrameResult in a session with fb=: the backward flow as the (B,2,H,W) unpadded view, the dense
    squared round-trip error (B,1,H,W) fp32 and occlusion map (B,1,H,W) uint8, and per row of `matches` the error (B,N) fp32 and
    the status (B,N) uint8 (None without matches).  Session buffers: valid until the next push."""
    flow_bw: torch.Tensor
    err2: torch.Tensor
    occluded: torch.Tensor
    point_err2: Optional[torch.Tensor]
    status: Optional[torch.Tensor]


class Render(NamedTuple):
    """The flow images of a session (FrameSequence(render=...)).  max_flow: a fixed scale (finite, > 0) instead of each frame's
    own maximum magnitude, so that the colours do not pump from frame to frame; clip_flow (>= 0): np.clip(flow, 0, clip_flow) first,
    as the reference's flow_to_image does it; order ('rgb' / 'bgr') and layout ('hwc' / 'chw'): None means the session's own, so
    a session fed BGR HWC frames gets BGR HWC images; occluded: None, or the (r, g, b) triple of 0 .. 255 that the pixels of the
    forward-backward check's occlusion map are painted with (needs fb=); backward: also render the backward flow (needs fb=)."""
    max_flow: Optional[float] = None
    clip_flow: Optional[float] = None
    order: Optional[str] = None
    layout: Optional[str] = None
    occluded: Optional[tuple] = None
    backward: bool = False

    def validated(self):
        """-> self, or a ValueError that names `render` and the field."""
        if self.max_flow is not None and not (self.max_flow > 0 and self.max_flow != float("inf")):
            raise ValueError(f"render: max_flow={self.max_flow}: None (every frame's own maximum) or a finite value > 0")
        if self.clip_flow is not None and not self.clip_flow >= 0:
            raise ValueError(f"render: clip_flow={self.clip_flow}: None or a value >= 0")
        if self.order not in (None, "rgb", "bgr"):
            raise ValueError(f"render: order={self.order!r}: None (the session's), 'rgb' or 'bgr'")
        if self.layout not in (None, "hwc", "chw"):
            raise ValueError(f"render: layout={self.layout!r}: None (the session's), 'hwc' or 'chw'")
        c = self.occluded
        if c is not None and (not isinstance(c, (tuple, list)) or len(c) != 3
                              or not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x <= 255 for x in c)):
            raise ValueError(f"render: occluded={c!r}: None or an (r, g, b) triple of integers 0 .. 255")
        return self


def as_render(render) -> Optional[Render]:
    """None / False -> None, True -> the defaults, a Render -> itself, checked; anything else is a ValueError."""
    return as_config("render", render, Render)


class RenderResult(NamedTuple):
    """What a pair adds to a FrameResult in a session with render=: the flow image, uint8 (B,H,W,3) or (B,3,H,W); the maximum
    magnitude every sample's frame was scaled by, (B) fp32 (None with Render.max_flow); with Render.backward the image of the
    backward flow (its own maximum, no occlusion paint), else None.  Session buffers: valid until the next push."""
    image: torch.Tensor
    rad_max: Optional[torch.Tensor]
    image_bw: Optional[torch.Tensor]


class FrameResult(tuple):
    """(flow_low, flow_up, matches, valid, count): the named tuple a push returns.  In tracks mode it is a TrackedFrameResult, the
    same with a sixth item `tracks` (a tracks.TrackResult); in a session with fb= it carries a trailing item `fb` (an FBResult)
    behind those: a CheckedFrameResult (six items) or a TrackedCheckedFrameResult (seven).  Without either the tuple has the five
    items it always had, so a caller that unpacks or walks them goes on working, and `.tracks` and `.fb` are None.  A session with
    epipolar= gets the shape it would have without, plus a last item `epi` (a geometry.EpiResult): Epi-, TrackedEpi-, CheckedEpi-
    and TrackedCheckedEpiFrameResult; `.epi` is None in the four shapes without.  A session with homography= likewise gets the
    shape it would have without, plus a last item `hom` (a geometry.HomResult): each of the eight has a subclass whose name
    puts Hom before FrameResult (HomFrameResult .. TrackedCheckedEpiHomFrameResult); `.hom` is None in the eight without.  A
    session with render= gets, again, the shape it would have without plus a last item `view` (a RenderResult): each of the sixteen
    has a subclass whose name puts Rendered before FrameResult (RenderedFrameResult .. TrackedCheckedEpiHomRenderedFrameResult);
    `.view` is None in the sixteen without.  The thirty-one subclasses are generated from one table (_OPTIONAL), and all
    thirty-two behave as typing.NamedTuple classes do: `_fields`, `_asdict()`, `_replace()`, `_make()`, copy, deepcopy and pickle."""
    __slots__ = ()
    _fields = ("flow_low", "flow_up", "matches", "valid", "count")

    def __new__(cls, flow_low, flow_up, matches, valid, count, tracks: Optional[TrackResult] = None, fb: Optional[FBResult] = None,
                epi: Optional[EpiResult] = None, hom: Optional[HomResult] = None, view: Optional[RenderResult] = None):
        extras = {f: x for f, x in zip(_OPTIONAL_FIELDS, (tracks, fb, epi, hom, view)) if x is not None}
        return tuple.__new__(_SHAPES[tuple(extras)], (flow_low, flow_up, matches, valid, count, *extras.values()))

    flow_low = property(itemgetter(0))
    flow_up = property(itemgetter(1))
    matches = property(itemgetter(2))
    valid = property(itemgetter(3))
    count = property(itemgetter(4))
    tracks = fb = epi = hom = view = property(lambda self: None)      # (a shape that has the item answers with it: _shape)

    def __getnewargs__(self):      # (copy, deepcopy and pickle rebuild through __new__, item by item)
        return tuple(self[:5]) + tuple(getattr(self, f) for f in _OPTIONAL_FIELDS)

    @classmethod
    def _make(cls, iterable):
        """From the items of any of the thirty-two shapes; an item behind the fifth is `fb` if it is an FBResult, `epi` if it is an
        EpiResult, `hom` if it is a HomResult, `view` if it is a RenderResult, else `tracks`."""
        items = tuple(iterable)
        if len(items) <= 5 or len(items) > 10:
            return FrameResult(*items)      # (too few or too many: the TypeError of __new__)
        extras = {}
        for x in items[5:]:
            name = next((f for f, _, kind in _OPTIONAL if isinstance(x, kind)), "tracks")
            if name in extras:
                raise TypeError(f"FrameResult._make: two items for `{name}`")
            extras[name] = x
        return FrameResult(*items[:5], **extras)

    def _asdict(self):
        return dict(zip(self._fields, self))

    def _replace(self, **kwargs):
        unknown = set(kwargs) - set(FrameResult._fields + _OPTIONAL_FIELDS)
        if unknown:
            raise ValueError(f"Got unexpected field names: {sorted(unknown)!r}")
        return FrameResult(**{**self._asdict(), **kwargs})

    def __repr__(self):
        return "FrameResult(" + ", ".join(f"{n}={v!r}" for n, v in zip(self._fields, self)) + ")"


# The optional items behind the fifth, in their order: the field, what its presence puts into the class name, the type that
# identifies it in _make.  The next check's result is one more row (and one more keyword of __new__).
_OPTIONAL = (("tracks", "Tracked", TrackResult), ("fb", "Checked", FBResult), ("epi", "Epi", EpiResult), ("hom", "Hom", HomResult),
             ("view", "Rendered", RenderResult))
_OPTIONAL_FIELDS = tuple(row[0] for row in _OPTIONAL)


def _shape(rows):
    """The class of a FrameResult with the optional items `rows` (a non-empty selection from _OPTIONAL, in its order).  A shape
    whose last item is `hom` or `view` is a subclass of the shape without that item, so the items before it stay where they
    are; every other one is a direct subclass of FrameResult."""
    fields, name = tuple(r[0] for r in rows), "".join(r[1] for r in rows) + "FrameResult"
    base = _SHAPES[fields[:-1]] if fields[-1] in ("hom", "view") else FrameResult
    body = {"__slots__": (), "__module__": __name__, "__qualname__": name, "_fields": FrameResult._fields + fields,
            "__doc__": f"A FrameResult of a session with {', '.join(fields)}: {5 + len(fields)} items, those last.  Made by "
                       f"FrameResult(..., {', '.join(f + '=...' for f in fields)})."}
    body.update((f, property(itemgetter(5 + i))) for i, f in enumerate(fields))
    return type(name, (base,), body)


# the items present -> the shape.  All thirty-two are module attributes: pickle finds them by name
_SHAPES = {(): FrameResult}
for _n in range(1, 2 ** len(_OPTIONAL)):      # (`hom` and `view` are the highest bits: a shape without its last item is made before the one with it)
    _rows = [row for _i, row in enumerate(_OPTIONAL) if _n >> _i & 1]
    _cls = _shape(_rows)
    _SHAPES[_cls._fields[5:]] = globals()[_cls.__name__] = _cls
del _n, _rows, _cls


class ForwardBackward:
    """The forward-backward part of a session's step with the buffers it keeps: the backward pair's mask (unpadded and padded;
    None where the session's own mask serves) and the backward flow's start (None without FBCheck.warm).  Enqueues only."""

    def __init__(self, config: FBCheck):
        self.config = config
        self.mask_det = self.mask = self.init = None

    def prepare(self, b, h, w, hp, wp, device, own_mask):
        """The buffers for a (B,h,w) frame in an hp x wp field; own_mask: the session detects, so the backward pair needs a mask."""
        f32 = dict(dtype=torch.float32, device=device)
        if own_mask:      # (with caller-supplied masks the backward mask is the session's _mask_next)
            self.mask_det, self.mask = torch.zeros((b, 1, h, w), **f32), torch.zeros((b, 1, hp, wp), **f32)
        if self.config.warm:
            self.init = torch.zeros((b, 2, hp // 8, wp // 8), **f32)
            ops.negate(self.init, self.init)      # (makes the constant negate() reads now, not inside a capture)

    def reset(self):
        if self.init is not None:
            self.init.zero_()

    def __call__(self, seq, flow_low, flow_up, matches, valid, table) -> FBResult:
        """Behind the advance / the matches of session `seq`: the backward pair's mask, the backward flow's start, the backward
        flow, the dense check, the point check (which clears `valid` and culls the table)."""
        b, h, w = seq._bhw
        left, top, hp, wp = seq._pad
        fb, det, tb = self.config, seq.keypoints, seq._table
        mask = None
        if seq._reads_mask:
            if det is None:
                mask = seq._mask_next
            else:
                if tb is not None:      # the table as the advance left it, before any culling: the tracks in the newest frame
                    ops.tracks_mask(tb.pos, tb.ids, h, w, out=self.mask_det)
                else:
                    inner = seq._img2[:, :, top:top + h, left:left + w]
                    ops.good_features(inner, det.max_corners, det.quality_level, det.min_distance, out=self.mask_det, ws=det._workspace(inner))
                mask = ops.pad_replicate(self.mask_det, seq.pad_mode, out=self.mask)
        kw = {}
        if fb.warm:
            if seq.warm_start:      # (flow_init holds forward_interpolate(flow_low) already)
                ops.negate(seq._flow_init, self.init)
            else:
                ops.negate(ops.forward_interpolate(flow_low, out=self.init), self.init)
            kw = dict(flow_init=self.init)
        with seq._captured.guard(1):      # a captured forward zeroes and fills the capture's guard words: the backward one gets a pair of its own
            _, flow_bw = seq.model(seq._img2, seq._img1, mask, None, raft_iters=seq.iters if fb.iters is None else int(fb.iters), test_mode=True, **kw)
        err2, occluded = ops.fb_dense(flow_up, flow_bw, left, top, h, w, fb.alpha, fb.beta)
        point_err2 = status = None
        if matches is not None:
            point_err2, status = ops.fb_matches(matches, valid, flow_bw, left, top, h, w, fb.alpha, fb.beta, table=table)
        return FBResult(flow_bw[:, :, top:top + h, left:left + w], err2, occluded, point_err2, status)


class FlowRenderer:
    """ops.flow_to_image with a session's Render into the buffers it keeps: the image and the maximum it was scaled by (None with
    Render.max_flow), and with Render.backward the same for the backward flow.  order, layout: the session's.  Enqueues only."""

    def __init__(self, config: Render, order, layout):
        self.config, self.order, self.layout = config, config.order or order, config.layout or layout
        self.image = self.rad_max = self.image_bw = self.rad_max_bw = None

    def prepare(self, b, h, w, device):
        def pair():
            image = torch.zeros((b, h, w, 3) if self.layout == "hwc" else (b, 3, h, w), dtype=torch.uint8, device=device)
            return image, torch.zeros((b,), dtype=torch.float32, device=device) if self.config.max_flow is None else None
        self.image, self.rad_max = pair()
        if self.config.backward:
            self.image_bw, self.rad_max_bw = pair()

    def _paint(self, flow, left, top, h, w, image, rad_max, occluded):
        r = self.config
        ops.flow_to_image(flow, left, top, h, w, max_flow=r.max_flow, clip_flow=r.clip_flow, order=self.order, layout=self.layout,
                          occluded=occluded, occluded_color=r.occluded or (0, 0, 0), out=image if rad_max is None else (image, rad_max),
                          return_max=rad_max is not None)

    def __call__(self, flow_up, left, top, h, w, fb: Optional[FBResult]) -> RenderResult:
        """Behind the forward-backward check (its occlusion map), on the padded field flow_up: reads only."""
        self._paint(flow_up, left, top, h, w, self.image, self.rad_max, fb.occluded if self.config.occluded is not None else None)
        if self.config.backward:      # (fb.flow_bw is the crop of the padded backward field: the view is passed as it is)
            self._paint(fb.flow_bw, 0, 0, h, w, self.image_bw, self.rad_max_bw, None)
        return RenderResult(self.image, self.rad_max, self.image_bw)


class FrameSequence:
    """`model(image1, image2, mask1, None, raft_iters, flow_init, test_mode=True)` over the consecutive frames of a video.

    Every frame crosses the bus once, as uint8 (`copy_(frame, non_blocking=True)` into a static device buffer), and is
    converted and replicate-padded once (ops.frame_ingest: what permute, float and utils.InputPadder(pad_mode).pad do, bit
    for bit).  The session keeps two padded images, `image1` and `image2`.  Of the two ways to make this frame the next
    pair's image1 - ping-pong buffers behind two captured graphs, or a copy - it takes the COPY: every step begins with one
    device-to-device copy image1 <- image2 (and, with caller-supplied masks, mask1 <- the mask that came with that frame),
    then ingests the new frame into image2.  One graph, and what the last pair read stays in place until the next push.

    A step is: copy, ingest, detect, pad the mask, the model forward, forward_interpolate into the flow_init buffer
    (warm_start=True), matches.  graph=True: one hipGraph replay; the first frame after construction, reset() or a change
    of (B,H,W), mask dtype or device is only ingested, the graph is captured on the push after it, and such a change also
    starts a new sequence.  Capture, replay and the range guard around them are graph.CapturedStep's, as for
    graph.GraphedForward: static guard words, ops.guard_check before a replay, ops.guard_queue behind it.  graph=False: the
    same operations issued one by one.  push() adds no host synchronisation of its own (a capture waits for the device, as
    every capture does).

    keypoints=det (keypoints.GoodFeatures): det runs on the unpadded interior of image1, as the reference makes its masks
    from the original image; the mask is then replicate-padded as evaluate.evaluate_loader pads masks, mask1 =
    InputPadder.pad(det(frame)), and the points feed the matches.  Plain RAFT (use_fusion=None) reads no mask: there a
    detector feeds the matches only and `mask1` is None.  FF-RAFT without a detector takes push(frame, mask=m), m (B,1,H,W)
    or (B,H,W), uint8 or fp32, unpadded: it is padded on the device and read when this frame is image1; `matches`, `valid`
    and `count` are then None.  mask2 is always None: init_mask overwrites it in every mode (ff_raft.py:23-72).

    tracks=True (as many slots as det.max_corners) or tracks=N (1 .. 4096): the session keeps a tracks.TrackTable.  Behind the
    detector the step replenishes it (ops.tracks_replenish: detections no nearer than det.min_distance to a live track take the
    free slots and new ids), the model's mask1 becomes the rasterised TRACKS (ops.tracks_mask, padded as before) instead of the
    detector's mask, and behind forward_interpolate the tracks advance by the flow at their sub-pixel positions
    (ops.tracks_advance) in place of the matches at the detector's points.  `matches` and `valid` are then per slot, `count` is
    the number of live tracks the pair started with, and the result carries `tracks` (ids and age of the rows, births).  reset()
    empties the table and ids go on counting; a new shape drops it with the other buffers.

    fb=True or fb=FBCheck(...): behind the advance (or the matches) the step runs the model a second time, on (image2, image1),
    and checks the forward flow against that backward flow.  Its mask (for models that read one) is `fb_mask`: with tracks the
    rasterised table as the advance left it - the points being followed, now in the newest frame -, with a detector alone the
    detector run on image2, with caller-supplied masks the mask that came with this frame.  With FBCheck.warm it starts from the
    negated forward_interpolate of the forward flow (the splatted forward flow sits at its targets, and the backward flow is
    about minus that), in a buffer of its own.  Then ops.fb_dense writes the squared round-trip error and the occlusion map of
    every pixel, and ops.fb_matches the error and status of every match row; it clears `valid` where the round trip is
    inconsistent and, with tracks, kills those slots: the table the next pair starts from is the culled one, and the next
    replenish refills what the check freed.  The result then carries a trailing `fb` (an FBResult).

    epipolar=True or epipolar=geometry.Epipolar(...) (needs keypoints=): the step ends with ops.epipolar_ransac on the pair's
    matches / valid, behind the advance (or the matches) and behind the forward-backward check when fb= is set, so its candidates
    are the rows that are still valid.  Where a pair gets a verdict it clears `valid` for the outliers and, with tracks (and
    Epipolar.cull), kills their slots: the table the next pair starts from is the culled one.  The draws follow an epoch word on
    the device that every step increments - a replay draws anew -; reset() leaves it alone, a new shape starts it at 0 with the
    other buffers.  The result then carries `epi` (a geometry.EpiResult) as its last item.  F is neither forced to rank 2 nor
    refitted: see geometry.

    homography=True or homography=geometry.Homography(...) (needs keypoints=): behind the forward-backward check and BEFORE the
    epipolar one the step runs ops.homography_ransac on the pair's matches / valid: does one homography - a planar scene, a camera
    that only rotates - explain the pair?  Homography.cull is False by default: the check then judges a copy of `valid` and touches
    neither `valid` nor the table, so the epipolar check behind it sees the same candidates (the outliers of a homography are
    the points off the plane, and HomResult.status names them); with cull it clears `valid` and kills the slots of its outliers
    as the epipolar check does.  With epipolar= and Homography.hold_epipolar a pair whose `planar` is set gets no epipolar verdict (its F would be
    arbitrary), by ops.epipolar_ransac(hold=hom.planar) inside the same graph.  With Homography.dense, ops.homography_residual
    writes what is left of the cropped flow_up once H's motion is removed.  The check has an epoch word of its own, kept as the
    epipolar one is.  The result then carries `hom` (a geometry.HomResult) as its last item.

    render=True or render=Render(...): behind the forward-backward check the step paints the flow (ops.flow_to_image on the padded
    flow_up with the session's left, top, h, w, so the maximum a frame is scaled by is that of the frame, not of the padding)
    into a static uint8 buffer of the session's layout and channel order (or Render's): two launches, one with Render.max_flow.
    With Render.occluded the occlusion map of fb= is painted over it, with Render.backward the backward flow is rendered too.
    Rendering only reads: every other item of the result is what the same session gives without render=.  The result then
    carries `view` (a RenderResult) as its last item.

    The tensors of a result are the session's static buffers: valid until the next push.  A frame in pinned host memory is
    read by an asynchronous copy: leave it alone until work enqueued after the push has finished (the event a consumer
    waits for anyway before it reads the matches)."""

    def __init__(self, model, raft_iters=12, warm_start=True, graph=True, keypoints=None, layout="hwc", order="rgb", pad_mode="sintel",
                 tracks=None, fb=None, epipolar=None, homography=None, render=None):
        if not isinstance(model, FF_RAFT_FUSION):
            raise ValueError(f"model: FrameSequence drives FF_RAFT_FUSION, whose forward takes flow_init; {type(model).__name__} "
                             "(FF_PWCNET has no flow_init) runs pair by pair through graph.GraphedForward")
        if layout not in ("hwc", "chw"):
            raise ValueError(f"layout={layout!r}: 'hwc' or 'chw'")
        if order not in ("rgb", "bgr"):
            raise ValueError(f"order={order!r}: 'rgb' or 'bgr'")
        self.model, self.iters, self.warm_start, self.graph = model, raft_iters, bool(warm_start), bool(graph)
        self.keypoints, self.layout, self.order, self.pad_mode = keypoints, layout, order, pad_mode
        self._slots = 0      # slots of the track table; 0: no tracks
        if tracks is not None and tracks is not False:
            if keypoints is None:
                raise ValueError("tracks: a track table is replenished from a detector's points: give the session keypoints=GoodFeatures(...)")
            self._slots = keypoints.max_corners if tracks is True else int(tracks)
            if not 1 <= self._slots <= MAX_SLOTS or keypoints.max_corners > MAX_SLOTS:
                raise ValueError(f"tracks: {self._slots} slots for a detector of max_corners={keypoints.max_corners}: both 1 .. {MAX_SLOTS}")
        self.fb = as_fb(fb)      # the FBCheck of the session; None: no forward-backward check
        self.epipolar = as_epipolar(epipolar)      # the geometry.Epipolar of the session; None: no epipolar check
        self.homography = as_homography(homography)      # the geometry.Homography of the session; None: no homography check
        for word, config in (("epipolar", self.epipolar), ("homography", self.homography)):
            if config is not None and keypoints is None:
                raise ValueError(f"{word}: the check judges the matches of key points: give the session keypoints=GoodFeatures(...)")
        self.render = as_render(render)      # the Render of the session; None: no flow images
        if self.render is not None and self.fb is None:
            for word, on in (("occluded", self.render.occluded is not None), ("backward", self.render.backward)):
                if on:
                    raise ValueError(f"render: {word}= paints what the forward-backward check computes: give the session fb=True")
        self._reads_mask = getattr(model, "mask_modal", None) is not None
        self._require_eval()
        self._key = None
        self._drop()

    def _require_eval(self):
        if self.model.training:
            raise ValueError("model: FrameSequence runs the eval-mode forward: call model.eval() first")

    def _drop(self):
        self._captured = None      # the graph.CapturedStep of `_step`; (the old graph's buffers go before the new ones come)
        self._u8 = self._mask_in = self._img1 = self._img2 = self._mask1 = self._mask_next = self._mask_det = self._flow_init = None
        self._table = None
        self._fb = None      # the ForwardBackward: the backward pair's mask and the backward flow's start
        self._epi = None      # the geometry.EpipolarCheck: workspace, outputs, the epoch word
        self._hom = self._hom_valid = None      # the geometry.HomographyCheck: the same, and the dense residual; the copy of `valid` it judges without cull
        self._painter = None      # the FlowRenderer: the flow images and the maxima they were scaled by
        self._frames = 0      # frames of the running sequence that have been ingested

    @property
    def mask1(self):
        """The padded (B,1,Hp,Wp) mask the last pair's forward read for its first frame; None before the first pair and
        for plain RAFT."""
        return self._mask1 if self._reads_mask and self._frames >= 2 else None

    @property
    def flow_init(self):
        """What the next pair starts from: the session's (B,2,Hp/8,Wp/8) buffer (zeros: a cold start); None without
        warm_start or before the first frame."""
        return self._flow_init

    @property
    def tracks(self):
        """The session's tracks.TrackTable, as the last pair's advance left it: positions in the newest frame.  None without
        tracks= or before the first frame."""
        return self._table

    @property
    def fb_mask(self):
        """The padded (B,1,Hp,Wp) mask the last pair's BACKWARD forward read for its first frame, the newest one; None without
        fb=, before the first pair and for plain RAFT."""
        if self.fb is None or not self._reads_mask or self._frames < 2:
            return None
        return self._fb.mask if self._fb.mask is not None else self._mask_next      # (caller-supplied: the mask that came with this frame)

    @property
    def _fb_init(self):
        """What the backward flow starts from (FBCheck.warm); None without."""
        return self._fb.init if self._fb is not None else None

    def reset(self):
        """A sequence boundary: the next push returns None and the pair after it starts cold, with an empty track table (ids
        go on counting)."""
        self._frames = 0
        if self._flow_init is not None:
            self._flow_init.zero_()
        if self._fb is not None:
            self._fb.reset()
        if self._table is not None:
            self._table.reset()

    # ---- inputs -----------------------------------------------------------------------------------------------------
    def _frame(self, frame):
        if not isinstance(frame, torch.Tensor):
            frame = torch.as_tensor(frame)
        if frame.dtype != torch.uint8:
            raise ValueError(f"frame: uint8 expected (the decoder's bytes), got {frame.dtype}; float images go to warm_start.FlowSequence")
        if frame.dim() == 3:
            frame = frame.unsqueeze(0)
        if frame.dim() != 4:
            raise ValueError(f"frame: (B,H,W,3) / (H,W,3) for layout 'hwc', (B,3,H,W) / (3,H,W) for 'chw', got {tuple(frame.shape)}")
        c = frame.shape[3] if self.layout == "hwc" else frame.shape[1]
        if c != 3:
            raise ValueError(f"frame: {c} channels in layout {self.layout!r} (shape {tuple(frame.shape)}), 3 expected: "
                             "pass frame[..., :3] of an RGBA frame")
        return frame

    def _mask(self, mask, b, h, w):
        if self.keypoints is not None and self._reads_mask:
            if mask is not None:
                raise ValueError("mask: this session detects mask1 itself (keypoints=...): pass no mask")
            return None
        if not self._reads_mask:
            if mask is not None:
                raise ValueError("mask: plain RAFT (use_fusion=None) reads no mask")
            return None
        if mask is None:
            raise ValueError("mask: this model reads a key-point mask of every frame: push(frame, mask=m), or give the session a detector (keypoints=...)")
        if not isinstance(mask, torch.Tensor):
            mask = torch.as_tensor(mask)
        if mask.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"mask: uint8 or float32 expected, got {mask.dtype}")
        if mask.dim() == 4 and mask.shape[1] == 1:
            mask = mask[:, 0]
        if tuple(mask.shape) != (b, h, w):
            raise ValueError(f"mask: ({b},1,{h},{w}) or ({b},{h},{w}) expected for this frame, got {tuple(mask.shape)}")
        return mask

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _allocate(self, frame, mask, device):
        b, h, w = self._bhw
        left, top, hp, wp = self._pad
        f32 = dict(dtype=torch.float32, device=device)
        self._u8 = torch.empty(tuple(frame.shape), dtype=torch.uint8, device=device)
        self._img1, self._img2 = torch.zeros((b, 3, hp, wp), **f32), torch.zeros((b, 3, hp, wp), **f32)
        if self._reads_mask:
            self._mask1 = torch.zeros((b, 1, hp, wp), **f32)
        if mask is not None:
            self._mask_in = torch.empty((b, h, w), dtype=mask.dtype, device=device)
            self._mask_next = torch.zeros((b, 1, hp, wp), **f32)
        if self.keypoints is not None:
            self._mask_det = torch.zeros((b, 1, h, w), **f32)
        if self.warm_start:
            self._flow_init = torch.zeros((b, 2, hp // 8, wp // 8), **f32)
        if self._slots:
            self._table = TrackTable(b, self._slots, device)
        if self.fb is not None:
            self._fb = ForwardBackward(self.fb)
            self._fb.prepare(b, h, w, hp, wp, device, own_mask=self._reads_mask and self.keypoints is not None)
        rows = self._slots or (self.keypoints.max_corners if self.keypoints is not None else 0)      # N of the matches the checks judge
        if self.epipolar is not None:
            self._epi = EpipolarCheck(self.epipolar)
            self._epi.prepare(b, rows, device)      # (now, not inside a capture)
        if self.homography is not None:
            self._hom = HomographyCheck(self.homography)
            self._hom.prepare(b, rows, device, h, w)
            if not self.homography.cull:
                self._hom_valid = torch.zeros((b, rows), dtype=torch.uint8, device=device)
        if self.render is not None:
            self._painter = FlowRenderer(self.render, self.order, self.layout)
            self._painter.prepare(b, h, w, device)
        labels = ("FrameSequence replay",) + ("FrameSequence replay (the backward flow)",) * (self.fb is not None)
        self._captured = CapturedStep(device, labels, getattr(self.model, "flow_net", None))

    def _ingest(self):
        """The uploaded frame (and mask) -> image2 (and the mask that goes with it)."""
        ops.frame_ingest(self._u8, self.layout, self.order, self.pad_mode, out=self._img2)
        if self._mask_in is not None:
            ops.pad_replicate(self._mask_in, self.pad_mode, out=self._mask_next)

    def _step(self):
        b, h, w = self._bhw
        left, top, hp, wp = self._pad
        self._img1.copy_(self._img2)
        if self._mask_next is not None:
            self._mask1.copy_(self._mask_next)
        self._ingest()
        det, tb, points, count = self.keypoints, self._table, None, None
        if det is not None:
            inner = self._img1[:, :, top:top + h, left:left + w]      # (a dense innermost dimension: no copy)
            _, points, count = ops.good_features(inner, det.max_corners, det.quality_level, det.min_distance, out=self._mask_det,
                                                 return_points=True, ws=det._workspace(inner))
            if tb is not None:
                born, live = ops.tracks_replenish(tb.pos, tb.ids, tb.age, tb.next_id, points, count, h, w, det.min_distance)
                if self._reads_mask:
                    ops.tracks_mask(tb.pos, tb.ids, h, w, out=self._mask_det)      # (over the detector's mask: the model reads the tracks)
            if self._reads_mask:
                ops.pad_replicate(self._mask_det, self.pad_mode, out=self._mask1)
        kw = dict(flow_init=self._flow_init) if self._flow_init is not None else {}
        flow_low, flow_up = self.model(self._img1, self._img2, self._mask1, None, raft_iters=self.iters, test_mode=True, **kw)
        if self.warm_start:
            ops.forward_interpolate(flow_low, out=self._flow_init)
        matches = valid = tracks = None
        if tb is not None:
            matches, valid, ids, age = ops.tracks_advance(tb.pos, tb.ids, tb.age, flow_up, left, top, h, w)
            count, tracks = live, TrackResult(ids, age, born)
        elif det is not None:
            matches, valid = ops.keypoint_matches(points, count, flow_up, left, top, h, w)
        table = None if tb is None else (tb.pos, tb.ids, tb.age)      # what the three checks cull
        fb = self._fb(self, flow_low, flow_up, matches, valid, table) if self._fb is not None else None
        view = self._painter(flow_up, left, top, h, w, fb) if self._painter is not None else None      # behind fb: its occlusion map
        flow_up = flow_up[:, :, top:top + h, left:left + w]
        epi = hom = None
        if self._hom is not None:      # behind fb, before epipolar: both see the same candidates unless Homography.cull
            # (without cull the check judges a copy of `valid`: off-plane rows stay candidates of the epipolar check and of the consumer)
            judged = valid if self.homography.cull else self._hom_valid.copy_(valid)
            hom = self._hom(matches, judged, h, w, table=table, flow=flow_up if self.homography.dense else None)
        if self._epi is not None:      # last: its candidates are the rows that are still valid
            hold = hom.planar if hom is not None and self.homography.hold_epipolar else None
            epi = self._epi(matches, valid, h, w, table=table, hold=hold)
        return FrameResult(flow_low, flow_up, matches, valid, count, tracks, fb, epi, hom, view)

    def _saved(self):
        """What the warm-up steps of a capture change, saved now: -> the callable that puts it back."""
        # (the warm-up steps would spend epochs: graph and eager draw alike)
        epochs = [c.epoch for c in (self._epi, self._hom) if c is not None]
        keep = [(t, t.clone()) for t in (self._img1, self._img2, self._mask1, self._mask_next, self._flow_init, *epochs) if t is not None]
        table = self._table.state() if self._table is not None else None      # (the warm-up steps would move tracks and spend ids)

        def put_back():
            for t, saved in keep:
                t.copy_(saved)
            if table is not None:
                self._table.load_state(table)
        return put_back

    def push(self, frame, mask=None):
        """The next frame of the video (and, for FF-RAFT without a detector, its unpadded key-point mask).  -> None for the
        first frame of a sequence, afterwards a FrameResult for the pair (previous frame, this frame)."""
        self._require_eval()
        frame = self._frame(frame)
        b, h, w = (frame.shape[0], frame.shape[1], frame.shape[2]) if self.layout == "hwc" else (frame.shape[0], frame.shape[2], frame.shape[3])
        mask = self._mask(mask, b, h, w)
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            raise ops._hip.FocusFlowHipError("FrameSequence: the model must be on a HIP device; there is no CPU fallback")
        key = (b, h, w, None if mask is None else mask.dtype, device)
        with torch.no_grad(), torch.cuda.device(device):
            if key != self._key:      # a new shape: new buffers, a new graph, a new sequence
                self._drop()
                self._key, self._bhw, self._pad = key, (b, h, w), ops.pad_offsets(h, w, self.pad_mode)
                self._allocate(frame, mask, device)
            self._u8.copy_(frame, non_blocking=True)
            if mask is not None:
                self._mask_in.copy_(mask, non_blocking=True)
            self._frames += 1
            if self._frames == 1:
                self._ingest()
                return None
            if not self.graph:
                return self._step()
            if self._captured.graph is None:
                self._captured.capture(self._step, self._saved())
            return self._captured.replay()
