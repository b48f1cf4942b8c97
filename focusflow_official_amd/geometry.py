"""The epipolar check: do the matches of a pair agree with one rigid camera motion?

A tracking or visual-odometry front end runs three outlier filters before it estimates a pose: a minimum distance between
tracks, the forward-backward round trip, and the fit of a fundamental matrix F with an inlier flag per match.  This module is
the third (csrc/epipolar.hip; the definition is in include/focusflow_hip.h): a RANSAC (Fischler & Bolles 1981) over 8-point
models in frame-normalised coordinates (Hartley 1997), scored by the Sampson distance, exact in fp32.

    check = EpipolarCheck(Epipolar(threshold=1.0, hypotheses=512))
    res = check(matches, valid, h, w)        # matches (B,N,4) [x, y, x', y'], valid (B,N) uint8: updated in place
    res.F, res.ok                            # (B,3,3) fp32 in pixel coordinates, x'^t F x = 0 (zeros where ok is 0); (B) uint8
    res.status, res.dist2                    # (B,N) uint8: 0 no row, 1 inlier, 2 not a candidate, 3 outlier, 4 no verdict;
                                             # (B,N) fp32 Sampson distance in px^2 (-1 no row, +inf without a verdict)
    res.inliers, res.candidates              # (B) int32

In a video session it is `frames.FrameSequence(..., epipolar=True | Epipolar(...))`.

F is the best minimal-sample model as it stands: it is NOT forced to rank 2 and NOT refitted on its inliers.  Both belong to
the consumer, who has the calibration (an essential matrix, a pose).  A stationary camera makes every skew-symmetric F fit; the
verdict is then harmless: every candidate is an inlier.

The homography check (csrc/homography.hip) is the model F is paired with, as in the initialisation of ORB-SLAM (Mur-Artal et
al. 2015): a dominant plane and a camera that only rotates both leave F under-determined - every [e']x H fits the matches -, and
ONE homography explains the pair instead.  A RANSAC over 4-point DLT models (Hartley & Zisserman, alg. 4.1), scored by the
transfer error in the second image, exact in fp32 as the epipolar check is:

    check = HomographyCheck(Homography(threshold=1.0, hypotheses=512))
    res = check(matches, valid, h, w)        # as above; valid is updated in place where there is a verdict
    res.H, res.ok, res.planar                # (B,3,3) fp32 in pixel coordinates, (x', y', 1) ~ H (x, y, 1); (B) uint8; (B) uint8: at
                                             # least planar_ratio of the candidates follow H: hold the epipolar check back
    res.status, res.dist2                    # as above; dist2 is the squared transfer error in px^2
    res.residual                             # with dense=True and check(..., flow=flow_up): (B,h,w) fp32, what is left of the flow
                                             # once H's motion is removed, in px^2 (-1 without a verdict)

H is the best minimal-sample model as it stands: no least-squares refit, no decomposition into rotation and plane.
"""
from typing import NamedTuple, Optional

import torch

from . import ops

MAX_HYPOTHESES = 4096      # csrc/epipolar.hip


class Epipolar(NamedTuple):
    """The epipolar check of a session (FrameSequence(epipolar=...)) or of an EpipolarCheck.  threshold: the Sampson distance
    in px up to which a match is an inlier; hypotheses: minimal samples drawn per pair (1 .. 4096); a pair gets a verdict where
    the best model has at least min_inliers inliers (a minimal sample always fits its own 8 rows) and min_ratio of the
    candidates; cull: with tracks, the slots of outliers die; seed: of the draws."""
    threshold: float = 1.0
    hypotheses: int = 512
    min_inliers: int = 16
    min_ratio: float = 0.5
    cull: bool = True
    seed: int = 0

    def validated(self):
        """-> self, or a ValueError that names `epipolar` and the field."""
        if not (isinstance(self.threshold, (int, float)) and 0 <= self.threshold < float("inf")):
            raise ValueError(f"epipolar: threshold={self.threshold}: a finite number of pixels >= 0 (and no NaN)")
        if not (isinstance(self.hypotheses, int) and 1 <= self.hypotheses <= MAX_HYPOTHESES):
            raise ValueError(f"epipolar: hypotheses={self.hypotheses}: 1 .. {MAX_HYPOTHESES}")
        if not (isinstance(self.min_inliers, int) and self.min_inliers >= 1):
            raise ValueError(f"epipolar: min_inliers={self.min_inliers}: at least 1")
        if not (isinstance(self.min_ratio, (int, float)) and 0 <= self.min_ratio <= 1):
            raise ValueError(f"epipolar: min_ratio={self.min_ratio}: 0 .. 1 (and no NaN)")
        if not isinstance(self.seed, int):
            raise ValueError(f"epipolar: seed={self.seed!r}: an integer")
        return self

    @property
    def permille(self):
        return int(round(1000 * self.min_ratio))


class EpiResult(NamedTuple):
    """What a pair adds to a FrameResult in a session with epipolar=, and what an EpipolarCheck returns: F (B,3,3) fp32,
    inliers, candidates (B) int32, ok (B) uint8, and per row of `matches` status (B,N) uint8 and dist2 (B,N) fp32.  Session
    buffers: valid until the next push (the next call)."""
    F: torch.Tensor
    inliers: torch.Tensor
    candidates: torch.Tensor
    ok: torch.Tensor
    status: torch.Tensor
    dist2: torch.Tensor


def as_epipolar(epipolar) -> Optional[Epipolar]:
    """None / False -> None, True -> the defaults, an Epipolar -> itself, validated; anything else is a ValueError."""
    if epipolar is None or epipolar is False:
        return None
    if epipolar is True:
        return Epipolar()
    if not isinstance(epipolar, Epipolar):
        raise ValueError(f"epipolar: True or a geometry.Epipolar(threshold, hypotheses, min_inliers, min_ratio, cull, seed) expected, "
                         f"got {type(epipolar).__name__}")
    return epipolar.validated()


class EpipolarCheck:
    """ops.epipolar_ransac with the state it needs between calls: the epoch word (one int32 on the device, so that every call,
    a replay of a captured one too, draws anew) and, per shape, the workspace and the outputs.  Enqueues only."""

    def __init__(self, config=True):
        self.config = as_epipolar(config)
        if self.config is None:
            raise ValueError("epipolar: an EpipolarCheck needs a configuration: True or an Epipolar(...)")
        self.epoch = None      # the int32 word on the device; made by the first call
        self._key = self._ws = self._out = None

    def prepare(self, b, n, device):
        """The epoch word, the workspace and the outputs for (B, N) on `device`, made once per shape: a session asks for them
        before it captures.  -> (ws, out)"""
        key = (b, n, device)
        if key != self._key:
            if self.epoch is None or self.epoch.device != device:
                self.epoch = torch.zeros((), dtype=torch.int32, device=device)
            self._ws = torch.empty(max(ops.epipolar_ws(b, n, self.config.hypotheses), 16), dtype=torch.uint8, device=device)
            self._out = (torch.empty((b, 3, 3), dtype=torch.float32, device=device), torch.empty((b,), dtype=torch.int32, device=device),
                         torch.empty((b,), dtype=torch.int32, device=device), torch.empty((b,), dtype=torch.uint8, device=device),
                         torch.empty((b, n), dtype=torch.uint8, device=device), torch.empty((b, n), dtype=torch.float32, device=device))
            self._key = key
        return self._ws, self._out

    def __call__(self, matches, valid, h, w, table=None, hold=None) -> EpiResult:
        """matches (B,N,4) fp32, valid (B,N) uint8 (updated in place), the frame's h and w, table: None or (pos, ids, age), hold:
        None or (B) uint8, samples that get no verdict (HomResult.planar)."""
        c = self.config
        ws = out = None
        if isinstance(matches, torch.Tensor) and matches.is_cuda and matches.dim() == 3:      # (else the wrapper names what is wrong)
            ws, out = self.prepare(matches.shape[0], matches.shape[1], matches.device)
        return EpiResult(*ops.epipolar_ransac(matches, valid, h, w, c.threshold, c.hypotheses, c.min_inliers, c.permille, c.seed, self.epoch,
                                              table=table, cull=c.cull, out=out, ws=ws, hold=hold))


class Homography(NamedTuple):
    """The homography check of a session (FrameSequence(homography=...)) or of a HomographyCheck.  threshold: the transfer error
    in px (in the second image) up to which a match is an inlier; hypotheses: minimal samples drawn per pair (1 .. 4096); a pair
    gets a verdict where the best model has at least min_inliers inliers (a minimal sample always fits its own 4 rows) and
    min_ratio of the candidates, and is `planar` - one plane or a pure rotation explains it - where it has planar_ratio of them.
    planar_ratio=0.9 is a stated default and NOT validated on real video: that needs trained weights, which this repository does
    not have; a consumer should set it from its own footage.  cull defaults to False, unlike Epipolar.cull: in a general scene
    the outliers of a homography are simply the points off the plane, good tracks that the epipolar check behind it needs; set it
    for a camera known to rotate only, where an outlier is a mismatch or a moving object.  hold_epipolar: in a session with
    epipolar=, a planar pair gets no epipolar verdict (its F would be arbitrary, and would cull off-plane tracks against it).
    dense: also write the residual of the dense flow against H (HomResult.residual).  seed: of the draws."""
    threshold: float = 1.0
    hypotheses: int = 512
    min_inliers: int = 8
    min_ratio: float = 0.5
    planar_ratio: float = 0.9
    cull: bool = False
    hold_epipolar: bool = True
    dense: bool = False
    seed: int = 0

    def validated(self):
        """-> self, or a ValueError that names `homography` and the field."""
        if not (isinstance(self.threshold, (int, float)) and 0 <= self.threshold < float("inf")):
            raise ValueError(f"homography: threshold={self.threshold}: a finite number of pixels >= 0 (and no NaN)")
        if not (isinstance(self.hypotheses, int) and 1 <= self.hypotheses <= MAX_HYPOTHESES):
            raise ValueError(f"homography: hypotheses={self.hypotheses}: 1 .. {MAX_HYPOTHESES}")
        if not (isinstance(self.min_inliers, int) and self.min_inliers >= 1):
            raise ValueError(f"homography: min_inliers={self.min_inliers}: at least 1")
        if not (isinstance(self.min_ratio, (int, float)) and 0 <= self.min_ratio <= 1):
            raise ValueError(f"homography: min_ratio={self.min_ratio}: 0 .. 1 (and no NaN)")
        if not (isinstance(self.planar_ratio, (int, float)) and 0 <= self.planar_ratio <= 1):
            raise ValueError(f"homography: planar_ratio={self.planar_ratio}: 0 .. 1 (and no NaN)")
        if not isinstance(self.seed, int):
            raise ValueError(f"homography: seed={self.seed!r}: an integer")
        return self

    @property
    def permille(self):
        return int(round(1000 * self.min_ratio))

    @property
    def planar_permille(self):
        return int(round(1000 * self.planar_ratio))


class HomResult(NamedTuple):
    """What a pair adds to a FrameResult in a session with homography=, and what a HomographyCheck returns: H (B,3,3) fp32,
    inliers, candidates (B) int32, ok, planar (B) uint8, per row of `matches` status (B,N) uint8 and dist2 (B,N) fp32, and the
    dense residual (B,h,w) fp32 (None without Homography.dense).  Session buffers: valid until the next push (the next call)."""
    H: torch.Tensor
    inliers: torch.Tensor
    candidates: torch.Tensor
    ok: torch.Tensor
    planar: torch.Tensor
    status: torch.Tensor
    dist2: torch.Tensor
    residual: Optional[torch.Tensor]


def as_homography(homography) -> Optional[Homography]:
    """None / False -> None, True -> the defaults, a Homography -> itself, validated; anything else is a ValueError."""
    if homography is None or homography is False:
        return None
    if homography is True:
        return Homography()
    if not isinstance(homography, Homography):
        raise ValueError(f"homography: True or a geometry.Homography({', '.join(Homography._fields)}) expected, got {type(homography).__name__}")
    return homography.validated()


class HomographyCheck:
    """ops.homography_ransac (and, with Homography.dense, ops.homography_residual) with the state it needs between calls: an
    epoch word of its own and, per shape, the workspace and the outputs.  Enqueues only."""

    def __init__(self, config=True):
        self.config = as_homography(config)
        if self.config is None:
            raise ValueError("homography: a HomographyCheck needs a configuration: True or a Homography(...)")
        self.epoch = None      # the int32 word on the device; made by the first call
        self._key = self._ws = self._out = self._residual = None

    def prepare(self, b, n, device, h=None, w=None):
        """The epoch word, the workspace and the outputs for (B, N) - and, with dense, the residual of an h x w frame - on
        `device`, made once per shape: a session asks for them before it captures.  -> (ws, out)"""
        key = (b, n, device)
        if key != self._key:
            if self.epoch is None or self.epoch.device != device:
                self.epoch = torch.zeros((), dtype=torch.int32, device=device)
            self._ws = torch.empty(max(ops.homography_ws(b, n, self.config.hypotheses), 16), dtype=torch.uint8, device=device)
            self._out = (torch.empty((b, 3, 3), dtype=torch.float32, device=device), torch.empty((b,), dtype=torch.int32, device=device),
                         torch.empty((b,), dtype=torch.int32, device=device), torch.empty((b,), dtype=torch.uint8, device=device),
                         torch.empty((b,), dtype=torch.uint8, device=device), torch.empty((b, n), dtype=torch.uint8, device=device),
                         torch.empty((b, n), dtype=torch.float32, device=device))
            self._key, self._residual = key, None
        if self.config.dense and h is not None and (self._residual is None or tuple(self._residual.shape) != (b, h, w)):
            self._residual = torch.empty((b, h, w), dtype=torch.float32, device=device)
        return self._ws, self._out

    def __call__(self, matches, valid, h, w, table=None, flow=None) -> HomResult:
        """matches (B,N,4) fp32, valid (B,N) uint8 (updated in place), the frame's h and w, table: None or (pos, ids, age); flow:
        with Homography.dense the (B,2,h,w) flow of the pair, any strides."""
        c = self.config
        if c.dense and flow is None:
            raise ValueError("homography: dense=True needs the pair's flow: check(matches, valid, h, w, flow=flow_up)")
        ws = out = None
        if isinstance(matches, torch.Tensor) and matches.is_cuda and matches.dim() == 3:      # (else the wrapper names what is wrong)
            ws, out = self.prepare(matches.shape[0], matches.shape[1], matches.device, h if c.dense else None, w)
        res = ops.homography_ransac(matches, valid, h, w, c.threshold, c.hypotheses, c.min_inliers, c.permille, c.planar_permille, c.seed, self.epoch,
                                    table=table, cull=c.cull, out=out, ws=ws)
        residual = ops.homography_residual(flow, res[0], res[3], out=self._residual) if c.dense else None
        return HomResult(*res, residual)
