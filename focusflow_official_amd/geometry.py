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

MAX_HYPOTHESES = 4096      # csrc/ransac_common.h


def _validated(config, ratios=("min_ratio",)):
    """-> config, or a ValueError that names the check (the configuration's class name in lower case) and the field."""
    word = type(config).__name__.lower()
    if not (isinstance(config.threshold, (int, float)) and 0 <= config.threshold < float("inf")):
        raise ValueError(f"{word}: threshold={config.threshold}: a finite number of pixels >= 0 (and no NaN)")
    if not (isinstance(config.hypotheses, int) and 1 <= config.hypotheses <= MAX_HYPOTHESES):
        raise ValueError(f"{word}: hypotheses={config.hypotheses}: 1 .. {MAX_HYPOTHESES}")
    if not (isinstance(config.min_inliers, int) and config.min_inliers >= 1):
        raise ValueError(f"{word}: min_inliers={config.min_inliers}: at least 1")
    for name in ratios:
        ratio = getattr(config, name)
        if not (isinstance(ratio, (int, float)) and 0 <= ratio <= 1):
            raise ValueError(f"{word}: {name}={ratio}: 0 .. 1 (and no NaN)")
    if not isinstance(config.seed, int):
        raise ValueError(f"{word}: seed={config.seed!r}: an integer")
    return config


def _permille(ratio):
    return int(round(1000 * ratio))


def as_config(word, value, cls):
    """The option `word` of a session, or of a check, as its configuration: None / False -> None, True -> the defaults, a `cls`
    (a NamedTuple with a validated() method) -> itself, validated; anything else is a ValueError headed by `word`."""
    if value is None or value is False:
        return None
    if value is True:
        return cls()
    if not isinstance(value, cls):
        raise ValueError(f"{word}: True or a {cls.__module__.rpartition('.')[2]}.{cls.__name__}({', '.join(cls._fields)}) expected, "
                         f"got {type(value).__name__}")
    return value.validated()


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
        return _validated(self)

    permille = property(lambda self: _permille(self.min_ratio))


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
    return as_config("epipolar", epipolar, Epipolar)


class _RansacCheck:
    """What EpipolarCheck and HomographyCheck keep between calls: the configuration, the epoch word (one int32 on the device, so
    that every call, a replay of a captured one too, draws anew) and, per shape, the workspace and the outputs."""
    _config = None      # the check's NamedTuple; its name in lower case opens the messages and names ops.<name>_ws
    _per_sample = (torch.int32, torch.int32, torch.uint8)      # dtypes of the (B) outputs between the model and status, dist2

    def __init__(self, config=True):
        cls, a = self._config.__name__, "an" if self._config.__name__[0] in "AEIOU" else "a"
        self.config = as_config(cls.lower(), config, self._config)
        if self.config is None:
            raise ValueError(f"{cls.lower()}: {a} {type(self).__name__} needs a configuration: True or {a} {cls}(...)")
        self.epoch = None      # the int32 word on the device; made by the first call
        self._key = self._ws = self._out = None

    def prepare(self, b, n, device):
        """The epoch word, the workspace and the outputs for (B, N) on `device`, made once per shape: a session asks for them
        before it captures.  -> (ws, out)"""
        key = (b, n, device)
        if key != self._key:
            if self.epoch is None or self.epoch.device != device:
                self.epoch = torch.zeros((), dtype=torch.int32, device=device)
            ws_bytes = getattr(ops, self._config.__name__.lower() + "_ws")
            self._ws = torch.empty(max(ws_bytes(b, n, self.config.hypotheses), 16), dtype=torch.uint8, device=device)
            self._out = (torch.empty((b, 3, 3), dtype=torch.float32, device=device),
                         *(torch.empty((b,), dtype=dtype, device=device) for dtype in self._per_sample),
                         torch.empty((b, n), dtype=torch.uint8, device=device), torch.empty((b, n), dtype=torch.float32, device=device))
            self._key = key
        return self._ws, self._out

    def _buffers(self, matches, *frame):
        """prepare() for the shape of `matches`; (None, None) where it is no 3-D device tensor: the wrapper then names what is wrong."""
        if isinstance(matches, torch.Tensor) and matches.is_cuda and matches.dim() == 3:
            return self.prepare(matches.shape[0], matches.shape[1], matches.device, *frame)
        return None, None


class EpipolarCheck(_RansacCheck):
    """ops.epipolar_ransac with the state it needs between calls (the epoch word, the workspace, the outputs).  Enqueues only."""
    _config = Epipolar

    def __call__(self, matches, valid, h, w, table=None, hold=None) -> EpiResult:
        """matches (B,N,4) fp32, valid (B,N) uint8 (updated in place), the frame's h and w, table: None or (pos, ids, age), hold:
        None or (B) uint8, samples that get no verdict (HomResult.planar)."""
        c = self.config
        ws, out = self._buffers(matches)
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
        return _validated(self, ("min_ratio", "planar_ratio"))

    permille = property(lambda self: _permille(self.min_ratio))
    planar_permille = property(lambda self: _permille(self.planar_ratio))


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
    return as_config("homography", homography, Homography)


class HomographyCheck(_RansacCheck):
    """ops.homography_ransac (and, with Homography.dense, ops.homography_residual) with the state it needs between calls: an
    epoch word of its own, the workspace, the outputs and the dense residual.  Enqueues only."""
    _config = Homography
    _per_sample = _RansacCheck._per_sample + (torch.uint8,)      # planar
    _residual = None

    def prepare(self, b, n, device, h=None, w=None):
        """As every check's - and, with dense, the residual of an h x w frame.  -> (ws, out)"""
        if (b, n, device) != self._key:
            self._residual = None
        if self.config.dense and h is not None and (self._residual is None or tuple(self._residual.shape) != (b, h, w)):
            self._residual = torch.empty((b, h, w), dtype=torch.float32, device=device)
        return super().prepare(b, n, device)

    def __call__(self, matches, valid, h, w, table=None, flow=None) -> HomResult:
        """matches (B,N,4) fp32, valid (B,N) uint8 (updated in place), the frame's h and w, table: None or (pos, ids, age); flow:
        with Homography.dense the (B,2,h,w) flow of the pair, any strides."""
        c = self.config
        if c.dense and flow is None:
            raise ValueError("homography: dense=True needs the pair's flow: check(matches, valid, h, w, flow=flow_up)")
        ws, out = self._buffers(matches, h if c.dense else None, w)
        res = ops.homography_ransac(matches, valid, h, w, c.threshold, c.hypotheses, c.min_inliers, c.permille, c.planar_permille, c.seed, self.epoch,
                                    table=table, cull=c.cull, out=out, ws=ws)
        residual = ops.homography_residual(flow, res[0], res[3], out=self._residual) if c.dense else None
        return HomResult(*res, residual)
