"""The homography check: csrc/homography.hip (ff_homography_ws, ff_homography_ransac, ff_homography_residual), the hold of the
epipolar check (ff_epipolar_ransac_hold), ops.homography_*, geometry.Homography / HomographyCheck and
frames.FrameSequence(homography=...).

The definition is exact (include/focusflow_hip.h), so the kernels and the session are held to the numpy restatement of
tests/homography_ref.py with equality: there are no tolerances here.  The restatement itself is held to ground truth: synthetic
scenes under a known homography whose planted inliers it has to find, all of them and nothing else.  The models, frames and
shapes of the session tests are those of tests/test_tracks.py and tests/test_epipolar.py."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import epipolar_ref as E
import fb_ref as FB
import homography_ref as HR
import tracks_ref as R
import test_tracks as T
from test_tracks import models      # noqa: F401  (the module-scoped fixture: FF-RAFT on det_sd and the plain spec)

DEV = T.DEV
ENTRY_POINTS = ("ff_homography_ws", "ff_homography_ransac", "ff_homography_residual", "ff_epipolar_ransac_hold")
H, W = T.H, T.W
F32 = np.float32
INF = F32(np.inf)
ITERS, FRAMES = T.ITERS, 4
SH, SW = 128, 160                   # the frame of the synthetic scenes
_same = T._same


# ----------------------------------------------------------------------------
# synthetic scenes under a known homography
# ----------------------------------------------------------------------------
def true_homography(rng, h=SH, w=SW):
    """A pinhole camera (f = 120 px) turns by a few hundredths of a radian and moves in front of a slanted plane: K (R + t n^t / d)
    K^-1 in pixel coordinates, float64."""
    kc = np.array([[120.0, 0, (w - 1) / 2], [0, 120.0, (h - 1) / 2], [0, 0, 1]])
    rv = rng.uniform(-0.03, 0.03, 3)
    th = np.linalg.norm(rv)
    k = rv / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    rot = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    t, n = rng.uniform(-0.3, 0.3, 3), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
    return kc @ (rot + np.outer(t, n) / 5.0) @ np.linalg.inv(kc)


def scene(seed, n=64, outliers=16, h=SH, w=SW):
    """n points of the frame and their images under true_homography, rounded to float32; `outliers` of the matches are displaced by
    30 px in a random direction.  -> (matches (1,n,4) float32, inlier (n) bool, the homography (3,3) float64)."""
    rng = np.random.default_rng(seed)
    hm = true_homography(rng, h, w)
    x = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), np.ones(n)])
    x2 = hm @ x
    x2 = x2 / x2[2]
    bad = np.zeros(n, bool)
    bad[rng.choice(n, outliers, replace=False)] = True
    ang = rng.uniform(0, 2 * np.pi, n)
    x2[0, bad] += 30.0 * np.cos(ang[bad])
    x2[1, bad] += 30.0 * np.sin(ang[bad])
    return np.stack([x[0], x[1], x2[0], x2[1]], 1).astype(F32)[None], ~bad, hm


# chosen by running the restatement on seeds 0 .. 11: all twelve qualify (a homography needs 4 clean rows of 64, not 8), the first five are taken
EXACT_SCENES = (0, 1, 2, 3, 4)
LOW_INLIER_SCENE = 100              # 38 of 64 displaced: the best of 64 hypotheses stays below 50 %: no verdict


def _table_for(m, first_id=100):
    """A track table whose slots are the rows of m: live where m holds a row, at the row's target."""
    b, n, _ = m.shape
    tb = R.empty_table(b, n, next_id=first_id + b * n)
    row = ~(m[..., 0] < 0)
    tb["pos"][row] = m[..., 2:][row]
    tb["ids"][row] = (first_id + np.arange(b * n).reshape(b, n))[row]
    tb["age"][row] = 1 + (np.arange(b * n).reshape(b, n) % 5)[row]
    return tb


def _equal_tables(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=k == "pos") for k in b)


# ----------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    from focusflow_official_amd import _hip, build
    hdr = open(os.path.join(ROOT, "include", "focusflow_hip.h")).read()
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    bound = _hip.load()
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), f"{name} is not declared in focusflow_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.EXPORTS
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, flags=re.M | re.S).group(1)
        args = getattr(bound, name).argtypes
        assert len(decl.split(",")) == len(args), f"{name}: {len(args)} bound arguments, the header declares {len(decl.split(','))}"
    assert all(n in _hip._SIGS for n in ENTRY_POINTS[1:])
    assert len(_hip._SIGS["ff_epipolar_ransac_hold"]) == len(_hip._SIGS["ff_epipolar_ransac"]) + 1
    assert len(_hip._SIGS["ff_homography_ransac"]) == len(_hip._SIGS["ff_epipolar_ransac"]) + 2      # planar_permille, planar
    history = hdr.split("#define FF_ABI_VERSION")[0]
    assert "7 (unchanged): entry points only: ff_homography_ws, ff_homography_ransac, ff_homography_residual, ff_epipolar_ransac_hold" in history
    assert "7 (unchanged): entry points only: ff_epipolar_ws, ff_epipolar_ransac" in history      # (the earlier lines stay)
    lib.ff_abi_version.restype = ctypes.c_int
    assert lib.ff_abi_version() == int(re.search(r"#define FF_ABI_VERSION (\d+)", hdr).group(1)) == _hip.ABI_VERSION == 7
    # the workspace size is a plain function of the shape: no device needed
    assert bound.ff_homography_ws(1, 500, 512) == 4 * (1 + 4 * 500 + 10 * 512) and bound.ff_homography_ws(2, 4096, 4096) > 0
    assert bound.ff_homography_ws(1, 4097, 1) == 0 and bound.ff_homography_ws(1, 8, 4097) == 0 and bound.ff_homography_ws(0, 8, 8) == 0
    assert all(bound.ff_homography_ws(b, n, k) == bound.ff_epipolar_ws(b, n, k) for b, n, k in ((1, 1, 1), (3, 70, 70), (1024, 4096, 1)))


def test_wrappers_raise_on_cpu_tensors():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    from focusflow_official_amd.geometry import Homography, HomographyCheck
    m, v, e = torch.zeros(1, 8, 4), torch.ones(1, 8, dtype=torch.uint8), torch.zeros((), dtype=torch.int32)
    with pytest.raises(FocusFlowHipError, match="matches"):
        ops.homography_ransac(m, v, 5, 7, 1.0, 8, 4, 0, 900, 0, e)
    with pytest.raises(FocusFlowHipError, match="matches"):
        HomographyCheck()(m, v, 5, 7)
    with pytest.raises(FocusFlowHipError, match="flow"):
        ops.homography_residual(torch.zeros(1, 2, 5, 7), torch.zeros(1, 3, 3), torch.ones(1, dtype=torch.uint8))
    with pytest.raises(FocusFlowHipError, match="matches"):
        ops.epipolar_ransac(m, v, 5, 7, 1.0, 8, 8, 0, 0, e, hold=torch.zeros(1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="homography.*flow"):
        HomographyCheck(Homography(dense=True))(m, v, 5, 7)


def test_bad_configurations_are_refused():
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.geometry import Homography, HomographyCheck, HomResult
    from focusflow_official_amd.keypoints import GoodFeatures
    plain, det = FF_RAFT_FUSION(use_fusion=None).eval(), GoodFeatures()
    for bad, field in ((Homography(threshold=-1.0), "threshold"), (Homography(threshold=float("nan")), "threshold"), (Homography(hypotheses=0), "hypotheses"),
                       (Homography(hypotheses=4097), "hypotheses"), (Homography(min_ratio=-0.1), "min_ratio"), (Homography(min_ratio=1.5), "min_ratio"),
                       (Homography(min_ratio=float("nan")), "min_ratio"), (Homography(planar_ratio=1.5), "planar_ratio"),
                       (Homography(planar_ratio=float("nan")), "planar_ratio"), (Homography(min_inliers=0), "min_inliers"), (Homography(seed=0.5), "seed"),
                       ("yes", "homography"), (0.5, "homography")):
        with pytest.raises(ValueError, match="homography: " + (field if field != "homography" else "")):
            FrameSequence(plain, keypoints=det, homography=bad)
        with pytest.raises(ValueError, match="homography"):
            HomographyCheck(bad)
        if isinstance(bad, Homography):
            with pytest.raises(ValueError, match="homography: " + field):
                bad.validated()
    with pytest.raises(ValueError, match="homography.*keypoints"):
        FrameSequence(plain, homography=True)      # no keypoints=
    assert FrameSequence(plain, keypoints=det).homography is None and FrameSequence(plain, keypoints=det, homography=False).homography is None
    assert FrameSequence(plain, keypoints=det, homography=True).homography == Homography() == (1.0, 512, 8, 0.5, 0.9, False, True, False, 0)
    assert Homography._fields == ("threshold", "hypotheses", "min_inliers", "min_ratio", "planar_ratio", "cull", "hold_epipolar", "dense", "seed")
    assert Homography().permille == 500 and Homography().planar_permille == 900 and Homography(planar_ratio=0.3335).planar_permille == 334
    assert HomResult._fields == ("H", "inliers", "candidates", "ok", "planar", "status", "dist2", "residual")
    seq = FrameSequence(plain, keypoints=det, tracks=True, fb=True, epipolar=True, homography=Homography(threshold=2.0, hypotheses=4096, seed=7, dense=True))
    assert seq.homography.threshold == 2.0 and seq.homography.hypotheses == 4096 and seq.homography.seed == 7 and seq.epipolar is not None


def test_sampler_draws_four_distinct_ranks():
    k = np.arange(300)
    for m in (4, 5, 17, 64, 4096):
        d = HR.draws(3, 1, 0, k, m)
        assert d.shape == (300, 4) and d.min() >= 0 and d.max() < m
        assert all(len(set(row)) == 4 for row in d.tolist()), m
        assert (HR.draws(3, 1, 0, k, m) == d).all()
        if m == 4:
            assert (np.sort(d, 1) == np.arange(4)).all()
    d = HR.draws(3, 1, 0, k, 64)
    assert len({tuple(r) for r in d.tolist()}) == 300                                              # another hypothesis
    for other in (HR.draws(3, 2, 0, k, 64), HR.draws(3, 1, 1, k, 64), HR.draws(4, 1, 0, k, 64)):       # another epoch, sample, seed
        assert (other != d).any(1).mean() > 0.99
    assert (HR.draws(3, 1, 0, np.asarray([5]), 64) == d[5]).all() and d[:, 0].max() <= 60 and len(set(d[:, 3].tolist())) > 32
    # the counters are 4 k + j of the shared hash
    assert d[7, 0] == int(E.word(3, 1, 0, 4 * 7)) % 61 and HR.draws(3, 1, 0, np.asarray([4095]), 4096)[0, 0] == int(E.word(3, 1, 0, 4 * 4095)) % 4093


def test_definition_finds_the_planted_inliers():
    """A condition on the DEFINITION: fp32 elimination of the DLT system on frame-normalised coordinates and 64 hypotheses recover
    exactly the planted inlier sets, with orders of magnitude to spare on both sides of the threshold."""
    ones = np.ones((1, 64), np.uint8)
    for seed in EXACT_SCENES:
        m, inlier, true = scene(seed)
        r = HR.ransac(m, ones, SH, SW, 1.0, 64, 8, 500, 900, seed=0, epoch=0)
        d = r["dist2"][0]
        print(f"scene {seed}: best {int(r['best'][0])}, inliers {int(r['inliers'][0])}, largest inlier dist2 {d[inlier].max():.3g} px^2, "
              f"smallest outlier dist2 {d[~inlier].min():.3g} px^2")
        assert r["ok"][0] == 1 and r["planar"][0] == 0 and r["candidates"][0] == 64 and r["inliers"][0] == 48      # (48 / 64 < 90 %)
        assert ((r["status"][0] == HR.INLIER) == inlier).all() and ((r["status"][0] == HR.OUTLIER) == ~inlier).all()
        assert d[inlier].max() < 1e-3 and d[~inlier].min() > 100
        assert (r["valid"][0] == inlier).all() and r["epoch"] == 1
        # H in pixel coordinates is the planted map up to scale (fp64 on the fp32 H), with w > 0 on the frame
        got = r["H"][0].astype(np.float64)
        assert got[2, 2] > 0 and np.abs(got / got[2, 2] - true / true[2, 2]).max() < 1e-2, (got / got[2, 2], true / true[2, 2])
        x = np.c_[m[0, :, :2], np.ones(64)].astype(np.float64)
        y = got @ x.T
        assert (y[2] > 0).all() and np.abs(y[:2] / y[2] - m[0, :, 2:].T)[:, inlier].max() < 0.05
        assert HR.ransac(m, ones, SH, SW, 1.0, 64, 8, 500, 750, seed=0, epoch=0)["planar"][0] == 1          # 48 / 64 = 75 %
    m, inlier, _ = scene(LOW_INLIER_SCENE, outliers=38)
    r = HR.ransac(m, ones, SH, SW, 1.0, 64, 8, 500, 900, seed=0, epoch=0)
    assert r["ok"][0] == 0 and r["planar"][0] == 0 and r["inliers"][0] == 0 and (r["status"][0] == HR.NO_VERDICT).all() and (r["valid"] == 1).all()
    assert not r["H"].any() and (r["dist2"] == INF).all()
    loose = HR.ransac(m, ones, SH, SW, 1.0, 64, 8, 0, 0, seed=0, epoch=0)      # the same draws without the ratios: a verdict, and planar with it
    assert loose["ok"][0] == 1 and loose["planar"][0] == 1 and 4 <= loose["inliers"][0] < 32


def _fold_sample():
    """Four matches whose only homography sends the line at infinity through the quadrilateral: (0,0), (1,0), (1,1), (0,1) of a
    unit square go to a bow tie (two targets swapped), so w changes sign between the four points."""
    src = np.asarray([[40, 30], [100, 30], [100, 90], [40, 90]], F32)
    dst = np.asarray([[40, 30], [100, 30], [40, 90], [100, 90]], F32)
    return np.concatenate([src, dst], 1)[None]


def _degenerate_cases():
    """-> [(name, matches (B,N,4), valid (B,N), verdict expected: True, False, or None where the definition's own rounding decides)]"""
    good, _, _ = scene(0)
    few = good[:, :8].copy()
    few_valid = np.asarray([[1, 0, 1, 0, 0, 1, 0, 0]], np.uint8)                           # M = 3
    four = good[:, :4].copy()                                                              # N = M = 4: every draw is these rows
    t = np.linspace(5, 120, 20, dtype=F32)
    # every source point on one line.  On the frame's own axis y = cy the normalised y is exactly 0: three columns of every system
    # are exactly zero and stay so, hence a pivot of 0 in every hypothesis.  On a slanted line the rounding of the normalisation
    # breaks the collinearity, the pivots are tiny instead of 0, and what comes out is the definition's to say (the device must
    # say the same)
    line = np.stack([t, np.full_like(t, (SH - 1) / 2), t + F32(2), F32(0.5) * t + F32(4)], 1)[None]
    slanted = np.stack([t, F32(0.5) * t + F32(3), t + F32(2), F32(0.5) * t + F32(4)], 1)[None]
    same = np.tile(np.asarray([[[40.5, 30.25, 42.0, 31.5]]], F32), (1, 20, 1))
    mixed = good.copy()
    mixed[0, 3, 2], mixed[0, 9, 1], mixed[0, 11, 0] = np.nan, np.inf, np.nan              # non-finite rows with valid = 1
    mixed[0, [6, 20, 63]] = -1                                                            # no-rows
    mixed_valid = np.ones((1, 64), np.uint8)
    mixed_valid[0, [6, 20, 63, 30, 31]] = 0
    return [("M < 4", few, few_valid, False), ("M = 4", four, np.ones((1, 4), np.uint8), True), ("collinear", line, np.ones((1, 20), np.uint8), False),
            ("collinear, slanted", slanted, np.ones((1, 20), np.uint8), None),
            ("one point", same, np.ones((1, 20), np.uint8), False), ("a fold", _fold_sample(), np.ones((1, 4), np.uint8), False),
            ("non-finite rows and no-rows", mixed, mixed_valid, True)]


def test_degenerate_inputs():
    f, good = E.solve(np.zeros((2, 8, 9), F32))
    assert not good.any()
    for name, m, valid, verdict in _degenerate_cases():
        tb = _table_for(m)
        for epoch in (0, 5):
            r = HR.ransac(m, valid, SH, SW, 1.0, 32, 4, 0, 900, seed=1, epoch=epoch, table=tb, cull=True)
            st = r["status"][0]
            assert r["epoch"] == epoch + 1, name
            assert r["inliers"][0] == (st == HR.INLIER).sum(), name
            row = ~(m[0, :, 0] < 0)
            finite = np.isfinite(m[0]).all(1)
            cand = row & finite & (valid[0] == 1)
            assert r["candidates"][0] == cand.sum() and ((st == HR.NO_ROW) == ~row).all() and ((st == HR.NOT_CANDIDATE) == (row & ~cand)).all(), name
            assert (r["dist2"][0][~row] == -1).all() and (r["dist2"][0][row & ~finite] == INF).all(), name
            assert verdict is None or r["ok"][0] == verdict, name
            if verdict is None:
                continue
            if not verdict:
                assert not r["H"].any() and (st[cand] == HR.NO_VERDICT).all() and r["planar"][0] == 0, name
                assert (r["valid"] == valid).all() and _equal_tables(r["table"], tb), name
                assert (r["dist2"][0][row] == INF).all(), name
            elif name == "M = 4":
                # the one sample there is fits its own rows: everything an inlier, and planar
                assert r["planar"][0] == 1 and (st == HR.INLIER).all() and r["dist2"].max() < 1e-3 and (r["valid"] == 1).all() and _equal_tables(r["table"], tb)
            else:
                assert (st[cand] != HR.NO_VERDICT).all() and (st == HR.OUTLIER).any(), name
                dead = st == HR.OUTLIER
                assert (r["valid"][0] == (valid[0] & ~dead)).all() and (r["valid"][0][[3, 9, 11]] == 1).all(), name      # (status 2 leaves valid alone)
                assert (r["table"]["ids"][0][dead] == -1).all() and (r["table"]["ids"][0][~dead] == tb["ids"][0][~dead]).all(), name
                assert (r["table"]["pos"][0][dead] == -1).all() and (r["table"]["age"][0][dead] == 0).all(), name
                kept = HR.ransac(m, valid, SH, SW, 1.0, 32, 4, 0, 900, seed=1, epoch=epoch, table=tb)      # cull=False, the default
                assert (kept["status"] == r["status"]).all() and (kept["valid"] == r["valid"]).all() and _equal_tables(kept["table"], tb)
    # the fold: the system has a solution (it is a regular 8 x 8 problem), and it is refused for the sign of w alone
    fold = _fold_sample()
    s, cx, cy, _, _ = E.frame_constants(SH, SW, 1.0)
    xn = np.stack([(fold[0, :, 0] - cx) * s, (fold[0, :, 1] - cy) * s, (fold[0, :, 2] - cx) * s, (fold[0, :, 3] - cy) * s])
    hs, good, picks = HR.hypotheses(xn, 1, 0, 0, 8)
    _, solved = E.solve(HR.system(*(xn[i][picks] for i in range(4))))
    assert solved.all() and not good.any()
    w = (hs[:, 6, None] * xn[0][picks] + hs[:, 7, None] * xn[1][picks]) + hs[:, 8, None]
    assert ((w > 0).any(1) & (w < 0).any(1)).all()
    # a stationary camera: H is the identity up to scale, every candidate an inlier, planar
    still, _, _ = scene(3)
    still[0, :, 2:] = still[0, :, :2]
    r = HR.ransac(still, np.ones((1, 64), np.uint8), SH, SW, 1.0, 32, 8, 500, 900, seed=1, epoch=0)
    g = r["H"][0].astype(np.float64)
    assert r["ok"][0] == 1 and r["planar"][0] == 1 and r["inliers"][0] == 64 and (r["status"] == HR.INLIER).all() and r["dist2"].max() < 1e-6
    assert g[2, 2] > 0 and np.abs(g / g[2, 2] - np.eye(3)).max() < 1e-4, g
    # the arguments are left alone
    name, m, valid, _ = _degenerate_cases()[-1]
    assert valid[0, 0] == 1 and _table_for(m)["ids"][0, 0] == 100


def test_frame_result_has_sixteen_shapes():
    """What tests/test_epipolar.py::test_frame_result_has_eight_shapes holds for the results without hom, for all sixteen shapes;
    and the eight without are what they were."""
    import copy
    import pickle
    from focusflow_official_amd import frames
    from focusflow_official_amd.frames import FBResult, FrameResult
    from focusflow_official_amd.geometry import EpiResult, HomResult
    from focusflow_official_amd.tracks import TrackResult
    tr = TrackResult(torch.arange(4)[None], torch.zeros(1, 4, dtype=torch.int32), torch.tensor([4], dtype=torch.int32))
    fb = FBResult(torch.ones(1, 2, 3, 3), torch.zeros(1, 1, 3, 3), torch.ones(1, 1, 3, 3, dtype=torch.uint8), torch.ones(1, 4), torch.ones(1, 4, dtype=torch.uint8))
    epi = EpiResult(torch.eye(3)[None], torch.tensor([3], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), torch.ones(1, dtype=torch.uint8),
                    torch.ones(1, 4, dtype=torch.uint8), torch.zeros(1, 4))
    hom = HomResult(2 * torch.eye(3)[None], torch.tensor([3], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), torch.ones(1, dtype=torch.uint8),
                    torch.zeros(1, dtype=torch.uint8), torch.ones(1, 4, dtype=torch.uint8), torch.zeros(1, 4), None)
    base = (torch.ones(2), torch.zeros(3), torch.ones(1, 4, 4), torch.ones(1, 4, dtype=torch.uint8), torch.tensor([4], dtype=torch.int32))

    def same(a, b):
        if isinstance(a, tuple):
            return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))

    old = {(): "FrameResult", ("tracks",): "TrackedFrameResult", ("fb",): "CheckedFrameResult", ("tracks", "fb"): "TrackedCheckedFrameResult",
           ("epi",): "EpiFrameResult", ("tracks", "epi"): "TrackedEpiFrameResult", ("fb", "epi"): "CheckedEpiFrameResult",
           ("tracks", "fb", "epi"): "TrackedCheckedEpiFrameResult"}
    names = dict(old)
    names.update({extra + ("hom",): cls.replace("FrameResult", "HomFrameResult") for extra, cls in old.items()})
    assert len(names) == 16 and len(set(names.values())) == 16 and names[("hom",)] == "HomFrameResult"
    assert names[("tracks", "fb", "epi", "hom")] == "TrackedCheckedEpiHomFrameResult"
    given = {"tracks": tr, "fb": fb, "epi": epi, "hom": hom}
    for extra, cls in names.items():
        res = FrameResult(*base, **{k: given[k] for k in extra})
        n = 5 + len(extra)
        assert type(res) is getattr(frames, cls) and isinstance(res, FrameResult) and len(res) == n and type(res).__name__ == cls
        assert type(res).__module__ == frames.__name__ and type(res).__qualname__ == cls
        assert res._fields == ("flow_low", "flow_up", "matches", "valid", "count") + extra and list(res._asdict()) == list(res._fields)
        assert all(getattr(res, f) is v for f, v in zip(res._fields, res))
        assert all(getattr(res, k) is (given[k] if k in extra else None) for k in given)
        for clone in (copy.copy(res), copy.deepcopy(res), pickle.loads(pickle.dumps(res)), FrameResult._make(res), res._replace()):
            assert clone is not res and same(clone, res), (cls, type(clone))
        assert copy.copy(res)[0] is res[0] and copy.deepcopy(res)[0] is not res[0]
        moved = res._replace(count=7)
        assert moved.count == 7 and type(moved) is type(res) and moved.flow_low is res.flow_low and moved.hom is res.hom and moved.epi is res.epi
        with pytest.raises(ValueError):
            res._replace(homography=1)
        with pytest.raises(ValueError):
            res._replace(flow=1)
        if "hom" in extra:
            assert res[-1] is hom and res._fields[-1] == "hom" and type(res._replace(hom=None)).__name__ == names[extra[:-1]]
            assert isinstance(res, getattr(frames, names[extra[:-1]]))      # (a subclass of the shape without: tracks, fb, epi stay where they are)
        else:
            assert "hom" not in res._asdict() and type(res._replace(hom=hom)).__name__ == names[extra + ("hom",)]
    # the eight shapes without hom are what they were: positional construction, lengths, class names, direct subclasses
    made = (FrameResult(*base), FrameResult(*base, tr), FrameResult(*base, None, fb), FrameResult(*base, tr, fb), FrameResult(*base, None, None, epi),
            FrameResult(*base, tr, None, epi), FrameResult(*base, None, fb, epi), FrameResult(*base, tr, fb, epi))
    assert [type(r).__name__ for r in made] == list(old.values()) and [len(r) for r in made] == [5, 6, 6, 7, 6, 7, 7, 8]
    assert all(type(r).__mro__[1:] == (FrameResult, tuple, object) for r in made[1:]) and all(r.hom is None for r in made)
    assert type(FrameResult(*base, tr, fb, epi, hom)).__name__ == "TrackedCheckedEpiHomFrameResult"
    with pytest.raises(TypeError):
        FrameResult._make(base + (tr, fb, epi, hom, hom))
    with pytest.raises(TypeError):
        FrameResult._make(base + (hom, hom))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_homography_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "homography.hip"))
    assert len(kernels) >= 5, kernels      # compact, hypotheses, score, select, residual
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"homography.hip: kernels with scratch (bytes per lane): {spilled}"
    hyp = [k for k in kernels if "ransac_hypotheses_kernel" in k["name"] and "Homography" in k["name"]]      # (the template's instantiation)
    assert len(hyp) == 1 and 64 * 72 * 4 <= int(hyp[0].get("LDS", "0")) <= 65536, f"the hypotheses kernel keeps 64 systems of 8 x 9 in LDS: {hyp}"
    res = [k for k in kernels if "hom_residual_kernel" in k["name"]]
    assert len(res) == 1 and int(res[0].get("LDS", "0")) == 0, res


# ----------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------
NAMES = ("H", "inliers", "candidates", "ok", "planar", "status", "dist2")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_op(m, valid, h, w, cfg, epoch, table, cull, what):
    """ops.homography_ransac on copies of the inputs against the restatement, value for value."""
    from focusflow_official_amd import ops
    threshold, k, min_inliers, permille, planar, seed = cfg
    want = HR.ransac(m, valid, h, w, threshold, k, min_inliers, permille, planar, seed=seed, epoch=epoch, table=table, cull=cull)
    dm, dv, de = _t(m), _t(valid), torch.tensor(epoch, dtype=torch.int32, device=DEV)
    dt = None if table is None else T._dev(table)
    got = ops.homography_ransac(dm, dv, h, w, threshold, k, min_inliers, permille, planar, seed, de,
                                table=None if dt is None else (dt["pos"], dt["ids"], dt["age"]), cull=cull)
    torch.cuda.synchronize()
    for name, g in zip(NAMES, got):
        _same(g, want[name], f"{what}: {name}")
    _same(dv, want["valid"], what + ": valid")
    _same(dm, m, what + ": matches are left alone")
    assert int(de) == want["epoch"] == epoch + 1, what
    if table is not None:
        T._same_table({k_: v.cpu().numpy() for k_, v in dt.items()}, want["table"], what + ": the table")
    assert int(want["inliers"].sum()) == int((want["status"] == HR.INLIER).sum())
    return want


def _op_case(b, n, seed, drop=0.1, norow=0.1):
    """b scenes of n rows (a quarter displaced) in one batch; some rows not valid, some no-rows."""
    rng = np.random.default_rng(1000 + seed)
    m = np.concatenate([scene(seed + i, n=n, outliers=n // 4)[0] for i in range(b)])
    valid = (rng.uniform(size=(b, n)) >= drop).astype(np.uint8)
    gone = rng.uniform(size=(b, n)) < norow
    m[gone], valid[gone] = -1, 0
    return m, valid


@pytest.mark.gpu
def test_op_equals_the_restatement_on_the_scenes():
    """The scenes of test_definition_finds_the_planted_inliers and the degenerate inputs, on the device."""
    ones = np.ones((1, 64), np.uint8)
    for seed in EXACT_SCENES + (5,):
        m, _, _ = scene(seed)
        for epoch in (0, 5):
            r = _run_op(m, ones, SH, SW, (1.0, 64, 8, 500, 750, 0), epoch, _table_for(m), True, f"scene {seed} epoch {epoch}")
        assert r["ok"][0] == 1
    m, _, _ = scene(LOW_INLIER_SCENE, outliers=38)
    assert _run_op(m, ones, SH, SW, (1.0, 64, 8, 500, 900, 0), 0, _table_for(m), True, "the 40 % scene")["ok"][0] == 0
    for name, m, valid, verdict in _degenerate_cases():
        for table in (None, _table_for(m)):
            assert _run_op(m, valid, SH, SW, (1.0, 32, 4, 0, 900, 1), 5, table, True, name)["ok"][0] in ((0, 1) if verdict is None else (verdict,))
    still, _, _ = scene(3)
    still[0, :, 2:] = still[0, :, :2]
    assert _run_op(still, ones, SH, SW, (1.0, 32, 8, 500, 900, 1), 0, None, False, "a stationary camera")["planar"][0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("b,n,k", [(2, 4, 4), (1, 70, 1), (1, 70, 70), (2, 70, 70), (1, 4096, 192)], ids=lambda v: str(v))
def test_op_equals_the_restatement(b, n, k):
    """N = 4 with M = 4: the minimal sample is the whole input; N = 70: a wave's tail, one hypothesis and a block's tail of them;
    N = 4096: every thread of the compaction takes four rows, three blocks of hypotheses."""
    if n == 4:
        m, valid = np.concatenate([scene(20 + i, n=4, outliers=0)[0] for i in range(b)]), np.ones((b, 4), np.uint8)
    else:
        m, valid = _op_case(b, n, 30 + n + k)
    verdicts = []
    for epoch, table, cull, (min_inliers, permille, planar) in ((0, True, True, (4, 0, 900)), (5, False, True, (4, 0, 0)), (5, True, False, (4, 0, 900)),
                                                                 (5, False, False, (4, 0, 700)), (0, True, True, (8, 500, 750))):
        r = _run_op(m, valid, SH, SW, (1.0, k, min_inliers, permille, planar, 3), epoch, _table_for(m) if table else None, cull,
                    f"B {b} N {n} K {k} epoch {epoch} table {table} cull {cull} min_inliers {min_inliers} planar {planar}")
        verdicts.append(r["ok"].tolist())
        print(f"B {b} N {n} K {k} epoch {epoch}: candidates {r['candidates'].tolist()}, inliers {r['inliers'].tolist()}, ok {r['ok'].tolist()}, "
              f"planar {r['planar'].tolist()}, status {np.bincount(r['status'].ravel(), minlength=5).tolist()}")
    assert any(any(v) for v in verdicts), "no configuration of this case reaches a verdict"
    if n == 4:
        assert r["candidates"].tolist() == [4] * b


@pytest.mark.gpu
def test_wrappers_refuse_by_name():
    from focusflow_official_amd import _hip, ops
    from focusflow_official_amd._hip import FocusFlowHipError
    m, valid = _op_case(1, 16, 1)
    dm, dv, de = _t(m), _t(valid), torch.zeros((), dtype=torch.int32, device=DEV)
    tb = T._dev(_table_for(m))
    off = torch.empty(1 * 16 * 4 + 1, dtype=torch.float32, device=DEV)[1:].view(1, 16, 4)
    call = lambda **kw: ops.homography_ransac(**{**dict(matches=dm, valid=dv, h=SH, w=SW, threshold=1.0, hypotheses=8, min_inliers=4, permille=0,      # noqa: E731
                                                        planar_permille=900, seed=0, epoch=de), **kw})
    for kw, word in ((dict(hypotheses=0), "K"), (dict(hypotheses=4097), "K"), (dict(h=(1 << 24) + 1), "H"), (dict(threshold=-1.0), "threshold"),
                     (dict(threshold=float("nan")), "threshold"), (dict(min_inliers=0), "min_inliers"), (dict(permille=1001), "permille"),
                     (dict(planar_permille=-1), "planar_permille"), (dict(matches=dm[:, :, :3]), "matches"), (dict(matches=off), "matches must be 16-byte aligned"),
                     (dict(matches=dm.double()), "matches"), (dict(valid=dv[:, :8]), "valid"), (dict(epoch=torch.zeros(2, dtype=torch.int32, device=DEV)), "epoch"),
                     (dict(epoch=torch.zeros((), dtype=torch.int64, device=DEV)), "epoch"), (dict(table=(tb["pos"], tb["ids"], None)), "table"),
                     (dict(table=(tb["pos"][:, :8].contiguous(), tb["ids"][:, :8].contiguous(), tb["age"][:, :8].contiguous())), "table"),
                     (dict(ws=torch.empty(16, dtype=torch.uint8, device=DEV)), "ws"), (dict(out=(de,)), "out")):
        with pytest.raises(FocusFlowHipError, match=word):
            call(**kw)
    with pytest.raises(FocusFlowHipError, match="hold"):
        ops.epipolar_ransac(dm, dv, SH, SW, 1.0, 8, 8, 0, 0, de, hold=torch.zeros(2, dtype=torch.uint8, device=DEV))
    with pytest.raises(FocusFlowHipError, match="hold"):
        ops.epipolar_ransac(dm, dv, SH, SW, 1.0, 8, 8, 0, 0, de, hold=torch.zeros(1, dtype=torch.int32, device=DEV))
    flow, hm, ok = torch.zeros(1, 2, 5, 7, device=DEV), torch.eye(3, device=DEV)[None], torch.ones(1, dtype=torch.uint8, device=DEV)
    for args, word in (((flow[:, :1], hm, ok), "flow"), ((flow.double(), hm, ok), "flow"), ((flow, hm[0], ok), "H"), ((flow, hm, ok.int()), "ok"),
                       ((flow, hm, torch.ones(2, dtype=torch.uint8, device=DEV)), "ok")):
        with pytest.raises(FocusFlowHipError, match=word):
            ops.homography_residual(*args)
    with pytest.raises(FocusFlowHipError, match="out"):
        ops.homography_residual(flow, hm, ok, out=torch.zeros(1, 5, 8, device=DEV))
    # the C ABI names its own: a partial table, N = 0
    P = ops._p
    outs = [torch.empty(64, dtype=torch.float32, device=DEV) for _ in range(7)]
    ws = torch.empty(ops.homography_ws(1, 16, 8), dtype=torch.uint8, device=DEV)

    def raw(n=16, pos=None, ids=None, age=None):
        _hip.call("ff_homography_ransac", P(dm), P(dv), 1, n, SH, SW, 1.0, 8, 4, 0, 900, 0, P(de), 1, P(pos), P(ids), P(age), *(P(o) for o in outs), P(ws),
                  ws.numel(), None)

    for kw, word in ((dict(pos=tb["pos"]), "ff_homography_ransac: a track table is pos, ids and age"), (dict(n=0), "ff_homography_ransac: N = 0"),
                     (dict(n=4097), "ff_homography_ransac: N = 4097")):
        with pytest.raises(FocusFlowHipError, match=word):
            raw(**kw)
    with pytest.raises(FocusFlowHipError, match="ff_homography_residual: B = 0"):
        _hip.call("ff_homography_residual", P(flow), 70, 35, 7, 1, P(hm), P(ok), 0, 5, 7, P(outs[0]), None)
    assert int(de) == 0      # (a refused call launches nothing)
    raw()
    assert int(de) == 1


def _epi_args(dm, dv, de, dt, cfg=(1.0, 32, 8, 0, 1)):
    return (dm, dv, SH, SW) + cfg + (de,), dict(table=None if dt is None else (dt["pos"], dt["ids"], dt["age"]), cull=True)


@pytest.mark.gpu
def test_epipolar_hold():
    """hold=None IS ops.epipolar_ransac; with hold = [1, 0] sample 0 has no verdict and its valid and table are untouched, sample 1
    is what it is unheld, and the epoch has advanced by one."""
    from focusflow_official_amd import ops
    import test_epipolar as TE
    m, valid = TE._op_case(2, 70, 7)
    tb = TE._table_for(m)
    runs = {}
    for key, hold in (("plain", "absent"), ("none", None), ("zeros", [0, 0]), ("held", [1, 0]), ("both", [1, 255])):
        dm, dv, de, dt = _t(m), _t(valid), torch.tensor(3, dtype=torch.int32, device=DEV), T._dev(tb)
        args, kw = _epi_args(dm, dv, de, dt)
        if hold != "absent":
            kw["hold"] = None if hold is None else torch.tensor(hold, dtype=torch.uint8, device=DEV)
        got = ops.epipolar_ransac(*args, **kw)
        torch.cuda.synchronize()
        runs[key] = dict(zip(("F", "inliers", "candidates", "ok", "status", "dist2"), (g.cpu().numpy() for g in got)), valid=dv.cpu().numpy(),
                         table={k: v.cpu().numpy() for k, v in dt.items()}, epoch=int(de))
        want = HR.epipolar_hold(m, valid, SH, SW, [0, 0] if hold in ("absent", None) else hold, threshold=1.0, hypotheses_=32, min_inliers=8, permille=0,
                                seed=1, epoch=3, table=tb, cull=True)
        for name in ("F", "inliers", "candidates", "ok", "status", "dist2", "valid"):
            _same(runs[key][name], want[name], f"hold {key}: {name}")
        T._same_table(runs[key]["table"], want["table"], f"hold {key}: the table")
        assert runs[key]["epoch"] == 4 == want["epoch"]
    plain, held = runs["plain"], runs["held"]
    assert plain["ok"].tolist() == [1, 1] and (plain["status"] == E.OUTLIER).any(1).all()      # (the unheld call does cull in both samples)
    for key in ("none", "zeros"):
        for name in ("F", "inliers", "candidates", "ok", "status", "dist2", "valid"):
            assert np.array_equal(runs[key][name], plain[name]), (key, name)
        T._same_table(runs[key]["table"], plain["table"], key)
    assert held["ok"].tolist() == [0, 1] and not held["F"][0].any() and held["inliers"][0] == 0 and held["candidates"][0] == plain["candidates"][0]
    assert (held["valid"][0] == valid[0]).all() and set(np.unique(held["status"][0])) <= {E.NO_ROW, E.NOT_CANDIDATE, E.NO_VERDICT}
    assert all(np.array_equal(held["table"][k][0], tb[k][0]) for k in ("pos", "ids", "age"))
    for name in ("F", "inliers", "ok", "status", "dist2", "valid"):
        assert np.array_equal(held[name][1], plain[name][1]), name
    assert runs["both"]["ok"].tolist() == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(5, 7), (33, 65)], ids=lambda v: str(v))
def test_residual_equals_the_restatement(h, w):
    """B = 2, ok = [1, 0]; the flow is a strided crop of a larger tensor (at an odd offset: the scalar path, and at an aligned one
    in a width that is a multiple of four: the float4 path with rows of both kinds); one H puts w <= 0 on part of the frame."""
    from focusflow_official_amd import ops
    rng = np.random.default_rng(h * w)
    big = rng.uniform(-4, 4, (2, 2, h + 9, w + 15)).astype(F32)
    hm = np.stack([np.asarray([[1.01, 0.02, -0.5], [-0.01, 0.99, 0.75], [-2.0 / w, 0.001, 1.0]], F32),      # w = 1 - 2 x / W: <= 0 on the right half
                   np.eye(3, dtype=F32)])
    dbig = _t(big)
    for top, left, ok in ((3, 5, [1, 0]), (4, 8, [1, 1]), (0, 0, [0, 1])):
        crop, dcrop = big[:, :, top:top + h, left:left + w], dbig[:, :, top:top + h, left:left + w]
        assert not dcrop.is_contiguous()
        want = HR.residual(crop, hm, ok)
        got = ops.homography_residual(dcrop, _t(hm), torch.tensor(ok, dtype=torch.uint8, device=DEV))
        torch.cuda.synchronize()
        _same(got, want, f"{h}x{w} crop at ({top},{left}) ok {ok}")
        if ok[0]:
            assert np.isinf(want[0]).any() and np.isfinite(want[0]).any() and (want[0][np.isfinite(want[0])] >= 0).all()
        assert (want[[i for i in range(2) if not ok[i]]] == -1).all()
    # a wider aligned case takes the float4 path on every row; transposed strides (ld_col != 1) take the scalar one
    wide = rng.uniform(-4, 4, (2, 2, h, 4 * w)).astype(F32)
    _same(ops.homography_residual(_t(wide), _t(hm), torch.tensor([1, 1], dtype=torch.uint8, device=DEV)), HR.residual(wide, hm, [1, 1]), "aligned")
    turned = _t(np.ascontiguousarray(wide.transpose(0, 1, 3, 2))).transpose(2, 3)
    assert turned.stride(3) != 1
    _same(ops.homography_residual(turned, _t(hm), torch.tensor([1, 1], dtype=torch.uint8, device=DEV)), HR.residual(wide, hm, [1, 1]), "transposed strides")
    # an exact flow under H leaves nothing: the identity and a zero flow
    zero = ops.homography_residual(torch.zeros(1, 2, h, w, device=DEV), _t(np.eye(3, dtype=F32)[None]), torch.ones(1, dtype=torch.uint8, device=DEV))
    assert float(zero.abs().max()) == 0


@pytest.mark.gpu
def test_homography_check_keeps_the_epoch():
    """geometry.HomographyCheck outside a session: consecutive calls run at epochs 0, 1, 2 - across a change of shape too -, each
    equal to the restatement, with the dense residual behind it."""
    from focusflow_official_amd.geometry import Homography, HomographyCheck
    check = HomographyCheck(Homography(threshold=1.0, hypotheses=64, seed=9, cull=True, dense=True))
    rng = np.random.default_rng(2)
    firsts = []
    for epoch, n in enumerate((64, 64, 48)):      # (the third call has another shape: new buffers, the same epoch word)
        m = scene(5, n=n, outliers=n // 4)[0]
        flow = rng.uniform(-2, 2, (1, 2, SH, SW)).astype(F32)
        dv = _t(np.ones((1, n), np.uint8))
        res = check(_t(m), dv, SH, SW, flow=_t(flow))
        want = HR.ransac(m, np.ones((1, n), np.uint8), SH, SW, 1.0, 64, 8, 500, 900, seed=9, epoch=epoch, cull=True)
        for name in NAMES:
            _same(getattr(res, name), want[name], f"HomographyCheck call {epoch}: {name}")
        _same(dv, want["valid"], f"HomographyCheck call {epoch}: valid")
        _same(res.residual, HR.residual(flow, want["H"], want["ok"]), f"HomographyCheck call {epoch}: residual")
        assert int(check.epoch) == epoch + 1 and want["ok"][0] == 1
        firsts.append(HR.draws(9, epoch, 0, np.arange(1), n).tolist())
    assert firsts[0] != firsts[1]


# ----------------------------------------------------------------------------
# sessions
# ----------------------------------------------------------------------------
# (threshold, hypotheses, min_inliers, min_ratio, planar_ratio) of the homography, (threshold, hypotheses, min_inliers, min_ratio) of the
# epipolar check behind it.  Random-weight flow rarely earns a verdict at the defaults; LOOSE gives every pair a verdict, and with
# planar_ratio = 0 every verdict is planar, so holds happen on every pair.
LOOSE, DEFAULT = ((1.0, 128, 4, 0.0, 0.0), (1.0, 128, 8, 0.0)), ((1.0, 512, 8, 0.5, 0.9), (1.0, 512, 16, 0.5))
# combination -> (fb, epipolar, hold_epipolar, cull, dense)
COMBOS = {"alone": (False, False, True, False, False), "fb": (True, False, True, False, False), "epi_hold": (False, True, True, False, False),
          "epi_free": (False, True, False, False, False), "fb_epi_hold": (True, True, True, False, False), "dense": (False, False, True, False, True),
          "cull_epi_hold": (False, True, True, True, False), "cull_epi_free_dense": (False, True, False, True, True)}
_RUNS = {}


def _frames():
    return T._u8_frames(1, H, W, FRAMES, T.SEED, T.SHIFT)


def _np(t):
    return t.detach().cpu().numpy()


def _expect(ref, det, frame, res, h, w, fb, combo, cfg, epoch):
    """One pair of a tracks session around the pair's own flows: tracks_ref.session_step, fb_ref behind it with fb = (alpha, beta),
    the restatement of the homography check at `epoch`, then that of the epipolar check, held where the pair is planar.
    -> (step, what HR.ransac gave, what the epipolar restatement gave or None, valid and table at the end of the step)"""
    _, epi, hold, cull, _ = COMBOS[combo]
    points, count = det.points(frame.to(DEV).permute(0, 3, 1, 2).float().contiguous())
    step = R.session_step(ref, _np(points), _np(count), _np(res.flow_up), h, w, det.min_distance)
    valid, table = step["valid"], step["table"]
    if fb:
        _, ws, valid, table = FB.matches(step["matches"], valid, _np(res.fb.flow_bw), 0, 0, h, w, fb[0], fb[1], table=table)
        _same(res.fb.status, ws, "fb status")
    hc, ec = cfg
    want = HR.ransac(step["matches"], valid, h, w, hc[0], hc[1], hc[2], int(round(1000 * hc[3])), int(round(1000 * hc[4])), seed=0, epoch=epoch, table=table,
                     cull=cull)
    if cull:
        valid, table = want["valid"], want["table"]
    else:
        assert _equal_tables(want["table"], table)      # (without cull the check touches neither the table nor, in a session, valid)
    wante = None
    if epi:
        wante = HR.epipolar_hold(step["matches"], valid, h, w, want["planar"] if hold else [0], threshold=ec[0], hypotheses_=ec[1], min_inliers=ec[2],
                                 permille=int(round(1000 * ec[3])), seed=0, epoch=epoch, table=table)
        valid, table = wante["valid"], wante["table"]
    return step, want, wante, valid, table


def _check_pair(res, seq, step, want, wante, valid, table, dense, what):
    _same(res.matches, step["matches"], what + ": matches")
    _same(res.tracks.ids, step["ids"], what + ": ids")
    for name in NAMES:
        _same(getattr(res.hom, name), want[name], f"{what}: hom.{name}")
    if dense:
        _same(res.hom.residual, HR.residual(_np(res.flow_up), want["H"], want["ok"]), what + ": hom.residual")
    else:
        assert res.hom.residual is None
    if wante is not None:
        for name in res.epi._fields:
            _same(getattr(res.epi, name), wante[name], f"{what}: epi.{name}")
    _same(res.valid, valid, what + ": valid")
    T._same_table(T._table_of(seq), table, what + ": seq.tracks (the table at the end of the step)")


def _fb_of(models, kind, fb):
    if not fb:
        return None
    from test_fb_check import _threshold      # (the threshold under which about half of the first pair's rows are consistent)
    return _threshold(models, kind)


def _session(models, kind, graph, fb, combo, cfg, max_corners=500, tracks=True):
    from focusflow_official_amd.frames import FBCheck, FrameSequence
    from focusflow_official_amd.geometry import Epipolar, Homography
    from focusflow_official_amd.keypoints import GoodFeatures
    _, epi, hold, cull, dense = COMBOS[combo]
    hc, ec = cfg
    det = GoodFeatures(max_corners=max_corners)
    seq = FrameSequence(models[kind], raft_iters=ITERS, graph=graph, keypoints=det, tracks=tracks, fb=None if fb is None else FBCheck(alpha=fb[0], beta=fb[1]),
                        epipolar=Epipolar(threshold=ec[0], hypotheses=ec[1], min_inliers=ec[2], min_ratio=ec[3]) if epi else None,
                        homography=Homography(threshold=hc[0], hypotheses=hc[1], min_inliers=hc[2], min_ratio=hc[3], planar_ratio=hc[4], cull=cull,
                                              hold_epipolar=hold, dense=dense))
    return seq, det


def _run_session(models, kind, graph, combo, cfg, max_corners=500):
    """One tracks session over the four frames, every pair held to the restatements.  Cached."""
    key = (kind, graph, combo, cfg)
    if key in _RUNS:
        return _RUNS[key]
    with_fb, epi, hold, cull, dense = COMBOS[combo]
    fb = _fb_of(models, kind, with_fb)
    seq, det = _session(models, kind, graph, fb, combo, cfg, max_corners)
    frames = _frames()
    assert seq.push(frames[0]) is None
    ref = R.empty_table(1, max_corners)
    pairs = []
    for t in range(FRAMES - 1):
        res = seq.push(frames[t + 1])
        what = f"{kind} graph={graph} {combo} {cfg} pair {t}"
        assert len(res) == 7 + bool(fb) + epi and res[-1] is res.hom and res._fields[-1] == "hom" and res.hom.status.shape == (1, max_corners)
        assert (res.epi is not None) == epi and (res.fb is not None) == bool(fb)
        step, want, wante, valid, table = _expect(ref, det, frames[t], res, H, W, fb, combo, cfg, epoch=t)      # (the first pair after the capture: epoch 0)
        _check_pair(res, seq, step, want, wante, valid, table, dense, what)
        assert int(seq._hom.epoch) == t + 1 and (not epi or int(seq._epi.epoch) == t + 1), what
        ref = table
        pairs.append({"status": want["status"], "ok": int(want["ok"][0]), "planar": int(want["planar"][0]), "epi_ok": None if wante is None else int(wante["ok"][0]),
                      "epi_status": None if wante is None else wante["status"], "table": T._table_of(seq), "valid_in": step["valid"], "valid": valid})
        print(what + f": candidates {int(want['candidates'][0])}, inliers {int(want['inliers'][0])}, ok {int(want['ok'][0])}, planar {int(want['planar'][0])}, "
              f"status 0 .. 4 {np.bincount(want['status'].ravel(), minlength=5).tolist()}"
              + ("" if wante is None else f"; epipolar: ok {int(wante['ok'][0])}, status {np.bincount(wante['status'].ravel(), minlength=5).tolist()}"))
    _RUNS[key] = {"pairs": pairs, "seq": seq, "table": T._table_of(seq), "det": det, "frames": frames}
    return _RUNS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [LOOSE, DEFAULT], ids=["loose", "defaults"])
@pytest.mark.parametrize("combo", ["alone", "fb", "epi_hold", "epi_free"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_equals_the_restatement(models, kind, graph, combo, cfg):
    pairs = _run_session(models, kind, graph, combo, cfg)["pairs"]      # (every pair is held to the restatements inside)
    if cfg != LOOSE:
        return
    _, epi, hold, _, _ = COMBOS[combo]
    # a verdict on every pair, planar with it (planar_ratio = 0); the check alone leaves valid as it found it (cull is False)
    assert all(p["ok"] == 1 and p["planar"] == 1 for p in pairs) and any((p["status"] == HR.OUTLIER).any() for p in pairs)
    if combo == "alone":
        assert all((p["valid"] == p["valid_in"]).all() for p in pairs)
    if not epi:
        return
    if hold:
        assert all(p["epi_ok"] == 0 and not (p["epi_status"] == E.OUTLIER).any() for p in pairs)      # every pair is held
    else:
        assert pairs[0]["epi_ok"] == 1 and (pairs[0]["epi_status"] == E.OUTLIER).any()                # the same pairs, not held: verdicts and culling


@pytest.mark.gpu
@pytest.mark.parametrize("combo", ["fb_epi_hold", "dense", "cull_epi_hold", "cull_epi_free_dense"])
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_graph_and_eager_end_with_identical_tables(models, kind, combo):
    """The capture's warm-up steps (which run the checks, cull, and spend epochs of both words) leave no trace; and the remaining
    combinations: all three checks in one session, the dense residual, culling by the homography."""
    g, e = _run_session(models, kind, True, combo, LOOSE), _run_session(models, kind, False, combo, LOOSE)
    T._same_table(g["table"], e["table"], f"{kind} {combo}: graph against eager after {FRAMES} frames")
    for t, (a, b) in enumerate(zip(g["pairs"], e["pairs"])):
        assert (a["status"] == b["status"]).all(), f"{kind} {combo}: pair {t}: status of graph and eager"
    if COMBOS[combo][3]:      # cull: the homography's outliers lose their slots
        first = g["pairs"][0]
        dead = first["status"][0] == HR.OUTLIER
        assert dead.any() and (first["table"]["ids"][0][dead] == -1).all() and (first["valid"][0][dead] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_graph_and_eager_agree_in_the_main_combinations(models, kind):
    for combo in ("alone", "fb", "epi_hold", "epi_free"):
        g, e = _run_session(models, kind, True, combo, LOOSE), _run_session(models, kind, False, combo, LOOSE)
        T._same_table(g["table"], e["table"], f"{kind} {combo}: graph against eager after {FRAMES} frames")


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_with_a_detector_only(models, kind, graph):
    """No table: the items are the restatements on the detector's rows; without cull the homography check leaves `valid` alone and
    the epipolar check behind it, not held, gates it."""
    from test_fb_check import _detector_rows
    seq, det = _session(models, kind, graph, None, "epi_free", LOOSE, tracks=None)
    frames = _frames()
    assert seq.push(frames[0]) is None and seq.tracks is None
    for t in range(2):
        res = seq.push(frames[t + 1])
        what = f"{kind} graph={graph} detector only, pair {t}"
        assert len(res) == 7 and res.tracks is None and res.fb is None and res[-1] is res.hom and res[-2] is res.epi and seq.tracks is None
        assert type(res).__name__ == "EpiHomFrameResult"
        points, count = det.points(frames[t].to(DEV).permute(0, 3, 1, 2).float().contiguous())
        m, valid = _detector_rows(_np(points), _np(count), _np(res.flow_up))
        want = HR.ransac(m, valid, H, W, 1.0, 128, 4, 0, 0, seed=0, epoch=t)
        wante = E.ransac(m, valid, H, W, 1.0, 128, 8, 0, seed=0, epoch=t)
        _same(res.matches, m, what + ": matches")
        for name in NAMES:
            _same(getattr(res.hom, name), want[name], f"{what}: hom.{name}")
        for name in res.epi._fields:
            _same(getattr(res.epi, name), wante[name], f"{what}: epi.{name}")
        _same(res.valid, wante["valid"], what + ": valid")
        assert want["ok"][0] == 1 and (want["status"] == HR.NO_ROW).sum() == 500 - int(count[0]) and (want["status"] == HR.OUTLIER).any()
        assert wante["ok"][0] == 1 and (wante["valid"] < valid).any()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_session_reset_and_a_new_shape(models, graph):
    """reset() empties the table and leaves both epoch words alone; a change of (B,H,W) drops the checks' buffers with the others:
    new ones, epoch 0, a residual of the new size."""
    combo = "cull_epi_free_dense"
    run = _run_session(models, "ffraft", graph, combo, LOOSE)      # (runs last on the cached session: it moves it on)
    seq, det, frames = run["seq"], run["det"], run["frames"]
    spent, epochs = int(seq.tracks.next_id[0]), int(seq._hom.epoch)
    assert epochs == FRAMES - 1 == int(seq._epi.epoch)
    seq.reset()
    assert int(seq._hom.epoch) == epochs == int(seq._epi.epoch) and not seq.tracks.live.any()
    assert seq.push(frames[0]) is None
    res = seq.push(frames[1])
    out = _expect(R.empty_table(1, 500, next_id=spent), det, frames[0], res, H, W, None, combo, LOOSE, epoch=epochs)
    _check_pair(res, seq, *out, True, f"graph={graph}: after reset()")
    assert int(seq._hom.epoch) == epochs + 1
    other = T._u8_frames(1, 128, 144, 2, T.SEED, T.SHIFT)
    assert seq.push(other[0]) is None and not seq.tracks.live.any() and int(seq._hom.epoch) == 0 and int(seq._epi.epoch) == 0
    res = seq.push(other[1])
    assert res.hom.status.shape == (1, 500) and res.flow_up.shape == (1, 2, 128, 144) and res.hom.residual.shape == (1, 128, 144)
    out = _expect(R.empty_table(1, 500), det, other[0], res, 128, 144, None, combo, LOOSE, epoch=0)
    _check_pair(res, seq, *out, True, f"graph={graph}: a new shape")
    assert int(seq._hom.epoch) == 1
