"""Key points on the device: csrc/keypoints.hip (ff_good_features), ops.good_features, keypoints.GoodFeatures, the detector
inside graph.GraphedForward / warm_start.FlowSequence and tools/generate_masks.py.

The yardstick is tests/keypoints_ref.py, the documented algorithm of cv.goodFeaturesToTrack(img, 500, 0.01, 10) restated
in exact integer and fp64 arithmetic; the device result must equal it bit for bit (mask, points, order, count).  OpenCV
itself is not available here: agreement with it is expected, not measured (tests/diagnostics/keypoints_vs_opencv.py)."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
import keypoints_ref as R

DEV = "cuda:0"
KINDS = ["noise", "blur1", "blur3", "flat", "tiled"]
SIZES = [(24, 32), (37, 53), (48, 64), (64, 96), (128, 160)]
GRAPH_VS_EAGER = 2e-4      # px: test_hip_parity.test_hipgraph_replay_matches_eager


@functools.lru_cache(maxsize=None)
def image(kind, h, w, seed=0):
    a = R.make_image(kind, h, w, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref(kind, h, w, seed=0, max_corners=500, quality_level=0.01, min_distance=10):
    """(mask, points, count, accepted without the cap, candidates) of a generated gray image, computed once."""
    return R.good_features_ref(image(kind, h, w, seed), max_corners, quality_level, min_distance, return_all=True)


def run(img_np, **kw):
    """(B,C,H,W) numpy -> (mask, points, count) numpy."""
    from focusflow_official_amd import ops
    out = ops.good_features(torch.from_numpy(np.array(img_np, np.float32)).to(DEV), return_points=True, **kw)
    return [t.cpu().numpy() for t in out]


def run1(img_np, **kw):
    """(C,H,W) numpy -> [mask (1,H,W), points, count] of the one sample."""
    return [t[0] for t in run(img_np[None], **kw)]


def assert_equal(got, want, what):
    mask, points, count = got
    assert int(count) == want[2], f"{what}: count {int(count)} != {want[2]}"
    assert np.array_equal(points, want[1]), f"{what}: points differ (first rows {points[:3].tolist()} vs {want[1][:3].tolist()})"
    assert mask.dtype == np.float32 and np.array_equal(mask, want[0]), f"{what}: mask differs at {int((mask != want[0]).sum())} pixels"


# ----------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    from focusflow_official_amd import _hip, build
    hdr = open(os.path.join(ROOT, "include", "focusflow_hip.h")).read()
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ("ff_good_features", "ff_good_features_ws"):
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), f"{name} is not declared in focusflow_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.EXPORTS
    assert "ff_good_features" in _hip._SIGS
    lib.ff_abi_version.restype = ctypes.c_int
    assert lib.ff_abi_version() == _hip.ABI_VERSION == 7 and "#define FF_ABI_VERSION 7" in hdr
    ws = _hip.load().ff_good_features_ws
    assert ws(1, 48, 64) > 0 and ws(8, 48, 64) == 8 * ws(1, 48, 64) and ws(1, 2, 64) == 0 and ws(1, 64, 2) == 0


def test_restatement_known_answers():
    img = np.zeros((1, 40, 56), np.float32)
    img[0, 10:30, 16:44] = 200
    mask, points, count = R.good_features_ref(img)
    assert count == 4 and points[:4].tolist() == [[16, 10], [43, 10], [16, 29], [43, 29]] and (points[4:] == -1).all()
    lam = R.min_eigenvalue(R.gray_u8(img))
    assert all(lam[y, x] == 1440000.0 for x, y in points[:4].tolist())
    assert mask.sum() == 4 * 255 and all(mask[0, y, x] == 255 for x, y in points[:4].tolist())
    ys, xs = np.mgrid[0:40, 0:56]
    for name, plane in (("vertical step", (xs >= 20) * 200), ("horizontal step", (ys >= 17) * 200), ("ramp", 4 * xs),
                        ("flat", image("flat", 40, 56)[0])):
        assert R.good_features_ref(plane.astype(np.float32)[None])[2] == 0, name
    img = np.zeros((1, 40, 56), np.float32)
    img[0, 20, 30] = 255
    _, points, count = R.good_features_ref(img)
    assert count == 1 and points[0].tolist() == [30, 20] and R.min_eigenvalue(R.gray_u8(img))[20, 30] == 780300.0
    img = np.zeros((1, 40, 56), np.float32)
    img[0, 1, 1] = 255
    _, points, count = R.good_features_ref(img)
    assert count == 1 and points[0].tolist() == [1, 1]
    # R,G,B -> gray: the 8-bit fixed-point luma, and rounding half to even with a clamp in front of it
    assert R.gray_u8(np.array([255, 255, 255], np.float32).reshape(3, 1, 1))[0, 0] == 255
    assert R.gray_u8(np.array([10, 200, 30], np.float32).reshape(3, 1, 1))[0, 0] == (4899 * 10 + 9617 * 200 + 1868 * 30 + 8192) >> 14
    assert R.gray_u8(np.array([[0.5, 1.5, 2.5, -3.0, 300.0, 254.5, 255.5]], np.float32)[None])[0].tolist() == [0, 2, 2, 0, 255, 254, 255]


def test_restatement_never_accepts_the_outer_ring():
    for kind in ("noise", "blur1", "tiled"):
        for h, w in SIZES[:4]:
            _, points, count, _, _ = ref(kind, h, w, min_distance=0)
            p = points[:count]
            assert count > 0 and p[:, 0].min() >= 1 and p[:, 0].max() <= w - 2 and p[:, 1].min() >= 1 and p[:, 1].max() <= h - 2


def test_restatement_walk_equals_parallel_rounds():
    lam = R.min_eigenvalue(R.gray_u8(image("noise", 128, 160)))
    order = R.candidates(lam, 0.01)
    for md, cap in ((10, 500), (3, 500), (10, 50), (0, 500)):
        walk = R.greedy(order, 128, 160, cap, md)
        rounds, n = R.greedy_parallel_rounds(order, lam, cap, md)
        print(f"min_distance {md} cap {cap}: {order.size} candidates, {walk.size} kept, {n} rounds")
        assert np.array_equal(walk, rounds)


def test_tiled_image_ties_exactly():
    """A repeated 16x16 tile: almost every candidate has a twin of exactly equal lambda, so the index rule decides."""
    lam = R.min_eigenvalue(R.gray_u8(image("tiled", 96, 128)))
    order = R.candidates(lam, 0.01)
    v = lam.reshape(-1)[order]
    ties = int((v[1:] == v[:-1]).sum())
    print(f"tiled 96x128: {order.size} candidates, {ties} neighbours in the order tie exactly")
    assert ties > order.size // 2
    assert (np.diff(order)[v[1:] == v[:-1]] > 0).all()


def test_cpu_tensor_raises():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    from focusflow_official_amd.keypoints import GoodFeatures
    with pytest.raises(FocusFlowHipError):
        ops.good_features(torch.zeros(1, 1, 24, 32))
    with pytest.raises(FocusFlowHipError):
        GoodFeatures()(torch.zeros(1, 3, 24, 32))


def test_flow_sequence_refuses_a_detector_for_plain_raft():
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.keypoints import GoodFeatures
    from focusflow_official_amd.warm_start import FlowSequence
    m = FF_RAFT_FUSION(use_fusion=None).eval()
    with pytest.raises(ValueError, match="plain RAFT"):
        FlowSequence(m, keypoints=GoodFeatures())
    assert FlowSequence(m).mask1 is None
    # the captured forward alone refuses as well, and so does a model that is not FF_RAFT_FUSION at all
    from focusflow_official_amd.graph import GraphedForward
    img = torch.zeros(1, 3, 128, 160)
    with pytest.raises(ValueError, match="reads no key-point mask"):
        GraphedForward(m, (img, img, None, None), keypoints=GoodFeatures())
    with pytest.raises(ValueError, match="Identity"):
        FlowSequence(torch.nn.Identity().eval(), keypoints=GoodFeatures())


def test_generate_masks_names_the_type_it_builds():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "generate_masks.py"), "in", "out", "--type", "orb"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "goodfeature" in p.stderr, (p.returncode, p.stderr)


def test_generated_mask_reads_back(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import generate_masks
    from focusflow_official_amd import frame_utils
    mask = np.zeros((37, 53), np.float32)
    mask[[1, 20, 35], [1, 30, 51]] = 255.0
    path = generate_masks.mask_path(str(tmp_path / "masks"), os.path.join("a", "b", "frame_0001.ppm"))
    assert path == str(tmp_path / "masks" / "a" / "b" / "frame_0001.png")
    generate_masks.write_mask(path, mask)
    back = np.asarray(frame_utils.read_gen(path))
    assert back.dtype == np.uint8 and back.shape == (37, 53) and np.array_equal(back, mask.astype(np.uint8))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_keypoint_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "keypoints.hip"))
    assert len(kernels) >= 5, kernels
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"keypoints.hip: kernels with scratch (bytes per lane): {spilled}"


# ----------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_equals_restatement(kind, size):
    h, w = size
    assert_equal(run1(image(kind, h, w)), ref(kind, h, w), f"{kind} {h}x{w} gray")
    rgb = np.concatenate([image(kind, h, w, seed) for seed in (1, 2, 3)])      # three different channels
    assert_equal(run1(rgb), R.good_features_ref(rgb), f"{kind} {h}x{w} R,G,B")


@pytest.mark.gpu
def test_equals_restatement_on_fractional_and_out_of_range_values():
    rng = np.random.default_rng(7)
    img = rng.integers(-40, 300, (3, 64, 96)).astype(np.float32) + rng.choice(np.array([0.0, 0.5, -0.5, 0.25, 0.75, 0.4999], np.float32), (3, 64, 96))
    assert (img < 0).any() and (img > 255).any() and (np.abs(img - np.trunc(img)) == 0.5).any()
    want = R.good_features_ref(img)
    assert want[2] > 10
    assert_equal(run1(img), want, "fractional R,G,B")
    assert_equal(run1(img[:1]), R.good_features_ref(img[:1]), "fractional gray")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,params", [("noise", dict(max_corners=50)), ("noise", dict(min_distance=3)), ("noise", dict(min_distance=0)),
                                         ("noise", dict(quality_level=0.3)), ("tiled", dict(max_corners=20)), ("noise", dict(min_distance=32)),
                                         ("noise", dict(min_distance=1, max_corners=2000)), ("noise256", dict(min_distance=0)),
                                         ("noise256", dict(min_distance=1, max_corners=3))],
                         ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_parameters(kind, params):
    h, w = {"noise": (128, 160), "tiled": (96, 128), "noise256": (256, 384)}[kind]
    kind = kind[:5]
    want = ref(kind, h, w, **params)
    if (h, w) == (256, 384):      # more accepted points than the kernel ranks through LDS (4096): its cut-off search runs
        assert want[3] > 4096
    print(f"{kind} {h}x{w} {params}: {want[4]} candidates, {want[3]} accepted, {want[2]} kept")
    if "max_corners" in params and params["max_corners"] < 100:
        assert want[3] > want[2] == params["max_corners"]      # the cap cuts
    if params.get("min_distance") == 3:
        assert want[3] > want[2] == 500
    assert_equal(run1(image(kind, h, w), **params), want, f"{kind} {params}")


@pytest.mark.gpu
def test_the_reference_call_at_larger_sizes():
    want = ref("noise", 256, 384)
    print(f"noise 256x384: {want[4]} candidates, {want[3]} accepted, {want[2]} kept")
    assert want[3] > want[2] == 500
    assert_equal(run1(image("noise", 256, 384)), want, "noise 256x384")
    want = ref("blur3", 384, 512)
    print(f"blur3 384x512: {want[4]} candidates, {want[3]} accepted, {want[2]} kept")
    assert_equal(run1(image("blur3", 384, 512)), want, "blur3 384x512")


@pytest.mark.gpu
def test_batch_views_and_out():
    from focusflow_official_amd import ops
    h, w = 48, 64
    kinds = ["noise", "blur1", "blur3", "flat", "tiled"]
    batch = np.stack([image(k, h, w) for k in kinds])
    want = [ref(k, h, w) for k in kinds]
    mask, points, count = run(batch)
    for i, k in enumerate(kinds):
        assert_equal([mask[i], points[i], count[i]], want[i], f"sample {i} ({k}) of a batch")
        assert (points[i, want[i][2]:] == -1).all()
    # the batch reversed, every sample a crop of a wider buffer
    wide = torch.full((len(kinds), 1, h + 3, w + 5), 7.0, device=DEV)
    wide[:, :, 1:-2, 2:-3] = torch.from_numpy(batch).to(DEV)
    view = wide.flip(0)[:, :, 1:-2, 2:-3]
    assert not view.is_contiguous()
    mask, points, count = [t.cpu().numpy() for t in ops.good_features(view, return_points=True)]
    for i, k in enumerate(reversed(kinds)):
        assert_equal([mask[i], points[i], count[i]], want[len(kinds) - 1 - i], f"sample {i} ({k}) of a reversed, cropped view")
    # out=
    dev = torch.from_numpy(batch).to(DEV)
    out = torch.full((len(kinds), 1, h, w), -3.0, device=DEV)
    assert ops.good_features(dev, out=out) is out
    assert np.array_equal(out.cpu().numpy(), np.stack([x[0] for x in want]))
    from focusflow_official_amd.keypoints import GoodFeatures
    det = GoodFeatures()
    assert torch.equal(det(dev), out)
    p, c = det.points(dev)
    assert np.array_equal(p.cpu().numpy(), points[::-1]) and np.array_equal(c.cpu().numpy(), count[::-1])


@pytest.mark.gpu
def test_generate_masks_end_to_end(tmp_path):
    """tools/generate_masks.py's own path: the walk, PIL reading (R,G,B order, gray files), batches of equal-sized images,
    detection and the PNGs, against the restatement of the same pixels."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import generate_masks
    from focusflow_official_amd import frame_utils
    src, dst = tmp_path / "images", tmp_path / "masks"
    want = {}
    for rel, kind, (h, w), rgb in (("a/f0.png", "noise", (48, 64), True), ("a/f1.png", "blur1", (48, 64), True), ("a/f2.png", "tiled", (48, 64), True),
                                   ("b/c/g0.ppm", "noise", (37, 53), True), ("b/g1.png", "blur1", (37, 53), False)):
        a = np.concatenate([image(kind, h, w, seed) for seed in ((4, 5, 6) if rgb else (4,))]).astype(np.uint8)
        os.makedirs(src / os.path.dirname(rel), exist_ok=True)
        Image.fromarray(a.transpose(1, 2, 0) if rgb else a[0]).save(src / rel)
        want[os.path.splitext(rel)[0] + ".png"] = R.good_features_ref(a.astype(np.float32))[0][0]
    generate_masks.main([str(src), str(dst), "--batch", "2"])
    assert sorted(generate_masks.find_images(str(dst))) == sorted(want)
    for rel, mask in want.items():
        back = np.asarray(frame_utils.read_gen(str(dst / rel)))
        assert mask.any() and back.dtype == np.uint8 and np.array_equal(back, mask.astype(np.uint8)), rel


@pytest.mark.gpu
def test_capture_and_replay():
    from focusflow_official_amd import ops
    h, w = 64, 96
    static = torch.from_numpy(image("noise", h, w)[None].copy()).to(DEV)
    mask = torch.empty(1, 1, h, w, device=DEV)
    ops.good_features(static, out=mask)      # (loads the kernels before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, points, count = ops.good_features(static, out=mask, return_points=True)
    for kind in ("noise", "noise", "noise", "blur1"):
        static.copy_(torch.from_numpy(image(kind, h, w)[None].copy()))
        mask.fill_(123.0)
        points.fill_(77)
        count.fill_(-5)
        graph.replay()
        assert_equal([mask[0].cpu().numpy(), points[0].cpu().numpy(), count[0].cpu().numpy()], ref(kind, h, w), f"replay on {kind}")


@pytest.mark.gpu
def test_refusals_name_the_argument():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    ok = torch.zeros(1, 1, 24, 32, device=DEV)
    for img, kw, word in ((torch.zeros(1, 2, 24, 32, device=DEV), {}, "channels"), (torch.zeros(1, 1, 2, 32, device=DEV), {}, "H = 2"),
                          (ok, dict(max_corners=0), "max_corners"), (ok, dict(quality_level=0.0), "quality_level"),
                          (ok, dict(quality_level=1.5), "quality_level"), (ok, dict(min_distance=33), "min_distance"),
                          (ok, dict(min_distance=-1), "min_distance")):
        with pytest.raises(FocusFlowHipError, match=word):
            ops.good_features(img, **kw)
    assert not ops.good_features(ok).any()


# ----------------------------------------------------------------------------
# the detector inside the graph and the session
# ----------------------------------------------------------------------------
def _ffraft(sd):
    from focusflow_official_amd import FF_RAFT_FUSION
    cfg = Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def _frames(b, h, w, frames=4, seed=0, shift=(3, -5)):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(b, 3, h // 4 + 2, w // 4 + 2, generator=g), size=(h, w), mode="bilinear", align_corners=False) * 255
    out = []
    for k in range(frames):
        img = torch.roll(base, shifts=(shift[0] * k, shift[1] * k), dims=(2, 3))
        if k:
            img = img + torch.randn(b, 3, h, w, generator=g) * 2
        out.append(img.clamp(0, 255).contiguous().to(DEV))
    return out


def _close(a, b, what):
    for x, y, n in zip(a, b, ("flow_low", "flow_up")):
        err = float((x.double() - y.double()).abs().max())
        print(f"{what}: {n} max |diff| {err:.3e} (bound {GRAPH_VS_EAGER:g})")
        assert err <= GRAPH_VS_EAGER, f"{what}: {n} max |diff| {err:.3e} > {GRAPH_VS_EAGER:g}"


@pytest.mark.gpu
def test_session_detects_inside_the_graph(det_sd):
    from focusflow_official_amd.graph import GraphedForward
    from focusflow_official_amd.keypoints import GoodFeatures
    from focusflow_official_amd.warm_start import FlowSequence
    m = _ffraft(det_sd)
    det = GoodFeatures()
    imgs = _frames(1, 128, 160, seed=51)
    detecting = FlowSequence(m, raft_iters=4, keypoints=det)
    supplied = FlowSequence(m, raft_iters=4)
    eager_detecting = FlowSequence(m, raft_iters=4, graph=False, keypoints=det)
    eager_supplied = FlowSequence(m, raft_iters=4, graph=False)
    blind = FlowSequence(m, raft_iters=4, warm_start=False)
    assert detecting.mask1 is None
    for t in range(3):
        i1, i2 = imgs[t], imgs[t + 1]
        mask = det(i1)
        want_mask = R.good_features_ref(i1[0].cpu().numpy())
        assert want_mask[2] > 20 and np.array_equal(mask[0].cpu().numpy(), want_mask[0])
        got = [x.clone() for x in detecting(i1, i2)]
        assert torch.equal(detecting.mask1, mask), f"frame {t}: seq.mask1 is the detector's mask of image1"
        _close(got, supplied(i1, i2, mask), f"frame {t}: in-graph detector vs the same mask supplied")
        got_eager = [x.clone() for x in eager_detecting(i1, i2)]
        assert torch.equal(eager_detecting.mask1, mask)
        _close(got_eager, eager_supplied(i1, i2, mask), f"frame {t}: graph=False, detector vs the same mask supplied")
        if t == 0:      # (cold on both sides) an all-zero mask gives another flow: the mask reaches the encoder
            zero = blind(i1, i2, torch.zeros_like(mask))
            assert float((zero[1] - got[1]).abs().max()) > 10 * GRAPH_VS_EAGER
        with pytest.raises(ValueError):
            detecting(i1, i2, mask)
    # a new shape: recaptured, still detecting
    other = _frames(1, 128, 192, frames=2, seed=52)
    got = [x.clone() for x in detecting(*other)]
    mask = det(other[0])
    assert detecting.mask1.shape == (1, 1, 128, 192) and torch.equal(detecting.mask1, mask) and mask.any()
    _close(got, FlowSequence(m, raft_iters=4)(*other, mask), "128x192 after a shape change")
    # GraphedForward itself: None for mask1, a tensor is refused
    gf = GraphedForward(m, (imgs[0], imgs[1], None, None), raft_iters=4, keypoints=det)
    gf(imgs[1], imgs[2], None, None)
    assert torch.equal(gf.mask1, det(imgs[1]))
    with pytest.raises(ValueError):
        gf(imgs[1], imgs[2], det(imgs[1]))
