"""Video sessions at the application's boundary: csrc/frame_io.hip (ff_frame_ingest, ff_pad_replicate, ff_keypoint_matches),
their ops wrappers and frames.FrameSequence (uint8 frames in, key-point matches out).

The conversions are exact (uint8 -> fp32, copies, one fp32 add), so the kernels are held to the torch restatements of
tests/frame_io_ref.py with torch.equal.  The session is held to the route a caller has without it - convert, InputPadder.pad,
warm_start.FlowSequence with mask1 = pad(det(unpadded image1)), det.points, gather - within GRAPH_VS_EAGER, the project's bound for
a replay against eager issue (test_warm_start.py), and bit for bit wherever no convolution lies between the two."""
import ctypes
import functools
import os
import re
import shutil
import sys
from argparse import Namespace

import pytest
import torch

from conftest import ROOT, golden_spec
import frame_io_ref as R

DEV = "cuda:0"
GRAPH_VS_EAGER = 2e-4      # px: test_warm_start.py / test_hip_parity.test_hipgraph_replay_matches_eager
ENTRY_POINTS = ("ff_frame_ingest", "ff_pad_replicate", "ff_keypoint_matches")


# ----------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    """Entry points alone do not move FF_ABI_VERSION (the header's history: the warm start and the detector are both
    '7 (unchanged)', and test_abi_and_host / test_warm_start / test_keypoints pin 7): no struct or argument list changed.  What is
    checked here is that header, library and bindings agree on the version and that the three entry points are in all of them."""
    from focusflow_official_amd import _hip, build
    hdr = open(os.path.join(ROOT, "include", "focusflow_hip.h")).read()
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), f"{name} is not declared in focusflow_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.EXPORTS and name in _hip._SIGS
        assert name in hdr.split("#define FF_ABI_VERSION")[0], f"{name} is missing from the header's version history"
    lib.ff_abi_version.restype = ctypes.c_int
    ver = int(re.search(r"#define FF_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.ff_abi_version() == ver == _hip.ABI_VERSION
    # the argument lists of the bindings are those of the header
    for name in ENTRY_POINTS:
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_hip._SIGS[name]), f"{name}: {len(_hip._SIGS[name])} bound arguments, the header declares {len(decl.split(','))}"


def test_wrappers_raise_on_cpu_tensors():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    with pytest.raises(FocusFlowHipError, match="frame"):
        ops.frame_ingest(torch.zeros(1, 5, 7, 3, dtype=torch.uint8))
    with pytest.raises(FocusFlowHipError, match="mask"):
        ops.pad_replicate(torch.zeros(1, 1, 5, 7))
    with pytest.raises(FocusFlowHipError, match="points"):
        ops.keypoint_matches(torch.zeros(1, 4, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 8, 8), 0, 1, 5, 7)


def test_padding_offsets_equal_input_padder():
    from focusflow_official_amd import ops
    from focusflow_official_amd.utils import InputPadder
    for mode in ("sintel", "kitti"):
        for h in range(1, 18):
            for w in range(1, 18):
                l, r, t, b = InputPadder((h, w), mode)._pad
                want = (l, t, h + t + b, w + l + r)
                assert R.pad_offsets(h, w, mode) == want, (mode, h, w)
                assert ops.pad_offsets(h, w, mode) == want, (mode, h, w)
                assert want[2] % 8 == 0 and want[3] % 8 == 0


def test_restatement_of_matches_known_answers():
    points = torch.tensor([[[0, 0], [4, 2], [6, 4], [-1, -1]]], dtype=torch.int32)
    flow = torch.zeros(1, 2, 8, 8)
    flow[0, 0, 1 + 2, 4] = 2.5      # u at (4, 2): top = 1, left = 0
    flow[0, 1, 1 + 2, 4] = -3.0     # v: the target leaves the frame
    flow[0, 0, 1 + 4, 6] = 9.0      # (beyond the count: never read)
    m, valid = R.matches(points, torch.tensor([2], dtype=torch.int32), flow, 0, 1, 5, 7)
    assert m[0].tolist() == [[0, 0, 0, 0], [4, 2, 6.5, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]] and valid[0].tolist() == [1, 0, 0, 0]
    m, valid = R.matches(points, torch.tensor([0], dtype=torch.int32), flow, 0, 1, 5, 7)
    assert (m == -1).all() and not valid.any()


def test_session_refuses_without_a_gpu():
    """The refusals that need no device: they are decided before anything is enqueued."""
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    from focusflow_official_amd.pwcnet import FF_PWCNET
    plain = FF_RAFT_FUSION(use_fusion=None)
    with pytest.raises(ValueError, match="model"):
        FrameSequence(plain.train())
    seq = FrameSequence(plain.eval(), keypoints=GoodFeatures())
    with pytest.raises(ValueError, match="frame"):
        seq.push(torch.zeros(1, 16, 24, 3))
    with pytest.raises(ValueError, match="frame"):
        seq.push(torch.zeros(1, 16, 24, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):
        seq.push(torch.zeros(1, 16, 24, 3, dtype=torch.uint8), mask=torch.zeros(1, 1, 16, 24))
    cfg = Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION="parallel", FUSION_TYPE="1x1conv"))
    with pytest.raises(ValueError, match="GraphedForward"):
        FrameSequence(FF_PWCNET(cfg).eval())


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_frame_io_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "frame_io.hip"))
    assert len(kernels) >= 3, kernels      # the padding kernel for uint8 and for fp32, and the matches
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"frame_io.hip: kernels with scratch (bytes per lane): {spilled}"


# ----------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------
def _bytes(shape, seed):
    """Random uint8 that certainly holds 0 and 255."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    flat = x.view(-1)
    flat[0], flat[-1], flat[flat.numel() // 2] = 0, 255, 255
    flat[1] = 0
    return x


def _torch_route(src, layout, order, mode):
    from focusflow_official_amd.utils import InputPadder
    x = R.as_float_rgb_nchw(src, layout, order)
    return InputPadder(x.shape, mode).pad(x)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sintel", "kitti"])
@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("size", [(5, 7), (37, 53), (40, 64), (125, 157)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ingest_is_exact(size, b, layout, order, mode):
    from focusflow_official_amd import ops
    h, w = size
    src = _bytes((b, h, w, 3) if layout == "hwc" else (b, 3, h, w), seed=h * 1000 + w + b).to(DEV)
    assert int(src.min()) == 0 and int(src.max()) == 255
    want = _torch_route(src, layout, order, mode)
    got = ops.frame_ingest(src, layout, order, mode)
    assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == want.shape and got.shape[2] % 8 == 0 and got.shape[3] % 8 == 0
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} values differ"
    assert torch.equal(got, R.ingest(src, layout, order, mode))
    out = torch.full_like(want, -7.0)
    assert ops.frame_ingest(src, layout, order, mode, out=out) is out and torch.equal(out, want)
    if b == 1:      # a single frame without the batch dimension
        assert torch.equal(ops.frame_ingest(src[0], layout, order, mode), want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sintel", "kitti"])
def test_ingest_reads_views(mode):
    from focusflow_official_amd import ops
    big = _bytes((2, 60, 90, 3), seed=5).to(DEV)
    crop = big[:, 11:48, 20:73]                   # 37 x 53 of a larger frame: row stride 270 > 3 W
    assert not crop.is_contiguous() and crop.stride(1) > 3 * crop.shape[2]
    assert torch.equal(ops.frame_ingest(crop, "hwc", "rgb", mode), _torch_route(crop, "hwc", "rgb", mode))
    assert torch.equal(ops.frame_ingest(crop, "hwc", "bgr", mode), _torch_route(crop, "hwc", "bgr", mode))
    rgba = _bytes((2, 37, 53, 4), seed=6).to(DEV)
    view = rgba[..., :3]
    assert view.stride(2) == 4
    assert torch.equal(ops.frame_ingest(view, "hwc", "rgb", mode), _torch_route(view, "hwc", "rgb", mode))
    planar = _bytes((2, 3, 60, 90), seed=7).to(DEV)[:, :, 11:48, 20:73]
    assert torch.equal(ops.frame_ingest(planar, "chw", "bgr", mode), _torch_route(planar, "chw", "bgr", mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sintel", "kitti"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["uint8", "fp32"])
@pytest.mark.parametrize("size", [(37, 53), (40, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pad_replicate_is_exact(size, dtype, mode):
    import torch.nn.functional as F
    from focusflow_official_amd import ops
    from focusflow_official_amd.utils import InputPadder
    h, w = size
    m = _bytes((2, 1, h, w), seed=h + w).to(DEV)
    if dtype == torch.float32:
        m = m.float() * 0.37 - 11.0      # (values that are no integers: fp32 is copied, not converted)
    pad = InputPadder((h, w), mode)._pad
    want = F.pad(m.float(), pad, mode="replicate")
    got = ops.pad_replicate(m, mode)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(ops.pad_replicate(m[:, 0], mode), want)      # (B,H,W)
    assert torch.equal(got, R.pad_mask(m, mode))
    wide = torch.zeros((2, 1, h + 4, w + 6), dtype=dtype, device=DEV)
    wide[:, :, 1:1 + h, 5:5 + w] = m
    view = wide[:, :, 1:1 + h, 5:5 + w]
    out = torch.full_like(want, 3.0)
    assert not view.is_contiguous() and ops.pad_replicate(view, mode, out=out) is out and torch.equal(out, want)


def _match_case(n, counts, seed):
    """B = 2, a 37 x 53 frame inside a 40 x 56 field (left 1, top 1): random points, the four borders and corners among them,
    rows of -1 from the count on, a flow that pushes part of the targets out of the frame."""
    h, w, hp, wp, left, top = 37, 53, 40, 56, 1, 1
    assert R.pad_offsets(h, w) == (left, top, hp, wp)
    g = torch.Generator().manual_seed(seed)
    points = torch.stack([torch.randint(0, w, (2, n), generator=g), torch.randint(0, h, (2, n), generator=g)], dim=-1).to(torch.int32)
    border = torch.tensor([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [0, 17], [w - 1, 20], [25, 0], [30, h - 1]], dtype=torch.int32)
    k = min(n, border.shape[0])
    points[0, :k] = border[:k]
    if n == 1:
        points[1, 0] = border[3]
    count = torch.tensor(counts, dtype=torch.int32)
    for bi in range(2):
        points[bi, counts[bi]:] = -1
    flow = torch.randn(2, 2, hp, wp, generator=g) * 12
    flow[0, :, top, left] = torch.tensor([-0.0, 0.0])                        # the corner stays on the corner: valid
    if n > 1:
        flow[0, :, top, left + w - 1] = torch.tensor([0.25, 0.0])            # a quarter pixel beyond the right border: not valid
    return points.to(DEV), count.to(DEV), flow.to(DEV), (left, top, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("n,counts", [(500, (500, 3)), (500, (0, 500)), (500, (3, 0)), (1, (1, 0)), (1, (0, 1))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_matches_are_exact(n, counts):
    from focusflow_official_amd import ops
    points, count, flow, (left, top, h, w) = _match_case(n, counts, seed=n + counts[0])
    want_m, want_v = R.matches(points, count, flow, left, top, h, w)
    got_m, got_v = ops.keypoint_matches(points, count, flow, left, top, h, w)
    assert got_m.dtype == torch.float32 and got_m.shape == (2, n, 4) and got_v.dtype == torch.uint8 and got_v.shape == (2, n)
    assert torch.equal(got_m, want_m), f"{int((got_m != want_m).sum())} fields differ"
    assert torch.equal(got_v, want_v), f"{int((got_v != want_v).sum())} validity bytes differ"
    for bi, c in enumerate(counts):
        assert (got_m[bi, c:] == -1).all() and not got_v[bi, c:].any()
        assert torch.equal(got_m[bi, :c, :2], points[bi, :c].float())
    if n == 500 and max(counts) == 500:
        bi = counts.index(500)
        assert 0 < int(got_v[bi].sum()) < 500      # the flow keeps some targets in the frame and pushes some out
    if n == 500 and counts[0] >= 3:
        assert got_v[0, 0] == 1 and got_m[0, 0].tolist() == [0, 0, 0, 0]
        assert got_v[0, 1] == 0 and got_m[0, 1].tolist() == [w - 1, 0, w - 0.75, 0]
    # a strided flow_up: channels and rows of a larger tensor
    big = torch.zeros(2, 3, 44, 70, device=DEV)
    view = big[:, 1:, 2:42, 9:65]
    view.copy_(flow)
    assert not view.is_contiguous()
    out_m, out_v = torch.full((2, n, 4), 5.0, device=DEV), torch.full((2, n), 9, dtype=torch.uint8, device=DEV)
    r = ops.keypoint_matches(points, count, view, left, top, h, w, out=out_m, valid=out_v)
    assert r[0] is out_m and r[1] is out_v and torch.equal(out_m, want_m) and torch.equal(out_v, want_v)


@pytest.mark.gpu
def test_wrappers_refuse_by_name():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    src = torch.zeros(1, 5, 7, 3, dtype=torch.uint8, device=DEV)
    points, count = torch.zeros(1, 4, 2, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    flow = torch.zeros(1, 2, 8, 8, device=DEV)
    for fn, word in ((lambda: ops.frame_ingest(src.float()), "frame"),
                     (lambda: ops.frame_ingest(torch.zeros(1, 5, 7, 4, dtype=torch.uint8, device=DEV)), "channels"),
                     (lambda: ops.frame_ingest(src, layout="nhwc"), "layout"),
                     (lambda: ops.frame_ingest(src, order="gbr"), "order"),
                     (lambda: ops.frame_ingest(src, out=torch.zeros(1, 3, 8, 8, dtype=torch.float64, device=DEV)), "out"),
                     (lambda: ops.frame_ingest(src, out=torch.zeros(1, 3, 8, 16, device=DEV)), "out"),
                     (lambda: ops.pad_replicate(torch.zeros(1, 1, 5, 7, dtype=torch.int32, device=DEV)), "mask"),
                     (lambda: ops.pad_replicate(torch.zeros(1, 2, 5, 7, device=DEV)), "mask"),
                     (lambda: ops.pad_replicate(torch.zeros(1, 1, 5, 7, device=DEV), out=torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=DEV)), "out"),
                     (lambda: ops.keypoint_matches(points.float(), count, flow, 0, 1, 5, 7), "points"),
                     (lambda: ops.keypoint_matches(points, count.long(), flow, 0, 1, 5, 7), "count"),
                     (lambda: ops.keypoint_matches(points, count, flow[:, :1], 0, 1, 5, 7), "flow_up"),
                     (lambda: ops.keypoint_matches(points, count, flow, 0, 1, 5, 7, valid=torch.zeros(1, 4, device=DEV)), "valid"),
                     (lambda: ops.keypoint_matches(points, count, flow, 0, 1, 5, 7, out=torch.zeros(1, 4, 4, dtype=torch.float64, device=DEV)), "out"),
                     (lambda: ops.keypoint_matches(points, count, flow, 2, 1, 5, 7), "left"),      # 2 + 7 > 8: refused by the library
                     (lambda: ops.keypoint_matches(points, count, flow, 0, 4, 5, 7), "top")):
        with pytest.raises(FocusFlowHipError, match=word):
            fn()
    m, v = ops.keypoint_matches(points, count, flow, 0, 1, 5, 7)
    assert (m == -1).all() and not v.any()


# ----------------------------------------------------------------------------
# the session
# ----------------------------------------------------------------------------
def _cfg():
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))


@pytest.fixture(scope="module")
def ffraft(det_sd):
    """As tests/test_keypoints.py::_ffraft builds it."""
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg())
    m.load_state_dict(det_sd, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def plain_model():
    from focusflow_official_amd import FF_RAFT_FUSION
    from oracle.weights import det_tensor
    m = FF_RAFT_FUSION(use_fusion=None)
    m.load_state_dict({k: det_tensor(k, s) for k, s, _ in golden_spec("state_dict_spec_plain")}, strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _u8_frames(b, h, w, frames=4, seed=0, shift=(3, -5)):
    """tests/test_keypoints.py::_frames, rounded to uint8 and laid out as a decoder delivers them: (B,H,W,3), on the host."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(b, 3, h // 4 + 2, w // 4 + 2, generator=g), size=(h, w), mode="bilinear", align_corners=False) * 255
    out = []
    for k in range(frames):
        img = torch.roll(base, shifts=(shift[0] * k, shift[1] * k), dims=(2, 3))
        if k:
            img = img + torch.randn(b, 3, h, w, generator=g) * 2
        out.append(img.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    return tuple(out)


class _TodaysRoute:
    """What a caller does without the session: upload, convert, InputPadder.pad, FlowSequence, det.points, gather, unpad."""

    def __init__(self, model, det, mode, reads_mask=True, **kw):
        from focusflow_official_amd.warm_start import FlowSequence
        self.seq, self.det, self.mode, self.reads_mask = FlowSequence(model, raft_iters=4, **kw), det, mode, reads_mask

    def __call__(self, f1, f2, mask=None):
        from focusflow_official_amd.utils import InputPadder
        i1, i2 = R.as_float_rgb_nchw(f1.to(DEV)), R.as_float_rgb_nchw(f2.to(DEV))
        padder = InputPadder(i1.shape, self.mode)
        p1, p2 = padder.pad(i1, i2)
        mask1 = None
        if self.reads_mask:
            mask1 = padder.pad(self.det(i1) if mask is None else mask.to(DEV).float().reshape(i1.shape[0], 1, *i1.shape[2:]))[0]
        flow_low, flow_up = self.seq(p1, p2, mask1)
        points, count = self.det.points(i1) if self.det is not None else (None, None)
        return flow_low.clone(), padder.unpad(flow_up).clone(), mask1, points, count


def _close(got, want, what):
    for x, y, n in zip(got, want, ("flow_low", "flow_up")):
        assert x.shape == y.shape, f"{what}: {n} {tuple(x.shape)} vs {tuple(y.shape)}"
        err = float((x.double() - y.double()).abs().max())
        print(f"{what}: {n} max |diff| {err:.3e} (bound {GRAPH_VS_EAGER:g})")
        assert err <= GRAPH_VS_EAGER, f"{what}: {n} max |diff| {err:.3e} > {GRAPH_VS_EAGER:g}"


def _check_pair(res, seq, want, what, reads_mask=True, min_points=20):
    """One pushed pair against today's route (flow_low, unpadded flow_up, mask1, points, count)."""
    flow_low, flow_up, mask1, points, count = want
    _close((res.flow_low, res.flow_up), (flow_low, flow_up), what)
    if reads_mask:
        assert torch.equal(seq.mask1, mask1), f"{what}: seq.mask1 is pad(det(unpadded image1))"
    else:
        assert seq.mask1 is None
    if points is None:
        assert res.matches is None and res.valid is None and res.count is None
        return
    b, _, h, w = flow_up.shape
    assert int(count.min()) > min_points, f"{what}: the detector found {count.tolist()} points: too few to test with"
    assert torch.equal(res.count, count), f"{what}: count {res.count.tolist()} vs {count.tolist()}"
    assert res.matches.shape == (b, points.shape[1], 4) and torch.equal(res.matches[..., :2], points.float()), f"{what}: the points of the matches"
    # the last two fields and the validity: the gather from the session's OWN flow_up (already unpadded: left = top = 0)
    own_m, own_v = R.matches(points, count, res.flow_up, 0, 0, h, w)
    assert torch.equal(res.matches, own_m), f"{what}: matches vs the gather from res.flow_up"
    assert torch.equal(res.valid, own_v), f"{what}: valid vs the gather from res.flow_up"
    for bi in range(b):
        c = int(count[bi])
        assert (res.matches[bi, c:] == -1).all() and not res.valid[bi, c:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_session_equals_todays_route(ffraft, graph):
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    det = GoodFeatures()
    frames = _u8_frames(1, 125, 157, seed=51)
    seq = FrameSequence(ffraft, raft_iters=4, graph=graph, keypoints=det)
    today = _TodaysRoute(ffraft, det, "sintel")
    assert seq.mask1 is None and seq.push(frames[0]) is None and seq.mask1 is None
    for t in range(3):
        res = seq.push(frames[t + 1])
        assert res.flow_up.shape == (1, 2, 125, 157) and res.flow_low.shape == (1, 2, 16, 20)
        _check_pair(res, seq, today(frames[t], frames[t + 1]), f"125x157 pair {t} (graph={graph})")
        assert float(res.flow_up.abs().max()) > 1.0 and 0 < int(res.valid.sum()) <= int(res.count.sum())      # a real flow, real matches
        if t == 1:
            warm = res.flow_up.clone()
    # a sequence boundary: None again, then a cold pair
    seq.reset()
    assert seq.push(frames[1]) is None
    res = seq.push(frames[2])
    _check_pair(res, seq, _TodaysRoute(ffraft, det, "sintel", warm_start=False)(frames[1], frames[2]), f"after reset() (graph={graph})")
    assert float((res.flow_up - warm).abs().max()) > 10 * GRAPH_VS_EAGER      # the same pair, warm: another flow
    # a new shape: a new sequence, captured again
    other = _u8_frames(1, 128, 192, frames=3, seed=52)
    today = _TodaysRoute(ffraft, det, "sintel")
    assert seq.push(other[0]) is None
    for t in range(2):
        res = seq.push(other[t + 1])
        assert res.flow_up.shape == (1, 2, 128, 192)
        _check_pair(res, seq, today(other[t], other[t + 1]), f"128x192 pair {t} after a shape change (graph={graph})")


@pytest.mark.gpu
def test_session_kitti_padding_and_frame_sources(ffraft):
    """128 x 160 needs no padding at all; 125 x 157 in the KITTI layout pads the bottom only.  Frames come as numpy, pinned
    host and device tensors, B = 2."""
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    det = GoodFeatures()
    for (h, w), seed in (((128, 160), 53), ((125, 157), 54)):
        frames = _u8_frames(2, h, w, frames=3, seed=seed)
        seq = FrameSequence(ffraft, raft_iters=4, keypoints=det, pad_mode="kitti")
        today = _TodaysRoute(ffraft, det, "kitti")
        assert seq.push(frames[0].numpy()) is None
        for t, src in enumerate((frames[1].pin_memory(), frames[2].to(DEV))):
            res = seq.push(src)
            assert res.flow_up.shape == (2, 2, h, w)
            _check_pair(res, seq, today(frames[t], frames[t + 1]), f"kitti {h}x{w} pair {t}")


@pytest.mark.gpu
def test_session_layout_and_order(ffraft):
    """(3,H,W) planar B,G,R frames are the same H,W,3 R,G,B frames: the same mask and points bit for bit, the same flow
    within the bound between two captures."""
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    frames = _u8_frames(1, 125, 157, frames=3, seed=51)
    a = FrameSequence(ffraft, raft_iters=4, keypoints=GoodFeatures())
    b = FrameSequence(ffraft, raft_iters=4, keypoints=GoodFeatures(), layout="chw", order="bgr")
    for f in frames:
        ra, rb = a.push(f), b.push(f[0].permute(2, 0, 1).flip(0).contiguous())
        if ra is not None:
            _close((ra.flow_low, ra.flow_up), (rb.flow_low, rb.flow_up), "chw / bgr vs hwc / rgb")
            assert torch.equal(a.mask1, b.mask1) and torch.equal(ra.count, rb.count) and torch.equal(ra.matches[..., :2], rb.matches[..., :2])


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_session_plain_raft_with_a_detector(plain_model, graph):
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    det = GoodFeatures()
    frames = _u8_frames(1, 125, 157, seed=51)
    seq = FrameSequence(plain_model, raft_iters=4, graph=graph, keypoints=det)
    today = _TodaysRoute(plain_model, det, "sintel", reads_mask=False)
    assert seq.push(frames[0]) is None
    for t in range(3):
        _check_pair(seq.push(frames[t + 1]), seq, today(frames[t], frames[t + 1]), f"plain RAFT pair {t} (graph={graph})", reads_mask=False)
    bare = FrameSequence(plain_model, raft_iters=4, graph=graph)      # no detector either: flow only
    assert bare.push(frames[0]) is None
    res = bare.push(frames[1])
    assert res.matches is None and res.flow_up.shape == (1, 2, 125, 157)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["uint8", "fp32"])
def test_session_with_supplied_masks(ffraft, dtype):
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    det = GoodFeatures()
    frames = _u8_frames(1, 125, 157, seed=51)
    masks = [det(R.as_float_rgb_nchw(f.to(DEV))).to(dtype) for f in frames]      # (B,1,H,W), unpadded, 0 / 255
    assert all(int((m > 0).sum()) > 20 for m in masks)
    seq = FrameSequence(ffraft, raft_iters=4)
    today = _TodaysRoute(ffraft, None, "sintel")
    assert seq.push(frames[0], mask=masks[0]) is None
    for t in range(3):
        m = masks[t + 1] if t != 1 else masks[t + 1][:, 0].cpu()      # (B,H,W) on the host is as good
        res = seq.push(frames[t + 1], mask=m)
        _check_pair(res, seq, today(frames[t], frames[t + 1], mask=masks[t]), f"supplied {dtype} masks, pair {t}")
        assert res.matches is None and res.valid is None and res.count is None
    with pytest.raises(ValueError, match="mask"):
        seq.push(frames[0])
    with pytest.raises(ValueError, match="mask"):
        seq.push(frames[0], mask=masks[0][:, :, :100])


@pytest.mark.gpu
def test_results_are_static_buffers_until_the_next_push(ffraft):
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    frames = _u8_frames(1, 125, 157, seed=51)
    seq = FrameSequence(ffraft, raft_iters=4, keypoints=GoodFeatures())
    seq.push(frames[0])
    first = seq.push(frames[1])
    kept = [t.clone() for t in first] + [seq.mask1.clone()]
    torch.cuda.synchronize()
    again = [t.clone() for t in first] + [seq.mask1.clone()]
    assert all(torch.equal(x, y) for x, y in zip(kept, again))      # nothing moves while nobody pushes
    second = seq.push(frames[2])
    now = [t.clone() for t in second] + [seq.mask1.clone()]
    assert all(torch.equal(x, y) for x, y in zip(kept, again))      # the clones are the caller's
    for name, x, y in zip(("flow_low", "flow_up", "matches", "valid", "count", "mask1"), kept, now):
        if name in ("valid", "count"):      # (may coincide by chance)
            continue
        assert not torch.equal(x, y), f"{name} did not change with the next frame"
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(first, second))      # graph=True: the same buffers


@pytest.mark.gpu
def test_a_captured_graph_goes_with_its_owner(ffraft):
    """A session's and a GraphedForward's hipGraph (graph.CapturedStep) are freed by reference count when their owner goes: no
    cycle leaves them to the garbage collector, which may run inside a later capture, where a graph cannot be destroyed."""
    import gc
    import weakref
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.graph import GraphedForward
    from focusflow_official_amd.keypoints import GoodFeatures
    frames = _u8_frames(1, 125, 157, frames=2, seed=7)
    seq = FrameSequence(ffraft, raft_iters=2, keypoints=GoodFeatures(), fb=True)
    assert seq.push(frames[0]) is None and seq.push(frames[1]) is not None
    img = torch.zeros(1, 3, 128, 160, device=DEV)
    gf = GraphedForward(ffraft, (img, img, torch.zeros(1, 1, 128, 160, device=DEV), None), raft_iters=2)
    refs = [weakref.ref(seq._captured), weakref.ref(gf._captured)]
    assert all(r().graph is not None for r in refs)
    gc.disable()      # (a collector run between the two lines below would hide a cycle)
    try:
        del seq, gf
        assert [r() for r in refs] == [None, None]
    finally:
        gc.enable()


@pytest.mark.gpu
def test_session_refusals_name_the_argument(ffraft):
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd._hip import FocusFlowHipError
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    from focusflow_official_amd.pwcnet import FF_PWCNET
    frame = _u8_frames(1, 125, 157, seed=51)[0]
    seq = FrameSequence(ffraft, raft_iters=4, keypoints=GoodFeatures())
    for fn, word in ((lambda: seq.push(frame.float()), "frame"),
                     (lambda: seq.push(torch.zeros(1, 125, 157, 4, dtype=torch.uint8)), "frame"),
                     (lambda: seq.push(frame.permute(0, 3, 1, 2)), "frame"),      # planar, but the session was told 'hwc'
                     (lambda: seq.push(frame, mask=torch.zeros(1, 1, 125, 157)), "mask"),
                     (lambda: FrameSequence(ffraft, layout="nhwc"), "layout"),
                     (lambda: FrameSequence(ffraft, order="gbr"), "order")):
        with pytest.raises((ValueError, FocusFlowHipError), match=word):
            fn()
    assert seq.push(frame) is None      # (none of the refused pushes counted as a frame)
    m = FF_RAFT_FUSION(use_fusion=None).to(DEV)
    with pytest.raises(ValueError, match="model"):
        FrameSequence(m.train())
    m.eval()
    live = FrameSequence(m)
    m.train()
    with pytest.raises(ValueError, match="model"):
        live.push(frame)
    cfg = Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION="parallel", FUSION_TYPE="1x1conv"))
    with pytest.raises(ValueError, match="GraphedForward"):
        FrameSequence(FF_PWCNET(cfg).to(DEV).eval())
