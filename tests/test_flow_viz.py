"""Flow images: csrc/flow_viz.hip (ff_flow_rad_max, ff_flow_to_image), ops.flow_to_image, the flow_viz module with the reference's
API, frames.FrameSequence(render=...) and tools/render_flows.py.

The yardstick is tests/flow_viz_ref.py, the numpy restatement of the definition in include/focusflow_hip.h; the golden file ties
it to the reference's core/utils/flow_viz.py byte for byte (no GPU needed).  Against it the kernels are held to three criteria:

  * rad_max is bit-identical: fp32 products, sum and a correctly rounded root, and a maximum, which has no rounding at all;
  * no byte differs by more than one level;
  * over all bytes of all cases together at most BYTE_SHARE = 1e-3 differ.  The one step with latitude is the fp32 angle: one
    ulp of it moves 255 col by at most about 3e-4 of a level, so even an atan2 that is an ulp off EVERYWHERE flips fewer than
    3e-4 of the bytes.  The cap is that condition with room for the kernel's fp64 angle against numpy's atan2f, not a measurement
    (the reference against its own chain with an fp64 angle: 0 of 5 883, 2 of 1 339 392, 1 of 589 824, 0 of 768 bytes).

The session's images are the same kernel on the session's own flow, so they are held to a standalone ops.flow_to_image bit for bit."""
import copy
import ctypes
import functools
import json
import os
import pickle
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import flow_viz_ref as V
import test_tracks as T
from test_tracks import models      # noqa: F401  (the module-scoped fixture: FF-RAFT on det_sd and the plain spec)

DEV = T.DEV
ENTRY_POINTS = ("ff_flow_rad_max", "ff_flow_to_image")
F32 = np.float32
BYTE_SHARE = 1e-3
H, W = T.H, T.W            # 125 x 157: padded to 128 x 160, the frame at (1, 1)
ITERS = 3
gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(GOLDEN, "flow_viz.npz"))
    return {k: z[k] for k in z.files}, json.loads(bytes(z["cases"]).decode())


def _golden_names():
    return sorted(_golden()[1])


# ----------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", _golden_names())
def test_restatement_equals_the_reference(name):
    """What ties the definition to the reference under this numpy: byte for byte, clip_flow, convert_to_bgr and max_flow included."""
    z, meta = _golden()
    kw = meta[name]
    flow, want = z[name + "_in"], z[name + "_out"]
    got, m = V.flow_to_image(flow.transpose(2, 0, 1)[None], max_flow=kw.get("max_flow"), clip_flow=kw.get("clip_flow"),
                             order="bgr" if kw.get("convert_to_bgr") else "rgb")
    assert got.dtype == np.uint8 and got.shape == (1,) + want.shape and m.dtype == F32
    assert np.array_equal(got[0], want), f"{name}: {int((got[0] != want).sum())} of {want.size} bytes differ from the reference"
    # the planar layout and the per-sample form are the same image
    chw, _ = V.flow_to_image(np.stack([flow.transpose(2, 0, 1)] * 2), max_flow=kw.get("max_flow"), clip_flow=kw.get("clip_flow"),
                             order="bgr" if kw.get("convert_to_bgr") else "rgb", layout="chw")
    assert np.array_equal(chw[1].transpose(1, 2, 0), want)


def test_restatement_beyond_the_reference():
    """Geometry, the per-sample maximum, the occlusion paint and the non-finite rule of the restatement itself."""
    g = np.random.default_rng(3)
    field = g.standard_normal((2, 2, 16, 24)).astype(F32)
    field[1] *= 50
    field[0, :, 0, 0] = 1e6      # in the padding
    img, m = V.flow_to_image(field, left=2, top=1, h=13, w=20)
    inner = np.ascontiguousarray(field[:, :, 1:14, 2:22])
    for b in range(2):
        one, mb = V.flow_to_image(inner[b:b + 1])
        assert np.array_equal(one[0], img[b]) and mb[0] == m[b]
    assert m[0] < 10 < m[1] and np.array_equal(m, V.rad_max(field, 2, 1, 13, 20))
    bad = inner.copy()
    bad[0, 0, 3, 4], bad[0, 1, 5, 6] = np.nan, np.inf
    img2, m2 = V.flow_to_image(bad)
    assert m2[0] <= m[0] and not img2[0, 3, 4].any() and not img2[0, 5, 6].any()
    occ = g.integers(0, 2, (2, 1, 13, 20)).astype(np.uint8) * 7
    img3, _ = V.flow_to_image(inner, occluded=occ, occluded_color=(255, 0, 254), order="bgr")
    plain, _ = V.flow_to_image(inner, order="bgr")
    assert (img3[occ[:, 0] != 0] == (254, 0, 255)).all() and np.array_equal(img3[occ[:, 0] == 0], plain[occ[:, 0] == 0])
    assert (V.flow_to_image(np.zeros((1, 2, 5, 7), F32))[0] == 255).all()
    nothing = np.full((1, 2, 3, 3), np.nan, F32)
    img4, m4 = V.flow_to_image(nothing)
    assert m4[0] == 0 and not img4.any()


def test_make_colorwheel_equals_the_golden_wheel():
    from focusflow_official_amd import flow_viz
    wheel = flow_viz.make_colorwheel()
    assert wheel.dtype == np.float64 and wheel.shape == (55, 3)
    assert np.array_equal(wheel, _golden()[0]["wheel"]) and np.array_equal(V.make_colorwheel(), wheel)


def test_entry_points_declared_exported_and_bound():
    from focusflow_official_amd import _hip, build
    hdr = open(os.path.join(ROOT, "include", "focusflow_hip.h")).read()
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), f"{name} is not declared in focusflow_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.EXPORTS and name in _hip._SIGS
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_hip._SIGS[name]), f"{name}: {len(_hip._SIGS[name])} bound arguments, the header declares {len(decl.split(','))}"
    history = hdr.split("#define FF_ABI_VERSION")[0]
    assert "7 (unchanged): entry points only: ff_flow_rad_max, ff_flow_to_image" in history
    lib.ff_abi_version.restype = ctypes.c_int
    assert lib.ff_abi_version() == int(re.search(r"#define FF_ABI_VERSION (\d+)", hdr).group(1)) == _hip.ABI_VERSION == 7
    src = open(os.path.join(ROOT, "focusflow_official_amd", "csrc", "flow_viz.hip")).read()
    assert "#pragma clang fp contract(off)" in src      # (build.py then adds -ffp-contract=off: a fused multiply-add changes bytes)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_flow_viz_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "flow_viz.hip"))
    assert len(kernels) >= 3, kernels      # the maximum, the dense and the strided painter
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"flow_viz.hip: kernels with scratch (bytes per lane): {spilled}"


def test_wrappers_raise_on_cpu_tensors():
    from focusflow_official_amd import flow_viz, ops
    from focusflow_official_amd._hip import FocusFlowHipError
    with pytest.raises(FocusFlowHipError, match="flow"):
        ops.flow_to_image(torch.zeros(1, 2, 8, 8))
    with pytest.raises(FocusFlowHipError, match="no CPU fallback"):
        flow_viz.flow_to_image(torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match="flow_uv"):
        flow_viz.flow_to_image(np.zeros((8, 8, 3), F32))


def test_render_refusals_name_their_argument():
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.frames import FrameSequence, Render, as_render
    assert as_render(None) is None and as_render(False) is None and as_render(True) == Render()
    assert Render() == (None, None, None, None, None, False)
    ok = Render(max_flow=24.0, clip_flow=0.0, order="bgr", layout="chw", occluded=(255, 0, 255), backward=True)
    assert as_render(ok) is ok
    for bad in (Render(max_flow=0.0), Render(max_flow=-1.0), Render(max_flow=float("inf")), Render(max_flow=float("nan"))):
        with pytest.raises(ValueError, match="render: max_flow"):
            as_render(bad)
    for bad in (Render(clip_flow=-0.5), Render(clip_flow=float("nan"))):
        with pytest.raises(ValueError, match="render: clip_flow"):
            as_render(bad)
    for bad in (Render(occluded=(255, 0)), Render(occluded=(256, 0, 0)), Render(occluded=(0, -1, 0)), Render(occluded=(0.5, 0, 0)), Render(occluded=7)):
        with pytest.raises(ValueError, match="render: occluded"):
            as_render(bad)
    with pytest.raises(ValueError, match="render: order"):
        as_render(Render(order="gbr"))
    with pytest.raises(ValueError, match="render: layout"):
        as_render(Render(layout="nhwc"))
    with pytest.raises(ValueError, match="render: True or a frames.Render"):
        as_render("yes")
    plain = FF_RAFT_FUSION(use_fusion=None).eval()
    with pytest.raises(ValueError, match="render: occluded"):
        FrameSequence(plain, render=Render(occluded=(255, 0, 255)))
    with pytest.raises(ValueError, match="render: backward"):
        FrameSequence(plain, render=Render(backward=True))
    with pytest.raises(ValueError, match="render: max_flow"):
        FrameSequence(plain, render=Render(max_flow=0))
    seq = FrameSequence(plain, fb=True, render=Render(occluded=(255, 0, 255), backward=True))
    assert seq.render.occluded == (255, 0, 255) and FrameSequence(plain).render is None and FrameSequence(plain, render=True).render == Render()


def test_frame_result_has_thirty_two_shapes():
    """What tests/test_homography.py::test_frame_result_has_sixteen_shapes holds for the results without view, for all thirty-two."""
    from focusflow_official_amd import frames
    from focusflow_official_amd.frames import FBResult, FrameResult, RenderResult
    from focusflow_official_amd.geometry import EpiResult, HomResult
    from focusflow_official_amd.tracks import TrackResult
    tr = TrackResult(torch.arange(4)[None], torch.zeros(1, 4, dtype=torch.int32), torch.tensor([4], dtype=torch.int32))
    fb = FBResult(torch.ones(1, 2, 3, 3), torch.zeros(1, 1, 3, 3), torch.ones(1, 1, 3, 3, dtype=torch.uint8), torch.ones(1, 4), torch.ones(1, 4, dtype=torch.uint8))
    epi = EpiResult(torch.eye(3)[None], torch.tensor([3], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), torch.ones(1, dtype=torch.uint8),
                    torch.ones(1, 4, dtype=torch.uint8), torch.zeros(1, 4))
    hom = HomResult(2 * torch.eye(3)[None], torch.tensor([3], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), torch.ones(1, dtype=torch.uint8),
                    torch.zeros(1, dtype=torch.uint8), torch.ones(1, 4, dtype=torch.uint8), torch.zeros(1, 4), None)
    view = RenderResult(torch.full((1, 3, 3, 3), 9, dtype=torch.uint8), torch.ones(1), None)
    base = (torch.ones(2), torch.zeros(3), torch.ones(1, 4, 4), torch.ones(1, 4, dtype=torch.uint8), torch.tensor([4], dtype=torch.int32))

    def same(a, b):
        if isinstance(a, tuple):
            return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))

    given = {"tracks": tr, "fb": fb, "epi": epi, "hom": hom, "view": view}
    word = {"tracks": "Tracked", "fb": "Checked", "epi": "Epi", "hom": "Hom", "view": "Rendered"}
    names = {}
    for n in range(32):
        extra = tuple(f for i, f in enumerate(given) if n >> i & 1)
        names[extra] = "".join(word[f] for f in extra) + "FrameResult"
    assert len(names) == 32 and len(set(names.values())) == 32 and names[("view",)] == "RenderedFrameResult"
    assert names[("tracks", "fb", "epi", "hom", "view")] == "TrackedCheckedEpiHomRenderedFrameResult"
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
        assert moved.count == 7 and type(moved) is type(res) and moved.flow_low is res.flow_low and moved.view is res.view and moved.hom is res.hom
        with pytest.raises(ValueError):
            res._replace(render=1)
        if "view" in extra:
            assert res[-1] is view and res._fields[-1] == "view" and type(res._replace(view=None)).__name__ == names[extra[:-1]]
            assert isinstance(res, getattr(frames, names[extra[:-1]]))      # (a subclass of the shape without: the other items stay where they are)
            assert tuple(res[:-1]) == tuple(res._replace(view=None))
        else:
            assert "view" not in res._asdict() and type(res._replace(view=view)).__name__ == names[extra + ("view",)]
    assert type(FrameResult(*base, tr, fb, epi, hom, view)).__name__ == "TrackedCheckedEpiHomRenderedFrameResult" and len(FrameResult(*base, tr, fb, epi, hom, view)) == 10
    assert type(FrameResult._make(base + (view,))).__name__ == "RenderedFrameResult"
    with pytest.raises(TypeError):
        FrameResult._make(base + (tr, fb, epi, hom, view, view))
    with pytest.raises(TypeError):
        FrameResult._make(base + (view, view))


def test_render_flows_path_mapping(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_flows
    for rel in ("a.flo", os.path.join("clean", "alley_1", "frame_0001.flo"), os.path.join("x", "B.FLO"), os.path.join("x", "notes.txt"), "c.png"):
        path = tmp_path / "flo" / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(b"")
    rels = render_flows.find_flows(str(tmp_path / "flo"))
    assert rels == sorted(["a.flo", os.path.join("clean", "alley_1", "frame_0001.flo"), os.path.join("x", "B.FLO")])
    assert render_flows.png_path("out", os.path.join("clean", "alley_1", "frame_0001.flo")) == os.path.join("out", "clean", "alley_1", "frame_0001.png")
    assert render_flows.png_path("out", "a.flo") == os.path.join("out", "a.png")


# ----------------------------------------------------------------------------
# the kernels against the restatement
# ----------------------------------------------------------------------------
def _noise(shape, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(F32)


def _grid():
    gy, gx = np.meshgrid(np.arange(-8, 8, dtype=F32), np.arange(-8, 8, dtype=F32), indexing="ij")
    return np.stack([gx, gy])[None]      # exact zeros, axis-aligned vectors, diagonals


def _seam():
    """v = +-0.0 with u of either sign (a = -1 / +1: k0 = 0 / 54 and the wrap of k1), and the neighbourhood of the seam."""
    f = np.zeros((1, 2, 4, 8), F32)
    f[0, 0] = np.array([3, 1, 0.5, 1e-3, -3, -1, -0.5, -1e-3], F32)
    f[0, 1, 0], f[0, 1, 1], f[0, 1, 2], f[0, 1, 3] = 0.0, -0.0, 1e-7, -1e-7
    return f


def _cases():
    """name -> (field (B,2,Hp,Wp), keyword arguments of both ops.flow_to_image and the restatement, how the field is stored, how
    `out` is made)."""
    c = {}
    c["one_1x1"] = (_noise((1, 2, 1, 1), 1), {}, "nchw", None)
    c["small_5x7"] = (_noise((1, 2, 5, 7), 2), {}, "nchw", None)
    batch = _noise((3, 2, 37, 53), 3)
    batch[0] *= 0.01
    batch[2] *= 100
    c["batch3_37x53"] = (batch, {}, "nchw", None)      # very different maxima per sample
    padded = _noise((2, 2, 128, 160), 4)
    padded[:, :, 0, :], padded[:, :, :, 0] = 1e6, -1e6      # in the padding: must not reach the maximum
    padded[:, :, 126:, :], padded[:, 0, :, 158:], padded[:, 1, :, 158:] = 3e5, np.inf, np.nan
    c["frame_125x157_in_128x160"] = (padded, dict(left=1, top=1, h=125, w=157), "nchw", None)
    c["nhwc_view_37x53"] = (_noise((2, 2, 37, 53), 5), {}, "nhwc", None)
    for w in (5, 6, 7, 8):      # 3 W = 15, 18, 21, 24: the tails of the dword stores, and none
        c[f"tail_w{w}_b1"] = (_noise((1, 2, 3, w), 10 + w), {}, "nchw", None)
        c[f"tail_w{w}_b2"] = (_noise((2, 2, 3, w), 20 + w), {}, "nchw", None)
    c["tail_3x2x37x53"] = (_noise((3, 2, 37, 53), 6), {}, "nchw", None)      # 3 x 37 x 53 pixels: one left over for the byte stores
    lay = _noise((2, 2, 37, 53), 7)
    for layout in ("hwc", "chw"):
        for order in ("rgb", "bgr"):
            c[f"{layout}_{order}"] = (lay, dict(layout=layout, order=order), "nchw", None)
            c[f"{layout}_{order}_out_strided"] = (lay, dict(layout=layout, order=order), "nchw", "strided")
    c["hwc_out_unaligned"] = (lay, {}, "nchw", "unaligned")
    c["grid_16x16"] = (_grid(), {}, "nchw", None)
    c["grid_16x16_max"] = (_grid(), dict(max_flow=8.0), "nchw", None)
    c["seam_4x8"] = (_seam(), {}, "nchw", None)
    c["zero_5x7"] = (np.zeros((1, 2, 5, 7), F32), {}, "nchw", None)
    huge = _noise((1, 2, 9, 11), 8, 1e-3)
    huge[0, :, 4, 5] = (3e4, -1e4)
    c["huge_among_tiny"] = (huge, {}, "nchw", None)
    c["max_flow_beyond"] = (lay, dict(max_flow=2.0), "nchw", None)      # most vectors lie beyond it: the 0.75 branch
    c["max_flow_within"] = (lay, dict(max_flow=40.0), "nchw", None)
    c["clip_negative_components"] = (lay, dict(clip_flow=1.5), "nchw", None)
    c["clip_zero"] = (lay, dict(clip_flow=0.0), "nchw", None)
    c["clip_and_max_flow"] = (lay, dict(clip_flow=3.0, max_flow=1.5, order="bgr"), "nchw", None)
    bad = _noise((2, 2, 9, 11), 9)
    bad[0, 0, 2, 3], bad[0, 1, 4, 4], bad[0, :, 6, 6], bad[0, 0, 7, 1] = np.nan, np.inf, (-np.inf, np.nan), 3e38      # (3e38: a magnitude that overflows)
    bad[1] = np.nan      # a frame without a single vector: maximum 0, all black
    c["nan_and_inf"] = (bad, {}, "nchw", None)
    c["nan_and_inf_clip"] = (bad, dict(clip_flow=2.0, layout="chw"), "nchw", None)
    occ = (np.random.default_rng(11).integers(0, 3, (2, 1, 37, 53)) == 0).astype(np.uint8) * 255
    c["occluded"] = (lay, dict(occluded=occ, occluded_color=(255, 0, 254)), "nchw", None)
    c["occluded_bgr_chw_max"] = (lay, dict(occluded=occ[:, 0], occluded_color=(1, 2, 3), order="bgr", layout="chw", max_flow=5.0), "nchw", None)
    return c


def _make_out(how, shape, layout):
    if how is None:
        return None
    if how == "unaligned":      # contiguous, but not on a 4-byte address: the byte-store kernel
        n = int(np.prod(shape))
        return torch.full((n + 8,), 77, dtype=torch.uint8, device=DEV)[1:1 + n].view(shape)
    b, h, w = (shape[0], shape[1], shape[2]) if layout == "hwc" else (shape[0], shape[2], shape[3])
    if layout == "hwc":      # the RGB of an RGBA canvas with a margin
        return torch.full((b, h + 2, w + 3, 4), 77, dtype=torch.uint8, device=DEV)[:, 1:h + 1, 2:w + 2, :3]
    return torch.full((b, 3, h + 1, w + 5), 77, dtype=torch.uint8, device=DEV)[:, :, :h, 1:w + 1]


_RESULTS = {}


def _run_case(name):
    """-> (got image, want image, got rad_max, want rad_max), numpy; computed once per case."""
    if name in _RESULTS:
        return _RESULTS[name]
    from focusflow_official_amd import ops
    field, kw, store, out_how = _cases()[name]
    t = torch.from_numpy(field)
    dev = t.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2) if store == "nhwc" else t.to(DEV)
    assert store != "nhwc" or not dev.is_contiguous()
    want, want_max = V.flow_to_image(field, **kw)
    kwd = dict(kw)
    if "occluded" in kwd:
        occ = torch.from_numpy(kwd["occluded"])
        if occ.dim() == 3:      # a strided plane: every second column of a wider one
            wide = torch.zeros(occ.shape[0], occ.shape[1], occ.shape[2] * 2, dtype=torch.uint8)
            wide[:, :, ::2] = occ
            kwd["occluded"] = wide.to(DEV)[:, :, ::2]
        else:
            kwd["occluded"] = occ.to(DEV)
    out = _make_out(out_how, want.shape, kw.get("layout", "hwc"))
    canvas = out._base.clone() if out is not None and out._base is not None else None
    img, m = ops.flow_to_image(dev, out=out, return_max=True, **kwd)
    torch.cuda.synchronize()
    assert img.dtype == torch.uint8 and tuple(img.shape) == want.shape and m.dtype == torch.float32 and tuple(m.shape) == (field.shape[0],)
    if out is not None:
        assert img is out
        if canvas is not None and out_how == "strided":      # nothing outside the view was written
            after = out._base.clone()
            probe = torch.zeros_like(after, dtype=torch.bool)
            sel = probe[:, 1:-1, 2:-1, :3] if kw.get("layout", "hwc") == "hwc" else probe[:, :, :-1, 1:-4]
            sel[...] = True
            assert torch.equal(after[~probe], canvas[~probe]), f"{name}: bytes outside the out view changed"
    else:
        assert img.is_contiguous()
        # without return_max and with max_flow: the same image (one launch less)
        again = ops.flow_to_image(dev, **kwd)
        assert torch.equal(again, img), f"{name}: the image without return_max differs"
    _RESULTS[name] = (img.cpu().numpy(), want, m.cpu().numpy(), want_max)
    return _RESULTS[name]


def _differing(got, want, what):
    """Asserts the per-byte criterion; -> (bytes that differ, bytes)."""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    n = int((d != 0).sum())
    print(f"{what}: {n} of {d.size} bytes differ ({n / d.size:.2e}), by at most {int(d.max()) if d.size else 0}")
    assert d.max() <= 1, f"{what}: a byte differs by {int(d.max())} levels at {np.unravel_index(int(d.argmax()), d.shape)}"
    return n, d.size


@gpu
@pytest.mark.parametrize("name", list(_cases()))
def test_flow_to_image_against_the_restatement(name):
    got, want, m, want_max = _run_case(name)
    assert np.array_equal(m.view(np.uint32), want_max.view(np.uint32)), f"{name}: rad_max {m} vs {want_max}"
    _differing(got, want, name)
    if name == "zero_5x7":
        assert (got == 255).all()
    if name.startswith("nan_and_inf"):
        hwc = got if got.shape[-1] == 3 else got.transpose(0, 2, 3, 1)
        assert not hwc[0, 2, 3].any() and not hwc[0, 4, 4].any() and not hwc[0, 6, 6].any() and not hwc[1].any()
        assert name.endswith("clip") or not hwc[0, 7, 1].any()      # (clipped to 2.0 the magnitude no longer overflows)
        assert m[1] == 0 and hwc[0].any()
    if name == "frame_125x157_in_128x160":
        assert m.max() < 100      # (the planted 1e6, 3e5 and inf of the padding stayed out)
    if name == "batch3_37x53":
        assert m[0] * 30 < m[1] and m[1] * 30 < m[2]
    if name == "max_flow_beyond":
        assert (m > 2.0).all()


@gpu
def test_share_of_differing_bytes_over_all_cases():
    """The third criterion: over all bytes of all cases together at most 1e-3 differ (the module docstring says where that is from)."""
    n = total = 0
    for name in _cases():
        got, want, _, _ = _run_case(name)
        n, total = n + int((got != want).sum()), total + got.size
    print(f"ops.flow_to_image against the restatement: {n} of {total} bytes differ, a share of {n / total:.2e}")
    assert n <= BYTE_SHARE * total, f"{n} of {total} bytes differ: {n / total:.2e} > {BYTE_SHARE}"


@gpu
def test_numpy_in_numpy_out_against_the_golden_images():
    """flow_viz.flow_to_image with the reference's API on what a caller of the reference passes, against the reference's own images."""
    from focusflow_official_amd import flow_viz
    z, meta = _golden()
    n = total = 0
    for name in sorted(meta):
        got = flow_viz.flow_to_image(z[name + "_in"], **meta[name])
        want = z[name + "_out"]
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape
        k, size = _differing(got, want, "golden " + name)
        n, total = n + k, total + size
    print(f"flow_viz.flow_to_image against the reference: {n} of {total} bytes differ, a share of {n / total:.2e}")
    assert n <= BYTE_SHARE * total
    # a device tensor stays on the device: (2,H,W) -> (H,W,3), (B,2,H,W) -> (B,H,W,3)
    flow = torch.from_numpy(z["noise_37x53_in"]).permute(2, 0, 1).to(DEV)
    one, two = flow_viz.flow_to_image(flow, convert_to_bgr=True), flow_viz.flow_to_image(torch.stack([flow, flow * 2]), max_flow=4.0)
    assert one.is_cuda and tuple(one.shape) == (37, 53, 3) and two.is_cuda and tuple(two.shape) == (2, 37, 53, 3)
    _differing(one.cpu().numpy(), z["noise_37x53_bgr_out"], "device tensor (2,H,W), bgr")
    _differing(two[0].cpu().numpy(), z["noise_37x53_max_out"], "device tensor (B,2,H,W), max_flow")


@gpu
def test_flow_to_image_refusals_name_their_argument():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    flow = torch.zeros(2, 2, 16, 24, device=DEV)
    for kw, word in ((dict(max_flow=0.0), "max_flow"), (dict(max_flow=float("inf")), "max_flow"), (dict(max_flow=float("nan")), "max_flow"),
                     (dict(clip_flow=-1.0), "clip_flow"), (dict(clip_flow=float("nan")), "clip_flow"), (dict(order="gbr"), "order"), (dict(layout="nhwc"), "layout"),
                     (dict(left=20, w=8), "left"), (dict(top=-1), "top"), (dict(h=17), "frame"), (dict(occluded_color=(0, 0)), "occluded_color"),
                     (dict(occluded_color=(0, 0, 256)), "occluded_color"), (dict(occluded_color=(0.5, 0, 0)), "occluded_color"),
                     (dict(occluded=torch.zeros(2, 1, 16, 24, device=DEV)), "occluded"), (dict(occluded=torch.zeros(2, 16, 23, dtype=torch.uint8, device=DEV)), "occluded"),
                     (dict(occluded=torch.zeros(2, 16, 24, dtype=torch.uint8)), "occluded"),
                     (dict(out=torch.zeros(2, 3, 16, 24, dtype=torch.uint8, device=DEV)), "out"), (dict(out=torch.zeros(2, 16, 24, 3, device=DEV)), "out"),
                     (dict(out=(torch.zeros(2, 16, 24, 3, dtype=torch.uint8, device=DEV), torch.zeros(2, device=DEV))), "out")):
        with pytest.raises(FocusFlowHipError, match=word):
            ops.flow_to_image(flow, **kw)
    for bad in (torch.zeros(2, 3, 16, 24, device=DEV), torch.zeros(2, 16, 24, device=DEV), torch.zeros(2, 2, 16, 24, device=DEV, dtype=torch.float64)):
        with pytest.raises(FocusFlowHipError, match="flow"):
            ops.flow_to_image(bad)


@gpu
def test_captured_maximum_is_not_stale():
    """This feature's one stateful bug: the same captured graph replayed on a field with SMALLER motion than the last must leave
    the smaller maximum (the words are cleared inside the entry point's own enqueued work)."""
    from focusflow_official_amd import ops
    big, small = _noise((2, 2, 37, 53), 30, 50.0), _noise((2, 2, 37, 53), 31, 0.5)
    field = torch.from_numpy(big).to(DEV)
    image, rad_max = torch.zeros(2, 37, 53, 3, dtype=torch.uint8, device=DEV), torch.zeros(2, device=DEV)
    ops.flow_to_image(field, out=(image, rad_max), return_max=True)      # (not inside the capture: the first call loads the library)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.flow_to_image(field, out=(image, rad_max), return_max=True)
    for data in (big, small, big, small, small):
        field.copy_(torch.from_numpy(data))
        graph.replay()
        want, want_max = V.flow_to_image(data)
        assert np.array_equal(rad_max.cpu().numpy().view(np.uint32), want_max.view(np.uint32)), (rad_max.cpu().numpy(), want_max)
        assert torch.equal(image, ops.flow_to_image(field))
        _differing(image.cpu().numpy(), want, "replay")
    assert V.rad_max(small).max() * 10 < V.rad_max(big).min()


# ----------------------------------------------------------------------------
# the session
# ----------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _frames(layout="hwc", order="rgb"):
    """Five frames of B = 2 videos: the second a shift of the first by many pixels, the third the second again, the fourth the
    first again, the fifth the second: the last pair is the first pair once more."""
    a, b = T._u8_frames(2, H, W, 2, T.SEED, (9, -12))
    frames = [a, b, b.clone(), a.clone(), b.clone()]
    if order == "bgr":
        frames = [f.flip(-1) for f in frames]
    if layout == "chw":
        frames = [f.permute(0, 3, 1, 2).contiguous() for f in frames]
    return frames


_RUNS = {}


def _items(x):
    """Every tensor of a result, nested items included, as numpy; None stays None."""
    if isinstance(x, tuple):
        return [y for item in x for y in _items(item)]
    return [_np(x)]


def _run(models, kind, graph, render, fb=None, layout="hwc", order="rgb", cold=False):
    """One session over the first four frames; cold: over all five and without warm start, so that every pair stands alone.  With render= every pair is held to a standalone ops.flow_to_image on the pair's own
    flow (bit for bit: it is the same kernel) and to the restatement.  -> per pair a dict of numpy copies.  Cached."""
    key = (kind, graph, render, fb, layout, order, cold)
    if key in _RUNS:
        return _RUNS[key]
    from focusflow_official_amd import ops
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    det = GoodFeatures(max_corners=100) if kind == "ffraft" else None      # (FF-RAFT reads a mask of every frame; plain RAFT has none)
    seq = FrameSequence(models[kind], raft_iters=ITERS, graph=graph, keypoints=det, fb=fb, render=render, layout=layout, order=order, warm_start=not cold)
    frames = _frames(layout, order)
    assert seq.push(frames[0]) is None
    pairs = []
    for t in (1, 2, 3, 4) if cold else (1, 2, 3):
        res = seq.push(frames[t])
        what = f"{kind} graph={graph} render={render} pair {t}"
        pair = {"items": _items(tuple(res[:len(res) - (render is not None)])), "fields": res._fields, "flow_up": _np(res.flow_up)}
        if render is None:
            assert res.view is None and "view" not in res._fields
        else:
            r = seq.render
            lay, ordr = r.layout or layout, r.order or order
            assert res[-1] is res.view and res._fields[-1] == "view" and type(res).__name__.endswith("RenderedFrameResult")
            assert tuple(res.view.image.shape) == ((2, H, W, 3) if lay == "hwc" else (2, 3, H, W)) and res.view.image.dtype == torch.uint8
            kw = dict(max_flow=r.max_flow, clip_flow=r.clip_flow, order=ordr, layout=lay)
            occ = dict(occluded=res.fb.occluded, occluded_color=r.occluded) if r.occluded is not None else {}
            # the result's own padded flow: flow_up is the crop of the padded field, and the view is passed as it is
            assert not res.flow_up.is_contiguous() and ops.pad_offsets(H, W)[:2] == (1, 1)
            alone, alone_max = ops.flow_to_image(res.flow_up, 0, 0, H, W, return_max=True, **kw, **occ)
            assert torch.equal(res.view.image, alone), what + ": the session's image is not the standalone render of its flow"
            want, want_max = V.flow_to_image(pair["flow_up"], **kw, **({"occluded": _np(res.fb.occluded), "occluded_color": r.occluded} if occ else {}))
            pair["differing"] = _differing(_np(res.view.image), want, what)
            if r.max_flow is None:
                assert torch.equal(res.view.rad_max, alone_max) and np.array_equal(_np(res.view.rad_max).view(np.uint32), want_max.view(np.uint32)), what
            else:
                assert res.view.rad_max is None
            if occ:
                plain = ops.flow_to_image(res.flow_up, 0, 0, H, W, **kw)
                paint = torch.tensor(r.occluded if ordr == "rgb" else r.occluded[::-1], dtype=torch.uint8, device=DEV)
                mask = (res.fb.occluded[:, 0] != 0)[..., None]
                assert lay == "hwc" and torch.equal(res.view.image, torch.where(mask, paint, plain)), what + ": the painted pixels are not exactly fb.occluded != 0"
                pair["occluded"] = int(mask.sum())
            if r.backward:
                assert torch.equal(res.view.image_bw, ops.flow_to_image(res.fb.flow_bw, 0, 0, H, W, **kw)), what + ": image_bw"
                _differing(_np(res.view.image_bw), V.flow_to_image(_np(res.fb.flow_bw), **kw)[0], what + " (backward)")
            else:
                assert res.view.image_bw is None
            pair["image"], pair["rad_max"] = _np(res.view.image), _np(res.view.rad_max)
        pairs.append(pair)
    _RUNS[key] = pairs
    return pairs


def _same_items(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")), f"{what}: item {i}"


@gpu
@pytest.mark.parametrize("kind", ["plain", "ffraft"])
def test_session_renders_its_own_flow(models, kind, graph=True):
    """res.view.image is ops.flow_to_image of the result's own flow, bit for bit, and meets the kernels' criteria against the
    restatement (both inside _run); rendering only reads: every other item is what the same session gives without render=."""
    with_view = _run(models, kind, graph, True)
    without = _run(models, kind, graph, None)
    n = total = 0
    for t, (a, b) in enumerate(zip(with_view, without)):
        assert a["fields"] == b["fields"] + ("view",)
        _same_items(a["items"], b["items"], f"{kind} graph={graph} pair {t + 1}: with render= against without")
        n, total = n + a["differing"][0], total + a["differing"][1]
    assert n <= BYTE_SHARE * total, f"{n} of {total} bytes differ from the restatement"


@gpu
@pytest.mark.parametrize("kind", ["plain", "ffraft"])
def test_session_graph_and_eager_agree(models, kind):
    for t, (g, e) in enumerate(zip(_run(models, kind, True, True), _run(models, kind, False, True))):
        print(f"{kind} pair {t + 1}: max |flow_up graph - eager| = {np.abs(g['flow_up'] - e['flow_up']).max():.3e}, "
              f"{int((g['image'] != e['image']).sum())} of {g['image'].size} image bytes differ, rad_max {g['rad_max']} / {e['rad_max']}")
    for t, (g, e) in enumerate(zip(_run(models, kind, True, True), _run(models, kind, False, True))):
        assert np.array_equal(g["image"], e["image"]) and np.array_equal(g["rad_max"], e["rad_max"]), f"{kind} pair {t + 1}"


@gpu
def test_session_across_replays_has_no_stale_maximum(models):
    """A pair with large motion (a frame shifted by many pixels), then a pair of identical frames, then the shift back and the
    first pair again, through the same captured graph: every maximum and image is that of a fresh standalone render of that
    pair's flow (held inside _run, repeated here against the restatement).  The session runs without warm start, so every pair
    stands alone and the last maximum is the first again: maxima that differ at all must then fall somewhere.  That they do is
    asserted, not assumed: in every sample some replay follows one with a LARGER maximum, so a maximum left over from the replay
    before would have shown.  (With warm start the flow of random weights grows from pair to pair: 5.9, 11.6, 16.1 px.)"""
    pairs = _run(models, "plain", True, True, cold=True)
    maxima = np.stack([p["rad_max"] for p in pairs])      # (pairs, B)
    print(f"rad_max of the shifted pair {maxima[0]}, of the identical pair {maxima[1]}, of the pair shifted back {maxima[2]}, of the first pair again {maxima[3]}")
    assert ((maxima[1:] < maxima[:-1]).any(axis=0)).all(), f"no replay follows a larger maximum: {maxima}"
    assert (maxima[0] != maxima[1]).all() and not np.array_equal(pairs[0]["image"], pairs[1]["image"])
    for p in pairs:
        want, want_max = V.flow_to_image(p["flow_up"])
        assert np.array_equal(p["rad_max"].view(np.uint32), want_max.view(np.uint32))


@gpu
def test_session_paints_the_occlusion_map_and_renders_the_backward_flow(models):
    from focusflow_official_amd.frames import Render
    render = Render(occluded=(255, 0, 255), backward=True)
    with_view = _run(models, "plain", True, render, fb=True)
    without = _run(models, "plain", True, None, fb=True)
    for t, (a, b) in enumerate(zip(with_view, without)):
        assert a["fields"] == b["fields"] + ("view",) and a["fields"][-2:] == ("fb", "view")
        _same_items(a["items"], b["items"], f"pair {t + 1}: with render= against without")
    painted = [a["occluded"] for a in with_view]
    print(f"occluded pixels painted per pair: {painted} of {2 * H * W}")
    assert any(0 < k < 2 * H * W for k in painted), "the occlusion maps of these pairs are empty or full: the paint was not exercised"


@gpu
def test_bgr_chw_session_returns_bgr_chw(models):
    """order / layout None: the session's own.  A session fed BGR CHW frames gets BGR CHW images, and Render can say otherwise."""
    from focusflow_official_amd.frames import Render
    own = _run(models, "plain", True, True, layout="chw", order="bgr")
    rgb = _run(models, "plain", True, Render(order="rgb", layout="hwc", max_flow=24.0), layout="chw", order="bgr")
    ref = _run(models, "plain", True, True)      # the same video as RGB HWC frames: the same fp32 images, so the same flow
    for a, b, c in zip(own, rgb, ref):
        assert a["image"].shape == (2, 3, H, W) and b["image"].shape == (2, H, W, 3) and b["rad_max"] is None
        assert np.array_equal(a["flow_up"], c["flow_up"]) and np.array_equal(a["image"], c["image"][..., ::-1].transpose(0, 3, 1, 2))


@gpu
def test_render_flows_tool(tmp_path):
    """Two tiny .flo files of different sizes and one more of the first size through tools/render_flows.py's function: PNGs at
    the same relative paths, equal to ops.flow_to_image."""
    from PIL import Image
    from focusflow_official_amd import frame_utils, ops
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_flows
    flows = {"a.flo": _noise((9, 11, 2), 40), os.path.join("seq", "b.flo"): _noise((6, 7, 2), 41), os.path.join("seq", "c.flo"): _noise((9, 11, 2), 42, 30.0)}
    for rel, f in flows.items():
        os.makedirs(os.path.dirname(str(tmp_path / "flo" / rel)), exist_ok=True)
        frame_utils.writeFlow(str(tmp_path / "flo" / rel), f)
    for max_flow, root in ((None, "png"), (5.0, "png_max")):
        rels = render_flows.render_tree(str(tmp_path / "flo"), str(tmp_path / root), max_flow=max_flow, batch=2)
        assert rels == sorted(flows)
        for rel, f in flows.items():
            with Image.open(render_flows.png_path(str(tmp_path / root), rel)) as im:
                got = np.asarray(im.convert("RGB"))
            want = ops.flow_to_image(torch.from_numpy(f).to(DEV).permute(2, 0, 1)[None], max_flow=max_flow)[0].cpu().numpy()
            assert np.array_equal(got, want), (rel, max_flow)
