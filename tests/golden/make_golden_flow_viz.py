#!/usr/bin/env python
"""Generate tests/golden/flow_viz.npz with the reference's flow_to_image (core/utils/flow_viz.py; `max_flow` is the extension of
the copy under core/models/ff-flowformer/FF_FlowFormer_Core/utils/flow_viz.py, which is otherwise the same file).
Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_flow_viz.py

Stored per case: the [H,W,2] float32 input, the keyword arguments and the reference's [H,W,3] uint8 image; and the wheel.  While
it runs it asserts that the restatement of tests/flow_viz_ref.py equals the reference on every case, byte for byte, and that both
copies of the reference agree where both apply."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("ref_flow_viz", "/root/reference/core/utils/flow_viz.py")
ref_mf = _load("ref_flow_viz_mf", "/root/reference/core/models/ff-flowformer/FF_FlowFormer_Core/utils/flow_viz.py")
sys.path.insert(0, os.path.dirname(HERE))
import flow_viz_ref as R  # noqa: E402


def cases():
    g = np.random.default_rng(21)
    f32 = np.float32
    noise = (g.standard_normal((37, 53, 2)) * 3).astype(f32)
    yield "noise_37x53", noise, {}
    yield "noise_37x53_bgr", noise, {"convert_to_bgr": True}
    yield "noise_37x53_clip", noise, {"clip_flow": 2.5}
    yield "noise_37x53_clip_bgr", noise, {"clip_flow": 1.0, "convert_to_bgr": True}
    yield "noise_37x53_max", noise, {"max_flow": 4.0}
    yield "noise_37x53_max_small", noise, {"max_flow": 0.1}
    yield "noise_37x53_max_clip", noise, {"max_flow": 1.5, "clip_flow": 3.0}
    big = (g.standard_normal((125, 157, 2)) * np.array([20.0, 0.3])).astype(f32)
    yield "noise_125x157", big, {}
    ys, xs = np.meshgrid(np.arange(64, dtype=f32), np.arange(96, dtype=f32), indexing="ij")
    ramp = np.stack([(xs - 47.5) / 7, (ys - 31.5) / 5], axis=-1).astype(f32)
    yield "ramp_64x96", ramp, {}
    yield "ramp_64x96_max", ramp, {"max_flow": 3.0}
    gy, gx = np.meshgrid(np.arange(-8, 8, dtype=f32), np.arange(-8, 8, dtype=f32), indexing="ij")
    grid = np.stack([gx, gy], axis=-1)       # exact zeros, axis-aligned vectors, diagonals
    yield "grid_16x16", grid, {}
    yield "grid_16x16_max", grid, {"max_flow": 8.0}
    # the seam of the wheel: v = +-0.0 with u of either sign (a = -1 / +1: k0 = 0 / 54 and the wrap of k1), and its neighbourhood
    seam = np.zeros((4, 8, 2), f32)
    seam[..., 0] = np.array([3, 1, 0.5, 1e-3, -3, -1, -0.5, -1e-3], f32)
    seam[0, :, 1], seam[1, :, 1], seam[2, :, 1], seam[3, :, 1] = 0.0, -0.0, 1e-7, -1e-7
    yield "seam_4x8", seam, {}
    yield "zero_5x7", np.zeros((5, 7, 2), f32), {}
    huge = (g.standard_normal((9, 11, 2)) * 1e-3).astype(f32)
    huge[4, 5] = (3e4, -1e4)
    yield "huge_9x11", huge, {}
    yield "one_1x1", np.array([[[0.25, -2.0]]], f32), {}


out, meta, pixels = {"wheel": ref.make_colorwheel()}, {}, 0
assert np.array_equal(out["wheel"], ref_mf.make_colorwheel()) and np.array_equal(out["wheel"], R.make_colorwheel())
for name, flow, kw in cases():
    image = ref_mf.flow_to_image(flow.copy(), **kw)
    if "max_flow" not in kw:
        assert np.array_equal(image, ref.flow_to_image(flow.copy(), **kw)), name
    mine, _ = R.flow_to_image(flow.transpose(2, 0, 1)[None], max_flow=kw.get("max_flow"), clip_flow=kw.get("clip_flow"),
                              order="bgr" if kw.get("convert_to_bgr") else "rgb")
    differ = int((mine[0] != image).sum())
    assert differ == 0, (name, differ, image.size)
    out[name + "_in"], out[name + "_out"], meta[name] = flow, image, kw
    pixels += flow.shape[0] * flow.shape[1]
out["cases"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
path = os.path.join(HERE, "flow_viz.npz")
np.savez_compressed(path, **out)
print(f"{len(meta)} cases, {pixels} pixels, numpy {np.__version__}: the restatement equals the reference; {os.path.getsize(path)} bytes")
