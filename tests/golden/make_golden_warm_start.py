#!/usr/bin/env python
"""Generate tests/golden/warm_start.npz with the reference's forward_interpolate (core/utils/utils.py:26-54).
Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_warm_start.py

20 cases: planes 14x18, 46x62, 48x64, 68x120 times flows randn*2, randn*8, a smooth bicubic field of +-6 px, the constant
(3,-1) and zero.  While it runs it asserts that the fp64 brute-force restatement of tests/test_warm_start.py equals the
reference on every case and that no pixel of any case has a tied minimum (scipy's tie order is its tree's own)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/core")
from utils.utils import forward_interpolate  # noqa: E402  (reference)

sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from test_warm_start import FLOWS, PLANES, brute_force_interpolate  # noqa: E402


def make_flow(kind, h, w, g):
    if kind == "randn2":
        return torch.randn(2, h, w, generator=g) * 2
    if kind == "randn8":
        return torch.randn(2, h, w, generator=g) * 8
    if kind == "smooth6":
        f = F.interpolate(torch.randn(1, 2, h // 8 + 2, w // 8 + 2, generator=g), size=(h, w), mode="bicubic", align_corners=False)[0]
        return f * (6.0 / f.abs().max())
    if kind == "const":
        return torch.stack([torch.full((h, w), 3.0), torch.full((h, w), -1.0)])
    assert kind == "zero"
    return torch.zeros(2, h, w)


out, pixels, differing, tied = {}, 0, 0, 0
g = torch.Generator().manual_seed(20)
for h, w in PLANES:
    for kind in FLOWS:
        f = make_flow(kind, h, w, g).float().contiguous()
        ref = forward_interpolate(f).numpy()
        mine, ties = brute_force_interpolate(f.numpy())
        pixels += h * w
        differing += int((mine != ref).any(axis=0).sum())
        tied += int(ties.sum())
        out[f"{h}x{w}_{kind}_in"] = f.numpy()
        out[f"{h}x{w}_{kind}_out"] = ref
assert differing == 0 and tied == 0, (differing, tied)
path = os.path.join(HERE, "warm_start.npz")
np.savez_compressed(path, **out)
print(f"{len(out) // 2} cases, {pixels} pixels: {differing} differ from the restatement, {tied} tied; {os.path.getsize(path)} bytes")
