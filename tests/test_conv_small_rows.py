"""conv_small.hip - the 1- / 2-channel 3x3 heads in fp32 rows - against F.conv2d in float64, on both of its kernels.

ff::conv2d_fwd_small sends inputs of 128 channels or more to the tile kernel (partial products on the exact-fp32 MFMA,
summed over the 3x3 neighbourhood through LDS) and narrower ones to the run kernel; FF_SMALL_TILE=0 sends everything to the
run kernel.  The switch is read once per process, so the cases run twice: in this process (the shipped route) and in one
child process with the switch at 0, which writes its outputs to a file.  Every case is then held to the same bound on
both routes, and the two sets are compared bit for bit: equal below 128 channels (the same kernel), different above (a
different summation order - if they were equal the switch would not switch).

Bound, per output:  |y - y64| <= gamma_K * sum |x_i| |w_i|,  gamma_K = K u / (1 - K u),  K = 9 Cin + 2,  u = 2^-24:
the error of a sum of K rounded products in ANY order, so it holds for both kernels without knowing theirs.  The epilogue
options are applied to the float64 result, and every further rounded operation adds u times the magnitude of its result
(and scales the bound it inherits): bias, out_scale, ch_scale and ch_shift (two roundings), the residual add; ReLU is
1-Lipschitz and adds nothing.

Shapes are the smallest at which the kernels can go wrong: one pixel; a plane smaller than one 6 x 8 tile; 70 columns
(nine tiles and nine runs of 8, the last ragged) with odd heights, 64 columns and 17; Cin 4 and 36 (run kernel), 256 (one full
pass), 260 and 320 (a second pass with 1 and 4 of its 16 channel steps; 260 ends inside a step), 128 + 64 + 4 in three
segments (segment borders inside a wave's channels), and both halves of a 512-channel tensor (ld > C, a non-zero
16-byte-aligned offset).
"""
import os
import subprocess
import sys
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

DEV = "cuda:0"
U = 2.0 ** -24
SWITCH = "FF_SMALL_TILE"
TILE_MIN_CIN = 128            # conv_small.hip: `cin >= 128`

Case = namedtuple("Case", "name segs bhw cout opt layout")


def _cases():
    cs = []
    for bhw in [(2, 1, 1), (1, 3, 5), (2, 5, 70), (1, 7, 64), (2, 9, 17)]:
        cs.append(Case(f"geom{bhw}", (256,), bhw, 2, None, "dense"))
    for cin in (4, 36, 260, 320):
        cs.append(Case(f"cin{cin}", (cin,), (2, 5, 70), 2, None, "dense"))
    cs.append(Case("cout1-256", (256,), (1, 7, 64), 1, None, "dense"))
    cs.append(Case("cout1-4", (4,), (2, 9, 17), 1, None, "dense"))
    cs.append(Case("cout1-320", (320,), (1, 3, 5), 1, None, "dense"))
    cs.append(Case("cout1-260", (260,), (2, 5, 70), 1, None, "dense"))
    cs.append(Case("seg3", (128, 64, 4), (2, 5, 70), 2, None, "dense"))
    cs.append(Case("seg3-cout1", (128, 64, 4), (2, 9, 17), 1, None, "dense"))
    cs.append(Case("half-lo", (256,), (2, 5, 70), 2, None, "lo"))
    cs.append(Case("half-hi", (256,), (2, 5, 70), 2, None, "hi"))
    for opt in ("bias", "out_scale", "ch_scale", "relu", "res"):
        cs.append(Case(f"opt-{opt}", (256,), (2, 5, 70), 2, opt, "dense"))
        cs.append(Case(f"opt-{opt}-36", (36,), (2, 9, 17), 1, opt, "dense"))
    cs.append(Case("coords", (256,), (2, 5, 70), 2, "coords", "dense"))
    cs.append(Case("nonfinite", (256,), (2, 5, 70), 2, "nonfinite", "dense"))
    cs.append(Case("nonfinite-36", (36,), (2, 5, 70), 2, "nonfinite", "dense"))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def _problem(c):
    """CPU fp32 tensors of a case: NHWC segments, OIHW weights, and the operands of its option."""
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    b, h, w = c.bhw
    cin = sum(c.segs)
    xs = [torch.randn(b, h, w, s, generator=g) for s in c.segs]
    wt = torch.randn(c.cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    extra = {
        "bias": torch.randn(c.cout, generator=g),
        "ch_scale": 1 + 0.25 * torch.randn(c.cout, generator=g),
        "ch_shift": torch.randn(c.cout, generator=g),
        "res": torch.randn(b, h, w, c.cout, generator=g),
        "coords": 50 * torch.randn(b, h, w, 2, generator=g),
    }
    if c.opt == "nonfinite":          # image corners: the padding select must neither hide them nor spread them
        xs[0][0, 0, 0, 3] = float("nan")
        xs[0][b - 1, h - 1, w - 1, 5] = float("inf")
    return xs, wt, extra


def _run_case(ops, c):
    """The case on the GPU -> dict of CPU tensors."""
    xs, wt, ex = _problem(c)
    b, h, w = c.bhw
    cin = sum(c.segs)
    if c.layout == "dense":
        xd = [x.to(DEV) for x in xs]
    else:                       # one half of a 512-channel tensor, the other half filled with a value that would show
        wide = torch.full((b, h, w, 512), 1e6, device=DEV)
        lo = c.layout == "lo"
        view = wide[..., :256] if lo else wide[..., 256:]
        view.copy_(xs[0].to(DEV))
        xd = [view]
    wp = torch.empty(c.cout, 9 * cin, device=DEV)
    ops.pack_conv_weight(wt.to(DEV), wp, cin)
    kw = {}
    if c.opt == "bias":
        kw["bias"] = ex["bias"].to(DEV)
    elif c.opt == "out_scale":
        kw["out_scale"] = 0.25
    elif c.opt == "ch_scale":
        kw["ch_scale"], kw["ch_shift"] = ex["ch_scale"].to(DEV), ex["ch_shift"].to(DEV)
    elif c.opt == "relu":
        kw["act"] = ops.ACT_RELU
    elif c.opt == "res":
        kw["res"], kw["act_res"] = ex["res"].to(DEV), ops.ACT_RELU
    out = {}
    if c.opt == "coords":
        c1, f4 = ex["coords"].to(DEV), torch.full((b, h, w, 4), 7.0, device=DEV)
        kw["ep_coords"] = (c1, f4)
    y = ops.conv2d(xd, wp, kw.pop("bias", None), c.cout, 3, 3, 1, (1, 1), **kw)
    torch.cuda.synchronize()
    out["y"] = y.cpu().clone()
    if c.opt == "coords":
        out["coords1"], out["flow4"] = c1.cpu(), f4.cpu()
    return out


def _run_all(ops):
    return {c.name: _run_case(ops, c) for c in CASES}


def _reference(c):
    """-> (y64 NHWC, bound NHWC): the float64 result with the case's option applied, and the bound of the module docstring."""
    xs, wt, ex = _problem(c)
    cin = sum(c.segs)
    x64 = torch.cat(xs, 3).double().permute(0, 3, 1, 2)
    w64 = wt.double()
    v = F.conv2d(x64, w64, padding=1).permute(0, 2, 3, 1)
    k = 9 * cin + 2
    e = (k * U / (1 - k * U)) * F.conv2d(x64.abs(), w64.abs(), padding=1).permute(0, 2, 3, 1)

    def rounded(v, e):          # one more rounded operation
        return v, e + U * (v.abs() + e)

    if c.opt == "bias":
        v, e = rounded(v + ex["bias"].double(), e)
    elif c.opt == "out_scale":
        v, e = rounded(v * 0.25, e * 0.25)
    elif c.opt == "ch_scale":
        s, t = ex["ch_scale"].double(), ex["ch_shift"].double()
        v, e = rounded(v * s, e * s.abs())
        v, e = rounded(v + t, e)
    elif c.opt == "relu":
        v = v.clamp_min(0)
    elif c.opt == "res":
        v, e = rounded(v + ex["res"].double(), e)
        v = v.clamp_min(0)
    return v, e


@pytest.fixture(scope="module")
def ops():
    from focusflow_official_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def references():
    return {c.name: _reference(c) for c in CASES}


@pytest.fixture(scope="module")
def shipped(ops):
    assert os.environ.get(SWITCH) in (None, "1"), f"{SWITCH} is set: this module tests the shipped route against {SWITCH}=0 itself"
    return _run_all(ops)


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    """The same cases in a child process with the switch at 0 (it is read once per process)."""
    path = str(tmp_path_factory.mktemp("conv_small") / "off.pt")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), path], cwd=ROOT, env=dict(os.environ, **{SWITCH: "0"}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(path)


def _check(c, got, ref):
    y64, bound = ref
    y = got["y"].double()
    assert y.shape == y64.shape
    if c.opt == "nonfinite":
        assert torch.equal(torch.isnan(y), torch.isnan(y64)), "NaN outputs are not exactly the pixels that see the NaN"
        inf = torch.isinf(y64)
        assert torch.equal(y[inf], y64[inf]), "Inf outputs"
        ok = torch.isfinite(y64)
        y, y64, bound = y[ok], y64[ok], bound[ok]
        assert ok.sum() > ok.numel() - 20 and torch.isfinite(bound).all()
    err = (y - y64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{c.name}: max err {float(err.max()):.3g}, largest err / bound {worst:.3g}")
    assert bool((err <= bound).all()), f"{c.name}: err / bound up to {worst:.3g}"
    if c.opt == "coords":       # the kernel's own delta, the two steps separately rounded: bit for bit
        _, _, ex = _problem(c)
        b, h, w = c.bhw
        c1 = ex["coords"] + got["y"]
        grid = torch.stack(torch.meshgrid(torch.arange(w, dtype=torch.float32), torch.arange(h, dtype=torch.float32), indexing="xy"), -1)
        assert torch.equal(got["coords1"], c1), "coords1 != coords + delta"
        assert torch.equal(got["flow4"][..., :2], c1 - grid), "flow4_next != coords1 - grid"
        assert torch.equal(got["flow4"][..., 2:], torch.zeros(b, h, w, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_shipped_route_against_fp64(name, shipped, references):
    _check(BY_NAME[name], shipped[name], references[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_switch_at_0_against_fp64(name, switched_off, references):
    _check(BY_NAME[name], switched_off[name], references[name])


@pytest.mark.gpu
def test_the_switch_switches(shipped, switched_off):
    """Below 128 channels both processes ran the run kernel: bit-identical (NaN included).  From 128 on the shipped route is
    the tile kernel, whose sums are taken in another order: some bits differ in every such case with more than a few outputs."""
    for c in CASES:
        same = all(torch.equal(shipped[c.name][k].view(torch.int32), switched_off[c.name][k].view(torch.int32)) for k in shipped[c.name])
        if sum(c.segs) < TILE_MIN_CIN:
            assert same, f"{c.name}: declined by the tile kernel, yet not the run kernel's bits"
        elif c.bhw[1] * c.bhw[2] >= 64:
            assert not same, f"{c.name}: bit-identical to the run kernel - did the tile kernel run?"


def test_threshold_still_stands_in_the_source():
    with open(os.path.join(ROOT, "focusflow_official_amd", "csrc", "conv_small.hip")) as f:
        text = f.read()
    assert f"if (tile_enabled && cin >= {TILE_MIN_CIN})" in text and f'getenv("{SWITCH}")' in text


if __name__ == "__main__":      # the child of `switched_off`
    from focusflow_official_amd import ops as _ops
    torch.save(_run_all(_ops), sys.argv[1])
