"""The encoders' output stage as one launch (csrc/encoder_tail.hip, ff_encoder_tail_fwd): fusion4, conv2 / mask_conv2 and
fusion5 of a Condition Control Encoder are linear from end to end (parallel_fusion.py:237-242), so inference runs them as ONE
1x1 convolution 256 -> 256 over the segments [x | m] whose weight cce.BasicParallelFusionLayer._tail_weights composes from the ten
parameters in float64.

Shapes: 128 + 128 -> 256 channels are fixed; (1, 6, 10) is 60 pixels - not a whole 64-pixel tile; (3, 8, 16) several images of
whole tiles with per-image coefficient tables; (2, 16, 12) three tiles per image; (3, 5, 9) tiles that straddle images (45 pixels
per image: the loader indexes the coefficient tables per item) with a partial last tile.
Bounds: the operator against float64 at the project's close(rtol=2e-5) (atol 2e-5 max(1, max|ref|)) - the composed weight is
rounded once, the three-term f16 product carries 22 bits; lazy against materialised inputs and graph replay against eager
bit for bit; whole forwards at the bounds of test_forward_with_and_without_the_fusion_unit_kernel (1e-4 px on / off, 1e-3 px
against the oracle)."""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 6, 10), (3, 8, 16), (2, 16, 12), (3, 5, 9)]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_encoder_tail_kernel_compiles_without_scratch():
    """CPU side: both instances for gfx950 use no scratch memory (tests/test_kernel_resources.py's method)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "encoder_tail.hip"))
    assert len(kernels) == 2, kernels
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"encoder_tail.hip: kernels with scratch (bytes per lane): {spilled}"
    assert all(int(k["Occupancy"]) >= 2 for k in kernels), kernels       # two 64 KB blocks per CU


# ---------------------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"
gpu = pytest.mark.gpu


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous()


def close(a, b, rtol=2e-5, atol=None, what=""):
    """tests/test_hip_parity.py's close(); returns the largest absolute error for the record."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if atol is None:
        atol = rtol * max(1.0, float(np.abs(b).max()))
    err = np.abs(a - b) - rtol * np.abs(b)
    assert err.max() <= atol, f"{what}: max violation {err.max():.3e} (atol {atol:.3e}), max|ref| {np.abs(b).max():.3e}"
    return float(np.abs(a - b).max())


def _cfg(ft="1x1conv"):
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE=ft, LOAD_MODULE_TO_BRANCH=False))


def _tail_convs(enc):
    f4 = enc.fusion4
    return [f4.mask2img.conv, enc.conv2, enc.mask_conv2, enc.fusion5.mask2img.conv] + ([f4.img2mask.conv] if f4.img2mask is not None else [])


def _encoder(ft="1x1conv", norm="batch", seed=0):
    """A CCE encoder whose output-stage parameters (weights and biases) are random."""
    from focusflow_official_amd import cce
    torch.manual_seed(100 + seed)
    enc = cce.BasicParallelFusionLayer(3, 3, output_dim=256, norm_fn=norm, cfg=_cfg(ft))
    if ft != "concat":
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for cv in _tail_convs(enc):
                cv.weight.copy_(torch.randn(cv.weight.shape, generator=g) / cv.in_channels ** 0.5)
                cv.bias.copy_(torch.randn(cv.bias.shape, generator=g))
    return enc.to(DEV).eval()


def _ref64(enc, x, m):
    """parallel_fusion.py:237-242 step by step in float64 (NCHW, CPU)."""
    cv = lambda c, t: F.conv2d(t, c.weight.detach().double().cpu(), c.bias.detach().double().cpu())     # noqa: E731
    x, m = x.double(), m.double()
    f4 = enc.fusion4
    x4 = x + cv(f4.mask2img.conv, m)
    m4 = m + cv(f4.img2mask.conv, x) if f4.img2mask is not None else m
    m5, x5 = cv(enc.mask_conv2, m4), cv(enc.conv2, x4)
    return x5 + cv(enc.fusion5.mask2img.conv, m5)


def _old_route(enc, x, m):
    """The launches the kernel replaces: the last five lines of cce.BasicParallelFusionLayer.forward."""
    from focusflow_official_amd import fn
    m, x = enc.fusion4.run(m, x)
    m, x = fn.conv(enc._mout, m), enc._run_out(x)
    m, x = enc.fusion5.run(m, x)
    return x


def _inputs(b, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 13 * h + b)
    return torch.randn(b, 128, h, w, generator=g) * 1.5 + 0.2, torch.randn(b, 128, h, w, generator=g) * 1.5 - 0.1


@gpu
@pytest.mark.parametrize("ft", ["1x1conv", "1x1conv-unidirection"])
@pytest.mark.parametrize("shape", SHAPES)
def test_operator_against_float64(shape, ft):
    from focusflow_official_amd import ops
    b, h, w = shape
    enc = _encoder(ft, seed=h)
    x, m = _inputs(b, h, w)
    ref = _ref64(enc, x, m)
    with torch.no_grad():
        tail = enc._tail_weights()
        assert tail is not None
        y = ops.encoder_tail(nhwc(x), nhwc(m), tail[0], tail[1], ops.w_format())
        old = _old_route(enc, nhwc(x), nhwc(m))
    assert y.shape == (b, h, w, 256)
    e_old = float((nchw(old).double() - ref).abs().max())
    e_new = float((nchw(y).double() - ref).abs().max())
    print(f"encoder tail {shape} {ft}: max|err| one launch {e_new:.3e}, four launches {e_old:.3e}, max|ref| {float(ref.abs().max()):.3e}")
    close(nchw(y), ref, rtol=2e-5, what=f"encoder tail {shape} {ft}")


@gpu
@pytest.mark.parametrize("kind", ["stage", "stem", "mixed"])
@pytest.mark.parametrize("shape", SHAPES)
def test_lazy_loader_is_norm_apply(shape, kind):
    """LazyAct inputs against ops.norm_apply's materialised outputs of the same ingredients: the same kernel, so any difference
    would be the loader's.  stage: relu(res + relu(norm(t))) on both branches; stem: relu(norm(t)); mixed: one lazy, one plain."""
    from focusflow_official_amd import ops
    b, h, w = shape
    enc = _encoder(seed=3)
    g = torch.Generator().manual_seed(7 * h + b)
    td = [nhwc(torch.randn(b, 128, h, w, generator=g) * 2 + 0.3) for _ in range(2)]
    rd = [nhwc(torch.randn(b, 128, h, w, generator=g)) for _ in range(2)]
    res = rd if kind != "stem" else [None, None]
    with torch.no_grad():
        tail = enc._tail_weights()
        stats = [ops.norm_stats(v, per_sample=True) for v in td]
        mat = [ops.norm_apply(td[i].clone(), stats[i], True, 1e-5, act=ops.ACT_RELU, res=res[i]) for i in range(2)]
        lazy = [ops.LazyAct(td[i].clone(), stats[i], h * w, 1e-5, ops.ACT_RELU, res[i]) for i in range(2)]
        if kind == "mixed":
            lazy[1] = mat[1].clone()
        assert ops.encoder_tail_inputs_ok(*lazy)
        y_lazy = ops.encoder_tail(lazy[0], lazy[1], tail[0], tail[1], ops.w_format())
        y_mat = ops.encoder_tail(mat[0], mat[1], tail[0], tail[1], ops.w_format())
    assert torch.isfinite(y_mat).all()
    assert torch.equal(y_lazy, y_mat), f"max |diff| {float((y_lazy - y_mat).abs().max()):.3e}"


@gpu
def test_kernel_refuses_what_it_cannot_read():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    enc = _encoder()
    with torch.no_grad():
        wf, bias = enc._tail_weights()
    wide = torch.zeros(1, 8, 16, 256, device=DEV)
    assert not ops.encoder_tail_inputs_ok(wide[..., :128], wide[..., 128:])
    with pytest.raises(FocusFlowHipError, match="contiguous"):
        ops.encoder_tail(wide[..., :128], wide[..., 128:], wf, bias, 1)          # channel slices: ld != C
    x64 = torch.zeros(1, 8, 16, 64, device=DEV)
    assert not ops.encoder_tail_inputs_ok(x64, x64.clone())
    with pytest.raises(FocusFlowHipError, match="C = 64"):
        ops.encoder_tail(x64, x64.clone(), wf, bias, 1)
    x = torch.zeros(1, 8, 16, 128, device=DEV)
    with pytest.raises(FocusFlowHipError, match="w_format"):
        ops.encoder_tail(x, x.clone(), wf, bias, 0)                                # fp32 rows: not this kernel's


def _count_calls(monkeypatch):
    from focusflow_official_amd import ops
    calls, real = [], ops.encoder_tail

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "encoder_tail", counted)
    return calls


@gpu
def test_fall_backs_take_the_old_route(monkeypatch):
    from focusflow_official_amd import cce, ops
    calls = _count_calls(monkeypatch)
    g = torch.Generator().manual_seed(5)
    img, msk = (torch.randn(2, 32, 48, 4, generator=g).to(DEV) for _ in range(2))

    def run(enc, grad=False):
        del calls[:]
        ops.begin_forward(DEV)
        with torch.enable_grad() if grad else torch.no_grad():
            out = enc(img, msk)
        assert out.shape == (2, 4, 6, 256)
        return len(calls), out

    for norm in ("batch", "instance"):       # plain inputs (BatchNorm folded) and lazy ones
        enc = _encoder(norm=norm, seed=1)
        n, y = run(enc)
        assert n == 1
        monkeypatch.setattr(cce, "_ENCODER_TAIL", False)
        n, y_old = run(enc)
        assert n == 0
        monkeypatch.setattr(cce, "_ENCODER_TAIL", True)
        close(y.cpu(), y_old.cpu(), rtol=2e-5, what=f"encoder ({norm}) with the stage as one launch against the old route")
        assert run(enc, grad=True)[0] == 0                   # a grad-enabled call records the reference's five steps
    assert run(_encoder("1x1conv-unidirection"))[0] == 1
    assert run(_encoder("concat"))[0] == 0
    monkeypatch.setattr(ops, "_conv_precision", "fp32")
    assert run(_encoder(seed=2))[0] == 0
    monkeypatch.setattr(ops, "_conv_precision", "f16x3")
    # every single weight inside the split format's limit, the composed one (Wx A4: ~ 2000^2 larger) beyond it
    enc = _encoder(seed=1)
    with torch.no_grad():
        enc.conv2.weight.mul_(2000.0)
        enc.fusion4.mask2img.conv.weight.mul_(2000.0)
        assert float(enc.conv2.weight.abs().max()) < 4094 and float(enc.fusion4.mask2img.conv.weight.abs().max()) < 4094
    assert run(enc)[0] == 0 and enc._tail_weights() is None


@gpu
def test_composed_weight_follows_the_parameters():
    """An in-place update bumps the parameter's version: the composed weight is rebuilt; invalidate_packed drops it as well."""
    from focusflow_official_amd import cce, ops
    enc = _encoder(seed=4)
    x, m = _inputs(2, 8, 16, seed=4)
    with torch.no_grad():
        t0 = enc._tail_weights()
        assert enc._tail_weights() is t0                     # cached
        y0 = ops.encoder_tail(nhwc(x), nhwc(m), t0[0], t0[1], ops.w_format())
        close(nchw(y0), _ref64(enc, x, m), rtol=2e-5, what="before the update")
        ref0 = _ref64(enc, x, m)
        enc.mask_conv2.weight.mul_(1.5)
        enc.fusion5.mask2img.conv.bias.add_(0.25)
        t1 = enc._tail_weights()
        assert t1 is not t0
        y1 = ops.encoder_tail(nhwc(x), nhwc(m), t1[0], t1[1], ops.w_format())
        ref1 = _ref64(enc, x, m)
        assert float((ref1 - ref0).abs().max()) > 0.1
        close(nchw(y1), ref1, rtol=2e-5, what="after the update")
        enc.conv2.weight.data.mul_(0.5)                      # through .data: no version bump - invalidate_packed's case
        assert cce.invalidate_packed(enc) > 0
        t2 = enc._tail_weights()
        assert t2 is not t1
        y2 = ops.encoder_tail(nhwc(x), nhwc(m), t2[0], t2[1], ops.w_format())
        close(nchw(y2), _ref64(enc, x, m), rtol=2e-5, what="after invalidate_packed")


@gpu
def test_whole_forward_on_off_oracle_and_graph(det_sd, monkeypatch):
    from focusflow_official_amd import cce
    from focusflow_official_amd.graph import GraphedForward
    from oracle import ffraft_ref as orc
    from test_hip_parity import _model
    calls = _count_calls(monkeypatch)
    inp = [t.to(DEV) for t in orc.shifted_pair(2, 128, 144, seed=17)]
    m = _model(det_sd)
    assert cce._ENCODER_TAIL
    with torch.no_grad():
        lo_n, up_n = [t.clone() for t in m(*inp, raft_iters=3, test_mode=True)]
        assert len(calls) == 2                               # feature and context encoder
        monkeypatch.setattr(cce, "_ENCODER_TAIL", False)
        lo_o, up_o = [t.clone() for t in m(*inp, raft_iters=3, test_mode=True)]
        assert len(calls) == 2
        monkeypatch.setattr(cce, "_ENCODER_TAIL", True)
        ref_lo, ref_up = orc.ffraft_forward(det_sd, *[t.cpu() for t in inp], raft_iters=3, test_mode=True)
    print(f"flow_up: one launch vs old route {float((up_n - up_o).abs().max()):.3e} px, vs oracle {float((up_n.cpu() - ref_up).abs().max()):.3e} px, "
          f"old route vs oracle {float((up_o.cpu() - ref_up).abs().max()):.3e} px")
    close(up_n.cpu(), up_o.cpu(), rtol=0, atol=1e-4, what="encoder tail on vs off")
    close(up_n.cpu(), ref_up, rtol=0, atol=1e-3, what="encoder tail on vs oracle")
    close(up_o.cpu(), ref_up, rtol=0, atol=1e-3, what="encoder tail off vs oracle")
    gf = GraphedForward(m, inp, raft_iters=3)
    n_before = len(calls)
    g_lo, g_up = [t.clone() for t in gf(*inp)]
    torch.cuda.synchronize()
    assert n_before == 2 + 2 * 4                             # three warm-up forwards and the capture took the route
    assert torch.equal(g_up, up_n) and torch.equal(g_lo, lo_n), f"graph vs eager: max |diff| {float((g_up - up_n).abs().max()):.3e}"
