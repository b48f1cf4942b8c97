"""The entry of a stride-2 residual block as one launch (csrc/conv_s2_pair.hip, ff_conv_s2_pair_fwd): conv1 (3x3, stride 2,
pad 1) and the shortcut (1x1, stride 2, pad 0) read the same input - the shortcut is the 3x3's centre tap - so one kernel
stages the input patch once and writes both outputs, with bias / folded BatchNorm / activation and the InstanceNorm statistics
of both from its epilogue.

Shapes (B, H, W, Cin -> Cout): (2, 16, 32, 64 -> 96) whole 4 x 16 output tiles; (3, 37, 45, 64 -> 96) an odd plane whose 19 x 23
output is ragged both ways and whose last row and column meet the padding; (2, 24, 34, 96 -> 128) an output 17 wide, one column
into a new tile; (1, 9, 33, 96 -> 128) exactly one patch.
Bounds: the operator against float64 at the project's close(rtol=2e-5) (atol 2e-5 max(1, max|ref|)) for f16x3 - the three-term
f16 product carries 22 bits - and 4e-3 max(1, max|ref|) for the one-term f16 format; statistics at test_stem_conv_kernel's
tolerances, a nearly constant plane at test_instance_norm_statistics_from_the_conv_epilogue's; whole forwards at 1e-4 px on / off
and 1e-3 px against the oracle."""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 16, 32, 64, 96), (3, 37, 45, 64, 96), (2, 24, 34, 96, 128), (1, 9, 33, 96, 128)]
SENTINEL = -12345.678


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_conv_s2_pair_kernel_compiles_without_scratch():
    """CPU side: both term counts, 6 and 8 waves, for gfx950 use no scratch memory (tests/test_kernel_resources.py's method)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "conv_s2_pair.hip"))
    assert len(kernels) == 4, kernels
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"conv_s2_pair.hip: kernels with scratch (bytes per lane): {spilled}"
    assert all(int(k["Occupancy"]) >= 4 for k in kernels), kernels       # three 6-wave blocks or two 8-wave blocks per CU


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


_CASES = {}


def _case(shape):
    """Inputs, parameters and the float64 references of one shape - computed once, shared and left unchanged."""
    if shape not in _CASES:
        b, h, w, cin, cout = shape
        g = torch.Generator().manual_seed(1000 * h + w + cin)
        x = torch.randn(b, cin, h, w, generator=g) * 1.5 + 0.25
        w3 = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        w1 = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
        b3, b1, s3, h3 = (torch.randn(cout, generator=g) for _ in range(4))
        ref_a = F.conv2d(x.double(), w3.double(), b3.double(), stride=2, padding=1)
        ref_d = F.conv2d(x.double(), w1.double(), b1.double(), stride=2)
        _CASES[shape] = dict(x=x, w3=w3, w1=w1, b3=b3, b1=b1, s3=s3, h3=h3, ref_a=ref_a, ref_d=ref_d)
    return _CASES[shape]


def _frag(wt, fmt):
    """OIHW -> (split rows in fragment order, what PackedConv.frag() caches)."""
    from focusflow_official_amd import ops
    cout, cin, kh, kw = wt.shape
    rows = torch.empty(cout, kh * kw * cin, device=DEV)
    ops.pack_conv_weight(wt.to(DEV), rows, cin)
    return ops.pack_frag16(ops.pack_split(rows), cout)


def _sliced_input(x):
    """x as a channel slice of a wider buffer: ld = C + 32."""
    b, c, h, w = x.shape
    buf = torch.full((b, h, w, c + 32), 7.0, device=DEV)
    buf[..., 16:16 + c] = nhwc(x)
    return buf, buf[..., 16:16 + c]


def _guarded(b, ho, wo, cout):
    """An output view inside a buffer pre-filled with a finite sentinel: 8 channels and one batch element each side."""
    buf = torch.full((b + 2, ho, wo, cout + 16), SENTINEL, device=DEV)
    return buf, buf[1:b + 1, :, :, 8:8 + cout]


def _guards_intact(buf, b, cout):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:b + 1, :, :, 8:8 + cout] = False
    return bool((buf[mask].view(torch.int32) == torch.tensor(SENTINEL, device=DEV).view(torch.int32)).all())


@gpu
@pytest.mark.parametrize("fmt", ["f16x3", "f16"])
@pytest.mark.parametrize("mode", ["bias+stats", "scale+shift+relu"])
@pytest.mark.parametrize("shape", SHAPES)
def test_operator_against_float64(shape, mode, fmt):
    from focusflow_official_amd import ops
    b, h, w, cin, cout = shape
    cs = _case(shape)
    w_fmt = {"f16x3": 1, "f16": 2}[fmt]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert cs["ref_a"].shape == (b, cout, ho, wo) and cs["ref_d"].shape == (b, cout, ho, wo)
    xbuf, x = _sliced_input(cs["x"])
    w3f, w1f = _frag(cs["w3"], w_fmt), _frag(cs["w1"], w_fmt)
    b3, b1 = cs["b3"].to(DEV), cs["b1"].to(DEV)
    ref_a, ref_d = cs["ref_a"], cs["ref_d"]
    kw = dict(want_stats=True)
    if mode != "bias+stats":
        s3, h3 = cs["s3"], cs["h3"]
        ref_a = torch.relu(ref_a * s3.double().view(1, -1, 1, 1) + h3.double().view(1, -1, 1, 1))
        kw = dict(scale=(s3.to(DEV), None), shift=(h3.to(DEV), None), act=(ops.ACT_RELU, ops.ACT_NONE))
    runs = []
    for _ in range(2):
        (buf_a, ya), (buf_d, yd) = _guarded(b, ho, wo, cout), _guarded(b, ho, wo, cout)
        res = ops.conv_s2_pair(x, w3f, w1f, b3, b1, cout, w_fmt, out=(ya, yd), **kw)
        torch.cuda.synchronize()
        assert _guards_intact(buf_a, b, cout) and _guards_intact(buf_d, b, cout), "a store outside the output view"
        runs.append(res)
    first, second = runs
    for t0, t1 in zip(first, second):
        assert torch.equal(t0, t1), "a second call differs from the first"
    a, d = (first[0], first[2]) if mode == "bias+stats" else first
    assert second[0].data_ptr() == ya.data_ptr() and tuple(a.shape) == (b, ho, wo, cout)          # written where the caller said
    # f16x3: close(rtol=2e-5, atol=2e-5 max(1, max|ref|)); f16: 4e-3 max(1, max|ref|)
    tol = (lambda ref: dict(rtol=2e-5)) if fmt == "f16x3" else (lambda ref: dict(rtol=0, atol=4e-3 * max(1.0, float(ref.abs().max()))))
    e_a = float((nchw(a).double() - ref_a).abs().max())
    e_d = float((nchw(d).double() - ref_d).abs().max())
    print(f"conv_s2_pair {shape} {mode} {fmt}: max|err| 3x3 {e_a:.3e} (max|ref| {float(ref_a.abs().max()):.3e}), 1x1 {e_d:.3e} (max|ref| {float(ref_d.abs().max()):.3e})")
    close(nchw(a), ref_a, what=f"3x3 {shape} {mode} {fmt}", **tol(ref_a))
    close(nchw(d), ref_d, what=f"1x1 {shape} {mode} {fmt}", **tol(ref_d))
    assert bool((xbuf[..., :16] == 7.0).all()) and bool((xbuf[..., 16 + cin:] == 7.0).all())


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_statistics_from_the_epilogue(shape):
    """ff_norm_stats_finish of the launch's parts against the float64 mean and variance (test_stem_conv_kernel's tolerances)."""
    from focusflow_official_amd import ops
    b, h, w, cin, cout = shape
    cs = _case(shape)
    a, st_a, d, st_d = ops.conv_s2_pair(nhwc(cs["x"]), _frag(cs["w3"], 1), _frag(cs["w1"], 1), cs["b3"].to(DEV), cs["b1"].to(DEV), cout, 1, want_stats=True)
    n = a.shape[1] * a.shape[2]
    for name, st, ref in (("3x3", st_a, cs["ref_a"]), ("1x1", st_d, cs["ref_d"])):
        assert tuple(st.shape) == (b, cout, 2) and st.dtype == torch.float64
        close((st[..., 0] / n).cpu(), ref.mean(dim=(2, 3)), rtol=1e-5, atol=1e-6, what=f"mean of the {name} output {shape}")
        close((st[..., 1] / n - (st[..., 0] / n) ** 2).cpu(), ref.var(dim=(2, 3), unbiased=False), rtol=2e-4, atol=1e-7, what=f"variance of the {name} output {shape}")


@gpu
def test_statistics_of_a_nearly_constant_plane_and_parts_count():
    """A large bias over tiny variation (mean ~ 100, sigma ~ 1e-4): the pivot keeps the fp32 partial sums free of cancellation -
    test_instance_norm_statistics_from_the_conv_epilogue's bound for that case; the parts the kernel writes on a ragged shape
    are the host helper's count."""
    import ctypes as C
    from focusflow_official_amd import _hip, ops
    b, h, w, cin, cout = 3, 37, 45, 64, 96
    g = torch.Generator().manual_seed(3)
    x = torch.randn(b, h, w, cin, generator=g).to(DEV)
    w3 = torch.randn(cout, cin, 3, 3, generator=g) / 24 * 1e-4
    w1 = torch.randn(cout, cin, 1, 1, generator=g) / 8 * 1e-4
    bias = torch.full((cout,), 100.0, device=DEV)
    a, st_a, d, st_d = ops.conv_s2_pair(x, _frag(w3, 1), _frag(w1, 1), bias, bias, cout, 1, want_stats=True)
    n = a.shape[1] * a.shape[2]
    for name, y, st in (("3x3", a, st_a), ("1x1", d, st_d)):
        yd = y.double()
        var_true = yd.var(dim=(1, 2), unbiased=False)
        var = st[..., 1] / n - (st[..., 0] / n) ** 2
        assert float(var_true.max()) < 1e-4 and float(yd.mean()) > 99
        close(var.cpu(), var_true.cpu(), rtol=0, atol=2e-11, what=f"variance of a nearly constant plane ({name})")   # 2^-52 * mean^2
    # parts: one entry per 4 x 16 output tile - every entry of a buffer of exactly that size is written, none beyond it
    nparts = ops.conv_s2_pair_stats_parts(h, w)
    assert nparts == 5 * 2                                    # 19 x 23 output
    guard = 64
    parts = [torch.full((b * nparts * cout * 4 + guard,), SENTINEL, device=DEV) for _ in range(2)]
    ya, yd = torch.empty(b, 19, 23, cout, device=DEV), torch.empty(b, 19, 23, cout, device=DEV)
    p = _hip.FFConvS2Pair()
    p.x, p.x_ld, p.B, p.H, p.W, p.Cin, p.Cout = x.data_ptr(), cin, b, h, w, cin, cout
    p.k[0], p.stride[0], p.pad[0], p.k[1], p.stride[1], p.pad[1] = 3, 2, 1, 1, 2, 0
    wf = (_frag(w3, 1), _frag(w1, 1))
    p.w3_frag, p.w1_frag, p.w_format = wf[0].data_ptr(), wf[1].data_ptr(), 1
    for i, y in enumerate((ya, yd)):
        p.y[i], p.y_ld[i], p.bias[i], p.stats_part[i] = y.data_ptr(), cout, bias.data_ptr(), parts[i].data_ptr()
    _hip.call("ff_conv_s2_pair_fwd", C.byref(p), None)
    torch.cuda.synchronize()
    for t in parts:
        body, tail = t[:-guard].view(b, nparts, cout, 4), t[-guard:]
        assert bool((tail == SENTINEL).all()) and bool((body != SENTINEL).all())
        assert float(body[..., 3].sum(1).min()) == float(body[..., 3].sum(1).max()) == 19 * 23      # every pixel counted once


def _block_encoder(norm, seed=0):
    """A plain encoder (cce.BasicEncoder) whose stride-2 blocks' parameters are random."""
    from focusflow_official_amd import cce
    torch.manual_seed(200 + seed)
    enc = cce.BasicEncoder(3, 128, norm_fn=norm)
    if norm == "batch":
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for m in enc.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                    m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                    m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                    m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    return enc.to(DEV).eval()


def _count_calls(monkeypatch):
    from focusflow_official_amd import ops
    calls, real = [], ops.conv_s2_pair

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "conv_s2_pair", counted)
    return calls


@gpu
def test_refusals_and_fall_backs(monkeypatch):
    from focusflow_official_amd import cce, ops
    from focusflow_official_amd._hip import FocusFlowHipError
    g = torch.Generator().manual_seed(9)
    w3, w1 = torch.randn(96, 64, 3, 3, generator=g) / 24, torch.randn(96, 64, 1, 1, generator=g) / 8
    w3f, w1f = _frag(w3, 1), _frag(w1, 1)
    bias = torch.zeros(96, device=DEV)
    x = torch.randn(1, 16, 32, 64, generator=g).to(DEV)
    ops.conv_s2_pair(x, w3f, w1f, bias, bias, 96, 1)                                        # the plain call is taken
    x48 = torch.zeros(1, 16, 32, 48, device=DEV)
    assert not ops.conv_s2_pair_inputs_ok(x48, 96)
    with pytest.raises(FocusFlowHipError, match="Cin = 48"):
        ops.conv_s2_pair(x48, w3f, w1f, bias, bias, 96, 1)
    wide = torch.zeros(1, 16, 32, 96, device=DEV)
    assert not ops.conv_s2_pair_inputs_ok(wide[..., 1:65], 96)
    with pytest.raises(FocusFlowHipError, match="alignment"):
        ops.conv_s2_pair(wide[..., 1:65], w3f, w1f, bias, bias, 96, 1)                     # a view that starts 4 bytes into a pixel
    with pytest.raises(FocusFlowHipError, match="w_format"):
        ops.conv_s2_pair(x, w3f, w1f, bias, bias, 96, 0)                                    # fp32 rows: not this kernel's
    with pytest.raises(FocusFlowHipError, match="stride"):
        ops.conv_s2_pair(x, w3f, w1f, bias, bias, 96, 1, kernels=((3, 1, 1), (1, 1, 0)))
    with pytest.raises(FocusFlowHipError, match="aliases"):
        ops.conv_s2_pair(x, w3f, w1f, bias, bias, 96, 1, out=(x.view(-1)[:8 * 16 * 96].view(1, 8, 16, 96), torch.empty(1, 8, 16, 96, device=DEV)))
    # _block: what the entry cannot take runs the old route, bit for bit what the switch off gives
    calls = _count_calls(monkeypatch)
    enc = _block_encoder("instance", seed=1)
    blk = enc.layer2[0]

    def run(xin, grad=False):
        del calls[:]
        ops.begin_forward(DEV)
        with torch.enable_grad() if grad else torch.no_grad():
            out = enc._block(blk, xin)
        return len(calls), out

    n, y_on = run(x)
    assert n == 1
    monkeypatch.setattr(cce, "_S2_PAIR", False)
    n, y_off = run(x)
    assert n == 0
    monkeypatch.setattr(cce, "_S2_PAIR", True)
    close(y_on.cpu(), y_off.cpu(), rtol=2e-5, what="block entry as one launch against the old route")
    # (a misaligned view has no old route either: ff_conv2d_fwd refuses it as well)
    blk48 = cce.ResidualBlock(48, 96, "instance", stride=2).to(DEV)      # Cin 48: refused by the input check, the old route runs
    x48 = torch.randn(1, 16, 32, 48, generator=g).to(DEV)
    del calls[:]
    with torch.no_grad():
        y48 = enc._block(blk48, x48)
        assert len(calls) == 0
        monkeypatch.setattr(cce, "_S2_PAIR", False)
        assert torch.equal(enc._block(blk48, x48), y48)
    monkeypatch.setattr(cce, "_S2_PAIR", True)
    monkeypatch.setattr(ops, "_conv_precision", "fp32")       # fp32 rows
    n, y32 = run(x)
    assert n == 0
    monkeypatch.setattr(cce, "_S2_PAIR", False)
    assert torch.equal(run(x)[1], y32)
    monkeypatch.setattr(cce, "_S2_PAIR", True)
    monkeypatch.setattr(ops, "_conv_precision", "f16x3")
    assert run(x, grad=True)[0] == 0                           # a grad-enabled call keeps the separate launches
    assert run(x)[0] == 1
    none = _block_encoder("none")
    del calls[:]
    with torch.no_grad():
        none._block(none.layer2[0], x)
    assert len(calls) == 0                                     # norm_fn='none' keeps its launches


@gpu
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_encoders_on_against_off(norm, monkeypatch):
    from focusflow_official_amd import cce, ops
    calls = _count_calls(monkeypatch)
    torch.manual_seed(300)
    enc = cce.BasicParallelFusionLayer(3, 3, output_dim=256, norm_fn=norm, cfg=_cfg()).to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    img, msk = (torch.randn(2, 128, 144, 4, generator=g).to(DEV) for _ in range(2))

    def run():
        del calls[:]
        ops.begin_forward(DEV)
        with torch.no_grad():
            out = enc(img, msk)
        assert out.shape == (2, 16, 18, 256)
        return len(calls), out.clone()

    n, y = run()
    assert n == 4                                             # stages 2 and 3 of the frame and the mask branch
    monkeypatch.setattr(cce, "_S2_PAIR", False)
    n, y_old = run()
    assert n == 0
    print(f"encoder ({norm}): max |one launch - old route| {float((y - y_old).abs().max()):.3e}, max|out| {float(y_old.abs().max()):.3e}")
    close(y.cpu(), y_old.cpu(), rtol=2e-5, what=f"encoder ({norm}) with the block entries as one launch against the old route")


@gpu
def test_whole_forward_on_off_oracle_and_graph(det_sd, monkeypatch):
    from focusflow_official_amd import cce
    from focusflow_official_amd.graph import GraphedForward
    from oracle import ffraft_ref as orc
    from test_hip_parity import _model
    calls = _count_calls(monkeypatch)
    inp = [t.to(DEV) for t in orc.shifted_pair(2, 128, 144, seed=17)]
    m = _model(det_sd)
    assert cce._S2_PAIR
    with torch.no_grad():
        lo_n, up_n = [t.clone() for t in m(*inp, raft_iters=3, test_mode=True)]
        assert len(calls) == 8                               # feature and context encoder: two branches, two stages each
        monkeypatch.setattr(cce, "_S2_PAIR", False)
        lo_o, up_o = [t.clone() for t in m(*inp, raft_iters=3, test_mode=True)]
        assert len(calls) == 8
        monkeypatch.setattr(cce, "_S2_PAIR", True)
        ref_lo, ref_up = orc.ffraft_forward(det_sd, *[t.cpu() for t in inp], raft_iters=3, test_mode=True)
    print(f"flow_up: one launch vs old route {float((up_n - up_o).abs().max()):.3e} px, vs oracle {float((up_n.cpu() - ref_up).abs().max()):.3e} px, "
          f"old route vs oracle {float((up_o.cpu() - ref_up).abs().max()):.3e} px")
    close(up_n.cpu(), up_o.cpu(), rtol=0, atol=1e-4, what="block entries as one launch on vs off")
    close(up_n.cpu(), ref_up, rtol=0, atol=1e-3, what="block entries as one launch vs oracle")
    close(up_o.cpu(), ref_up, rtol=0, atol=1e-3, what="old route vs oracle")
    gf = GraphedForward(m, inp, raft_iters=3)
    n_before = len(calls)
    g_lo, g_up = [t.clone() for t in gf(*inp)]
    torch.cuda.synchronize()
    assert n_before == 8 + 8 * 4                             # three warm-up forwards and the capture took the route
    assert torch.equal(g_up, up_n) and torch.equal(g_lo, lo_n), f"graph vs eager: max |diff| {float((g_up - up_n).abs().max()):.3e}"


@gpu
def test_block_entry_follows_the_parameters():
    """An in-place update bumps the parameter's version: the packed weights are rebuilt; a write through .data needs
    invalidate_packed, which drops them (and the folded BatchNorm) as well."""
    from focusflow_official_amd import cce, ops
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 16, 32, 64, generator=g).to(DEV)

    def ref64(blk):
        """extractor.py:48-56 for a stride-2 block with eval BatchNorm, float64."""
        xd = x.double().cpu().permute(0, 3, 1, 2)
        cv = lambda c, t, **k: F.conv2d(t, c.weight.detach().double().cpu(), c.bias.detach().double().cpu(), **k)     # noqa: E731
        bn = lambda n, t: F.batch_norm(t, n.running_mean.double().cpu(), n.running_var.double().cpu(), n.weight.detach().double().cpu(),    # noqa: E731
                                       n.bias.detach().double().cpu(), False, 0.0, n.eps)
        y = torch.relu(bn(blk.norm1, cv(blk.conv1, xd, stride=2, padding=1)))
        y = torch.relu(bn(blk.norm2, cv(blk.conv2, y, padding=1)))
        return torch.relu(bn(blk.norm3, cv(blk.downsample[0], xd, stride=2)) + y)

    enc = _block_encoder("batch", seed=2)
    blk = enc.layer2[0]

    def run():
        ops.begin_forward(DEV)
        with torch.no_grad():
            return enc._block(blk, x)

    r0 = ref64(blk)
    close(nchw(run()), r0, rtol=2e-5, what="before the update")
    with torch.no_grad():
        blk.downsample[0].weight.mul_(1.5)
        blk.conv1.bias.add_(0.25)
    r1 = ref64(blk)
    assert float((r1 - r0).abs().max()) > 0.1
    close(nchw(run()), r1, rtol=2e-5, what="after the in-place update")
    blk.conv1.weight.data.mul_(0.5)                          # through .data: no version bump - invalidate_packed's case
    blk.norm3.running_mean.data.add_(0.5)
    r2 = ref64(blk)
    assert float((r2 - r1).abs().max()) > 0.1
    assert cce.invalidate_packed(enc) > 0
    close(nchw(run()), r2, rtol=2e-5, what="after invalidate_packed")
