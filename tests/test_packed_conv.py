"""cce.PackedConv over padded-piece inputs (`pieces`) and nn.ConvTranspose2d sources (`transposed`) - the two forms
FF-PWC's decoders need - against fp64 torch: forward at test_hip_pwc's tolerance, gradients through fn.conv at
test_hip_backward's.  The pad channels of the inputs hold finite non-zero values: the packed rows must have zero columns
there, and the input gradient of a pad channel is exactly zero."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_hip_backward import close as close_bwd
from test_hip_pwc import close as close_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=["fp32", "f16x3"])
def precision(request):
    from focusflow_official_amd import ops
    old = ops.conv_precision()
    ops.set_conv_precision(request.param)
    yield request.param
    ops.set_conv_precision(old)


def _nchw64(t_nhwc, real):
    return t_nhwc.detach().cpu().double()[..., real].permute(0, 3, 1, 2)


def test_pieces_forward_and_gradients(precision):
    from focusflow_official_amd import fn
    from focusflow_official_amd.cce import PackedConv
    torch.manual_seed(21)
    conv = nn.Conv2d(7, 6, 3, padding=1).to(DEV)
    pc = PackedConv([conv], pieces=[(5, 8), (2, 4)])
    assert pc.cin == pc.cin_pad == 12 and not pc.plain
    real, pads = [0, 1, 2, 3, 4, 8, 9], [5, 6, 7, 10, 11]
    x = torch.randn(1, 5, 7, 12, device=DEV).requires_grad_(True)
    gout = torch.randn(1, 5, 7, 6, device=DEV)
    y = fn.conv(pc, x)
    (y * gout).sum().backward()
    w64, b64 = conv.weight.detach().cpu().double().requires_grad_(True), conv.bias.detach().cpu().double().requires_grad_(True)
    x64 = _nchw64(x, real).requires_grad_(True)
    ref = F.conv2d(x64, w64, b64, padding=1)
    (ref * gout.cpu().double().permute(0, 3, 1, 2)).sum().backward()
    close_fwd(y.detach().cpu(), ref.detach().permute(0, 2, 3, 1), what=f"pieces forward ({precision})")
    assert conv.weight.grad.shape == conv.weight.shape
    close_bwd(conv.weight.grad.cpu(), w64.grad, what="pieces dW")
    close_bwd(conv.bias.grad.cpu(), b64.grad, what="pieces db")
    close_bwd(x.grad[..., real].cpu(), x64.grad.permute(0, 2, 3, 1), what="pieces dx")
    assert float(x.grad[..., pads].abs().max()) == 0.0
    with torch.no_grad():       # the launch without a tape gives the recorded forward's bits
        assert torch.equal(pc(x.detach()), y.detach())


def test_transposed_forward_and_gradients(precision):
    from focusflow_official_amd import fn, ops
    from focusflow_official_amd.cce import PackedConv
    torch.manual_seed(22)
    deconv = nn.ConvTranspose2d(6, 2, 4, 2, 1).to(DEV)
    pc = PackedConv([deconv], pieces=[(6, 8)], transposed=True)
    assert (pc.cout, pc.stride, pc.pad, pc.cin_pad) == (2, 1, (2, 2), 8) and not pc.plain
    x = torch.randn(1, 3, 5, 8, device=DEV)
    gout = torch.randn(1, 6, 10, 2, device=DEV)
    y = fn.conv(pc, ops.dilate2(x, 5, 9))
    assert y.shape == (1, 6, 10, 2)
    (y * gout).sum().backward()
    w64, b64 = deconv.weight.detach().cpu().double().requires_grad_(True), deconv.bias.detach().cpu().double().requires_grad_(True)
    ref = F.conv_transpose2d(_nchw64(x, list(range(6))), w64, b64, stride=2, padding=1)
    (ref * gout.cpu().double().permute(0, 3, 1, 2)).sum().backward()
    close_fwd(y.detach().cpu(), ref.detach().permute(0, 2, 3, 1), what=f"transposed forward ({precision})")
    assert deconv.weight.grad.shape == (6, 2, 4, 4)         # [Cin][Cout][k][k], the parameter's own order
    close_bwd(deconv.weight.grad.cpu(), w64.grad, what="transposed dW")
    close_bwd(deconv.bias.grad.cpu(), b64.grad, what="transposed db")
    # the fp32 rows the direct transposed-convolution kernel reads: the same layer without the zero-dilated copy
    out = torch.zeros(1, 6, 10, 4, device=DEV)
    ops.deconv4x4s2_small(x, pc.rows_f32(), pc.b, 2, out)
    close_fwd(out[..., :2].cpu(), ref.detach().permute(0, 2, 3, 1), what="deconv4x4s2_small over rows_f32")
