"""Plain fp64 references of the small kernels between the convolutions (tests/test_pointwise_ops.py): the norm layers in
their three modes, the activation derivatives from the forward output, and the table of norm cases.  CPU only, NHWC, no
project code: what a kernel is compared with must not share its arithmetic."""
from collections import namedtuple
from functools import lru_cache

import torch

EPS = 1e-5
NEAR_ZERO = 1e-4          # |pre-activation| below this: the fp32 kernel and the fp64 reference may disagree about a ReLU mask

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_LEAKY = 0, 1, 2, 3, 4        # include/focusflow_hip.h: FF_ACT_*


def act_forward(pre: torch.Tensor, act: int) -> torch.Tensor:
    return {ACT_NONE: lambda t: t.clone(), ACT_RELU: torch.relu, ACT_SIGMOID: torch.sigmoid, ACT_TANH: torch.tanh,
            ACT_LEAKY: lambda t: torch.nn.functional.leaky_relu(t, 0.1)}[act](pre)


def act_grad_from_output(y: torch.Tensor, act: int) -> torch.Tensor:
    """act'(.) written in terms of the forward OUTPUT y, in y's dtype."""
    one = torch.ones_like(y)
    if act == ACT_RELU:
        return torch.where(y > 0, one, torch.zeros_like(y))
    if act == ACT_SIGMOID:
        return y * (1 - y)
    if act == ACT_TANH:
        return 1 - y * y
    if act == ACT_LEAKY:
        return torch.where(y > 0, one, torch.full_like(y, 0.1))
    return one


# ---------------------------------------------------------------------------------------------------------------------
# norm layers
NormCase = namedtuple("NormCase", "mode relu res B C H W view offset seed")
#   mode: instance (per sample, no affine) | batch (statistics of the batch, gamma / beta) | frozen (running statistics)
#   C: 4 / 64 / 96 / 256 = 1 / 16 / 24 (does not divide 256) / 64 (the limit) float4 groups
#   planes: 1x1, 15x17 = 255, 16x16 = 256, 1x257 (either side of the 256-pixel slab) and 20x28 (three slabs)
NORM_CASES = [
    NormCase("instance", True, False, 3, 96, 20, 28, False, False, 1),
    NormCase("instance", True, True, 3, 64, 15, 17, False, False, 2),
    NormCase("instance", False, False, 1, 4, 1, 257, False, False, 3),
    NormCase("instance", True, True, 1, 256, 16, 16, False, False, 4),
    NormCase("batch", True, True, 3, 96, 16, 16, False, False, 5),
    NormCase("batch", False, False, 3, 256, 1, 1, False, False, 6),
    NormCase("batch", True, True, 3, 64, 1, 257, True, False, 7),            # x, dy, y and res are views
    NormCase("batch", True, False, 1, 64, 20, 28, False, True, 8),           # channel mean 8, standard deviation 0.25
    NormCase("frozen", True, True, 3, 96, 20, 28, False, False, 9),
    NormCase("frozen", False, False, 1, 256, 15, 17, False, False, 10),
    NormCase("frozen", True, False, 3, 64, 1, 1, False, False, 11),
    NormCase("frozen", True, True, 1, 4, 16, 16, True, False, 12),
    NormCase("frozen", True, True, 3, 4, 15, 17, False, False, 13),
]


def norm_case_id(c: NormCase) -> str:
    return (f"{c.mode}-relu{int(c.relu)}-res{int(c.res)}-b{c.B}-c{c.C}-{c.H}x{c.W}" + ("-view" if c.view else "")
            + ("-offset" if c.offset else ""))


def norm_forward(x, mode, gamma, beta, relu, res, rm=None, rv=None):
    """-> (y, pre0 = gamma xhat + beta, pre1 = relu?(pre0) + res or None); everything (B, H, W, C) in x's dtype."""
    if mode == "instance":
        mean, var = x.mean((1, 2), keepdim=True), x.var((1, 2), unbiased=False, keepdim=True)
    elif mode == "batch":
        mean, var = x.mean((0, 1, 2)), x.var((0, 1, 2), unbiased=False)
    else:
        mean, var = rm, rv
    pre0 = (x - mean) / torch.sqrt(var + EPS)
    if gamma is not None:
        pre0 = pre0 * gamma + beta
    y = torch.relu(pre0) if relu else pre0
    pre1 = None
    if res is not None:
        pre1 = y + res
        y = torch.relu(pre1)
    return y, pre0, pre1


@lru_cache(maxsize=None)
def norm_reference(case: NormCase):
    """The fp32 inputs of a case and its fp64 results, computed once: dict of CPU tensors.

    `near` marks the elements whose ReLU mask is undecided (a pre-activation within NEAR_ZERO of zero, either of the two with
    a residual).  Their upstream gradient dy is set to ZERO, for the kernel and for the reference alike: an element left out
    of an element-wise comparison would still sit in the sums behind dx, dgamma and dbeta, where one flipped mask moves a
    channel's sum by a whole |dy|."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    shape = (case.B, case.H, case.W, case.C)
    if case.offset:
        x = torch.randn(shape, generator=g) * 0.25 + 8.0
    else:
        x = torch.randn(shape, generator=g) * 2 + 0.5
    res = torch.randn(shape, generator=g) if case.res else None
    affine = case.mode != "instance"
    gamma = 1 + 0.2 * torch.randn(case.C, generator=g) if affine else None
    beta = 0.3 * torch.randn(case.C, generator=g) if affine else None
    dy = torch.randn(shape, generator=g)
    rm = rv = None
    if case.mode == "frozen":     # running statistics that are NOT the batch's own: a kernel that ignored the table would fail
        rm = (x.double().mean((0, 1, 2)) + 0.3).float()
        rv = (1.7 * x.double().var((0, 1, 2), unbiased=False)).float()
    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if case.res else None
    gr = gamma.double().requires_grad_(True) if affine else None
    br = beta.double().requires_grad_(True) if affine else None
    y, pre0, pre1 = norm_forward(xr, case.mode, gr, br, case.relu, rr, rm.double() if rm is not None else None,
                                 rv.double() if rv is not None else None)
    near = torch.zeros(shape, dtype=torch.bool)
    if case.relu:
        near |= pre0.detach().abs() < NEAR_ZERO
    if case.res:
        near |= pre1.detach().abs() < NEAR_ZERO
    dy = torch.where(near, torch.zeros_like(dy), dy)
    y.backward(dy.double())
    return dict(x=x, res=res, gamma=gamma, beta=beta, dy=dy, rm=rm, rv=rv, near=near, y=y.detach(), dx=xr.grad,
                dres=rr.grad if case.res else None, dgamma=gr.grad if affine else None, dbeta=br.grad if affine else None)
