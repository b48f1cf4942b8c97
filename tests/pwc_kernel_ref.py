"""CPU side of tests/test_pwc_kernels.py: the case tables, the fp64 references (oracle.pwc_ref evaluated in fp64, autograd for
the gradients), the derived error bounds, the exclusion maps of backwarp, the edge inputs with their expectations, and the
check functions.  No GPU and no project kernel code: what a kernel is compared with must not share its arithmetic.  The
check functions live here so that the planted-fault demonstrations (CPU) and the GPU tests call the very same ones.

Layout: the oracle is NCHW, the kernels are NHWC; every tensor this module hands out is NHWC on the CPU."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pwc_ref

ACT_NONE, ACT_LEAKY = 0, 4          # include/focusflow_hip.h: FF_ACT_*
SENTINEL = 3.0e4
U = 2.0 ** -24                      # unit roundoff of fp32
MEASURED = {}                       # kernel -> largest fraction of its bound / largest relative error seen in this process


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).contiguous()


# =====================================================================================================================
# check functions
def check_bound(kernel, got, ref, absref, n, what):
    """|got - ref| <= (n + 3) * 2^-24 * absref element by element, absref = the same reference evaluated on |inputs|
    (sum |a_i b_i|): any order of an fp32 sum of n products stays inside it; +3 = product rounding, the 1/C scaling and
    the leaky multiply.  Where absref is zero (every product of the element is a product with padding) the value must be
    exactly zero.  -> the largest fraction of the bound reached."""
    got, ref, absref = (np.asarray(t.detach().cpu().double().numpy()) for t in (got, ref, absref))
    assert got.shape == ref.shape == absref.shape, f"{what}: shapes {got.shape} {ref.shape} {absref.shape}"
    bound = (n + 3) * U * absref
    zero = bound == 0
    assert not np.any(got[zero] != 0), f"{what}: {int(np.count_nonzero(got[zero]))} non-zero values where every product is with padding"
    frac = 0.0
    if (~zero).any():
        frac = float((np.abs(got - ref)[~zero] / bound[~zero]).max())
    if np.isfinite(frac):
        MEASURED[kernel] = max(MEASURED.get(kernel, 0.0), frac)
    print(f"[{kernel}] {what}: {frac:.3f} of the bound")
    assert frac <= 1.0, f"{what}: {frac:.3e} of the derived bound (n = {n})"
    return frac


def rel_error(a, ref, mask=None):
    """max |a - ref| / (|ref| + max|ref|) - the measure of tests/test_pointwise_ops.check - over the elements of `mask`
    (broadcast over the channels)."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, f"shape {tuple(a.shape)} vs {tuple(ref.shape)}"
    if mask is not None:
        m = mask.unsqueeze(-1).expand_as(ref)
        a, ref = a[m], ref[m]
    if ref.numel() == 0:
        return 0.0
    top = max(1e-6, float(ref.abs().max()))
    return float(((a - ref).abs() / (ref.abs() + top)).max())


def check_rel(kernel, a, ref, tol, what, mask=None):
    need = rel_error(a, ref, mask)
    if np.isfinite(need):
        MEASURED[kernel] = max(MEASURED.get(kernel, 0.0), need)
    print(f"[{kernel}] {what}: {need:.3e} (tolerance {tol:.3e})")
    assert need <= tol, f"{what}: needs a tolerance of {need:.3e}, allowed {tol:.3e}"
    return need


# =====================================================================================================================
# cost volume
CvCase = namedtuple("CvCase", "B C H W product_splits library_splits")
#   product_splits: what pwc._cv_fwd asks for (1 = unsplit); library_splits: what ff_pwc_costvolume_fwd_ex makes of it
CV_CASES = [
    CvCase(1, 4, 1, 1, 1, 1),           # smallest legal input; 80 of 81 channels lie wholly in the padding
    CvCase(1, 20, 3, 5, 1, 1),          # C no multiple of 16; plane smaller than a tile and than the 4-pixel radius
    CvCase(2, 32, 17, 35, 1, 1),        # ragged tiles in both directions; batch
    CvCase(1, 196, 7, 16, 13, 13),      # last chunk holds 4 channels; 13 splits of one chunk
    CvCase(4, 96, 28, 64, 4, 3),        # 64 tiles, 6 chunks: 4 splits asked, 2 chunks each, 3 made
    CvCase(1, 64, 60, 100, 4, 4),       # 6000 pixels x 81 values: past cv_finish_kernel's 1024 blocks
    CvCase(1, 8, 100, 131, 1, 1),       # 13100 pixels x 81 values: past gout_transpose_kernel's 4096 blocks
]


def cv_case_id(c):
    return f"b{c.B}-c{c.C}-{c.H}x{c.W}"


def cv_chunks(c):
    return (c.C + 15) // 16


def cv_splits(c):
    """The explicit split counts a case runs with: 0 (unsplit), 2, 3, one chunk per split, more splits than chunks."""
    chunks = cv_chunks(c)
    return [0] if chunks == 1 else sorted({0, 2, 3, chunks, chunks + 5})


def cv_product_splits(c):
    """pwc._cv_fwd's decision, restated from its description: few tiles with many channels split the channel range."""
    tiles = c.B * ((c.H + 7) // 8) * ((c.W + 15) // 16)
    return min(cv_chunks(c), 256 // tiles) if (tiles < 128 and cv_chunks(c) >= 4) else 1


def cv_library_splits(channels, splits):
    """What ff_pwc_costvolume_fwd_ex makes of a request: whole 16-channel chunks per split, then as many splits as that needs."""
    if splits <= 1:
        return 1
    return -(-channels // cv_channels_per_split(channels, splits))


def cv_channels_per_split(channels, splits):
    chunks = -(-channels // 16)
    return -(-chunks // splits) * 16


@lru_cache(maxsize=None)
def cv_reference(case: CvCase):
    """fp32 inputs of a case, its fp64 volume and gradients, and the same quantities on |inputs| (the sums of |products|)."""
    g = torch.Generator().manual_seed(7000 + 13 * case.C + case.H)
    shape = (case.B, case.C, case.H, case.W)
    one, two = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    gy = torch.randn((case.B, 81, case.H, case.W), generator=g)
    res = dict(one=nhwc(one), two=nhwc(two), gy=nhwc(gy))
    for tag, f in (("", lambda t: t), ("abs_", torch.abs)):
        a, b = f(one).double().requires_grad_(True), f(two).double().requires_grad_(True)
        vol = pwc_ref.cost_volume(a, b)
        vol.backward(f(gy).double())
        res[tag + "vol"], res[tag + "g_one"], res[tag + "g_two"] = nhwc(vol), nhwc(a.grad), nhwc(b.grad)
    return res


def gout_transpose_ref(g):
    """G'[b, y, x, (p, o)] = g[b, y + p, x + o, (-p, -o)], zero outside: a permutation with zero fill.  NHWC (B, H, W, 81)."""
    b, h, w, _ = g.shape
    gp = F.pad(g, (0, 0, 4, 4, 4, 4))
    out = torch.zeros_like(g)
    for d in range(81):
        p, o = d // 9 - 4, d % 9 - 4
        out[..., d] = gp[:, 4 + p:4 + p + h, 4 + o:4 + o + w, (4 - p) * 9 + (4 - o)]
    return out


def cv_split_restatement(one, two, splits, act, drop_last=False, act_per_split=False):
    """The split mode in torch, fp32, NHWC in and out: partial volumes over channel ranges of whole chunks, added in order,
    the activation after the sum.  The two switches plant the faults of the demonstrations."""
    c = one.shape[-1]
    per = cv_channels_per_split(c, splits)
    o, t = nchw(one), nchw(two)
    parts = []
    for lo in range(0, c, per):
        hi = min(c, lo + per)
        parts.append(pwc_ref.cost_volume(o[:, lo:hi], t[:, lo:hi]) * ((hi - lo) / c))
    if drop_last:
        parts = parts[:-1]
    if act_per_split and act == ACT_LEAKY:
        parts = [F.leaky_relu(p, 0.1) for p in parts]
    vol = sum(parts)
    if act == ACT_LEAKY and not act_per_split:
        vol = F.leaky_relu(vol, 0.1)
    return nhwc(vol)


# =====================================================================================================================
# backwarp
BwCase = namedtuple("BwCase", "B C H W scale sd seed")
BW_CASES = [
    BwCase(2, 32, 28, 40, 5.0, 1.5, 1),
    BwCase(1, 196, 7, 16, 0.625, 1.5, 2),
    BwCase(1, 64, 17, 23, 2.5, 1.5, 3),
    BwCase(1, 4, 2, 2, 1.25, 0.3, 4),         # the smallest plane the entry point accepts
    BwCase(3, 8, 5, 33, 1.25, 2.0, 5),
    # 33280 pixels: past backwarp_bwd_kernel's 8192 blocks of 4, and x 32 channel groups past backwarp_kernel's 4096 blocks
    # (sd raised from 1.5 until a tenth of the plane is invalid: at 1.5, 93 % of the pixels are valid)
    BwCase(1, 128, 128, 260, 5.0, 4.0, 6),
]
EDGE_CASE = BW_CASES[2]             # the edge inputs use this shape and scale, and the tolerance of this case
TAU_FLOOR = 1e-5
THRESHOLD = 0.999


def bw_case_id(c):
    return f"b{c.B}-c{c.C}-{c.H}x{c.W}-s{c.scale}"


def sample_position(flow, scale, dtype):
    """(ux, uy), each (B, H, W): where backwarp samples, computed operation by operation as oracle.pwc_ref.backwarp and
    ATen's grid_sample (align_corners=False) do, in `dtype`.  flow: NHWC (B, H, W, 2) fp32, multiplied by `scale` first."""
    b, h, w, _ = flow.shape
    fl = flow.to(dtype) * scale
    hor = torch.linspace(-1.0 + (1.0 / w), 1.0 - (1.0 / w), w, dtype=dtype).view(1, 1, w)
    ver = torch.linspace(-1.0 + (1.0 / h), 1.0 - (1.0 / h), h, dtype=dtype).view(1, h, 1)
    gx = hor + fl[..., 0] / ((w - 1.0) / 2.0)
    gy = ver + fl[..., 1] / ((h - 1.0) / 2.0)
    return ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2


def weight_sum(ux, uy, h, w):
    """What the warped ones-channel holds: the bilinear weights of the corners that lie inside the plane."""
    x0, y0 = torch.floor(ux), torch.floor(uy)
    wx, wy = ux - x0, uy - y0
    total = torch.zeros_like(ux)
    for dy, fy in ((0, 1 - wy), (1, wy)):
        for dx, fx in ((0, 1 - wx), (1, wx)):
            inside = (x0 + dx >= 0) & (x0 + dx <= w - 1) & (y0 + dy >= 0) & (y0 + dy <= h - 1)
            total = total + torch.where(inside, fx * fy, torch.zeros_like(ux))
    return total


def backwarp_variant(x, flow, align_corners=False, threshold=THRESHOLD):
    """backwarp in torch, NCHW, in the dtype of its inputs; the two arguments plant the faults of the demonstrations."""
    b, _, h, w = flow.shape
    if align_corners:
        hor, ver = torch.linspace(-1.0, 1.0, w, dtype=flow.dtype), torch.linspace(-1.0, 1.0, h, dtype=flow.dtype)
    else:
        hor = torch.linspace(-1.0 + (1.0 / w), 1.0 - (1.0 / w), w, dtype=flow.dtype)
        ver = torch.linspace(-1.0 + (1.0 / h), 1.0 - (1.0 / h), h, dtype=flow.dtype)
    grid = torch.stack([hor.view(1, 1, w) + flow[:, 0] / ((w - 1.0) / 2.0), ver.view(1, h, 1) + flow[:, 1] / ((h - 1.0) / 2.0)], -1)
    out = F.grid_sample(torch.cat([x, flow.new_ones(b, 1, h, w)], 1), grid, mode="bilinear", padding_mode="zeros", align_corners=align_corners)
    return out[:, :-1] * (out[:, -1:] > threshold).to(x.dtype)


def bw_oracle(x, flow, scale, gout, dtype):
    """oracle.pwc_ref.backwarp and autograd in `dtype` on NHWC fp32 data -> (out, d_input, d_flow), NHWC; d_flow is with
    respect to the unscaled flow, as the kernel returns it."""
    xr = nchw(x).to(dtype).requires_grad_(True)
    fr = nchw(flow).to(dtype).requires_grad_(True)
    out = pwc_ref.backwarp(xr, fr * scale)
    out.backward(nchw(gout).to(dtype))
    return nhwc(out), nhwc(xr.grad), nhwc(fr.grad)


def bw_exclusions(flow, scale):
    """From the fp64 position alone -> dict: tau, pos_err, valid, near_thr (|weight sum - 0.999| < tau: left out of every
    comparison), near_int (valid and within tau of a cell border in x or y: left out of d_flow as well)."""
    _, h, w, _ = flow.shape
    ux, uy = sample_position(flow, scale, torch.float64)
    ux32, uy32 = sample_position(flow, scale, torch.float32)
    pos_err = max(float((ux32.double() - ux).abs().max()), float((uy32.double() - uy).abs().max()))
    tau = max(TAU_FLOOR, 4 * pos_err)
    ws = weight_sum(ux, uy, h, w)
    valid = ws > THRESHOLD
    near_thr = (ws - THRESHOLD).abs() < tau
    near_int = valid & (((ux - torch.round(ux)).abs() < tau) | ((uy - torch.round(uy)).abs() < tau))
    return dict(tau=tau, pos_err=pos_err, valid=valid, near_thr=near_thr, near_int=near_int, ux=ux, uy=uy, wsum=ws)


@lru_cache(maxsize=None)
def bw_reference(case: BwCase):
    """fp32 inputs of a random case, the exclusion maps, the fp64 results, and the error of the fp32 CPU oracle against them
    (`cpu_err`), from which the tolerances are taken (`tol` = 4 x).  The upstream gradient is ZERO at the pixels left out, for
    every side alike: a pixel dropped from an element-wise comparison would still scatter into d_input."""
    g = torch.Generator().manual_seed(9000 + case.seed)
    x = torch.randn((case.B, case.H, case.W, case.C), generator=g)
    flow = torch.randn((case.B, case.H, case.W, 2), generator=g) * case.sd
    gout = torch.randn((case.B, case.H, case.W, case.C), generator=g)
    ex = bw_exclusions(flow, case.scale)
    gout = gout * (~ex["near_thr"]).unsqueeze(-1)
    keep, keep_flow = ~ex["near_thr"], ~(ex["near_thr"] | ex["near_int"])
    out, din, dflow = bw_oracle(x, flow, case.scale, gout, torch.float64)
    o32, di32, df32 = bw_oracle(x, flow, case.scale, gout, torch.float32)
    cpu_err = dict(out=rel_error(o32, out, keep), din=rel_error(di32, din), dflow=rel_error(df32, dflow, keep_flow))
    return dict(x=x, flow=flow, gout=gout, out=out, din=din, dflow=dflow, keep=keep, keep_flow=keep_flow, ex=ex, cpu_err=cpu_err,
                tol={k: 4 * v for k, v in cpu_err.items()})


# ---------------------------------------------------------------------------------------------------------------------
# edge inputs: shape and flow_scale of EDGE_CASE.  The sample position is x + flow_x * scale * W / (W - 1) (the reference's
# grid is the pixel centres of align_corners=False and its flow normalisation is that of align_corners=True).
def edge_data():
    c = EDGE_CASE
    g = torch.Generator().manual_seed(9100)
    x = torch.randn((c.B, c.H, c.W, c.C), generator=g)
    gout = torch.randn((c.B, c.H, c.W, c.C), generator=g)
    return x, gout


def flow_for_offset(dx, dy):
    """A flow tensor's worth of (B, H, W, 2) whose sample position is (x + dx, y + dy); dx, dy: floats or (H, W) tensors."""
    c = EDGE_CASE
    fl = torch.zeros((c.B, c.H, c.W, 2), dtype=torch.float64)
    fl[..., 0] = torch.as_tensor(dx, dtype=torch.float64) * (c.W - 1) / c.W / c.scale
    fl[..., 1] = torch.as_tensor(dy, dtype=torch.float64) * (c.H - 1) / c.H / c.scale
    return fl.float()


SHIFTS = [(1, 0), (0, -2), (-3, 2)]          # (dx, dy) in whole pixels


def shifted_input(x, dx, dy):
    """-> (want, outside): want[y, x] = x[y + dy, x + dx] where that lies inside the plane, else 0; outside (H, W)."""
    _, h, w, _ = x.shape
    want = torch.zeros_like(x)
    ys, xs = torch.arange(h).view(h, 1) + dy, torch.arange(w).view(1, w) + dx
    inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    yy, xx = ys.expand(h, w)[inside], xs.expand(h, w)[inside]
    want[:, inside] = x[:, yy, xx]
    return want, ~inside


def threshold_input():
    """Flow zero inside; on the four borders the sample position lies 0.0005 (weight sum 0.9995: valid) or 0.0015 (0.9985:
    invalid) outside the plane, alternating along the border.  -> (flow, valid_px, invalid_px), the two maps (H, W) cover
    the border pixels."""
    c = EDGE_CASE
    h, w = c.H, c.W
    dx, dy = torch.zeros(h, w, dtype=torch.float64), torch.zeros(h, w, dtype=torch.float64)
    invalid = torch.zeros(h, w, dtype=torch.bool)
    border = torch.zeros(h, w, dtype=torch.bool)
    rows, cols = torch.arange(h), torch.arange(1, w - 1)
    for col, sign in ((0, -1.0), (w - 1, 1.0)):                   # left and right columns (with the corners): rows alternate
        inv = rows % 2 == 0
        dx[rows, col] = sign * torch.where(inv, torch.tensor(0.0015, dtype=torch.float64), torch.tensor(0.0005, dtype=torch.float64))
        invalid[rows, col] = inv
        border[rows, col] = True
    for row, sign in ((0, -1.0), (h - 1, 1.0)):                   # top and bottom rows between the corners: columns alternate
        inv = cols % 2 == 1
        dy[row, cols] = sign * torch.where(inv, torch.tensor(0.0015, dtype=torch.float64), torch.tensor(0.0005, dtype=torch.float64))
        invalid[row, cols] = inv
        border[row, cols] = True
    return flow_for_offset(dx, dy), border & ~invalid, invalid


def check_threshold_forward(kernel, out, ref, valid_px, invalid_px, tol):
    """The border pixels of threshold_input: invalid ones exactly zero, valid ones non-zero in every channel and within the
    tolerance of the fp64 reference.  No outlier budget."""
    out = out.detach().cpu()
    bad = out[:, invalid_px]
    assert bool((bad == 0).all()), f"{int((bad != 0).any(-1).sum())} pixels with weight sum 0.9985 are not exactly zero"
    assert bool((out[:, valid_px] != 0).all()), "a pixel with weight sum 0.9995 came out zero"
    assert bool((ref[:, valid_px] != 0).all())
    check_rel(kernel, out, ref, tol, "threshold input, valid border pixels", valid_px.unsqueeze(0).expand(out.shape[:3]))


# =====================================================================================================================
# direct transposed convolution
DcCase = namedtuple("DcCase", "Cin Cout B H W")
DC_CASES = [
    DcCase(4, 1, 1, 1, 1),
    DcCase(256, 2, 1, 3, 5),            # exactly one 256-channel pass
    DcCase(260, 2, 2, 3, 5),            # one lane in the second pass; W = 5: the second run of 8 output pixels holds 2
    DcCase(544, 2, 1, 7, 16),           # the product's narrowest level buffer
    DcCase(704, 2, 1, 5, 9),            # the widest; W = 9: the third run holds 2
]


def dc_case_id(c):
    return f"cin{c.Cin}-cout{c.Cout}-b{c.B}-{c.H}x{c.W}"


@lru_cache(maxsize=None)
def dc_reference(case: DcCase):
    """x NHWC, the ConvTranspose2d parameter wt [Cin][Cout][4][4], bias, and per bias mode the fp64 result with the result
    on |inputs| (+ |bias|)."""
    g = torch.Generator().manual_seed(8000 + case.Cin)
    x = torch.randn((case.B, case.Cin, case.H, case.W), generator=g)
    wt = torch.randn((case.Cin, case.Cout, 4, 4), generator=g) / (case.Cin * 4) ** 0.5
    bias = torch.randn(case.Cout, generator=g)
    res = dict(x=nhwc(x), wt=wt, bias=bias)
    for tag, b in (("", bias), ("nobias_", None)):
        res[tag + "ref"] = nhwc(F.conv_transpose2d(x.double(), wt.double(), None if b is None else b.double(), stride=2, padding=1))
        res[tag + "abs"] = nhwc(F.conv_transpose2d(x.abs().double(), wt.abs().double(), None if b is None else b.abs().double(), stride=2, padding=1))
    return res
