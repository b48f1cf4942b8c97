"""The fp16x3 split kernels held to their format over the whole input range (csrc/ff_common.h).

Every other module compares these kernels with fp64 on randn-scale inputs under 8 e32 or 2e-5 max|ref|.  At that scale a
loader that drops the subnormal second half (h1 is a subnormal half whenever |s v| < 2^-3) errs by 3e-6 of max|ref| and
passes; two to five powers of 32 lower it is 10 - 1000 times worse than the format allows.  Here every loader family and
every split store runs over inputs from 2^-16 to the format's limit, and is held ELEMENTWISE to

    |out - fp64| <= B + 8 e32,     B = 2^-22 sum|x||w| + (2^-25 / sx) sum|w| + (2^-25 / sw) sum|x|

(split_format_ref.format_bound: the sums over the taps of that element, from the same operation on absolute values in
fp64; sx = 4 * amax scale for activations and gradients, sw = 16 for packed rows; e32 = max|CPU fp32 - fp64| of the same
operation).  Nothing in the bound is measured on the kernels.  The CPU tests of this module hold the bound itself: the
format emulated to the letter (split_format_ref.emulate, fp64 accumulation of x0 w0 + x0 w1 + x1 w0) stays at or below
0.5 B on every element of every recipe, and the same emulation with subnormal halves flushed exceeds B + 8 e32.

Result of the first MI355X run: no kernel breaks the format.  Every loader, every store and the matrix pipe keep subnormal
halves; the largest error was 0.47 of the allowance (table below); nothing in csrc/ changed.

Recipes (split_format_ref.activations / gradients).  uniE: randn * 2^E, E in {-16, -10, -5, 0, 6, 12}, clamped to +-16000.
uniE+peak: the same with eight elements planted at +-16375.  wideE: randn * 2^(-16 u) * 2^E, u uniform in [0, 1], E in
{0, 12}.  Each family also runs once with weights * 2^-9 (every w1 subnormal) over the wide+0 input.  Gradients: randn *
2^E, E in {-60, -30, -14, 0, 20, 60}, and log-uniform over 24 binades below 2^E with twenty outliers at 3e4 * 2^E, E in
{-30, 0}; each with the amax word of the tensor itself (fresh) and with the word of the tensor times 2^12 (stale).
Where these go beyond the plainest reading of the recipes, the CPU tests forced it:
  * planted and unplanted uniform runs are separate.  e32 is a maximum over the whole output; one planted 16375 in a
    2^-10-scale tensor puts it a thousand times above the ordinary outputs, and a loader that flushes the activations' h1 then
    errs by 0.01 - 0.08 of the allowance: invisible.  Without planted values the same defect is 214 / 34 / 30 times the
    allowance at 2^-16 / 2^-10 / 2^-5 (and 3.5 times for wide+0).  The planted runs keep what they are for: the range limit
    next to tiny values, and flushed WEIGHT halves (4.7 - 40 times the allowance);
  * the same holds for gradients: with the fresh word the large values that set the scale also set e32, and a loader that
    flushes the gradient's h1 errs by 0.01 - 0.03 of the allowance in every recipe.  Under a word 2^12 too large every h1 of the
    gradient is subnormal with no large value in the tensor: 7.5 - 18 times (input gradient), 10 - 17 times (weight gradient);
  * planted values stand SIDE BY SIDE (channels 0.. of one pixel; consecutive pixels of one channel for the weight
    gradient, whose reduction runs over pixels).  An output that sees one planted 16375 alone is a single product; its error
    is one rounding of one small weight (up to 2^-29 absolute) - the whole of B, which is sized for sums: the emulation
    reached 0.91 - 1.00 B with scattered plants, at most 0.31 B side by side;
  * the small-weight run uses the wide+0 input, not a planted one (0.61 B with eight plants: all eight weights sit on the
    2^-29 floor); the weight gradient runs over wide+0 activations x (0.35 B; a planted x again gave 1.00 B);
  * for the two correlation kernels, where both operands are rows, "wide" draws u per ROW (pixel), not per element: with
    both operands wide per element the largest product dominates the 256-term sum (1.01 B).  32 values are planted at +-4000.

Where flushing shows on the CPU (flush emulation / (B + 8 e32); "both": every subnormal half, as a matrix pipe that drops
them would; "first" / "second": one operand's halves, as its loader would), all asserted:
  convolution (x first, sx = 4): both > 1 in every recipe (4.7 - 214); first: uni-16 214, uni-10 34, uni-5 30, wide+0 3.5;
  small weights: both 183, second 183;  input gradient (g first): both 5.7 - 15.7 (the weights' halves); under the stale word first 7.5 - 18;
  weight gradient (x first, g second): first 2.4 - 10; under the stale word second 10 - 17;
  correlation (rows, s = 16: subnormal below 2^-7): uni-16 92, uni-10 18, uni-5 8 for either operand; with planted values 314 / 44 / 3.
  Not visible, and not asserted: correlation rows at 2^0 and above and the row-wide recipes (0.00 - 0.64: a global e32 taken
  from the largest rows hides the small ones); the gradient operand under its fresh word (above).
Largest CPU-emulation err / B: convolution 0.31, small weights 0.33, input gradient 0.18, weight gradient 0.35, correlation 0.34.

Largest err / B per family and recipe, one MI355X run (the RANGE-ERR lines).  err / B above 1 is fp32 accumulation (the 8 e32
part of the allowance); in the planted runs e32 is large and so are these ratios.
Forward families, err / B in the order uni-16 -10 -5 +0 +6 +12 | the same six +peak | wide+0 wide+12 (corr: rowwide) | small weights;
then the family's largest err / (B + 8 e32).  '-': above 100, see the note below.
  split 64x64 t3 uni         0.41 0.38 0.35 0.82 0.76 0.70 | 0.39 0.43 0.44 0.66 0.82 0.79 | 1.47 1.60 | 0.75 ; 0.43
  split 64x64 t3 gen         0.18 0.16 0.34 0.62 0.67 0.60 | 0.36 1.11 0.94 1.13 1.95 0.64 | 1.12 1.19 | 0.40 ; 0.33
  patch occ th4 t3           0.19 0.18 0.28 0.53 0.57 0.54 | 0.29 0.86 1.08 1.09 2.83 0.50 | 0.98 1.38 | 0.44 ; 0.38
  patch occ th4 t3 +splitk   0.04 0.05 0.05 0.07 0.09 0.09 | 0.33 1.71 0.91 1.60 0.92 0.08 | 0.16 0.20 | 0.10 ; 0.21
  patch gen th4 ni8 t3       0.11 0.11 0.25 0.42 0.52 0.50 | 0.37 2.16 3.32 2.97 1.04 0.52 | 0.95 1.00 | 0.24 ; 0.22
  dma_f32 3x3 th4            0.09 0.11 0.23 0.55 0.55 0.51 | 0.40 2.25 2.58 1.94 2.93 0.51 | 0.93 1.10 | 0.24 ; 0.27
  dma_f32 1x5 th4            0.14 0.15 0.26 0.61 0.54 0.56 | 0.41 1.34 1.20 2.70 3.18 0.63 | 1.04 1.18 | 0.38 ; 0.35
  dma_f32 5x1 th4            0.13 0.13 0.27 0.57 0.49 0.56 | 0.33 1.34 1.21 1.84 2.01 0.66 | 1.04 1.35 | 0.29 ; 0.28
  stem                       0.27 0.23 0.37 0.67 0.77 0.75 | 0.62 1.01 1.54 1.34 2.37 0.81 | 1.15 1.60 | 0.72 ; 0.47
  conv_dma split-pair input  0.11 0.13 0.25 0.44 0.49 0.44 | 0.36 1.69 2.23 2.17 2.02 0.58 | 0.84 1.28 | 0.21 ; 0.28
  fusion_pair C64 img'       0.35 0.35 0.35 0.54 0.62 0.57 | - - - - 12.67 0.58 | 1.00 2.08 | 18.14 ; 0.35
  fusion_pair C64 mask'      0.33 0.36 0.35 0.53 0.64 0.55 | - - - - 8.63 0.57 | 1.03 2.77 | 18.79 ; 0.33
  fusion_pair C96 img'       0.32 0.28 0.30 0.70 0.56 0.59 | - - - - 6.60 0.61 | 1.12 1.31 | 10.79 ; 0.32
  fusion_pair C96 mask'      0.32 0.28 0.31 0.59 0.80 0.57 | - - - - 6.91 0.60 | 1.11 1.72 | 12.60 ; 0.32
  corr_build level 0         0.15 0.15 0.44 0.69 0.72 0.55 | 0.33 0.26 0.53 1.14 1.76 0.68 | 0.44 0.70 | 0.19 ; 0.32
  corr_alt_lookup            - - - - - - | - - - - - - | - - | - ; 0.18
  gru_pass 1x5               0.21 0.19 0.13 0.04 0.01 0.00 | 0.00 0.00 0.00 0.00 0.00 0.01 | 0.14 0.01 | 1.33 ; 0.21
  gru_pass 5x1               0.23 0.19 0.13 0.04 0.01 0.01 | 0.00 0.00 0.00 0.00 0.00 0.01 | 0.14 0.04 | 1.54 ; 0.23
  mask_upsample              24.98 11.15 1.93 0.07 - - | - - 46.80 36.69 - - | 0.19 - | 42.64 ; 0.13
Gradient families, err / B in the order uni-60 -30 -14 +0 +20 +60 wide-30 wide+0, fresh word | the same eight under a word 2^12 too
large | stale word 2^20, max|g| 2^-140 where run; then the family's largest err / (B + 8 e32).
  dgrad patch occ th4 t3         0.59 0.61 0.55 0.56 0.50 0.55 0.59 0.65 | 0.35 0.48 0.43 0.43 0.37 0.36 0.32 0.29 | 0.20 0.00 ; 0.19
  dgrad dma_f32 3x3 th4          0.47 0.65 0.52 0.53 0.54 0.54 0.95 1.14 | 0.34 0.36 0.27 0.34 0.37 0.32 0.40 0.31 | 0.10 0.00 ; 0.23
  dgrad split 64x64 t3 uni       0.62 0.63 0.61 0.54 0.66 0.60 0.43 0.53 | 0.42 0.38 0.38 0.44 0.42 0.49 0.35 0.44 | 0.36 0.00 ; 0.34
  dgrad split 64x64 t3 gen       0.79 0.55 0.55 0.66 0.56 0.62 0.88 1.18 | 0.41 0.45 0.36 0.43 0.38 0.42 0.38 0.68 | not run ; 0.10
  dgrad patch gen th4 ni8 t3     0.50 0.43 0.54 0.42 0.47 0.54 1.30 2.25 | 0.34 0.30 0.38 0.43 0.36 0.37 0.36 0.55 | not run ; 0.18
  dgrad patch occ th4 t3 +splitk 0.09 0.07 0.09 0.08 0.08 0.09 0.58 0.70 | 0.07 0.06 0.07 0.06 0.06 0.07 0.05 0.06 | not run ; 0.11
  wgrad split 64x128 dW          0.28 0.25 0.26 0.28 0.42 0.33 1.03 0.62 | 0.22 0.19 0.18 0.17 0.17 0.20 0.29 0.30 | 0.21 0.00 ; 0.21
  wgrad split 64x128 db          0.06 0.07 0.06 0.10 0.10 0.06 0.01 0.01 | 0.04 0.07 0.04 0.04 0.06 0.04 0.00 0.00 | 0.00 0.00 ; 0.08
  wgrad split 128x64 dW          0.34 0.31 0.39 0.36 0.37 0.34 0.84 0.90 | 0.25 0.30 0.34 0.27 0.33 0.31 0.38 0.38 | not run ; 0.13
  wgrad split 128x64 db          0.06 0.06 0.05 0.10 0.07 0.05 0.02 0.02 | 0.04 0.04 0.06 0.04 0.05 0.03 0.00 0.00 | not run ; 0.07
  wgrad split 128x128 dW         0.54 0.59 0.74 0.66 0.53 0.65 0.73 0.81 | 0.42 0.48 0.57 0.42 0.44 0.49 0.46 0.85 | not run ; 0.19
  wgrad split 128x128 db         0.14 0.09 0.11 0.10 0.12 0.07 0.02 0.02 | 0.08 0.07 0.08 0.07 0.07 0.05 0.00 0.00 | not run ; 0.07
  wgrad patch 3x3 dW             0.36 0.38 0.37 0.40 0.38 0.49 0.55 0.98 | 0.25 0.23 0.27 0.29 0.28 0.26 0.24 0.36 | 0.28 0.00 ; 0.24
  wgrad patch 3x3 db             0.06 0.05 0.06 0.04 0.07 0.04 0.06 0.01 | 0.05 0.05 0.03 0.03 0.05 0.02 0.02 0.00 | 0.00 0.00 ; 0.05
  wgrad patch 5x1 dW             0.67 0.47 0.78 0.62 0.50 0.61 0.55 0.37 | 0.53 0.45 0.38 0.50 0.37 0.41 0.43 0.34 | not run ; 0.13
  wgrad patch 5x1 db             0.08 0.10 0.12 0.07 0.08 0.14 0.04 0.03 | 0.04 0.06 0.06 0.10 0.04 0.09 0.02 0.01 | not run ; 0.09
  wgrad patch 1x5 dW             0.60 0.60 0.63 0.65 0.60 0.84 0.77 0.63 | 0.45 0.39 0.46 0.49 0.51 0.46 0.49 0.38 | not run ; 0.10
  wgrad patch 1x5 db             0.14 0.08 0.12 0.09 0.11 0.07 0.04 0.02 | 0.08 0.05 0.07 0.05 0.08 0.04 0.02 0.01 | not run ; 0.09
Epilogue stores (decoded pair against the fp32 output, as a multiple of max(2^-22 |v|, 2^-27)): patch occ th4 t1 1.000, dma_f32 1x5 th4 1.000, split 64x64 t1 gen 1.000, split 64x64 t3 uni 1.000.
Notes.  fusion_pair adds its fp32 residual (the planted 16375) after the product: the error there is that sum's fp32
rounding, far above the product's B and inside 8 e32.  corr_alt_lookup: the fp64 sampler leaves weights of 1e-16 on taps
next to the ones an integer coordinate hits, where B is 1e-23 and the kernel gives an exact zero: err / B means nothing
there.  mask_upsample: where the soft-max is saturated the +- evaluation of the reference moves nothing and B is 0.
gru_pass with small weights: the one unplanted case above B (1.3 - 1.5), at 0.2 of the allowance: v_exp_f32 / v_rcp_f32 in
the gates (ff_common.h: 2e-7 absolute), which B does not know and 8 e32 of the blend covers.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

import split_format_ref as sf
from conftest import ROOT
from test_conv_routes import ROUTE_CASES, _packed, _problem, _route_of, route

DEV = "cuda:0"
NONE = 0


def _gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ----------------------------------------------------------------------------
# reference, bound and the check (shared by the CPU demonstration and the GPU tests)
# ----------------------------------------------------------------------------
def _bound(op, x, w, sx, sw):
    """B per output element of the bilinear `op`: the operation itself on absolute values (and on ones) in fp64."""
    xa, wa = x.double().abs(), w.double().abs()
    return sf.format_bound(op(xa, wa), op(torch.ones_like(xa), wa), op(xa, torch.ones_like(wa)), sx, sw)


def _ref(op, x, w):
    """-> (fp64 result, e32)"""
    ref = op(x.double(), w.double())
    return ref, float((op(x.float(), w.float()).double() - ref).abs().max())


def _hold(got, ref, allowed, bnd, family, recipe):
    """Every output finite, |got - fp64| <= allowed elementwise; prints the RANGE-ERR line first."""
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    tiny = 1e-300
    print(f"RANGE-ERR | {family} | {recipe} | max err/B {float((err / bnd.clamp_min(tiny)).max()):.3f} | "
          f"max err/(B + 8 e32) {float((err / allowed.clamp_min(tiny)).max()):.3f}")
    assert bool(torch.isfinite(got).all()), f"{family} [{recipe}]: non-finite output"
    bad = err > allowed
    if bool(bad.any()):
        i = int((err / allowed.clamp_min(tiny)).argmax())
        raise AssertionError(f"{family} [{recipe}]: {int(bad.sum())} of {bad.numel()} elements beyond B + 8 e32; worst: err {float(err.reshape(-1)[i]):.3e}, "
                             f"allowed {float(allowed.reshape(-1)[i]):.3e} (B {float(bnd.reshape(-1)[i]):.3e}), ref {float(ref.reshape(-1)[i]):.3e}")


def _conv_op(stride=1, pad=(0, 0), dil=1):
    return lambda a, b: F.conv2d(a, b, stride=stride, padding=pad, dilation=dil)


def _mm(a, b):
    return a @ b.transpose(-1, -2)


# ----------------------------------------------------------------------------
# CPU: the model against the header, the bound against the emulation
# ----------------------------------------------------------------------------
def test_format_constants_still_stand_in_the_header():
    """split_format_ref restates ff_common.h; its literals are found there by plain text search."""
    with open(os.path.join(ROOT, "focusflow_official_amd", "csrc", "ff_common.h")) as f:
        text = f.read()
    for needle in (f"constexpr float XSPLIT = {sf.XSPLIT:.0f}.f, WSPLIT = {sf.WSPLIT:.0f}.f, SPLIT_INV = 1.f / {1 / sf.SPLIT_INV:.0f}.f;",
                   f"int k = {sf.AMAX_BIAS} - e;", f"k = k > {sf.AMAX_CLAMP} ? {sf.AMAX_CLAMP} : (k < -{sf.AMAX_CLAMP} ? -{sf.AMAX_CLAMP} : k);",
                   "const int e = (int)((*x_amax >> 23) & 0xffu);", "if (e > 0 && e < 255) {",
                   "xs = __uint_as_float((unsigned)(127 + k) << 23);",
                   "const float sv = v[j] * XSPLIT;", "h1[j] = (_Float16)(sv - (float)a);",
                   f"Limits: |x| < {sf.X_LIMIT:.0f} (activations), |w| < {sf.W_LIMIT:.0f} (packed rows)."):
        assert needle in text, f"ff_common.h no longer holds `{needle}`: the format changed - update split_format_ref.py"
    assert sf.SPLIT_INV == 1.0 / (sf.XSPLIT * sf.WSPLIT)


def test_amax_scale_restates_input_scale():
    assert sf.amax_scale(1.0) == 2.0 ** 10 and sf.amax_scale(1.999) == 2.0 ** 10 and sf.amax_scale(2.0) == 2.0 ** 9
    assert sf.amax_scale(3e4) == 2.0 ** -4 and sf.amax_scale(2.0 ** -60) == 2.0 ** 70
    assert sf.amax_scale(2.0 ** -100) == 2.0 ** 100 and sf.amax_scale(2.0 ** -126) == 2.0 ** 100      # clamp (k = 110, 136)
    assert sf.amax_scale(2.0 ** 120) == 2.0 ** -100                                                        # clamp (k = -110)
    assert sf.amax_scale(0.0) == 1.0 and sf.amax_scale(2.0 ** -140) == 1.0 and sf.amax_scale(float("inf")) == 1.0
    assert sf.amax_scale(sf.f32_bits(5.0)) == sf.amax_scale(5.0) == 2.0 ** 8
    for v in (1.0, 3.7, 2.0 ** -30, 1e20):          # max|x| lands in [2^10, 2^11)
        assert 2.0 ** 10 <= v * sf.amax_scale(v) < 2.0 ** 11


def _range_values(n, lo, hi, g, planted):
    v = torch.exp2(lo + (hi - lo) * torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    idx = torch.randperm(n, generator=g)[:len(planted)]
    v[idx] = torch.tensor(planted, dtype=torch.float32)
    return v


X_PLANTED = [0.0, -0.0, 2.0 ** -5, -2.0 ** -5, 2.0 ** -27, -2.0 ** -27, 2.0 ** -28, -2.0 ** -28, 16375.0, -16375.0]
W_PLANTED = [0.0, -0.0, 2.0 ** -7, -2.0 ** -7, 2.0 ** -29, -2.0 ** -29, 2.0 ** -30, -2.0 ** -30, 4093.0, -4093.0]


def test_split_model_keeps_the_promised_precision():
    """max(2^-22 |v|, 2^-25 / s) over the whole range of both scales, subnormal halves kept; the flushing splitter breaks it."""
    g = _gen("model")
    for s, hi, planted in ((sf.XSPLIT, 13.9, X_PLANTED), (sf.WSPLIT, 11.9, W_PLANTED)):
        v = _range_values(20000, -30.0, hi, g, planted)
        h0, h1 = sf.split(v, s)
        err = (sf.decode(h0, h1, s).double() - v.double()).abs()
        assert bool((err <= sf.value_bound(v, s)).all())
        assert bool(((h1.float().abs() < sf.F16_MIN_NORMAL) & (h1 != 0)).any()), "no subnormal h1 in the sample"
        f0, f1 = sf.split_flush(v, s)
        assert bool(((sf.decode(f0, f1, s).double() - v.double()).abs() > sf.value_bound(v, s)).any())
    h0, h1 = sf.split(torch.tensor([2.0 ** -5, 16375.0, -0.0]), 4.0)
    assert h0.tolist() == [0.125, 65504.0, -0.0] and h1.tolist() == [0.0, -4.0, 0.0]


def _emulation_case(model, recipe):
    """-> (op, x, w, sx, sw) of one CPU demonstration: small instances of what the GPU tests run."""
    g = _gen("cpu", model, recipe)
    if model in ("conv", "conv small weights"):
        w = torch.randn(72, 64, 3, 3, generator=g) / 24 * (2.0 ** -9 if model != "conv" else 1.0)
        return _conv_op(pad=(1, 1)), sf.activations((1, 64, 12, 20), recipe, g), w, sf.XSPLIT, sf.WSPLIT
    stale = 2.0 ** STALE if model.endswith("stale") else 1.0
    if model.startswith("dgrad"):
        w = torch.randn(72, 64, 3, 3, generator=g) / 24
        x = sf.gradients((1, 64, 12, 20), recipe, g)
        return _conv_op(pad=(1, 1)), x, w, sf.XSPLIT * sf.amax_scale(float(x.abs().max()) * stale), sf.WSPLIT
    if model.startswith("wgrad"):      # x (activations) is the first operand, g the second
        x = sf.activations((2, 64, 12, 20), "wide+0", g)
        gr = sf.gradients((2, 72, 12, 20), recipe, g, along="pixels")
        return (lambda a, b: conv2d_weight(a, (72, 64, 3, 3), b, padding=1)), x, gr, sf.XSPLIT, sf.XSPLIT * sf.amax_scale(float(gr.abs().max()) * stale)
    assert model == "corr"
    a, b = (sf.activations((323, 256), recipe, g, clamp=4000.0, peak=4000.0, nplant=32) for _ in range(2))
    return _mm, a, b, sf.WSPLIT, sf.WSPLIT


STALE = 12          # a word 2^12 too large: the scale 2^12 too small, every h1 of the gradient subnormal

# (model, recipe, which flushed operands must be seen: "both" = every subnormal half (a matrix pipe that drops them), "first" /
# "second" = the halves of that operand alone (its loader))
EMULATION = ([("conv", r, ("both", "first") if r in ("uni-16", "uni-10", "uni-5", "wide+0") else ("both",)) for r in sf.FWD_RECIPES]
             + [("conv small weights", "wide+0", ("both", "second"))]
             + [("dgrad", r, ("both",)) for r in sf.GRAD_RECIPES]
             + [("dgrad stale", r, ("both", "first")) for r in sf.GRAD_RECIPES]
             + [("wgrad", r, ("both", "first")) for r in sf.GRAD_RECIPES]
             + [("wgrad stale", r, ("both", "first", "second")) for r in sf.GRAD_RECIPES]
             + [("corr", r, ("both", "first", "second") if r[:6] in ("uni-16", "uni-10") or r[:5] == "uni-5" else ()) for r in sf.CORR_RECIPES])


@pytest.mark.parametrize("model,recipe,must_see", EMULATION, ids=[f"{m}-{r}".replace(" ", "_") for m, r, _ in EMULATION])
def test_bound_holds_the_format_and_sees_a_flushing_loader(model, recipe, must_see):
    """The format to the letter stays at or below 0.5 B on every element; with subnormal halves flushed - all of them, or
    those of one operand - it exceeds B + 8 e32 where the module docstring says it must.  (A recipe that fails the first is
    changed, never the factor.)"""
    op, x, w, sx, sw = _emulation_case(model, recipe)
    ref, e32 = _ref(op, x, w)
    bnd = _bound(op, x, w, sx, sw)
    spec = float(((sf.emulate(op, x, w, sx, sw) - ref).abs() / bnd.clamp_min(1e-300)).max())
    over = lambda fx, fw: float(((sf.emulate(op, x, w, sx, sw, fx, fw) - ref).abs() / (bnd + 8 * e32).clamp_min(1e-300)).max())
    flush = {"both": over(sf.split_flush, sf.split_flush), "first": over(sf.split_flush, sf.split), "second": over(sf.split, sf.split_flush)}
    print(f"RANGE-CPU | {model} | {recipe} | spec err/B {spec:.3f} | flush err/(B + 8 e32): " + ", ".join(f"{k} {v:.2f}" for k, v in flush.items()))
    assert spec <= 0.5, f"{model} [{recipe}]: the emulation to the spec reaches {spec:.3f} B"
    for which in must_see:
        assert flush[which] > 1.0, f"{model} [{recipe}]: flushing the subnormal halves of `{which}` would pass ({flush[which]:.2f} of the allowance)"


# ----------------------------------------------------------------------------
# GPU: the storage format, bit for bit
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from focusflow_official_amd import ops as _ops
    assert _ops.conv_precision() == "f16x3"
    return _ops


def _halves(t):
    """raw fp32-typed storage -> the fp16 values it holds, last dimension doubled"""
    return t.cpu().contiguous().view(torch.float16)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (1, 3, 5, 96)], ids=["2x5x7x64", "1x3x5x96"])
def test_split_copy_stores_the_format_bit_for_bit(ops, shape):
    g = _gen("split_copy", shape)
    n = math.prod(shape)
    x = _range_values(n, -30.0, 13.9, g, X_PLANTED).view(shape)
    b, h, w, c = shape
    sp = ops.split_copy(x.to(DEV))
    raw = _halves(sp.t).view(b, h, w, c // 32, 2, 32)                    # [chunk][h0 | h1][32]
    h0, h1 = sf.split(x.view(b, h, w, c // 32, 32), sf.XSPLIT)
    assert _same_bits(raw[..., 0, :], h0), "first 64 bytes of the chunks: h0"
    assert _same_bits(raw[..., 1, :], h1), "second 64 bytes of the chunks: h1 (subnormal halves kept)"
    back = ops.split_copy(sp.t, to_split=False).cpu()
    assert torch.equal(back.view(torch.int32), sf.decode(h0, h1, sf.XSPLIT).view(shape).view(torch.int32)), "to_split=False: (h0 + h1) / 4 exactly"
    assert bool(((back.double() - x.double()).abs() <= sf.value_bound(x, sf.XSPLIT)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("rows,k", [(7, 96), (5, 70)], ids=["7x96", "5x70"])
def test_pack_split_stores_the_row_format_bit_for_bit(ops, rows, k):
    """[rows][ceil(K / 32)][h0: 32 fp16 | h1: 32 fp16] at scale 16, columns past K zero (ops.pack_split)."""
    g = _gen("pack_split", rows, k)
    wv = _range_values(rows * k, -30.0, 11.9, g, W_PLANTED).view(rows, k)
    assert float(wv.abs().max()) < sf.W_LIMIT
    nkc = (k + 31) // 32
    raw = ops.pack_split(wv.to(DEV)).cpu().view(torch.float16).view(rows, nkc, 2, 32)
    padded = torch.zeros(rows, nkc * 32)
    padded[:, :k] = wv
    h0, h1 = sf.split(padded.view(rows, nkc, 32), sf.WSPLIT)
    assert _same_bits(raw[:, :, 0], h0) and _same_bits(raw[:, :, 1], h1)


def _case(variant, ysplit=False):
    rows = [c for c in ROUTE_CASES if c.variant == variant and c.ysplit == ysplit]
    assert rows, variant
    return rows[0]


YSPLIT_FAMILIES = [c for c in ROUTE_CASES if c.ysplit and (c.variant.startswith("patch occ th4") or (c.variant.startswith("dma_f32") and c.variant.endswith("th4"))
                                                        or c.variant.startswith("split 64x64"))]


def test_every_split_store_family_has_its_row():
    names = sorted(c.variant for c in YSPLIT_FAMILIES)
    assert len(names) == 4 and names[0].startswith("dma_f32") and names[1].startswith("patch occ th4") and "gen" in names[2] and "uni" in names[3], names


@pytest.mark.gpu
@pytest.mark.parametrize("c", YSPLIT_FAMILIES, ids=lambda c: c.variant.replace(" ", "_"))
def test_epilogue_stores_keep_subnormal_halves(ops, c):
    """y_split=True: the same convolution into fp32 and into a split pair, out_scale 2^-9 so that 4 y sits below 2^-3: the
    decoded pair is within max(2^-22 |v|, 2^-27) of the fp32 output on every element."""
    assert _route_of(c).name == c.variant + " ysplit"
    xs, wt = _problem(c)[:2]
    xd = [x.permute(0, 2, 3, 1).contiguous().to(DEV) for x in xs]
    fmt = {"f16x3": 1, "f16": 2}[c.fmt]
    wp = _packed(ops, wt, c.fmt)
    kw = dict(act=NONE, out_scale=2.0 ** -9, w_fmt=fmt, dilation=c.dil)
    plain = ops.conv2d(xd, wp, None, c.cout, c.kh, c.kw, c.stride, c.pad, **kw)
    sp = ops.conv2d(xd, wp, None, c.cout, c.kh, c.kw, c.stride, c.pad, y_split=True, **kw)
    torch.cuda.synchronize()
    full = sp.t if sp.t.shape[3] % 32 == 0 else None
    if full is None:       # Cout off 32: the view's storage holds whole chunks (ops.conv2d)
        b, ho, wo, _ = sp.t.shape
        ld = sp.t.stride(2)
        full = sp.t.as_strided((b, ho, wo, ld), (ho * wo * ld, wo * ld, ld, 1))
    got = ops.split_copy(full, to_split=False)[..., :c.cout].cpu().double()
    v = plain.cpu()
    err = (got - v.double()).abs()
    frac = float(((v.abs() * sf.XSPLIT < 2.0 ** -3) & (v != 0)).float().mean())
    print(f"RANGE-STORE | {c.variant} | max err/bound {float((err / sf.value_bound(v, sf.XSPLIT)).max()):.3f} | outputs with subnormal h1 {frac:.2f}")
    assert frac > 0.9, "out_scale 2^-9 no longer puts the outputs where h1 is subnormal"
    assert bool(torch.isfinite(got).all()) and bool((err <= sf.value_bound(v, sf.XSPLIT)).all())


# ----------------------------------------------------------------------------
# GPU: every f16x3 loader over the input range, forward
# ----------------------------------------------------------------------------
FWD_FAMILIES = ["split 64x64 t3 uni", "split 64x64 t3 gen", "patch occ th4 t3", "patch occ th4 t3 +splitk", "patch gen th4 ni8 t3", "dma_f32 3x3 th4",
                "dma_f32 1x5 th4", "dma_f32 5x1 th4", "stem"]
FWD_RUNS = [(r, 1.0) for r in sf.FWD_RECIPES] + [("wide+0", 2.0 ** -9)]          # (input recipe, weight factor)
_RUN_IDS = [r if f == 1.0 else r + "-w2^-9" for r, f in FWD_RUNS]


def _nhwc_dev(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _conv_inputs(key, segs, cout, kh, kw, b, h, w, recipe, wfac, maker=sf.activations):
    g = _gen(key, recipe, wfac)
    cin = sum(segs)
    x = maker((b, cin, h, w), recipe, g)
    if cin == 4:             # the stem's NHWC4 image: the fourth channel is padding
        x[:, 3:] = 0
    wt = torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5 * wfac
    return x, wt


def _fwd_conv(ops, c, x, wt, split_in=False, **kw):
    xd, o = [], 0
    for s in c.segs:
        t = _nhwc_dev(x[:, o:o + s])
        xd.append(ops.split_copy(t) if split_in else t)
        o += s
    out = ops.conv2d(xd, _packed(ops, wt, "f16x3"), None, c.cout, c.kh, c.kw, c.stride, c.pad, act=NONE, w_fmt=1, dilation=c.dil, **kw)
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,wfac", FWD_RUNS, ids=_RUN_IDS)
@pytest.mark.parametrize("variant", FWD_FAMILIES, ids=lambda v: v.replace(" ", "_"))
def test_forward_loader_over_the_input_range(ops, variant, recipe, wfac):
    c = _case(variant)
    assert c.h * c.w <= 41 * 57 and _route_of(c).name == variant
    x, wt = _conv_inputs(variant, c.segs, c.cout, c.kh, c.kw, c.b, c.h, c.w, recipe, wfac)
    assert float(x.abs().max()) < sf.X_LIMIT and float(wt.abs().max()) < sf.W_LIMIT
    op = _conv_op(c.stride, c.pad, c.dil)
    ref, e32 = _ref(op, x, wt)
    bnd = _bound(op, x, wt, sf.XSPLIT, sf.WSPLIT)
    _hold(_fwd_conv(ops, c, x, wt), ref, bnd + 8 * e32, bnd, variant, recipe if wfac == 1.0 else recipe + " w*2^-9")


SPLIT_IN = ROUTE_CASES[0]._replace(variant="conv_dma split-pair input", segs=(128,), cout=64, kh=3, kw=3, stride=1, pad=(1, 1), dil=1, b=1, h=19, w=33, fmt="f16x3", ysplit=False)


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,wfac", FWD_RUNS, ids=_RUN_IDS)
def test_split_pair_input_over_the_input_range(ops, recipe, wfac):
    """The same convolution fed a split pair made by split_copy (conv_dma.hip's LDS-DMA loader; shape of test_hip_split.py)."""
    c = SPLIT_IN
    x, wt = _conv_inputs(c.variant, c.segs, c.cout, c.kh, c.kw, c.b, c.h, c.w, recipe, wfac)
    op = _conv_op(c.stride, c.pad)
    ref, e32 = _ref(op, x, wt)
    bnd = _bound(op, x, wt, sf.XSPLIT, sf.WSPLIT)
    _hold(_fwd_conv(ops, c, x, wt, split_in=True), ref, bnd + 8 * e32, bnd, c.variant, recipe if wfac == 1.0 else recipe + " w*2^-9")


def _frag(ops, wt):
    """OIHW weight -> (fragment-order split rows, split rows)"""
    cout, cin, kh, kw = wt.shape
    rows = _packed(ops, wt, "f16x3")
    return ops.pack_frag16(rows, cout), rows


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,wfac", FWD_RUNS, ids=_RUN_IDS)
@pytest.mark.parametrize("shape", [(1, 8, 16, 64), (2, 8, 12, 96)], ids=["c64", "c96"])
def test_fusion_pair_over_the_input_range(ops, shape, recipe, wfac):
    """ff_fusion_pair_fwd, plain inputs: img' = img + conv1x1(mask), mask' = mask + conv1x1(img); the residual is fp32."""
    b, h, w, c = shape
    g = _gen("fusion", shape, recipe, wfac)
    img, mask = (sf.activations((b, c, h, w), recipe, g) for _ in range(2))
    wa, wb = (torch.randn(c, c, 1, 1, generator=g) / c ** 0.5 * wfac for _ in range(2))
    fa, fb = _frag(ops, wa)[0], _frag(ops, wb)[0]
    img_o, mask_o = ops.fusion_pair(_nhwc_dev(img), _nhwc_dev(mask), (fa, fb), (None, None), 1)
    torch.cuda.synchronize()
    for name, got, base, x, wt in (("img'", img_o, img, mask, wa), ("mask'", mask_o, mask, img, wb)):
        ref = base.double() + F.conv2d(x.double(), wt.double())
        e32 = float(((base + F.conv2d(x, wt)).double() - ref).abs().max())
        bnd = _bound(F.conv2d, x, wt, sf.XSPLIT, sf.WSPLIT)
        _hold(got.permute(0, 3, 1, 2), ref, bnd + 8 * e32, bnd, f"fusion_pair C{c} {name}", recipe if wfac == 1.0 else recipe + " w*2^-9")


def _corr_maps(recipe, wfac, h=17, w=19):
    g = _gen("corr", recipe, wfac)
    f1, f2 = (sf.activations((h * w, 256), recipe, g, clamp=4000.0, peak=4000.0, nplant=32) for _ in range(2))
    f2 = f2 * wfac
    assert max(float(f1.abs().max()), float(f2.abs().max())) < sf.W_LIMIT
    return f1, f2


CORR_RUNS = [(r, 1.0) for r in sf.CORR_RECIPES] + [("rowwide+0", 2.0 ** -9)]
_CORR_IDS = [r if f == 1.0 else r + "-w2^-9" for r, f in CORR_RUNS]


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,wfac", CORR_RUNS, ids=_CORR_IDS)
def test_corr_build_over_the_input_range(ops, recipe, wfac):
    """ff_corr_build, level 0 at 17 x 19: both operands are rows (s = 16); the second run scales fmap2 by 2^-9."""
    h, w = 17, 19
    f1, f2 = _corr_maps(recipe, wfac)
    op = lambda a, b: _mm(a, b) / 16.0
    ref, e32 = _ref(op, f1, f2)
    bnd = _bound(op, f1, f2, sf.WSPLIT, sf.WSPLIT)
    pyr = ops.corr_build(f1.view(1, h, w, 256).to(DEV), f2.view(1, h, w, 256).to(DEV))
    got = pyr.rowmajor(0).view(h * w, h * w)
    torch.cuda.synchronize()
    _hold(got, ref, bnd + 8 * e32, bnd, "corr_build level 0", recipe if wfac == 1.0 else recipe + " fmap2*2^-9")


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,wfac", CORR_RUNS, ids=_CORR_IDS)
def test_corr_alt_lookup_over_the_input_range(ops, recipe, wfac):
    """ff_corr_alt_lookup at integer coordinates, 17 x 19: every output is a convex combination of dot products of fmap1 rows
    with rows of the pooled fmap2 levels, so the bound is the reference itself on absolute values (and on ones)."""
    from test_alt_corr import _pooled, alt_lookup_ref
    h, w = 17, 19
    f1, f2 = _corr_maps(recipe, wfac)
    n1, n2 = f1.view(1, h, w, 256).permute(0, 3, 1, 2).contiguous(), f2.view(1, h, w, 256).permute(0, 3, 1, 2).contiguous()
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    coords = torch.stack([xs, ys]).float().view(1, 2, h, w)
    look = lambda a, lv, dt: alt_lookup_ref(a.to(dt), [l.to(dt) for l in lv], coords.to(dt))
    lv64 = _pooled(n2.double())
    ref = look(n1, lv64, torch.float64)
    e32 = float((look(n1, _pooled(n2), torch.float32).double() - ref).abs().max())
    lva, ones = [l.abs() for l in lv64], [torch.ones_like(l) for l in lv64]
    bnd = sf.format_bound(look(n1.abs(), lva, torch.float64), look(torch.ones_like(n1), lva, torch.float64), look(n1.abs(), ones, torch.float64), sf.WSPLIT, sf.WSPLIT)
    alt = ops.corr_alt_prepare(_nhwc_dev(n1), _nhwc_dev(n2))
    got = ops.corr_alt_lookup(alt, _nhwc_dev(coords))
    torch.cuda.synchronize()
    _hold(got.permute(0, 3, 1, 2), ref, bnd + 8 * e32, bnd, "corr_alt_lookup", recipe if wfac == 1.0 else recipe + " fmap2*2^-9")


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,wfac", FWD_RUNS, ids=_RUN_IDS)
@pytest.mark.parametrize("direction", [0, 1], ids=["1x5", "5x1"])
def test_gru_pass_over_the_input_range(ops, direction, recipe, wfac):
    """ff_gru_pass at (1, 7, 50): z|r = sigmoid(conv([h, m])), q = tanh(conv([r h, m])), h' = (1 - z) h + z q, no bias and zero
    pre-activation terms.  B + 8 e32 of each pre-activation goes through sigmoid' <= 1/4 and tanh' <= 1; the error of r reaches
    the second convolution through |h| dr and |wq|; the blend adds |q - h| dz + z dq + dz dq and 8 times its own fp32 error."""
    b, h, w, c = 1, 7, 50, 128
    kh, kw = ((1, 5), (5, 1))[direction]
    pad = (kh // 2, kw // 2)
    g = _gen("gru", direction, recipe, wfac)
    x = sf.activations((b, 2 * c, h, w), recipe, g)
    hst, mot = x[:, :c].contiguous(), x[:, c:].contiguous()
    wzr = torch.randn(2 * c, 2 * c, kh, kw, generator=g) / (2 * c * 5) ** 0.5 * wfac
    wq = torch.randn(c, 2 * c, kh, kw, generator=g) / (2 * c * 5) ** 0.5 * wfac
    op = _conv_op(1, pad)
    # fp64 reference with the error budget carried along
    pre1, e1 = _ref(op, x, wzr)
    d1 = (_bound(op, x, wzr, sf.XSPLIT, sf.WSPLIT) + 8 * e1) / 4                      # sigmoid' <= 1/4
    zr = torch.sigmoid(pre1)
    z, r, dz, dr = zr[:, :c], zr[:, c:], d1[:, :c], d1[:, c:]
    x2 = torch.cat([r * hst.double(), mot.double()], 1)
    pre2, e2 = _ref(op, x2, wq)
    dx2 = torch.cat([hst.double().abs() * dr, torch.zeros_like(dr)], 1)
    dq = _bound(op, x2, wq, sf.XSPLIT, sf.WSPLIT) + 8 * e2 + op(dx2, wq.double().abs())    # tanh' <= 1
    q = torch.tanh(pre2)
    ref = (1 - z) * hst.double() + z * q
    z32, q32 = z.float(), q.float()
    e3 = float((((1 - z32) * hst + z32 * q32).double() - ref).abs().max())
    allowed = (q - hst.double()).abs() * dz + z * dq + dz * dq + 8 * e3
    bnd = allowed - 8 * e3
    hp, mp = _nhwc_dev(hst), _nhwc_dev(mot)
    zeros = lambda n: torch.zeros(b, h, w, n, device=DEV)
    fzr, fq = _frag(ops, wzr)[0], _frag(ops, wq)[0]
    h1, h1s = ops.gru_pass(direction, ops.split_copy(hp), ops.split_copy(mp), hp, zeros(2 * c), zeros(c), fzr, fq, torch.zeros(2 * c, device=DEV),
                           torch.zeros(c, device=DEV), 1)
    torch.cuda.synchronize()
    name = recipe if wfac == 1.0 else recipe + " w*2^-9"
    _hold(h1.permute(0, 3, 1, 2), ref, allowed, bnd, f"gru_pass {kh}x{kw}", name)
    # the split-pair copy of the new state: the fp32 one rounded into the format
    dec = ops.split_copy(h1s.t, to_split=False).cpu()
    assert bool(((dec.double() - h1.cpu().double()).abs() <= sf.value_bound(h1.cpu(), sf.XSPLIT)).all()), "split-pair copy of the new state"


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,wfac", FWD_RUNS, ids=_RUN_IDS)
def test_mask_upsample_over_the_input_range(ops, recipe, wfac):
    """ff_mask_upsample_fwd at (1, 13, 21): 0.25 * conv1x1(hid) -> soft-max over the nine neighbours -> convex combination of
    8 * flow.  The allowed error is the fp64 reference evaluated at pre-activation +- (B + 8 e32), each of the nine logits moved
    towards (and away from) the side of its flow value that moves the output most, plus 8 times the fp32 error of the soft-max
    and combination themselves.  (Moving all nine logits the same way changes nothing: the soft-max is shift-invariant.)"""
    b, h, w = 1, 13, 21
    g = _gen("mask", recipe, wfac)
    hid = sf.activations((b, 256, h, w), recipe, g)
    wt = torch.randn(576, 256, 1, 1, generator=g) / 16 * wfac
    flow = torch.randn(b, 2, h, w, generator=g) * 3
    op = lambda a, k: 0.25 * F.conv2d(a, k)
    pre, e32 = _ref(op, hid, wt)
    d = (_bound(op, hid, wt, sf.XSPLIT, sf.WSPLIT) + 8 * e32).view(b, 1, 9, 8, 8, h, w)

    def combine(m, dt):
        uf = F.unfold(8 * flow.to(dt), [3, 3], padding=1).view(b, 2, 9, 1, 1, h, w)
        return torch.sum(torch.softmax(m.to(dt), dim=2) * uf, dim=2), uf

    m = pre.view(b, 1, 9, 8, 8, h, w)
    ref7, uf = combine(m, torch.float64)
    e_c = float((combine(m, torch.float32)[0].double() - ref7).abs().max())
    s = torch.sign(uf - ref7.unsqueeze(2))                       # raising a logit pulls the output towards its flow value
    up = torch.sum(torch.softmax(m + s * d, dim=2) * uf, dim=2) - ref7
    dn = ref7 - torch.sum(torch.softmax(m - s * d, dim=2) * uf, dim=2)
    bnd7 = torch.maximum(up, dn).clamp_min(0)
    fin = lambda t: t.permute(0, 1, 4, 2, 5, 3).reshape(b, 2, 8 * h, 8 * w)
    rows = torch.empty(576, 256, device=DEV)
    ops.pack_conv_weight(wt.to(DEV), rows, 256)
    flow4 = torch.zeros(b, h, w, 4, device=DEV)
    flow4[..., :2] = _nhwc_dev(flow)
    got = ops.mask_upsample(_nhwc_dev(hid), ops.mask_upsample_pack(ops.pack_split(rows)), 1, None, flow4, 0.25)
    torch.cuda.synchronize()
    _hold(got, fin(ref7), fin(bnd7) + 8 * e_c, fin(bnd7), "mask_upsample", recipe if wfac == 1.0 else recipe + " w*2^-9")


# ----------------------------------------------------------------------------
# GPU: the x_amax path - input gradients and weight gradients
# ----------------------------------------------------------------------------
def _amax_word(ops, g_nhwc):
    """The device word ff_act_bwd leaves: the bits of float32(max|g|), exactly."""
    b, h, w, c = g_nhwc.shape
    g2, word = ops.act_bwd(g_nhwc, None, NONE, 1.0, c, want_amax=True)
    assert g2.data_ptr() == g_nhwc.data_ptr()
    bits = int(word.cpu().item()) & 0xFFFFFFFF
    assert bits == sf.f32_bits(float(g_nhwc.abs().max().cpu())), "ff_act_bwd's amax word is not the bits of max|g|"
    return word, bits


# (variant of the input-gradient convolution, Cout of the forward conv = channels of g, Cin of the forward conv = channels of dx, kernel, B, H, W)
DGRAD_CASES = [
    ("patch occ th4 t3", 64, 72, (1, 5), 1, 19, 33),
    ("dma_f32 3x3 th4", 128, 72, (3, 3), 1, 19, 33),
    ("split 64x64 t3 uni", 64, 96, (1, 1), 1, 17, 23),
    ("split 64x64 t3 gen", 324, 250, (1, 1), 1, 16, 24),
    ("patch gen th4 ni8 t3", 32, 64, (7, 7), 1, 19, 33),
    ("patch occ th4 t3 +splitk", 672, 32, (3, 3), 1, 14, 32),
]
_DGRAD_IDS = [d[0].replace(" ", "_") for d in DGRAD_CASES]


def _dgrad_setup(ops, case):
    """-> (forward weight OIHW on the CPU, its input-gradient rows (ops.pack_conv_weight_dgrad + pack_split), geometry)"""
    variant, cg, cdx, (kh, kw), b, h, w = case
    pad = (kh // 2, kw // 2)
    assert route((cg,), cdx, kh, kw, 1, pad, 1, b, h, w, "f16x3").name == variant
    g = _gen("dgrad w", case)
    wt = torch.randn(cg, cdx, kh, kw, generator=g) / (cg * kh * kw) ** 0.5            # forward conv cdx -> cg
    rows = torch.zeros(cdx, kh * kw * cg, device=DEV)
    ops.pack_conv_weight_dgrad(wt.to(DEV), rows, cg, 0)
    return wt, ops.pack_split(rows), pad


def _dgrad_run(ops, case, wd, pad, g_nhwc, word):
    variant, cg, cdx, (kh, kw), b, h, w = case
    out = ops.conv2d([g_nhwc], wd, None, cdx, kh, kw, 1, (kh - 1 - pad[0], kw - 1 - pad[1]), w_fmt=1, x_amax=word)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("stale", [0, STALE], ids=["fresh", f"stale2^{STALE}"])
@pytest.mark.parametrize("recipe", sf.GRAD_RECIPES)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_DGRAD_IDS)
def test_input_gradient_over_the_gradient_range(ops, case, recipe, stale):
    """fresh: the word of g itself.  stale: the word of g * 2^12 - every h1 of g is then subnormal without a single large
    value in the tensor, which is where a gradient loader that flushes shows (CPU demonstration: 7 - 18 times the allowance;
    with the fresh word the large values that set it also set e32, and hide it)."""
    variant, cg, cdx, (kh, kw), b, h, w = case
    wt, wd, pad = _dgrad_setup(ops, case)
    g = sf.gradients((b, cg, h, w), recipe, _gen("dgrad g", case, recipe))
    gd = _nhwc_dev(g)
    word, bits = _amax_word(ops, gd * 2.0 ** stale)
    op = lambda a, k: F.conv_transpose2d(a, k, padding=pad)
    ref, e32 = _ref(op, g, wt)
    bnd = _bound(op, g, wt, sf.XSPLIT * sf.amax_scale(bits), sf.WSPLIT)
    out = _dgrad_run(ops, case, wd, pad, gd, word)
    _hold(out.permute(0, 3, 1, 2), ref, bnd + 8 * e32, bnd, "dgrad " + variant, recipe + (f" stale 2^{stale}" if stale else ""))


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", ["uni+0", "wide+0"])
@pytest.mark.parametrize("case", [d for d in DGRAD_CASES if "splitk" not in d[0]], ids=[i for i in _DGRAD_IDS if "splitk" not in i])
def test_input_gradient_is_scale_invariant_bit_for_bit(ops, case, recipe):
    """g * 2^k with its own amax word gives the output of g times 2^k, bit for bit: the scale is a power of two keyed on the
    exponent of max|g|, so the halves the matrix pipe sees are the same (variants without K splits or atomics)."""
    variant, cg, cdx, (kh, kw), b, h, w = case
    wt, wd, pad = _dgrad_setup(ops, case)
    g = sf.gradients((b, cg, h, w), recipe, _gen("dgrad g", case, recipe))
    gd = _nhwc_dev(g)
    base = _dgrad_run(ops, case, wd, pad, gd, _amax_word(ops, gd)[0])
    for k in (-40, 17):
        gk = gd * 2.0 ** k
        outk = _dgrad_run(ops, case, wd, pad, gk, _amax_word(ops, gk)[0])
        assert torch.equal(outk.view(torch.int32), (base * 2.0 ** k).view(torch.int32)), f"{variant}: g * 2^{k} is not the output of g times 2^{k}"


# (form, segments, Cout, kernel, stride, pad, B, H, W): conv_wgrad_split.hip's three tiles where conv_wgrad_patch.hip declines
# (1x1, stride 2), and conv_wgrad_patch.hip's three launch forms
WGRAD_CASES = [
    ("split 64x128", [64], 64, (1, 1), 1, (0, 0), 2, 16, 24),
    ("split 128x64", [64], 96, (3, 3), 2, (1, 1), 2, 32, 48),
    ("split 128x128", [96], 96, (3, 3), 2, (1, 1), 1, 23, 37),
    ("patch 3x3", [96], 96, (3, 3), 1, (1, 1), 1, 23, 37),
    ("patch 5x1", [32], 64, (5, 1), 1, (2, 0), 2, 9, 17),
    ("patch 1x5", [32, 32], 40, (1, 5), 1, (0, 2), 2, 8, 16),
]
_WGRAD_IDS = [c[0].replace(" ", "_") for c in WGRAD_CASES]


def test_weight_gradient_forms_still_stand_in_the_sources():
    """Which kernel a weight gradient gets, found in the sources by plain text search (a change there: re-derive WGRAD_CASES)."""
    csrc = os.path.join(ROOT, "focusflow_official_amd", "csrc")
    want = {"conv_wgrad_split.hip": ["if (p.Cout <= 64) return launch<64, 128>(a, M, s);", "const bool big = (p.Cout > 128 && a.K >= 1024) || (p.Cout == 96 && a.K >= 864);",
                                     "return launch<128, 64>(a, M, s);"],
            "conv_wgrad_patch.hip": ["if (p.stride != 1 || dlh != 1 || dlw != 1 || p.groups != 1) return 1;",
                                     "if (!((p.KH == 3 && p.KW == 3) || (p.KH == 1 && p.KW == 5) || (p.KH == 5 && p.KW == 1))) return 1;", "if (cin % 32) return 1;",
                                     "if (taps == 9) return launch<5, 6>(a, lds, splits, s);"]}
    for name, needles in want.items():
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        for n in needles:
            assert n in text, f"{name} no longer holds `{n}`"
    for form, segs, cout, (kh, kw), stride, pad, b, h, w in WGRAD_CASES:
        k = sum(segs) * kh * kw
        patch = stride == 1 and (kh, kw) in ((3, 3), (1, 5), (5, 1)) and all(s % 32 == 0 for s in segs)
        tile = "64x128" if cout <= 64 else "128x128" if (cout > 128 and k >= 1024) or (cout == 96 and k >= 864) else "128x64"
        assert form == (f"patch {kh}x{kw}" if patch else f"split {tile}"), form


def _wgrad_problem(case, recipe):
    form, segs, cout, (kh, kw), stride, pad, b, h, w = case
    g = _gen("wgrad", case, recipe)
    cin = sum(segs)
    ho, wo = (h + 2 * pad[0] - kh) // stride + 1, (w + 2 * pad[1] - kw) // stride + 1
    x = sf.activations((b, cin, h, w), "wide+0", g)
    gr = sf.gradients((b, cout, ho, wo), recipe, g, along="pixels") if isinstance(recipe, str) else recipe(b, cout, ho, wo, g)
    return x, gr


def _wgrad_run(ops, case, x, gr, word):
    form, segs, cout, (kh, kw), stride, pad, b, h, w = case
    xd, o = [], 0
    for s in segs:
        xd.append(_nhwc_dev(x[:, o:o + s]))
        o += s
    dw, db = ops.conv2d_wgrad(xd, _nhwc_dev(gr), cout, kh, kw, stride, pad, g_amax=word, want_db=True)
    torch.cuda.synchronize()
    return dw.view(cout, kh, kw, sum(segs)).permute(0, 3, 1, 2), db


def _wgrad_check(case, x, gr, gs, dw, db, recipe):
    """dW and db against fp64; x is split at scale 4, g at 4 * gs (conv_wgrad_split.hip / conv_wgrad_patch.hip: both operands
    as activations); db is a plain fp32 sum of g - held to the bound of a sum whose other operand is exactly 1."""
    form, segs, cout, (kh, kw), stride, pad, b, h, w = case
    op = lambda a, k: conv2d_weight(a, (cout, sum(segs), kh, kw), k, stride=stride, padding=pad)
    ref, e32 = _ref(op, x, gr)
    bnd = _bound(op, x, gr, sf.XSPLIT, sf.XSPLIT * gs)
    _hold(dw, ref, bnd + 8 * e32, bnd, "wgrad " + form + " dW", recipe)
    g64 = gr.double()
    rb = g64.sum(dim=(0, 2, 3))
    eb = float((gr.sum(dim=(0, 2, 3)).double() - rb).abs().max())
    bb = sf.REL * g64.abs().sum(dim=(0, 2, 3)) + sf.ABS / (sf.XSPLIT * gs) * (gr.numel() // cout)
    _hold(db, rb, bb + 8 * eb, bb, "wgrad " + form + " db", recipe)


@pytest.mark.gpu
@pytest.mark.parametrize("stale", [0, STALE], ids=["fresh", f"stale2^{STALE}"])
@pytest.mark.parametrize("recipe", sf.GRAD_RECIPES)
@pytest.mark.parametrize("case", WGRAD_CASES, ids=_WGRAD_IDS)
def test_weight_gradient_over_the_gradient_range(ops, case, recipe, stale):
    x, gr = _wgrad_problem(case, recipe)
    word, bits = _amax_word(ops, _nhwc_dev(gr) * 2.0 ** stale)
    dw, db = _wgrad_run(ops, case, x, gr, word)
    _wgrad_check(case, x, gr, sf.amax_scale(bits), dw, db, recipe + (f" stale 2^{stale}" if stale else ""))


EDGE_DGRAD = [DGRAD_CASES[0], DGRAD_CASES[2], DGRAD_CASES[1]]          # conv_patch.hip, conv_split.hip, conv_dma.hip
EDGE_WGRAD = [WGRAD_CASES[0], WGRAD_CASES[3]]                          # conv_wgrad_split.hip, conv_wgrad_patch.hip


@pytest.mark.gpu
def test_all_zero_gradient_gives_exact_zeros(ops):
    """max|g| = 0: the word is 0, the scale 1, and dx, dW, db are exactly zero (no 0 * inf)."""
    for case in EDGE_DGRAD:
        variant, cg, cdx, (kh, kw), b, h, w = case
        wt, wd, pad = _dgrad_setup(ops, case)
        gd = torch.zeros(b, h, w, cg, device=DEV)
        word, bits = _amax_word(ops, gd)
        assert bits == 0
        out = _dgrad_run(ops, case, wd, pad, gd, word)
        assert int((out != 0).sum()) == 0 and bool(torch.isfinite(out).all()), variant
    for case in EDGE_WGRAD:
        x, gr = _wgrad_problem(case, lambda b, c, ho, wo, g: torch.zeros(b, c, ho, wo))
        word, bits = _amax_word(ops, _nhwc_dev(gr))
        dw, db = _wgrad_run(ops, case, x, gr, word)
        assert bits == 0 and int((dw != 0).sum()) == 0 and int((db != 0).sum()) == 0, case[0]


@pytest.mark.gpu
def test_stale_amax_word_still_meets_its_own_bound(ops):
    """A word left from a 2^20 times larger tensor: the scale is 2^20 too small, the format coarser by as much - and the result
    within the bound computed with THAT word's scale."""
    for case in EDGE_DGRAD:
        variant, cg, cdx, (kh, kw), b, h, w = case
        wt, wd, pad = _dgrad_setup(ops, case)
        g = sf.gradients((b, cg, h, w), "uni+0", _gen("stale", case))
        gd = _nhwc_dev(g)
        word, bits = _amax_word(ops, gd * 2.0 ** 20)
        assert sf.amax_scale(bits) * 2.0 ** 20 == sf.amax_scale(float(g.abs().max()))
        op = lambda a, k: F.conv_transpose2d(a, k, padding=pad)
        ref, e32 = _ref(op, g, wt)
        bnd = _bound(op, g, wt, sf.XSPLIT * sf.amax_scale(bits), sf.WSPLIT)
        _hold(_dgrad_run(ops, case, wd, pad, gd, word).permute(0, 3, 1, 2), ref, bnd + 8 * e32, bnd, "dgrad " + variant, "stale word 2^20")
    for case in EDGE_WGRAD:
        x, gr = _wgrad_problem(case, "uni+0")
        word, bits = _amax_word(ops, _nhwc_dev(gr) * 2.0 ** 20)
        dw, db = _wgrad_run(ops, case, x, gr, word)
        _wgrad_check(case, x, gr, sf.amax_scale(bits), dw, db, "stale word 2^20")


@pytest.mark.gpu
def test_subnormal_amax_takes_scale_one(ops):
    """max|g| = 2^-140 (biased exponent 0): scale 1, finite outputs within the bound of scale 1."""
    tiny = lambda b, c, ho, wo, g: torch.randint(-8, 9, (b, c, ho, wo), generator=g).double().mul(2.0 ** -143).float()
    for case in EDGE_DGRAD:
        variant, cg, cdx, (kh, kw), b, h, w = case
        wt, wd, pad = _dgrad_setup(ops, case)
        g = tiny(b, cg, h, w, _gen("tiny", case))
        assert float(g.abs().max()) == 2.0 ** -140
        gd = _nhwc_dev(g)
        word, bits = _amax_word(ops, gd)
        assert sf.amax_scale(bits) == 1.0
        op = lambda a, k: F.conv_transpose2d(a, k, padding=pad)
        ref, e32 = _ref(op, g, wt)
        bnd = _bound(op, g, wt, sf.XSPLIT, sf.WSPLIT)
        _hold(_dgrad_run(ops, case, wd, pad, gd, word).permute(0, 3, 1, 2), ref, bnd + 8 * e32, bnd, "dgrad " + variant, "max|g| 2^-140")
    for case in EDGE_WGRAD:
        x, gr = _wgrad_problem(case, tiny)
        word, bits = _amax_word(ops, _nhwc_dev(gr))
        dw, db = _wgrad_run(ops, case, x, gr, word)
        _wgrad_check(case, x, gr, 1.0, dw, db, "max|g| 2^-140")
