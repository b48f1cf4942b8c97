"""The fp16x3 split format of csrc/ff_common.h as a CPU model (torch half keeps subnormals), written from that header alone.

An fp32 value v travels as h0 = f16(s v), h1 = f16(s v - h0) at ONE power-of-two scale s: 4 for activations (XSPLIT), 16
for packed rows (WSPLIT); gradients get the extra power of two of `input_scale` (FFConvParams.x_amax) that puts max|g| at
2^10.  A product is x w ~ (x0 w0 + x0 w1 + x1 w0) / (sx sw); x1 w1 is dropped.  The header promises a representation
error of max(2^-22 |v|, 2^-25 / s) per value, which rests on h1 being KEPT when it is a subnormal half (|s v| < 2^-3).
`split_flush` is the defect the range tests must be able to see: the same split with every subnormal half set to zero.

format_bound is the per-output-element error the format allows a dot product; a GPU result may differ from fp64 by
format_bound + 8 e32 (e32 = max|CPU fp32 - fp64| of the same operation, the factor the exact route is granted).
"""
import struct

import torch

XSPLIT, WSPLIT, SPLIT_INV = 4.0, 16.0, 1.0 / 64.0      # ff_common.h; held to it by test_split_range.py
AMAX_BIAS, AMAX_CLAMP = 137, 100                       # input_scale: k = clamp(137 - e, -100, 100)
REL = 2.0 ** -22                                       # relative error of a split value
ABS = 2.0 ** -25                                       # absolute error of s v (half an ulp of the smallest subnormal half, 2^-24)
F16_MIN_NORMAL = 2.0 ** -14
X_LIMIT, W_LIMIT = 16376.0, 4094.0                     # |x| < 16376 (activations), |w| < 4094 (packed rows)


def split(v, s):
    """-> (h0, h1) in torch.float16, round to nearest even, subnormal halves kept.  v: fp32 tensor, s: power of two."""
    sv = v.float() * torch.tensor(s, dtype=torch.float32)
    h0 = sv.half()
    h1 = (sv - h0.float()).half()
    return h0, h1


def _flush(h):
    return torch.where(h.float().abs() < F16_MIN_NORMAL, torch.zeros_like(h), h)


def split_flush(v, s):
    """split() as a loader that flushes subnormal halves would make it."""
    h0, h1 = split(v, s)
    h0 = _flush(h0)
    sv = v.float() * torch.tensor(s, dtype=torch.float32)
    return h0, _flush((sv - h0.float()).half())


def decode(h0, h1, s):
    """The fp32 value a pair stands for: (h0 + h1) / s (exact in fp32: 22 significant bits)."""
    return (h0.float() + h1.float()) / s


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def amax_scale(max_abs):
    """input_scale of ff_common.h: the power of two that puts max|x| at 2^10, from the biased exponent of the fp32 word
    holding max|x|.  `max_abs`: a float, or the word itself as an int."""
    word = max_abs if isinstance(max_abs, int) else f32_bits(max_abs)
    e = (word >> 23) & 0xFF
    if e == 0 or e == 255:
        return 1.0
    k = max(-AMAX_CLAMP, min(AMAX_CLAMP, AMAX_BIAS - e))
    return 2.0 ** k


def format_bound(absx_conv_absw, sum_absw, sum_absx, sx, sw):
    """B = 2^-22 sum|x||w| + (2^-25 / sx) sum|w| + (2^-25 / sw) sum|x|, the sums over the taps of one output element
    (tensors from the operation itself on absolute values in fp64, or floats)."""
    return REL * absx_conv_absw + (ABS / sx) * sum_absw + (ABS / sw) * sum_absx


def value_bound(v, s):
    """max(2^-22 |v|, 2^-25 / s): the representation error of one stored value."""
    return torch.clamp(REL * v.double().abs(), min=ABS / s)


def emulate(op, x, w, sx, sw, splitter=split, splitter_w=None):
    """The three-term product with fp64 accumulation: op(x0, w0) + op(x0, w1) + op(x1, w0), over (sx sw).  `op` is bilinear
    in fp64 tensors (F.conv2d, a matmul ...).  `splitter` makes the halves of x, `splitter_w` those of w (default: the same)."""
    x0, x1 = (h.double() for h in splitter(x, sx))
    w0, w1 = (h.double() for h in (splitter_w or splitter)(w, sw))
    return (op(x0, w0) + op(x0, w1) + op(x1, w0)) / (sx * sw)


# ----------------------------------------------------------------------------
# input recipes (shared by the CPU demonstration and the GPU tests)
# ----------------------------------------------------------------------------
# uniE: no planted values - the recipes that can see a flushing LOADER (a planted 16375 among 2^-10-scale values puts e32, a
# maximum over the whole output, a thousand times above the ordinary outputs).  uniE+peak: the same with planted values.
UNIFORM_E = (-16, -10, -5, 0, 6, 12)
WIDE_E = (0, 12)
FWD_RECIPES = [f"uni{e:+d}" for e in UNIFORM_E] + [f"uni{e:+d}+peak" for e in UNIFORM_E] + [f"wide{e:+d}" for e in WIDE_E]
CORR_RECIPES = [f"uni{e:+d}" for e in UNIFORM_E] + [f"uni{e:+d}+peak" for e in UNIFORM_E] + [f"rowwide{e:+d}" for e in WIDE_E]
GRAD_UNIFORM_E = (-60, -30, -14, 0, 20, 60)
GRAD_WIDE_E = (-30, 0)
GRAD_RECIPES = [f"uni{e:+d}" for e in GRAD_UNIFORM_E] + [f"wide{e:+d}" for e in GRAD_WIDE_E]


def _plant(x, g, values, along="channels"):
    """Plants `values` side by side where a reduction sees them together.  x: (B, C, H, W) or (rows, C).  "channels":
    channels 0 .. of one random pixel (of as many neighbouring pixels as it takes when the tensor has fewer channels) - for
    reductions over channels and taps; "pixels": consecutive pixels of channel 0 - for the weight gradient's reduction over
    pixels.  Side by side, because an output element that sees ONE planted value alone is a single product, whose error is
    one rounding of one operand: up to the whole of the format's bound, which is sized for sums."""
    c = x.shape[1]
    flat = x.view(x.shape[0], c, -1) if x.dim() == 4 else x.t().reshape(1, c, -1)
    per = c if along == "channels" else 1
    npix = -(-len(values) // per)
    b = int(torch.randint(flat.shape[0], (1,), generator=g))
    p0 = int(torch.randint(flat.shape[2] - npix + 1, (1,), generator=g))
    for i, v in enumerate(values):
        flat[b, i % per, p0 + i // per] = v
    if x.dim() != 4:
        x.copy_(flat[0].t().reshape(x.shape))
    return x


def activations(shape, recipe, g, clamp=16000.0, peak=16375.0, nplant=8):
    """uniE: randn * 2^E, clamped; uniE+peak: with `nplant` elements planted at +-peak (side by side: _plant).  wideE: randn *
    2^(-16 u) * 2^E, u uniform in [0, 1] per element; rowwideE: u per row of a (rows, C) operand (the correlation's recipe)."""
    planted = recipe.endswith("+peak")
    core = recipe[:-5] if planted else recipe
    e = float(core.lstrip("rowideun"))
    x = torch.randn(shape, generator=g)
    if core.startswith("rowwide"):
        x = x * torch.exp2(-16.0 * torch.rand((shape[0], 1), generator=g))
    elif core.startswith("wide"):
        x = x * torch.exp2(-16.0 * torch.rand(shape, generator=g))
    x = (x * 2.0 ** e).clamp(-clamp, clamp).contiguous()
    if planted:
        _plant(x, g, [peak, -peak] * (nplant // 2))
    return x


def gradients(shape, recipe, g, along="channels"):
    """uniE: randn * 2^E.  wideE: log-uniform over 24 binades below 2^E, twenty outliers at 3e4 * 2^E (side by side: _plant)."""
    e = float(recipe.lstrip("wideun"))
    x = torch.randn(shape, generator=g)
    if recipe.startswith("wide"):
        x = x * torch.exp2(-24.0 * torch.rand(shape, generator=g))
        _plant(x, g, [3e4, -3e4] * 10, along)
    return (x.double() * 2.0 ** e).float().contiguous()
