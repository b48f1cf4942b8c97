"""Plain references of the kernels that exist only for the recorded update loop (csrc/train_ops.hip, tests/test_train_ops.py):
the three gate-gradient steps between the input-gradient convolutions of a SepConvGRU pass, and the sum over a stack.  CPU
only, NHWC (channels last), no project code; every function computes in the dtype it is handed - the tests hand it float64.

    blend    h' = (1 - z) h + z q        d = d h' (+ the later pass's d h)      g_z = d (q - h) z (1 - z)
                                          g_q = d z (1 - q^2)                    d h = d (1 - z)
    rh       rh = r h                     g_r = d rh  h r (1 - r)                d h += d rh  r
    out      behind pass 1's z|r dgrad    d h += its first half                  g_m = (d m + its second half) [c < Cm, motion > 0]

`d m` collects the motion features' gradient: four contributions an iteration, the second halves of the four input-gradient
convolutions ([d h | d motion] of z|r, [d (r h) | d motion] of q).  The first one (pass 2's q) initialises it.
"""
from functools import lru_cache

import torch


def blend(dh_in, z, q, h, dzc=None, dm=None):
    """-> g_z, g_q, dh_out, dm_out.  dzc: (.., 2C) = [d h | d motion] of the LATER pass's z|r input gradient or None; with it
    dm_out = dm + its second half, without it dm comes back as it went in (None included)."""
    c = z.shape[-1]
    d = dh_in if dzc is None else dh_in + dzc[..., :c]
    dm_out = dm if dzc is None else dm + dzc[..., c:2 * c]
    return d * (q - h) * z * (1 - z), d * z * (1 - q * q), d * (1 - z), dm_out


def rh(dqc, r, h, dh, dm, dm_init):
    """-> g_r, dh_out, dm_out.  dqc: (.., 2C) = [d (r h) | d motion] of the q input gradient; dm_init: dm is not read."""
    c = r.shape[-1]
    drh, dmo = dqc[..., :c], dqc[..., c:2 * c]
    return drh * h * r * (1 - r), dh + drh * r, dmo.clone() if dm_init else dm + dmo


def out(dh, dzc, dm, motion, cm):
    """-> dh_out, g_m.  motion: the forward's [relu(.) in channels < cm | flow]; dm is only read."""
    c = dh.shape[-1]
    g = dm + dzc[..., c:2 * c]
    keep = (motion > 0) & (torch.arange(c) < cm)
    return dh + dzc[..., :c], torch.where(keep, g, torch.zeros_like(g))


def sum_stack(src):
    """(T, n) -> (n,)"""
    return src.sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# the operator tests' data: (B, H, W, C, Cm), fp32 draws and the fp64 results of the three steps on them, computed once
SHAPES = [
    (1, 1, 3, 128, 126),        # 96 work items: less than one block, whole waves idle
    (2, 5, 7, 8, 6),            # any C % 4 == 0; Cm cuts a 4-vector
    (2, 16, 24, 128, 126),      # the loop tests' size
    (3, 47, 61, 128, 126),      # 8601 pixels, 275232 items > 1024 x 256: the grid-stride loop, its second trip ragged
]


def shape_id(s):
    return "b{}-{}x{}-c{}-cm{}".format(*s)


@lru_cache(maxsize=None)
def case(shape, cm=None):
    """dict of CPU tensors: the fp32 inputs (z, r as rand; q, h as tanh(randn); motion as relu(randn), about half of it exact
    zeros; every gradient as randn) and, under "ref", the fp64 results of each step on exactly these values."""
    b, hh, ww, c, cm0 = shape
    cm = cm0 if cm is None else cm
    g = torch.Generator().manual_seed(7000 + b * hh * ww + c + cm)
    pix = (b, hh, ww)
    x = dict(z=torch.rand((*pix, c), generator=g), r=torch.rand((*pix, c), generator=g),
             q=torch.tanh(torch.randn((*pix, c), generator=g)), h=torch.tanh(torch.randn((*pix, c), generator=g)),
             motion=torch.relu(torch.randn((*pix, c), generator=g)),
             dh=torch.randn((*pix, c), generator=g), dm=torch.randn((*pix, c), generator=g),
             dzc=torch.randn((*pix, 2 * c), generator=g), dqc=torch.randn((*pix, 2 * c), generator=g))
    d = {k: v.double() for k, v in x.items()}
    ref = {}
    ref["blend"] = blend(d["dh"], d["z"], d["q"], d["h"])                              # g_z, g_q, dh_out, dm (= None)
    ref["blend_dzc"] = blend(d["dh"], d["z"], d["q"], d["h"], d["dzc"], d["dm"])
    ref["rh_init"] = rh(d["dqc"], d["r"], d["h"], d["dh"], None, True)                 # g_r, dh_out, dm_out
    ref["rh_add"] = rh(d["dqc"], d["r"], d["h"], d["dh"], d["dm"], False)
    ref["out"] = out(d["dh"], d["dzc"], d["dm"], d["motion"], cm)                      # dh_out, g_m
    x["ref"] = ref
    x["cm"] = cm
    return x
