"""Every convolution kernel variant the forward dispatchers can choose, against F.conv2d in float64.

Which kernel a convolution gets is decided from its shape alone (the product build reads no tuning variable:
csrc/ff_common.h tune_env returns null there).  `route()` below restates that decision - ff_conv2d_fwd (conv_mfma.hip),
conv2d_fwd_split (conv_split.hip), conv2d_fwd_patch (conv_patch.hip), f32_route (conv_dma.hip) and the split-K decision of
ops.conv2d - as block-count arithmetic; ROUTE_CASES holds, for every variant of ALL_VARIANTS, the smallest shapes that
reach it at least 10 % past its threshold, with ragged edges (M off 128, H off the tile height, W off 16, Cout off the N
tile).  The CPU tests hold the table to the mirror, the mirror's literal thresholds to the sources (a changed threshold
fails there: re-derive the shapes), and the mirror to the library's own host-side answers (ff_conv2d_stats_parts,
ff_conv2d_splitk_hint: tile height and K splits are visible in the counts).

Each forward case runs the whole epilogue (bias, out_scale, ch_scale / ch_shift, activation, residual + act_res) over
inputs that are channel slices of wider buffers, into the view buf[1:B+1, :, :, 8:8+Cout] of a buffer pre-filled with a
finite sentinel: values against fp64, every sentinel element bit-identical afterwards (a ragged tile that writes outside
its output), a second call bit-identical to the first.

Variants (name: instantiation)
  small                         conv_small.hip, 1- / 2-channel 3x3 heads in fp32 rows
  mfma32 64x64 / 128x64 / 128x96 / 128x128
                                conv_mfma.hip launch<2,2,1,1> / <2,2,2,1> / <4,1,1,3> / <2,2,2,2>
  stem                          conv_stem.hip (7x7 stride 2 over NHWC4, f16x3)
  split 64x64 | 128x64 | 128x96, t3 | t1, uni | gen
                                conv_split.hip launch<2,2,1,1> (ring of 3) / <2,2,2,1> (_occ, 4 blocks per CU) / <4,1,1,3> (_occ, 3);
                                three-term (f16x3) or one-term (f16); uniform (every segment % 32 == 0) or generic loader
  patch occ th8 | th4, t3 | t1  conv_patch.hip launch_occ<3,6,2,1,4> / <3,4,1,1,5>, launch_occ_f16<6,2,1,4> / <4,1,1,5>
        ... +splitk             the 4-row three-term variant with K splits (ops.conv2d asks ff_conv2d_splitk_hint)
  patch gen th8 ni10 | th4 ni8, t3 | t1
                                conv_patch.hip FF_PATCH_CASE(8,1,10) / (4,1,8)
  dma_f32 3x3 th8 nw6 | 3x3 th8 nw4 | 3x3 th4 | 1x5 th8 | 1x5 th4 | 5x1 th8 | 5x1 th4
                                conv_dma.hip launch_f32<3,3,8,3,6> / <3,3,8,3,4> / <3,3,4,4,4> / <1,5,8,3,4> / <1,5,4,4,4> /
                                <5,1,8,3,4> / <5,1,4,4,4>
MODE_CASES adds normalise-on-load (in_scale), epilogue statistics (want_stats) and both at once for every family that
has them (the four patch occ variants, the three dma_f32 3x3 variants): bit for bit against norm_apply followed by the
plain convolution, statistics against fp64 mean and variance.

Not reachable in the product build (no case is invented for them): FF_PATCH_CASE(8,1,6) and (4,1,4) are shadowed by the
occ variants (both split formats take them); FF_PATCH_CASE(8,2,*), (4,2,*) and (16,1,*) need FF_PATCH_TN / FF_PATCH_TH;
the 128x128 tile of conv_split.hip needs FF_SPLIT_F16_128; the ring depths 2 / 3 of the 128-row split tiles and the
non-occ forms of those tiles need FF_SPLIT_NST / FF_SPLIT_OCC; the 16x16x32 forms of the occ patch kernels need FF_MFMA16.
Outside this module: convolutions over split-pair inputs, the GRU / coordinate / motion-tail epilogues (ep_mode) and res2 are
held bit for bit to the kernels tested here by test_hip_split.py and test_hip_parity.py; `route()` knows `ep` only as far
as it moves a convolution from conv_dma.hip to conv_patch.hip.

Tolerances.  e32 = max|same computation in fp32 on the CPU - fp64|.  Exact-fp32 variants: 8 e32 (the factor
test_update_loop.py grants against the oracle's own fp32 spread).  f16x3 variants: F16X3_FACTOR e32, never more than the
2e-5 max(1, max|ref|) of test_conv2d.  f16 variants: 4e-3 max(1, max|ref|).  The backward cases keep test_conv_backward's
3e-5 for fp32; under f16 every gradient is a dot product of fp16-rounded operands like the forward, so it gets the forward's
4e-3 of max|ref| (and the cases use smooth activations: a ReLU mask taken from an f16 forward flips wherever |y| < 1e-3).

Kernel trace.  The GPU tests of this module were run once under `rocprofv3 --kernel-trace` (no counters) on an MI355X.
The conv kernel instantiations it shows, which are the ones the table names (and nothing else from the forward
dispatchers):
  conv_small_kernel<2>; conv_fwd_kernel<2,2,1,1>, <2,2,2,1>, <4,1,1,3>, <2,2,2,2>; conv_stem_kernel<false,true>;
  conv_split_kernel<2,2,1,1,TERMS,3,UNI> and conv_split_kernel_occ<2,2,2,1,TERMS,UNI,4>, <4,1,1,3,TERMS,UNI,3>, each for
  TERMS 1 / 3 and UNI false / true (12 in all);
  conv_patch_kernel_occ<T,6,2,1,4,true,0,NORM,false,false,0,STATS> and <T,4,1,1,5,true,0,NORM,false,false,0,STATS> for T 1 / 3
  and every NORM / STATS pair (16), conv_patch_kernel_occ<3,4,1,1,5,true,0,false,true,false,0,false> (K splits);
  conv_patch_kernel<T,10,2,1,0,2> and <T,8,1,1,0,2> for T 1 / 3;
  conv_dma_f32_kernel<3,3,8,3,6,X,S>, <3,3,8,3,4,X,S>, <3,3,4,4,4,X,S> for X 1 / 2 (normalise-on-load) and S false / true
  (12), <1,5,8,3,4,1,false>, <1,5,4,4,4,1,false>, <5,1,8,3,4,1,false>, <5,1,4,4,4,1,false>;
  backward: conv_wgrad_kernel<1>, <2>; conv_wgrad_split_kernel<1,64,128>, <1,128,64>, <1,128,128>.

Largest measured error per variant, max|out - fp64| / max|ref|, and as a multiple of e32 (f16: no multiple, the bound is 4e-3):
  small 7.9e-8 (0.5)  mfma32 64x64 7.2e-7 (2.6)  128x64 2.7e-6 (2.0)  128x96 4.7e-7 (1.7)  128x128 1.5e-7 (1.8)  stem 2.2e-7 (0.7)
  split t3: 64x64 uni 4.4e-7 (1.4) gen 3.6e-7 (0.7); 128x64 uni 8.7e-7 (2.3) gen 1.7e-7 (0.6); 128x96 uni 3.4e-7 (1.4) gen 3.1e-7 (1.3)
  split t1: 64x64 uni 1.9e-4 gen 1.6e-4; 128x64 uni 1.6e-4 gen 2.0e-4; 128x96 uni 2.5e-4 gen 3.6e-4
  patch occ t3: th8 3.4e-7 (2.0) th4 4.0e-7 (2.0) th4 +splitk 2.1e-7 (0.8); t1: th8 1.3e-3 th4 2.7e-4
  patch gen t3: th8 ni10 4.5e-7 (1.8) th4 ni8 4.0e-7 (1.6); t1: th8 ni10 3.6e-4 th4 ni8 1.0e-3
  dma_f32: 3x3 th8 nw6 5.2e-7 (2.4) nw4 4.6e-7 (2.5) th4 1.2e-7 (2.0); 1x5 th8 6.3e-7 (2.3) th4 2.6e-7 (2.8); 5x1 th8 2.3e-6 (2.3) th4 4.4e-7 (2.4)
No f16x3 variant came near 8 e32 (largest multiple 2.8), so F16X3_FACTOR is the 8 of the exact route.
Backward, largest max|err| / max|ref| over BWD_CASES: fp32 forward 1.8e-6, dx 1.7e-6, dW 9.4e-7, db 2.4e-7 (bound 3e-5);
f16 forward 6.7e-4, dx 3.2e-4, dW 3.7e-4, db 1.1e-4 (bound 4e-3).
"""
import ctypes
import math
import os
import zlib
from collections import namedtuple

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT

DEV = "cuda:0"
CSRC = os.path.join(ROOT, "focusflow_official_amd", "csrc")

# ----------------------------------------------------------------------------
# the dispatch mirror
# ----------------------------------------------------------------------------
# thresholds copied from the sources; test_thresholds_still_stand_in_the_sources finds each of them there
MFMA_128x128, MFMA_128x96, MFMA_128x64 = 200, 200, 400       # conv_mfma.hip: blocks of 128 rows that fill the chip
SPLIT_BIG = 512                                              # conv_split.hip: both 128-row tiles
PATCH_TH8 = 512                                              # conv_patch.hip: 8-row tiles from this many blocks
PATCH_OCC_NI = {8: 6, 4: 4}                                  # nitem limits of the occ variants ...
PATCH_GEN_NI = {8: 10, 4: 8}                                 # ... and of the generic ones
PATCH_ROWP, PATCH_LDS = 144, 96 * 1024
DMA_TH8 = {4: 384, 6: 256}                                   # conv_dma.hip f32_route: 8-row tiles, by waves per block
DMA_KEEP_SPLITK, DMA_MIN_CHUNKS = 256, 4
SPLITK_M, SPLITK_K, SPLITK_K_SHORT = 16384, 1152, 2304       # ops.conv2d
HINT_BLOCKS, HINT_NCI, HINT_STEPS, HINT_MAX, HINT_GRID = 256, 6, 72, 16, 768        # conv_patch.hip conv2d_splitk_hint


def _cdiv(a, b):
    return -(-a // b)


Route = namedtuple("Route", "name th parts splits")


def route(segs, cout, kh, kw, stride, pad, dil, b, h, w, fmt, in_scale=False, stats=False, ep=False, y_split=False):
    """-> Route(variant name, tile height or 0, entries of stats_part per image and channel or 0, K splits or 0).  An eager
    call (no graph capture); segments as the kernels see them (Cin 3 padded to 4)."""
    cin = sum(segs)
    ho, wo = (h + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1, (w + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
    m = b * ho * wo
    same = stride == 1 and dil == 1 and pad == (kh // 2, kw // 2) and kh % 2 == 1 and kw % 2 == 1
    blocks = lambda bm, bn: _cdiv(m, bm) * _cdiv(cout, bn)
    if fmt == "fp32":
        assert not (in_scale or stats or ep or y_split)
        if cout <= 2 and (kh, kw) == (3, 3) and same:
            return Route("small", 0, 0, 0)
        if cout > 96 and (cout % 128 == 0 or cout > 192) and blocks(128, 128) >= MFMA_128x128:
            return Route("mfma32 128x128", 0, 0, 0)
        if 64 < cout <= 96 and blocks(128, 96) >= MFMA_128x96:
            return Route("mfma32 128x96", 0, 0, 0)
        return Route("mfma32 128x64" if blocks(128, 64) >= MFMA_128x64 else "mfma32 64x64", 0, 0, 0)
    t = {"f16x3": "t3", "f16": "t1"}[fmt]
    seg32 = all(c % 32 == 0 for c in segs)
    tiles_x, nci = _cdiv(w, 16), cin // 32
    nitem = lambda th: _cdiv((th + kh - 1) * (16 + kw - 1), 32)
    patch_ok = same and kh <= 7 and kw <= 7 and kh * kw >= 3 and seg32
    patch8 = b * _cdiv(h, 8) * tiles_x * _cdiv(cout, 64)
    # K splits (ops.conv2d asks conv2d_splitk_hint for small planes with long reductions; short ones only under capture)
    splits = 0
    if not ep and not y_split and m <= SPLITK_M and cin * kh * kw > max(SPLITK_K, SPLITK_K_SHORT):
        blocks4 = b * _cdiv(h, 4) * tiles_x * _cdiv(cout, 64)
        if (fmt == "f16x3" and not in_scale and patch_ok and patch8 < PATCH_TH8 and nitem(4) <= PATCH_OCC_NI[4] and blocks4 <= HINT_BLOCKS
                and nci >= HINT_NCI and nci * kh * kw > HINT_STEPS):
            splits = min(HINT_MAX, nci // 2, HINT_GRID // blocks4)
            splits = splits if splits >= 2 else 0
    # the encoders' stem
    if (fmt == "f16x3" and (kh, kw, stride, dil) == (7, 7, 2, 1) and pad == (3, 3) and list(segs) == [4] and cout <= 64 and not (in_scale or ep or y_split or splits)):
        return Route("stem", 8, _cdiv(ho, 8) * _cdiv(wo, 16) * 2 if stats else 0, 0)
    # conv_dma.hip's fp32-input route
    if (fmt == "f16x3" and (kh, kw) in ((3, 3), (1, 5), (5, 1)) and same and seg32 and not splits and not ep and nci >= DMA_MIN_CHUNKS
            and not ((in_scale or stats) and (kh, kw) != (3, 3)) and not (in_scale and len(segs) > 1) and not (stats and cout % 4)):
        nw = 6 if (kh, kw) == (3, 3) and 64 < cout <= 96 else 4
        blocks8 = b * _cdiv(h, 8) * tiles_x * _cdiv(cout, 16 * nw)        # (under DMA_KEEP_SPLITK a workspace keeps conv_patch.hip: `splits` above)
        th = 8 if blocks8 >= DMA_TH8[nw] else 4
        name = f"dma_f32 {kh}x{kw} th{th}" + (f" nw{nw}" if (kh, kw, th) == (3, 3, 8) else "")
        parts = _cdiv(h, th) * tiles_x if stats else 0
        return Route(name + (" +norm" if in_scale else "") + (" +stats" if parts else "") + (" ysplit" if y_split else ""), th, parts, 0)
    # the patch-stationary kernel
    if patch_ok:
        th = 8 if patch8 >= PATCH_TH8 else 4
        ni = nitem(th)
        occ = ni <= PATCH_OCC_NI[th]
        lds = ((th + kh - 1) * (16 + kw - 1) * PATCH_ROWP + 255) // 256 * 256 + (1 if occ else 2) * 64 * PATCH_ROWP
        if lds <= PATCH_LDS and not (y_split and (not occ or ep or splits)):
            if occ:
                splits = splits if th == 4 else 0
                parts = _cdiv(h, th) * tiles_x * 2 if stats and not splits and not ep else 0
                return Route(f"patch occ th{th} {t}" + (" +norm" if in_scale else "") + (" +stats" if parts else "") + (" +splitk" if splits else "")
                             + (" ep" if ep else "") + (" ysplit" if y_split else ""), th, parts, splits)
            assert not (in_scale or ep), "only the occ variants normalise while loading / carry the GRU epilogues: the library refuses"
            if ni <= PATCH_GEN_NI[th]:
                return Route(f"patch gen th{th} ni{PATCH_GEN_NI[th]} {t}", th, 0, 0)
    # im2col
    assert not (in_scale or ep), "in_scale / ep_mode need the patch kernel: the library refuses"
    uni = "uni" if seg32 and kh * kw <= 64 else "gen"
    if 64 < cout <= 96 and blocks(128, 96) >= SPLIT_BIG:
        return Route(f"split 128x96 {t} {uni}" + (" ysplit" if y_split else ""), 0, 0, 0)
    return Route(f"split {'128x64' if blocks(128, 64) >= SPLIT_BIG else '64x64'} {t} {uni}" + (" ysplit" if y_split else ""), 0, 0, 0)


ALL_VARIANTS = (["small", "stem"] + [f"mfma32 {t}" for t in ("64x64", "128x64", "128x96", "128x128")]
                + [f"split {tile} {t} {ld}" for tile in ("64x64", "128x64", "128x96") for t in ("t3", "t1") for ld in ("uni", "gen")]
                + [f"patch occ th{th} {t}" for th in (8, 4) for t in ("t3", "t1")] + ["patch occ th4 t3 +splitk"]
                + [f"patch gen th{th} ni{ni} {t}" for th, ni in ((8, 10), (4, 8)) for t in ("t3", "t1")]
                + ["dma_f32 3x3 th8 nw6", "dma_f32 3x3 th8 nw4", "dma_f32 3x3 th4", "dma_f32 1x5 th8", "dma_f32 1x5 th4", "dma_f32 5x1 th8", "dma_f32 5x1 th4"])
MODE_FAMILIES = [f"patch occ th{th} {t}" for th in (8, 4) for t in ("t3", "t1")] + ["dma_f32 3x3 th8 nw6", "dma_f32 3x3 th8 nw4", "dma_f32 3x3 th4"]
ALL_MODES = [f + m for f in MODE_FAMILIES for m in (" +norm", " +stats", " +norm +stats")]

NONE, RELU, SIGMOID, TANH, LEAKY = range(5)
Case = namedtuple("Case", "variant segs cout kh kw stride pad dil b h w fmt act act_res ysplit")


def _c(variant, segs, cout, k, b, h, w, fmt, act, act_res, stride=1, pad=None, dil=1, ysplit=False):
    kh, kw = k
    return Case(variant, tuple(segs), cout, kh, kw, stride, pad if pad is not None else (kh // 2, kw // 2), dil, b, h, w, fmt, act, act_res, ysplit)


# act_res None: no residual (the stem has none).  The planes: 113 x 125 / 150 x 241 / 129 x 141 (after stride 2) give M off
# 128; 123 / 137 rows are off the 8-row tile, 250 columns off 16; 19 x 33 is ragged against the 4-row tile.
ROUTE_CASES = [
    # ---- exact fp32 (conv_mfma.hip, conv_small.hip); K = 324 has a tail off BK = 32
    _c("small", [256], 2, (3, 3), 1, 19, 33, "fp32", NONE, RELU),
    _c("mfma32 64x64", [64], 96, (3, 3), 1, 33, 47, "fp32", RELU, NONE, stride=2, pad=(1, 1)),
    _c("mfma32 128x128", [36], 200, (3, 3), 1, 113, 125, "fp32", SIGMOID, RELU),            # 111 x 2 = 222 blocks, second N tile ragged
    _c("mfma32 128x96", [36], 72, (3, 3), 2, 113, 125, "fp32", TANH, LEAKY),                # 221
    _c("mfma32 128x64", [36], 100, (3, 3), 2, 113, 125, "fp32", LEAKY, RELU),               # 221 x 2 = 442: Cout neither % 128 nor > 192
    _c("mfma32 128x64", [36], 64, (3, 3), 4, 113, 125, "fp32", RELU, TANH),                 # 442
    _c("mfma32 64x64", [36], 200, (3, 3), 1, 113, 112, "fp32", RELU, NONE),                 # just under: 99 x 2 = 198 (and 396 of 128 x 64)
    _c("mfma32 64x64", [36], 72, (3, 3), 2, 113, 112, "fp32", NONE, SIGMOID),               # just under: 198 of 128 x 96, 396 of 128 x 64
    _c("mfma32 64x64", [36], 100, (3, 3), 2, 113, 112, "fp32", TANH, RELU),                 # just under: 396
    # ---- im2col (conv_split.hip): 569 / 566 / 565 blocks of 128 rows
    _c("split 128x96 t3 uni", [64], 96, (3, 3), 4, 258, 282, "f16x3", RELU, NONE, stride=2, pad=(1, 1)),
    _c("split 128x96 t1 uni", [64], 96, (3, 3), 4, 258, 282, "f16", LEAKY, RELU, stride=2, pad=(1, 1)),
    _c("split 128x96 t3 uni", [64], 88, (1, 1), 4, 257, 281, "f16x3", NONE, RELU, stride=2),
    _c("split 128x96 t1 uni", [64], 96, (1, 1), 4, 257, 281, "f16", TANH, NONE, stride=2),
    _c("split 128x96 t3 uni", [32, 32], 96, (1, 1), 2, 150, 241, "f16x3", SIGMOID, LEAKY),  # two segments
    _c("split 128x96 t3 gen", [36], 96, (3, 3), 2, 150, 241, "f16x3", LEAKY, NONE),
    _c("split 128x96 t1 gen", [36], 80, (3, 3), 2, 150, 241, "f16", RELU, SIGMOID),
    _c("split 128x64 t3 uni", [64], 120, (1, 1), 1, 150, 241, "f16x3", RELU, TANH),
    _c("split 128x64 t1 uni", [64], 128, (1, 1), 1, 150, 241, "f16", NONE, RELU),
    _c("split 128x64 t3 uni", [64], 64, (1, 1), 2, 150, 241, "f16x3", TANH, RELU),
    _c("split 128x64 t1 uni", [64], 60, (1, 1), 2, 150, 241, "f16", SIGMOID, NONE),
    _c("split 128x64 t3 uni", [128], 128, (3, 3), 1, 150, 241, "f16x3", LEAKY, NONE, pad=(2, 2), dil=2),     # FF-PWC's context net
    _c("split 128x64 t3 gen", [36], 64, (1, 1), 2, 150, 241, "f16x3", NONE, LEAKY),
    _c("split 128x64 t1 gen", [36], 128, (1, 1), 1, 150, 241, "f16", RELU, NONE),
    _c("split 64x64 t3 uni", [64], 96, (1, 1), 2, 32, 48, "f16x3", RELU, NONE, stride=2),
    _c("split 64x64 t1 uni", [64], 96, (3, 3), 1, 33, 47, "f16", NONE, RELU, stride=2, pad=(1, 1)),
    _c("split 64x64 t3 gen", [324], 250, (1, 1), 1, 16, 24, "f16x3", TANH, RELU),
    _c("split 64x64 t1 gen", [2 + 2], 128, (7, 7), 1, 17, 23, "f16", SIGMOID, NONE),
    _c("stem", [4], 64, (7, 7), 2, 41, 57, "f16x3", RELU, None, stride=2, pad=(3, 3)),
    # ---- patch kernel (conv_patch.hip): 8-row tiles from 512 blocks (here 768 / 1024), Cin 32..96 so that f32_route declines
    _c("patch occ th8 t3", [64], 72, (1, 5), 2, 123, 250, "f16x3", SIGMOID, RELU),
    _c("patch occ th8 t3", [96], 64, (5, 1), 3, 123, 250, "f16x3", TANH, NONE),
    _c("patch occ th8 t3", [32], 72, (3, 3), 2, 123, 250, "f16x3", RELU, LEAKY),
    _c("patch occ th8 t3", [32], 64, (1, 3), 3, 123, 250, "f16x3", LEAKY, RELU),
    _c("patch occ th8 t1", [128], 72, (3, 3), 2, 123, 250, "f16", RELU, NONE),
    _c("patch occ th8 t1", [64], 64, (1, 5), 3, 123, 250, "f16", NONE, TANH),
    _c("patch occ th8 t1", [32, 32], 70, (5, 1), 2, 123, 250, "f16", SIGMOID, RELU),        # Cout % 4 != 0: the scalar epilogue
    _c("patch occ th8 t1", [32], 72, (1, 7), 2, 123, 250, "f16", TANH, NONE),
    _c("patch occ th4 t3", [64], 72, (1, 5), 1, 19, 33, "f16x3", RELU, NONE),
    _c("patch occ th4 t3", [96], 64, (5, 1), 2, 19, 33, "f16x3", NONE, SIGMOID),
    _c("patch occ th4 t3", [32], 70, (3, 5), 1, 19, 33, "f16x3", LEAKY, RELU),               # 3x5: 6 x 20 patch pixels still fit the 4-row occ variant
    _c("patch occ th4 t1", [128], 72, (1, 5), 1, 19, 33, "f16", TANH, RELU),
    _c("patch occ th4 t1", [128], 64, (5, 1), 2, 19, 33, "f16", RELU, NONE),
    _c("patch occ th4 t1", [64], 72, (1, 7), 1, 19, 33, "f16", SIGMOID, LEAKY),
    _c("patch occ th4 t1", [64], 40, (1, 3), 1, 19, 33, "f16", NONE, RELU),
    _c("patch occ th4 t3 +splitk", [672], 32, (3, 3), 1, 14, 32, "f16x3", LEAKY, RELU),
    _c("patch gen th8 ni10 t3", [32], 72, (5, 5), 2, 123, 250, "f16x3", RELU, NONE),
    _c("patch gen th8 ni10 t1", [32], 72, (7, 7), 2, 123, 250, "f16", LEAKY, RELU),
    _c("patch gen th8 ni10 t1", [64], 72, (3, 5), 2, 123, 250, "f16", NONE, SIGMOID),
    _c("patch gen th8 ni10 t3", [32], 64, (5, 3), 3, 123, 250, "f16x3", TANH, RELU),
    _c("patch gen th8 ni10 t3", [64], 70, (7, 1), 2, 123, 250, "f16x3", SIGMOID, NONE),
    _c("patch gen th4 ni8 t1", [64], 72, (5, 5), 1, 19, 33, "f16", RELU, TANH),
    _c("patch gen th4 ni8 t3", [32], 64, (7, 7), 2, 19, 33, "f16x3", NONE, RELU),
    _c("patch gen th4 ni8 t1", [32, 32], 40, (5, 3), 1, 19, 33, "f16", TANH, NONE),
    _c("patch gen th4 ni8 t1", [32], 72, (7, 1), 1, 19, 33, "f16", LEAKY, RELU),
    _c("patch gen th4 ni8 t3", [64], 70, (5, 5), 1, 19, 33, "f16x3", SIGMOID, RELU),
    # ---- fp32 inputs by LDS-DMA (conv_dma.hip): Cin >= 128; 18 x 16 tiles of 8 rows = 288 (nw6) / 576 (nw4) blocks
    _c("dma_f32 3x3 th8 nw6", [128], 88, (3, 3), 1, 137, 250, "f16x3", RELU, NONE),
    _c("dma_f32 3x3 th8 nw4", [128], 120, (3, 3), 1, 137, 250, "f16x3", TANH, RELU),
    _c("dma_f32 3x3 th4", [64, 64], 72, (3, 3), 1, 19, 33, "f16x3", SIGMOID, RELU),
    _c("dma_f32 1x5 th8", [64, 64], 72, (1, 5), 1, 137, 250, "f16x3", NONE, SIGMOID),
    _c("dma_f32 1x5 th4", [128], 126, (1, 5), 1, 19, 33, "f16x3", LEAKY, NONE),
    _c("dma_f32 5x1 th8", [128], 128, (5, 1), 1, 137, 250, "f16x3", RELU, TANH),
    _c("dma_f32 5x1 th4", [160], 64, (5, 1), 2, 19, 33, "f16x3", NONE, RELU),
    # ---- fp32 in, split-pair out (y_split): written by the same kernels' epilogues; Cout rounded up to 32, batch guard only
    _c("patch occ th8 t3", [64], 72, (3, 3), 2, 123, 250, "f16x3", RELU, NONE, ysplit=True),
    _c("patch occ th4 t1", [128], 64, (1, 5), 2, 19, 33, "f16", TANH, RELU, ysplit=True),
    _c("dma_f32 3x3 th8 nw6", [128], 96, (3, 3), 1, 137, 250, "f16x3", NONE, RELU, ysplit=True),
    _c("dma_f32 1x5 th4", [128], 126, (1, 5), 1, 19, 33, "f16x3", SIGMOID, NONE, ysplit=True),
    _c("split 128x96 t3 uni", [64], 96, (1, 1), 2, 150, 241, "f16x3", LEAKY, RELU, ysplit=True),
    _c("split 64x64 t1 gen", [36], 100, (3, 3), 1, 19, 33, "f16", RELU, NONE, ysplit=True),
    _c("split 64x64 t3 uni", [32], 64, (5, 5), 1, 19, 33, "f16x3", RELU, NONE, ysplit=True),        # 5x5 on 4-row tiles is no occ variant: the patch kernel declines, im2col writes it
]

Mode = namedtuple("Mode", "family cin cout b h w fmt")
MODE_CASES = [
    Mode("patch occ th8 t3", 64, 72, 2, 123, 250, "f16x3"), Mode("patch occ th8 t1", 128, 64, 3, 123, 250, "f16"),
    Mode("patch occ th4 t3", 96, 72, 1, 19, 33, "f16x3"), Mode("patch occ th4 t1", 128, 64, 2, 19, 33, "f16"),
    Mode("dma_f32 3x3 th8 nw6", 128, 88, 1, 137, 250, "f16x3"), Mode("dma_f32 3x3 th8 nw4", 128, 128, 1, 137, 250, "f16x3"),
    Mode("dma_f32 3x3 th4", 160, 72, 2, 19, 33, "f16x3"),
]
MODES = [(False, True), (True, False), (True, True)]     # (in_scale, want_stats)


def _route_of(c, **flags):
    flags.setdefault("y_split", c.ysplit)
    return route(c.segs, c.cout, c.kh, c.kw, c.stride, c.pad, c.dil, c.b, c.h, c.w, c.fmt, **flags)


def _mode_route(mc, norm, stats):
    return route((mc.cin,), mc.cout, 3, 3, 1, (1, 1), 1, mc.b, mc.h, mc.w, mc.fmt, in_scale=norm, stats=stats)


def _id(c):
    return (f"{c.variant}-c{'+'.join(map(str, c.segs))}-o{c.cout}-k{c.kh}x{c.kw}-{c.b}x{c.h}x{c.w}" + ("-ysplit" if c.ysplit else "")).replace(" ", "_")


# ----------------------------------------------------------------------------
# CPU: the table against the mirror, the mirror against the sources and the library's host logic
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", ROUTE_CASES, ids=_id)
def test_mirror_names_the_intended_variant(c):
    assert _route_of(c).name == c.variant + (" ysplit" if c.ysplit else "")


def test_every_reachable_variant_has_a_case():
    have = {c.variant for c in ROUTE_CASES}
    assert have == set(ALL_VARIANTS), f"without a case: {sorted(set(ALL_VARIANTS) - have)}; not declared: {sorted(have - set(ALL_VARIANTS))}"
    modes = {_mode_route(mc, n, s).name for mc in MODE_CASES for n, s in MODES}
    assert modes == set(ALL_MODES), f"{sorted(modes ^ set(ALL_MODES))}"
    for mc in MODE_CASES:
        assert _mode_route(mc, False, False).name == mc.family


def _past(count, threshold):
    return count * 10 >= threshold * 11


@pytest.mark.parametrize("c", ROUTE_CASES, ids=_id)
def test_cases_sit_ten_percent_past_their_thresholds(c):
    """A case that reaches a big-tile variant does so with 10 % more blocks than the threshold asks (a small retune of the
    threshold must not silently move the case to another kernel); the 'just under' rows of the exact route are the exception
    and sit within 2 % below."""
    ho, wo = (c.h + 2 * c.pad[0] - c.dil * (c.kh - 1) - 1) // c.stride + 1, (c.w + 2 * c.pad[1] - c.dil * (c.kw - 1) - 1) // c.stride + 1
    m, v = c.b * ho * wo, c.variant
    blocks = lambda bm, bn: _cdiv(m, bm) * _cdiv(c.cout, bn)
    tiles8 = c.b * _cdiv(c.h, 8) * _cdiv(c.w, 16)
    if v.startswith("mfma32 128"):
        bn = int(v.split("x")[1])
        assert _past(blocks(128, bn), {128: MFMA_128x128, 96: MFMA_128x96, 64: MFMA_128x64}[bn])
    elif v == "mfma32 64x64" and m > 10000:
        bn, thr = (128, MFMA_128x128) if c.cout == 200 else (96, MFMA_128x96) if c.cout == 72 else (64, MFMA_128x64)
        assert thr * 0.98 <= blocks(128, bn) < thr
    elif v.startswith("split 128"):
        assert _past(blocks(128, int(v.split()[1].split("x")[1])), SPLIT_BIG)
    elif v.startswith("patch") and " th8" in v:
        assert _past(tiles8 * _cdiv(c.cout, 64), PATCH_TH8)
    elif v.startswith("dma_f32") and " th8" in v:
        nw = 6 if v.endswith("nw6") else 4
        assert _past(tiles8 * _cdiv(c.cout, 16 * nw), DMA_TH8[nw])
    elif " th4" in v:       # far from the 8-row tiles
        assert tiles8 * _cdiv(c.cout, 64) * 2 <= min(PATCH_TH8, DMA_TH8[6])
    ragged = m % 128 != 0 or c.h % 8 != 0
    assert ragged or m < 2000


def _src(name):
    with open(os.path.join(CSRC, name) if name.endswith((".hip", ".h")) else os.path.join(ROOT, "focusflow_official_amd", name)) as f:
        return f.read()


def test_thresholds_still_stand_in_the_sources():
    """The literal thresholds `route()` copies, found by plain text search.  A failure here means a dispatcher changed:
    update the mirror and re-derive the shapes of ROUTE_CASES with it."""
    want = {
        "ff_common.h": ["inline const char* tune_env(const char*) { return nullptr; }"],
        "conv_mfma.hip": [f"blocks(128, 128) >= {MFMA_128x128}) return launch<2, 2, 2, 2>", f"blocks(128, 96) >= {MFMA_128x96}) return launch<4, 1, 1, 3>",
                          f"blocks(128, 64) >= {MFMA_128x64}) return launch<2, 2, 2, 1>", "p.Cout > 96 && (p.Cout % 128 == 0 || p.Cout > 192)",
                          "return launch<2, 2, 1, 1>(a, s);"],
        "conv_small.hip": ["p.w_format != FF_W_F32 || p.Cout > 2 || p.KH != 3 || p.KW != 3"],
        "conv_stem.hip": ["p.KH == 7 && p.KW == 7 && p.stride == 2", "cin == 4 && p.x_c[0] == 4", "p.Cout <= 64 && !p.res"],
        "conv_split.hip": [f"p.Cout > 64 && p.Cout <= 96 && blocks(128, 96) >= {SPLIT_BIG}) return launch<4, 1, 1, 3, TERMS>",
                           f"if (blocks(128, 64) >= {SPLIT_BIG}) return launch<2, 2, 2, 1, TERMS>", "a.Cin % 32 == 0 && p.KH * p.KW <= 64",
                           'ff::tune_env("FF_SPLIT_F16_128")', "(TM * TN == 1 ? 3 : 1)"],
        "conv_patch.hip": [f"int th = nblocks(8, 1) < {PATCH_TH8} ? 4 : 8", f"(th == 8 && nitem <= {PATCH_OCC_NI[8]} && (wb1 & 1)) || (th == 4 && nitem <= {PATCH_OCC_NI[4]} && (wb1 & 2))",
                           f"FF_PATCH_CASE(8, 1, 6) FF_PATCH_CASE(8, 1, {PATCH_GEN_NI[8]})", f"FF_PATCH_CASE(4, 1, 4) FF_PATCH_CASE(4, 1, {PATCH_GEN_NI[4]})",
                           f"constexpr int ROWP = {PATCH_ROWP};", "if (lds > 96 * 1024) return 1;", "const int nitem = (npix * 8 + 255) / 256;",
                           "p.KH > 7 || p.KW > 7) return 1;", "if (p.KH * p.KW < 3) return 1;",
                           f"tiles_x * n_tiles < {PATCH_TH8} ? 4 : 8;", f"tiles_x * n_tiles >= {PATCH_TH8}) return 0;",
                           f"if (blocks > {HINT_BLOCKS} || nci < {HINT_NCI} || nci * p.KH * p.KW <= (p.splitk < 0 ? 36 : {HINT_STEPS})) return 0;",
                           f"std::min<long long>(std::min({HINT_MAX}, nci / 2), {HINT_GRID} / blocks)",
                           "return ((p.H + th - 1) / th) * tiles_x * 2;"],
        "conv_dma.hip": [f"if (blocks8 >= (nw == 4 ? {DMA_TH8[4]} : {DMA_TH8[6]})) return F32Route{{8, nw}};", f"if (blocks8 < {DMA_KEEP_SPLITK} && p.splitk_ws) return no;",
                         f'atoi(ff::tune_env("FF_DMA_F32_MINCH")) : {DMA_MIN_CHUNKS};', "const int nw = k33 && p.Cout > 64 && p.Cout <= 96 ? 6 : 4;",
                         "if ((p.in_scale || p.stats_part) && !k33) return no;", "return r.th ? ((p.H + r.th - 1) / r.th) * ((p.W + 15) / 16) : 0;",
                         "launch_f32<3, 3, 8, 3, 6>", "launch_f32<5, 1, 8, 3, 4>"],
        "ops.py": [f"b * ho * wo <= {SPLITK_M} and klen > {SPLITK_K}:", f"short = klen <= {SPLITK_K_SHORT}"],
    }
    for name, needles in want.items():
        text = _src(name)
        for n in needles:
            assert n in text, f"{name} no longer holds `{n}`: the dispatch changed - update route() and re-derive ROUTE_CASES"


@pytest.fixture(scope="module")
def host_lib():
    from focusflow_official_amd import _hip, build
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    for f in (lib.ff_conv2d_stats_parts, lib.ff_conv2d_splitk_hint):
        f.restype, f.argtypes = ctypes.c_int, [ctypes.POINTER(_hip.FFConvParams)]
    return lib


def _host_params(segs, cout, kh, kw, stride, pad, dil, b, h, w, fmt):
    from focusflow_official_amd import _hip
    p = _hip.FFConvParams()
    for i, s in enumerate(segs):
        p.x[i], p.x_c[i], p.x_ld[i] = 4096, s, s + 8          # fake, aligned pointers: nothing is dereferenced
    p.w, p.y, p.y_ld = 4096, 4096, (cout + 3) // 4 * 4 + 16
    p.groups, p.B, p.H, p.W, p.Cout = 1, b, h, w, cout
    p.KH, p.KW, p.stride, p.pad_h, p.pad_w, p.dil_h, p.dil_w = kh, kw, stride, pad[0], pad[1], dil, dil
    p.Ho, p.Wo = (h + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1, (w + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
    p.w_format = {"fp32": _hip.W_F32, "f16x3": _hip.W_F16X3, "f16": _hip.W_F16}[fmt]
    p.out_scale = 1.0
    return p


def test_library_answers_agree_with_the_mirror(host_lib):
    """Where the library answers for itself (host logic, nothing launched): ff_conv2d_stats_parts returns tiles * 2 for the
    patch kernel and the stem and tiles for conv_dma.hip's route, with the tile height in the count; ff_conv2d_splitk_hint
    returns the K splits.  Every row of both tables."""
    seen = set()
    for c in ROUTE_CASES:
        p = _host_params(c.segs, c.cout, c.kh, c.kw, c.stride, c.pad, c.dil, c.b, c.h, c.w, c.fmt)
        if c.ysplit:            # (no K splits and no statistics beside a split-pair output: ff_conv2d_fwd refuses)
            continue
        if c.fmt != "fp32":
            r = _route_of(c)
            assert host_lib.ff_conv2d_splitk_hint(ctypes.byref(p)) == r.splits, _id(c)
            if r.splits:        # ops.conv2d: a convolution with K splits takes its statistics from a norm_stats pass
                continue
            r = _route_of(c, stats=True)
            assert host_lib.ff_conv2d_stats_parts(ctypes.byref(p)) == r.parts, _id(c)
            seen.add((r.name.split(" ")[0], r.th, r.parts > 0))
        else:
            assert host_lib.ff_conv2d_stats_parts(ctypes.byref(p)) == 0 and host_lib.ff_conv2d_splitk_hint(ctypes.byref(p)) == 0
    assert {("patch", 8, True), ("patch", 4, True), ("dma_f32", 8, True), ("dma_f32", 4, True), ("stem", 8, True), ("split", 0, False)} <= seen
    for mc in MODE_CASES:
        p = _host_params((mc.cin,), mc.cout, 3, 3, 1, (1, 1), 1, mc.b, mc.h, mc.w, mc.fmt)
        r = _mode_route(mc, False, True)
        assert r.parts > 0 and host_lib.ff_conv2d_stats_parts(ctypes.byref(p)) == r.parts, mc


# ----------------------------------------------------------------------------
# the reference, the guard band and the checks (shared by the GPU tests and the CPU demonstration)
# ----------------------------------------------------------------------------
SENTINEL = -12345.625            # finite, exact in fp32, far from every output
OUT_SCALE = 0.75
GUARD = 8                        # channels left and right of the output view; one batch element before and after
F16X3_FACTOR = 8.0               # of e32 (measured multiples: module docstring)
_ACTF = [lambda v: v, torch.relu, torch.sigmoid, torch.tanh, lambda v: F.leaky_relu(v, 0.1)]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _problem(c):
    """CPU fp32 tensors of a case (NCHW): segments, weights, bias, channel scale / shift, residual (or None)."""
    g = torch.Generator().manual_seed(_seed(*c))
    cin = sum(c.segs)
    xs = [torch.randn(c.b, s, c.h, c.w, generator=g) for s in c.segs]
    if c.variant == "stem" or cin == 4:      # image / flow inputs: 3 or 2 channels zero-padded to 4
        xs[0][:, 3:] = 0
    wt = torch.randn(c.cout, cin, c.kh, c.kw, generator=g) / (cin * c.kh * c.kw) ** 0.5
    bias, sh = torch.randn(c.cout, generator=g), torch.randn(c.cout, generator=g)
    sc = 1 + 0.25 * torch.randn(c.cout, generator=g)
    ho, wo = (c.h + 2 * c.pad[0] - c.dil * (c.kh - 1) - 1) // c.stride + 1, (c.w + 2 * c.pad[1] - c.dil * (c.kw - 1) - 1) // c.stride + 1
    res = torch.randn(c.b, c.cout, ho, wo, generator=g) if c.act_res is not None else None
    return xs, wt, bias, sc, sh, res


def _reference(c, prob, dtype):
    """F.conv2d on the CPU in `dtype`, then the epilogue in the kernels' order: bias, out_scale, ch_scale / ch_shift, act,
    residual + act_res.  -> NHWC"""
    xs, wt, bias, sc, sh, res = [[u.to(dtype) for u in t] if isinstance(t, list) else (t.to(dtype) if t is not None else None) for t in prob]
    v = F.conv2d(torch.cat(xs, 1), wt, bias, stride=c.stride, padding=c.pad, dilation=c.dil) * OUT_SCALE
    v = _ACTF[c.act](v * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    if res is not None:
        v = _ACTF[c.act_res](v + res)
    return v.permute(0, 2, 3, 1).contiguous()


def _bound(fmt, e32, refmax):
    if fmt == "fp32":
        return 8 * e32
    if fmt == "f16x3":
        return min(F16X3_FACTOR * e32, 2e-5 * max(1.0, refmax))
    return 4e-3 * max(1.0, refmax)


def _guarded(b, ho, wo, cout, device, ysplit=False):
    """(buffer, view): the output view buf[1:b+1, :, :, 8:8+cout] of a sentinel-filled buffer whose rows stay 16-byte aligned.
    A split-pair output owns Cout rounded up to 32 channels of its rows (the x1 half of the last chunk): batch guard only."""
    if ysplit:
        buf = torch.full((b + 2, ho, wo, (cout + 31) // 32 * 32), SENTINEL, dtype=torch.float32, device=device)
        return buf, buf[1:b + 1, :, :, :cout]
    buf = torch.full((b + 2, ho, wo, (cout + 3) // 4 * 4 + 2 * GUARD), SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[1:b + 1, :, :, GUARD:GUARD + cout]


def _check_guard(buf, b, cout, ysplit=False):
    bits = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
    raw = buf.view(torch.int32)
    parts = [("leading batch element", raw[0]), ("trailing batch element", raw[b + 1])]
    if not ysplit:
        parts += [("channels left of the view", raw[1:b + 1, :, :, :GUARD]), ("channels right of the view", raw[1:b + 1, :, :, GUARD + cout:])]
    for what, part in parts:
        bad = int((part != bits).sum())
        assert bad == 0, f"guard band: {bad} sentinel elements changed in the {what}"


def _check_values(got, ref64, bound, what):
    err = float((got.double() - ref64).abs().max())
    assert math.isfinite(err) and err <= bound, f"{what}: max|out - fp64| {err:.3e} > bound {bound:.3e} (max|ref| {float(ref64.abs().max()):.3e})"
    return err


def test_a_wrong_variant_would_fail_on_the_cpu():
    """Without running a broken kernel: a restatement of the reference that drops the ragged N-tile column (channels 64..71
    of 72 never written) fails the value check, and one that writes one pixel past the output fails the guard band."""
    c = _c("demo", [32], 72, (3, 3), 2, 11, 19, "fp32", RELU, LEAKY)
    prob = _problem(c)
    ref64, ref32 = _reference(c, prob, torch.float64), _reference(c, prob, torch.float32)
    e32 = float((ref32.double() - ref64).abs().max())
    bound = _bound("fp32", e32, float(ref64.abs().max()))
    buf, view = _guarded(c.b, c.h, c.w, c.cout, "cpu")
    view.copy_(ref32)
    _check_values(view, ref64, bound, "sound")
    _check_guard(buf, c.b, c.cout)
    buf, view = _guarded(c.b, c.h, c.w, c.cout, "cpu")
    view[..., :64].copy_(ref32[..., :64])                 # the second N tile's columns are dropped
    with pytest.raises(AssertionError, match="max.out - fp64"):
        _check_values(view, ref64, bound, "dropped column")
    view.copy_(ref32)
    view[..., 71] = 0                                     # ... or only its last channel, left at zero
    with pytest.raises(AssertionError, match="max.out - fp64"):
        _check_values(view, ref64, bound, "dropped channel")
    for where in ("pixel", "channel"):
        buf, view = _guarded(c.b, c.h, c.w, c.cout, "cpu")
        view.copy_(ref32)
        if where == "pixel":                              # pixel M of the M the view holds: the first of the trailing batch element
            buf.view(-1, buf.shape[3])[(c.b + 1) * c.h * c.w, GUARD:GUARD + c.cout] = ref32[0, 0, 0]
        else:                                             # channel Cout of one pixel
            buf[1, 3, 5, GUARD + c.cout] = 1.0
        _check_values(view, ref64, bound, "values are all right")
        with pytest.raises(AssertionError, match="guard band"):
            _check_guard(buf, c.b, c.cout)


# ----------------------------------------------------------------------------
# GPU: forward, one case per row
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from focusflow_official_amd import ops as _ops
    return _ops


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _sliced(t_nhwc, lead=4, tail=4):
    """The tensor as a channel slice of a wider device buffer (ld != C)."""
    b, h, w, ch = t_nhwc.shape
    buf = torch.zeros(b, h, w, (ch + 3) // 4 * 4 + lead + tail, device=DEV)
    buf[..., lead:lead + ch] = t_nhwc.to(DEV)
    return buf[..., lead:lead + ch]


def _packed(ops, wt, fmt):
    cout, cin, kh, kw = wt.shape
    wp = torch.empty(cout, kh * kw * cin, device=DEV)
    ops.pack_conv_weight(wt.to(DEV), wp, cin)
    return ops.pack_split(wp) if fmt != "fp32" else wp


_W_FMT = {"fp32": 0, "f16x3": 1, "f16": 2}


def _raw_ptr(out):
    return (out.t if hasattr(out, "t") and not isinstance(out, torch.Tensor) else out).data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("c", ROUTE_CASES, ids=_id)
def test_forward_variant_against_fp64(ops, c):
    prob = _problem(c)
    ref64 = _reference(c, prob, torch.float64)
    refmax = float(ref64.abs().max())
    e32 = float((_reference(c, prob, torch.float32).double() - ref64).abs().max())
    bound = _bound(c.fmt, e32, refmax)
    xs, wt, bias, sc, sh, res = prob
    xd = [_sliced(_nhwc(x)) for x in xs]
    wp = _packed(ops, wt, c.fmt)
    rd = _sliced(_nhwc(res), 4, 8) if res is not None else None
    ho, wo = ref64.shape[1:3]
    bd, scd, shd = bias.to(DEV), sc.to(DEV), sh.to(DEV)
    outs = []
    for _ in range(2):
        buf, view = _guarded(c.b, ho, wo, c.cout, DEV, c.ysplit)
        out = ops.conv2d(xd, wp, bd, c.cout, c.kh, c.kw, c.stride, c.pad, act=c.act, out=view, res=rd, act_res=c.act_res or 0,
                         ch_scale=scd, ch_shift=shd, out_scale=OUT_SCALE, w_fmt=_W_FMT[c.fmt], dilation=c.dil, y_split=c.ysplit)
        torch.cuda.synchronize()
        assert _raw_ptr(out) == view.data_ptr()
        outs.append(buf)
    if c.ysplit:     # back to fp32: the format keeps 22 significant bits (csrc/ff_common.h), test_hip_split.py grants 2^-21 max(1, max|.|)
        got = ops.split_copy(outs[0][1:c.b + 1], to_split=False)[..., :c.cout].cpu()
        bound += 2.0 ** -21 * max(1.0, refmax)
    else:
        got = outs[0][1:c.b + 1, :, :, GUARD:GUARD + c.cout].cpu()
    err = float((got.double() - ref64).abs().max())
    print(f"ROUTE-ERR | {c.variant} | {_id(c)} | err/max|ref| {err / refmax:.3e} | e32/max|ref| {e32 / refmax:.3e} | err/e32 {err / e32:.2f} | "
          f"bound/max|ref| {bound / refmax:.3e}")
    _check_values(got, ref64, bound, c.variant)
    _check_guard(outs[0], c.b, c.cout, c.ysplit)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "a second call gives other bits"


@pytest.mark.gpu
def test_fragment_order_weights_give_the_bits_of_row_order(ops):
    """conv_dma.hip's fp32-input route reads the same split weights from rows or, given FFConvParams.w_frag, in
    MFMA-fragment order (ops.pack_frag16): 128 -> 40 channels, 3x3, f16x3, at 1x9x17 (ragged against the 8-row tile and
    the 16-column fragment, Cout off the N tile)."""
    assert route([128], 40, 3, 3, 1, (1, 1), 1, 1, 9, 17, "f16x3").name.startswith("dma_f32")
    g = torch.Generator().manual_seed(_seed("frag", 128, 40))
    x = torch.randn(1, 9, 17, 128, generator=g).to(DEV)
    wt, bias = torch.randn(40, 128, 3, 3, generator=g) / 34.0, torch.randn(40, generator=g).to(DEV)
    wp = _packed(ops, wt, "f16x3")
    rows = ops.conv2d([x], wp, bias, 40, 3, 3, 1, (1, 1), w_fmt=1, w_frag=None)
    frag = ops.conv2d([x], wp, bias, 40, 3, 3, 1, (1, 1), w_fmt=1, w_frag=ops.pack_frag16(wp, 40))
    assert torch.equal(rows, frag)
    ref = F.conv2d(x.cpu().double().permute(0, 3, 1, 2), wt.double(), bias.cpu().double(), padding=1).permute(0, 2, 3, 1)
    _check_values(rows.cpu(), ref, 2e-5 * max(1.0, float(ref.abs().max())), "dma_f32 from rows")


@pytest.mark.gpu
@pytest.mark.parametrize("norm,stats", MODES, ids=["stats", "norm", "norm+stats"])
@pytest.mark.parametrize("mc", MODE_CASES, ids=lambda mc: mc.family.replace(" ", "_"))
def test_normalise_on_load_and_epilogue_statistics(ops, mc, norm, stats):
    """in_scale / in_shift / in_act and want_stats on every variant that has them: normalise-on-load bit for bit against
    norm_apply followed by the plain convolution (as test_conv_normalises_its_input_while_loading), the output with statistics
    bit for bit against the one without, the statistics against fp64 mean and variance (as test_stem_conv_kernel), the
    output against fp64, the guard band."""
    g = torch.Generator().manual_seed(_seed(*mc))
    x = torch.randn(mc.b, mc.cin, mc.h, mc.w, generator=g) * 2 + 0.7
    wt = torch.randn(mc.cout, mc.cin, 3, 3, generator=g) / (9 * mc.cin) ** 0.5
    bias = torch.randn(mc.cout, generator=g)
    xd, wp, bd = _sliced(_nhwc(x)), _packed(ops, wt, mc.fmt), bias.to(DEV)
    fmt = _W_FMT[mc.fmt]
    kw = {}
    xin = xd
    if norm:
        st = ops.norm_stats(xd, per_sample=True)
        sc, sh = ops.norm_coeffs(st, mc.h * mc.w, 1e-5)
        kw = dict(in_scale=sc, in_shift=sh, in_act=1)
        xin = ops.norm_apply(xd, st, True, 1e-5, act=1)
    plain = ops.conv2d([xin], wp, bd, mc.cout, 3, 3, 1, 1, w_fmt=fmt)
    buf, view = _guarded(mc.b, mc.h, mc.w, mc.cout, DEV)
    got = ops.conv2d([xd], wp, bd, mc.cout, 3, 3, 1, 1, w_fmt=fmt, out=view, want_stats=stats, **kw)
    torch.cuda.synchronize()
    if stats:
        got, table = got
    assert torch.equal(got, plain), "in_scale / stats_part change the output bits"
    _check_guard(buf, mc.b, mc.cout)
    x64 = x.double()
    if norm:
        x64 = torch.relu((x64 - x64.mean(dim=(2, 3), keepdim=True)) / torch.sqrt(x64.var(dim=(2, 3), unbiased=False, keepdim=True) + 1e-5))
    ref64 = F.conv2d(x64, wt.double(), bias.double(), padding=1)
    refmax = float(ref64.abs().max())
    # (normalise-on-load adds the fp32 error of the normalisation itself to both sides of the bit comparison: the project's 2e-5 / 4e-3 hold it)
    _check_values(got.cpu(), _nhwc(ref64), (4e-3 if mc.fmt == "f16" else 2e-5) * max(1.0, refmax), mc.family)
    if stats:
        n = mc.h * mc.w
        ref = ref64 if mc.fmt != "f16" else got.cpu().double().permute(0, 3, 1, 2)     # f16: the statistics of the reduced-precision output itself
        mean, var = (table[..., 0] / n).cpu().double(), (table[..., 1] / n - (table[..., 0] / n) ** 2).cpu().double()
        rm, rv = ref.mean(dim=(2, 3)), ref.var(dim=(2, 3), unbiased=False)
        assert float(((mean - rm).abs() - 1e-5 * rm.abs()).max()) <= 1e-6, "mean from the epilogue"
        assert float(((var - rv).abs() - 2e-4 * rv.abs()).max()) <= 1e-7, "variance from the epilogue"


# ----------------------------------------------------------------------------
# GPU: backward under the other two formats
# ----------------------------------------------------------------------------
BWD_CASES = [
    # (segments, couts (group), kh, kw, stride, pad, B, H, W, act, res) - smooth activations only (module docstring)
    ([64], [64], 1, 1, 1, (0, 0), 2, 16, 24, 0, True),            # fp32 weight gradient: K = 64 (conv_wgrad_kernel<1>); split: Cout <= 64
    ([64], [96], 3, 3, 1, (1, 1), 1, 17, 25, 3, False),           # K = 576 (conv_wgrad_kernel<2>); split: Cout 96, K < 864 (128 x 64)
    ([3], [64], 7, 7, 2, (3, 3), 2, 32, 48, 0, False),            # Cin 3 padded to 4 (weight gradients only)
    ([64], [64], 3, 3, 1, (1, 1), 2, 16, 24, 2, False),           # split: Cout <= 64 (64 x 128)
    ([96], [96], 3, 3, 1, (1, 1), 1, 23, 37, 0, False),           # split: Cout 96, K = 864 (128 x 128)
    ([128], [256], 3, 3, 1, (1, 1), 1, 16, 24, 3, False),         # split: Cout > 128, K = 1152 (128 x 128)
    ([64], [192], 1, 1, 1, (0, 0), 1, 16, 24, 0, False),          # split: Cout > 128, short K (128 x 64)
    ([64], [96], 3, 3, 2, (1, 1), 2, 32, 48, 0, False),           # stride-2 input gradient (zero dilation)
    ([128, 128], [128, 128], 1, 5, 1, (0, 2), 1, 16, 24, 2, False),     # two segments, a group of two convolutions
    ([64], [96], 1, 1, 1, (0, 0), 2, 150, 241, 0, False),         # M = 72300: forward on a 128 x 96 tile, input gradient (96 -> 64) on a 128 x 64 tile
]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["fp32", "f16"])
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: f"c{'+'.join(map(str, c[0]))}-o{'+'.join(map(str, c[1]))}-k{c[2]}x{c[3]}-s{c[4]}-{c[6]}x{c[7]}x{c[8]}")
def test_conv_backward_in_the_other_formats(case, fmt):
    """test_conv_backward's comparison (forward, input / residual / weight / bias gradients of fn.conv against CPU autograd)
    in float64, under the exact-fp32 and the one-term f16 conv precision."""
    import copy
    from focusflow_official_amd import cce, fn, ops
    segs, couts, kh, kw, stride, pad, b, h, w, act, use_res = case
    g = torch.Generator().manual_seed(_seed(*case))
    cin = sum(segs)
    xs32 = [torch.randn(b, c, h, w, generator=g) for c in segs]
    convs = [nn.Conv2d(cin, co, (kh, kw), stride=stride, padding=pad) for co in couts]
    for cv in convs:
        with torch.no_grad():
            cv.weight.copy_(torch.randn(cv.weight.shape, generator=g) / (cin * kh * kw) ** 0.5)
            cv.bias.copy_(torch.randn(cv.bias.shape, generator=g))
    convs64 = [copy.deepcopy(cv).double() for cv in convs]
    xs = [x.double().requires_grad_(True) for x in xs32]
    actf = [lambda v: v, torch.relu, torch.sigmoid, torch.tanh][act]
    pre = torch.cat([cv(torch.cat(xs, 1)) for cv in convs64], 1)
    res = None
    if use_res:          # y = act(conv + res), out_scale 1
        res = torch.randn(pre.shape, generator=g).double().requires_grad_(True)
        ref = actf(pre + res)
    else:                # epilogue order: scale, then act
        ref = actf(pre * 0.5)
    gy = torch.randn(ref.shape, generator=g)
    ref.backward(gy.double())
    rel = {"fp32": 3e-5, "f16": 4e-3}[fmt]

    def close(a, r, what):
        a, r = a.double(), r.double()
        scale = max(1e-6, float(r.abs().max()))
        viol = float(((a - r).abs() - (rel if fmt == "fp32" else 0.0) * r.abs()).max())
        print(f"BWD-ERR | {fmt} | {what} | max|err|/max|ref| {float((a - r).abs().max()) / scale:.3e}")
        assert viol <= rel * scale, f"{what} [{fmt}]: max violation {viol:.3e} (allowed {rel * scale:.3e}), max|ref| {scale:.3e}"

    old = ops.conv_precision()
    ops.set_conv_precision(fmt)
    try:
        dconvs = [copy.deepcopy(cv).to(DEV) for cv in convs]
        pc = cce.PackedConv(dconvs)
        xd = [_nhwc(x).to(DEV).requires_grad_(True) for x in xs32]
        if cin % 4:      # image inputs: zero-padded to 4 channels, never differentiated
            xd = [F.pad(_nhwc(xs32[0]).to(DEV), (0, 4 - cin))]
        rd = _nhwc(res.detach().float()).to(DEV).requires_grad_(True) if use_res else None
        out = fn.conv(pc, xd, act=act, res=rd, out_scale=0.5 if not use_res else 1.0)
        nchw = lambda t: t.detach().cpu().permute(0, 3, 1, 2)
        close(nchw(out), ref.detach(), "forward")
        out.backward(_nhwc(gy).to(DEV))
        torch.cuda.synchronize()
        if cin % 4 == 0:
            for i, (x, xdv) in enumerate(zip(xs, xd)):
                close(nchw(xdv.grad), x.grad, f"dx[{i}]")
        if use_res:
            close(nchw(rd.grad), res.grad, "dres")
        for j, (cv, dcv) in enumerate(zip(convs64, dconvs)):
            close(dcv.weight.grad.cpu(), cv.weight.grad, f"dW[{j}]")
            close(dcv.bias.grad.cpu(), cv.bias.grad, f"db[{j}]")
    finally:
        ops.set_conv_precision(old)
