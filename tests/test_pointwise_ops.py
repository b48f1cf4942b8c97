"""Operator tests of the small kernels between the convolutions, each against a plain fp64 reference on the CPU
(tests/pointwise_ref.py, oracle.ffraft_ref.upsample_flow): the norm layers forward and backward in their three modes, the
activation gradients with their two routes and the max|g| words, the convex-upsampling backward on both sides of its row
split, the pieces of the SA / CA fusion units, and dilate2 / channel_sum / the GRU gate gradients.

Inputs are drawn in fp32 and the same fp32 values go to both sides.  A "view" is a channel slice of a wider buffer
(ld = C + 8 from channel 4 unless a case says otherwise) whose surroundings hold SENTINEL; after every call on views the
buffers of the inputs must be bit-identical to what they were and the surroundings of an output view must still hold
SENTINEL.

Tolerances.  `check(group, ...)` is close() of tests/test_hip_backward.py with rtol = atol_rel = TOL[group], and the number
it reports is the smallest such tolerance the data would pass: max |a - ref| / (|ref| + max|ref|).  Copies, masks, maxima
and arg-maxima are compared bit for bit.

Largest error seen on the MI355X against the fp64 reference, in that measure, per group (every one lay more than ten times
below the project's operator conventions - 3e-5, 1e-4 for the norm and upsampling gradients, 1e-5 for the upsampling
forward - so each group's tolerance is tightened to about four times what was measured):

    group               measured    tolerance   convention
    norm forward        1.10e-06    4.5e-06     3e-5      (the offset case; every other case <= 2.5e-07)
    norm backward       1.54e-06    6e-06       1e-4      (dx of the 3 x 256 x 1 x 1 batch-norm case: three values a channel;
                                                           every other dx <= 7e-08, dgamma <= 6.1e-07, dbeta <= 2.6e-08)
    act_bwd             4.84e-08    2e-07       3e-5
    upsample forward    1.07e-07    4.5e-07     1e-5
    upsample backward   2.21e-07    9e-07       1e-4
    attention           2.67e-07    1.1e-06     3e-5
    small ops           2.29e-08    1e-07       3e-5

Findings, neither of them a bug:
  * the offset norm case (channel mean 8, standard deviation 0.25) reaches max |y - fp64| = 5.58e-06, above the estimate of
    32 * 2^-24 * 2 = 4e-6: the estimate leaves out gamma (up to 1.6 here) and the rounding of the fp32 mean; the shift
    beta - mean * rstd * gamma is about 50 and is rounded twice (half an ulp of 50 is 1.9e-6 each);
  * arg-maxima follow "the first maximum wins" in chan_stats (lowest channel) and in spatial_stats (lowest pixel index,
    inside a slab and across slabs), as numpy.argmax: the documented rule and the kernels agree.
"""
import numpy as np
import pytest
import torch

import pointwise_ref as R
from oracle import ffraft_ref as orc

gpu = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 3.0e4

TOL = {                               # about 4 x the largest error measured (module docstring); the convention it replaces
    "norm forward": 4.5e-6,           # 3e-5
    "norm backward": 6e-6,            # 1e-4 (dx, dgamma, dbeta in test_norm_backward)
    "act_bwd": 2e-7,                  # 3e-5
    "upsample forward": 4.5e-7,       # 1e-5 (test_gru_and_upsample_backward)
    "upsample backward": 9e-7,        # 1e-4
    "attention": 1.1e-6,              # 3e-5
    "small ops": 1e-7,                # 3e-5
}
MEASURED = {}


def check(group, a, ref, what):
    a, ref = a.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert a.shape == ref.shape, f"{what}: shape {a.shape} vs {ref.shape}"
    top = max(1e-6, float(np.abs(ref).max()))
    need = float((np.abs(a - ref) / (np.abs(ref) + top)).max())
    MEASURED[group] = max(MEASURED.get(group, 0.0), need)
    print(f"[{group}] {what}: {need:.3e}")
    assert need <= TOL[group], f"{what}: needs a tolerance of {need:.3e}, {group} allows {TOL[group]:.1e} (max|ref| {top:.3e})"


@pytest.fixture(scope="module")
def ops():
    from focusflow_official_amd import ops
    yield ops
    print("\nlargest error per group against fp64:", {k: f"{v:.3e}" for k, v in sorted(MEASURED.items())})


def put(t, view, guards, lead=4, width=None):
    """CPU tensor -> device tensor; as a view it sits in channels [lead, lead + C) of a SENTINEL-filled buffer of `width`."""
    if not view:
        return t.to(DEV)
    c = t.shape[-1]
    buf = torch.full((*t.shape[:-1], width or c + 8), SENTINEL, dtype=t.dtype, device=DEV)
    buf[..., lead:lead + c] = t.to(DEV)
    guards.append((buf, buf.clone()))
    return buf[..., lead:lead + c]


def out_view(shape, lead=4, width=None):
    c = shape[-1]
    buf = torch.full((*shape[:-1], width or c + 8), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[..., lead:lead + c]


def untouched(guards):
    return all(torch.equal(buf, snap) for buf, snap in guards)


def surroundings_kept(buf, lead, c):
    return bool((buf[..., :lead] == SENTINEL).all()) and bool((buf[..., lead + c:] == SENTINEL).all())


def word_of(value: float):
    """An amax word holding the bits of `value`."""
    return torch.tensor([value], dtype=torch.float32).view(torch.int32).to(DEV)


def word_equals_max(word, g):
    """The word, viewed as a float, is bit-equal to max|g| (a maximum does not depend on the order)."""
    return torch.equal(word.view(torch.float32).cpu(), g.detach().abs().max().reshape(1).cpu())


# =====================================================================================================================
# 1. norm_stats / norm_apply / norm_bwd
def test_norm_cases_leave_out_at_most_a_thousandth_of_a_tensor():
    """No GPU: the share of elements whose ReLU mask is undecided (pointwise_ref.NEAR_ZERO), from the reference alone."""
    for case in R.NORM_CASES:
        ref = R.norm_reference(case)
        share = ref["near"].double().mean().item()
        assert share <= 1e-3, f"{R.norm_case_id(case)}: {share:.2e} of the elements lie within {R.NEAR_ZERO} of a ReLU's corner"
        assert not (case.relu or case.res) or bool((ref["dy"][ref["near"]] == 0).all())


def _norm_run(ops, case, guards):
    ref = R.norm_reference(case)
    per, fixed = case.mode == "instance", case.mode == "frozen"
    x, dy = put(ref["x"], case.view, guards), put(ref["dy"], case.view, guards)
    res = put(ref["res"], case.view, guards) if case.res else None
    gamma = ref["gamma"].to(DEV) if not per else None
    beta = ref["beta"].to(DEV) if not per else None
    if fixed:      # as the frozen-BatchNorm branch of _ResidualEncoder._conv_norm builds it from the running statistics
        n = float(case.B * case.H * case.W)
        rm, rv = ref["rm"].to(DEV).double(), ref["rv"].to(DEV).double()
        st = torch.stack([rm * n, (rv + rm * rm) * n], -1)[None].contiguous()
    else:
        st = ops.norm_stats(x, per_sample=per)
    return ref, per, fixed, x, dy, res, gamma, beta, st


@gpu
@pytest.mark.parametrize("case", R.NORM_CASES, ids=R.norm_case_id)
def test_norm_forward_and_backward(ops, case):
    guards = []
    ref, per, fixed, x, dy, res, gamma, beta, st = _norm_run(ops, case, guards)
    shape = tuple(x.shape)
    ybuf, yout = out_view(shape) if case.view else (None, None)
    y = ops.norm_apply(x, st, per, R.EPS, gamma, beta, act=R.ACT_RELU if case.relu else R.ACT_NONE, res=res, out=yout)
    check("norm forward", y, ref["y"], "y")
    if case.offset:     # fma(x, rstd g, b - mean rstd g) at |mean| / std = 32: estimated 32 * 2^-24 * 2 = 4e-6
        err = (y.cpu().double() - ref["y"]).abs().max().item()
        MEASURED["norm forward, offset case, absolute"] = err
        print(f"offset case: max |y - fp64| = {err:.3e} (estimate 4e-6)")
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    dx, dres, bst = ops.norm_bwd(x, dy, y if case.res else None, st, per, fixed, R.EPS, gamma, beta, case.relu, case.res, amax=word)
    check("norm backward", dx, ref["dx"], "dx")
    assert word_equals_max(word, dx), "dx_amax is not the bits of max|dx|"
    if case.res:        # dres = dy [y > 0]: a masked copy
        assert torch.equal(dres.cpu().double(), ref["dres"]), "dres"
    else:
        assert dres is None
    if not per:         # as NormFn.backward reads them
        check("norm backward", bst[0, :, 1].float(), ref["dgamma"], "dgamma")
        check("norm backward", bst[0, :, 0].float(), ref["dbeta"], "dbeta")
    # a caller-supplied zeroed bstats: the same sums (fp64 atomics: to the last bits) and the same dx (to an fp32 rounding)
    mine = torch.zeros_like(bst)
    dx2, _, bst2 = ops.norm_bwd(x, dy, y if case.res else None, st, per, fixed, R.EPS, gamma, beta, case.relu, case.res, bstats=mine)
    assert bst2.data_ptr() == mine.data_ptr()
    assert torch.allclose(bst2, bst, rtol=1e-12, atol=1e-12 * bst.abs().max().item())
    assert (dx2 - dx).abs().max().item() <= 2.0 ** -22 * dx.abs().max().item()
    assert untouched(guards), "an input buffer was written"
    if case.view:
        assert surroundings_kept(ybuf, 4, case.C), "norm_apply wrote outside its output slice"


# =====================================================================================================================
# 2. act_bwd, act_bwd_into and the amax words
ACTS = [R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID, R.ACT_TANH, R.ACT_LEAKY]
# name, C, (view, lead, width): the route is the library's choice (ff_act_bwd: `vec = ...`)
ACT_ROUTES = [
    ("vec-c4", 4, (False, 0, None)),
    ("vec-c128", 128, (False, 0, None)),
    ("vec-c128-view264", 128, (True, 4, 264)),
    ("scalar-c2-ld2", 2, (False, 0, None)),                 # C 2 -> Cpad 4
    ("scalar-c126-of-128", 126, (True, 0, 128)),            # C 126 -> Cpad 128
    ("scalar-c128-from-channel-1", 128, (True, 1, 136)),    # misaligned
]
ACT_PIXELS = [(1, 1, 1), (1, 5, 7), (1, 33, 47)]    # 33 x 47 x 128: 49 blocks, and an item count that is no multiple of four trips


def _act_data(shape, act, seed):
    g = torch.Generator().manual_seed(seed)
    pre, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    return dy, R.act_forward(pre, act)          # y = act(pre) in fp32 on the CPU


@gpu
@pytest.mark.parametrize("pix", ACT_PIXELS, ids=lambda p: f"{p[1]}x{p[2]}")
@pytest.mark.parametrize("route", ACT_ROUTES, ids=lambda r: r[0])
def test_act_bwd(ops, route, pix):
    _, c, (view, lead, width) = route
    cpad = (c + 3) // 4 * 4
    for act in ACTS:
        for scale in (1.0, 0.5):
            guards = []
            dy, y = _act_data((*pix, c), act, 100 * act + c)
            dyd = put(dy, view, guards, lead, width)
            yd = put(y, view, guards, lead, width) if act != R.ACT_NONE else None
            snap = dyd.clone()
            g, word = ops.act_bwd(dyd, yd, act, scale, c, want_amax=True)
            what = f"act {act} scale {scale}"
            alias = not view and c == cpad and act == R.ACT_NONE and scale == 1.0
            assert (g.data_ptr() == dyd.data_ptr()) == alias, what
            assert g.shape == (*pix, cpad) and torch.equal(dyd, snap), what
            ref = dy.double() * scale * R.act_grad_from_output(y.double(), act)
            check("act_bwd", g[..., :c], ref, what)
            assert bool((g[..., c:] == 0).all()), f"{what}: padding channels"
            if scale == 1.0 and act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY):     # a copy, a mask, one rounding of dy * 0.1f
                assert torch.equal(g[..., :c].cpu(), dy * R.act_grad_from_output(y, act)), f"{what}: not exact"
            assert word_equals_max(word, g), f"{what}: amax word"
            assert untouched(guards), f"{what}: an input buffer was written"


@gpu
def test_act_bwd_alias_mode_returns_dy_and_writes_nothing(ops):
    dy, _ = _act_data((1, 5, 7, 128), R.ACT_NONE, 7)
    dyd = dy.to(DEV)
    assert ops.act_bwd_is_alias(dyd, R.ACT_NONE, 1.0, 128)
    assert ops.act_bwd(dyd, None, R.ACT_NONE, 1.0, 128) is dyd
    g, word = ops.act_bwd(dyd, None, R.ACT_NONE, 1.0, 128, want_amax=True)      # measures only
    assert g is dyd and torch.equal(dyd.cpu(), dy) and word_equals_max(word, dyd)
    for other in (dict(act=R.ACT_RELU), dict(scale=0.5), dict(c=126)):
        kw = dict(act=R.ACT_NONE, scale=1.0, c=128)
        kw.update(other)
        assert not ops.act_bwd_is_alias(dyd, kw["act"], kw["scale"], kw["c"])
    guards = []
    assert not ops.act_bwd_is_alias(put(dy, True, guards), R.ACT_NONE, 1.0, 128)


@gpu
@pytest.mark.parametrize("pix", ACT_PIXELS[1:], ids=lambda p: f"{p[1]}x{p[2]}")
@pytest.mark.parametrize("lead,width", [(4, 264), (1, 136)], ids=["vec", "scalar"])
def test_act_bwd_into_a_view(ops, lead, width, pix):
    c = 128
    for act, scale in ((R.ACT_NONE, 1.0), (R.ACT_TANH, 0.5), (R.ACT_RELU, 1.0)):
        guards = []
        dy, y = _act_data((*pix, c), act, 11 + act)
        dyd = put(dy, True, guards, lead, width)
        yd = put(y, True, guards, lead, width) if act != R.ACT_NONE else None
        gbuf, g = out_view((*pix, c))
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert ops.act_bwd_into(dyd, yd, act, g, word, scale) is g
        check("act_bwd", g, dy.double() * scale * R.act_grad_from_output(y.double(), act), f"act_bwd_into act {act}")
        assert word_equals_max(word, g) and untouched(guards) and surroundings_kept(gbuf, 4, c)


@gpu
@pytest.mark.parametrize("entry", ["act_bwd", "act_bwd_into", "norm_bwd", "gru_bwd_blend", "gru_bwd_blend:q", "gru_bwd_rh", "gru_bwd_out"])
def test_amax_word_only_grows(ops, entry):
    """A word preloaded with a larger value keeps it, one with a smaller positive value grows to the maximum, and an all-zero
    gradient leaves a zeroed word at 0.  (gru_bwd_*: the three producers of csrc/train_ops.hip, called as train_loop.py calls
    them; the blend step writes two words, g_z's and - ":q" - g_q's.)"""
    dy, y = _act_data((1, 33, 47, 128), R.ACT_SIGMOID, 5)
    if entry.startswith("gru_bwd"):
        from focusflow_official_amd import _hip
        gen = torch.Generator().manual_seed(9)
        shp, n = (1, 33, 47, 128), 33 * 47
        z, r = (torch.rand(shp, generator=gen).to(DEV) for _ in range(2))
        q, h = (torch.tanh(torch.randn(shp, generator=gen)).to(DEV) for _ in range(2))
        mo = torch.relu(torch.randn(shp, generator=gen)).to(DEV)
        wide = torch.randn((1, 33, 47, 256), generator=gen).to(DEV)            # [d h | d motion] of an input-gradient convolution
        p, st = ops._p, ops._stream

        def run(word, zero):
            up, up2 = (dy.to(DEV) * 0, wide * 0) if zero else (dy.to(DEV), wide)
            g0, g1, dh, dm = (torch.empty(shp, device=DEV) for _ in range(4))
            other = torch.zeros(1, dtype=torch.int32, device=DEV)
            if entry.startswith("gru_bwd_blend"):
                first = entry == "gru_bwd_blend"
                _hip.call("ff_gru_bwd_blend", p(up), 128, None, 0, None, 128, p(z), 128, p(q), 128, p(h), 128, p(g0), 128, p(g1), 128, p(dh), 128,
                          p(word if first else other), p(other if first else word), n, 128, st())
                return g0 if first else g1
            if entry == "gru_bwd_rh":
                dh.copy_(up)
                _hip.call("ff_gru_bwd_rh", p(up2), 256, p(r), 128, p(h), 128, p(g0), 128, p(dh), 128, p(dm), 128, 1, p(word), n, 128, st())
            else:
                _hip.call("ff_gru_bwd_out", p(up), 128, p(up2), 256, p(up), 128, p(mo), 128, p(dh), 128, p(g0), 128, 126, p(word), n, 128, st())
            return g0
    elif entry == "norm_bwd":
        case = R.NORM_CASES[0]
        _, per, fixed, x, dyn, res, gamma, beta, st = _norm_run(ops, case, [])

        def run(word, zero):
            return ops.norm_bwd(x, torch.zeros_like(dyn) if zero else dyn, None, st, per, fixed, R.EPS, gamma, beta, case.relu, False,
                                amax=word)[0]
    elif entry == "act_bwd":
        def run(word, zero):
            return ops.act_bwd((dy * 0 if zero else dy).to(DEV), y.to(DEV), R.ACT_SIGMOID, 0.5, 128, want_amax=True, amax=word)[0]
    else:
        def run(word, zero):
            return ops.act_bwd_into((dy * 0 if zero else dy).to(DEV), y.to(DEV), R.ACT_SIGMOID, torch.empty(dy.shape, device=DEV), word, 0.5)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    m = run(word, False).abs().max().item()
    assert m > 0 and word.view(torch.float32).item() == m
    for preload, expect in ((2.0 * m, 2.0 * m), (0.5 * m, m)):
        word = word_of(preload)
        run(word, False)
        assert word.view(torch.float32).item() == expect, f"preloaded with {preload}: {word.view(torch.float32).item()}, expected {expect}"
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert run(word, True).abs().max().item() == 0 and word.item() == 0


# =====================================================================================================================
# 3. convex-upsampling backward: the launch splits a row over gridDim.z = 2 exactly when W >= 16
@gpu
@pytest.mark.parametrize("b,h,w", [(2, 10, 14), (2, 3, 16), (1, 1, 17), (2, 5, 33)], ids=lambda v: str(v))
def test_upsample_flow_backward(ops, b, h, w):
    from focusflow_official_amd import _hip
    g = torch.Generator().manual_seed(40 + w)
    flow = torch.randn(b, h, w, 2, generator=g)
    mask = torch.randn(b, h, w, 576, generator=g)
    gup = torch.randn(b, 2, 8 * h, 8 * w, generator=g)
    fr = flow.double().permute(0, 3, 1, 2).requires_grad_(True)
    mr = mask.double().permute(0, 3, 1, 2).requires_grad_(True)
    up = orc.upsample_flow(fr, mr)
    up.backward(gup.double())
    dflow_ref, dmask_ref = fr.grad.permute(0, 2, 3, 1), mr.grad.permute(0, 2, 3, 1)
    # the plain entry
    fd, md, gd = flow.to(DEV), mask.to(DEV), gup.to(DEV)
    check("upsample forward", ops.upsample_flow(fd, md), up, "upsample_flow")
    dflow, dmask = ops.upsample_flow_bwd(gd, fd, md)
    check("upsample backward", dflow, dflow_ref, "dflow")
    check("upsample backward", dmask, dmask_ref, "dmask")
    # the _ex entry, as the recorded training loop calls it: 4-wide flow and dflow, .25 * dmask, max|dmask| into a word
    guards = []
    f4 = put(torch.cat([flow, torch.full((b, h, w, 2), SENTINEL)], -1), False, guards)
    mv = put(mask, True, guards)
    d4 = torch.zeros(b, h, w, 4, device=DEV)
    d4[..., 2], d4[..., 3] = 5.0, -7.0
    dm = torch.empty(b, h, w, 576, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    _hip.call("ff_upsample_flow_bwd_ex", ops._p(gd), ops._p(f4), 4, ops._p(mv), ops._ld(mv), ops._p(d4), 4, ops._p(dm), 0.25, ops._p(word),
              b, h, w, ops._stream())
    check("upsample backward", d4[..., :2], dflow_ref, "_ex dflow")
    check("upsample backward", dm, 0.25 * dmask_ref, "_ex dmask")
    assert bool((d4[..., 2] == 5.0).all()) and bool((d4[..., 3] == -7.0).all()), "_ex wrote beyond the two flow columns"
    assert word_equals_max(word, dm) and untouched(guards)


# =====================================================================================================================
# 4. the pieces of the SA / CA fusion units
ATTN_C = [4, 64, 96, 132]            # below one wave, one wave, one and a half, two waves and a bit
DATA = ["gauss", "negative", "ties"]


def _data(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "gauss":
        return torch.randn(shape, generator=g)
    if kind == "negative":           # a maximum initialised with 0 would win everywhere
        return -torch.randn(shape, generator=g).abs() - 0.5
    return torch.randint(-2, 3, shape, generator=g).float()      # ties in almost every row


@gpu
@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("c", ATTN_C)
def test_chan_stats(ops, c, kind):
    for shape in ((1, 1, 1), (1, 5, 7), (1, 20, 28)):
        for view in (False, True):
            guards = []
            x = _data(kind, (*shape, c), 7 * c + shape[2])
            st, am = ops.chan_stats(put(x, view, guards))
            what = f"{shape} view {view}"
            check("attention", st[..., 0], x.double().mean(-1), f"chan mean {what}")
            assert torch.equal(st[..., 1].cpu(), x.max(-1).values), f"chan max {what}"
            assert bool((st[..., 2:] == 0).all())
            assert np.array_equal(am.cpu().numpy(), np.argmax(x.numpy(), -1)), f"chan argmax {what}: not the first maximum"
            assert untouched(guards)


@gpu
@pytest.mark.parametrize("c", ATTN_C)
def test_chan_stats_bwd(ops, c):
    for shape in ((1, 1, 1), (1, 5, 7), (2, 20, 28)):
        for view in (False, True):
            guards = []
            gen = torch.Generator().manual_seed(c + shape[1])
            g = torch.randn((*shape, 4), generator=gen)
            am = torch.randint(0, c, shape, generator=gen, dtype=torch.int32)
            gx = ops.chan_stats_bwd(put(g, view, guards), am.to(DEV), c)
            onehot = torch.nn.functional.one_hot(am.long(), c).double()
            check("attention", gx, g[..., 0:1].double() / c + onehot * g[..., 1:2].double(), f"chan_stats_bwd {shape} view {view}")
            assert untouched(guards)


def _plane(hw):
    return (20, 28) if hw == 560 else (1, hw)


# 64 slabs: fewer pixels than slabs, one per slab, two per slab with the tail empty (65, and 130 = 43 full slabs + one pixel)
SPATIAL_HW = [1, 5, 63, 64, 65, 130, 560]


@gpu
@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("hw", SPATIAL_HW)
def test_spatial_stats(ops, hw, kind):
    h, w = _plane(hw)
    for c in ATTN_C:
        for b in (1, 3):
            guards = []
            x = _data(kind, (b, h, w, c), 13 * c + hw + b)
            out, am = ops.spatial_stats(put(x, b == 3, guards))
            flat = x.reshape(b, hw, c)
            what = f"C {c} B {b}"
            assert out.shape == (2 * b, 1, 1, c) and am.shape == (b, c)
            check("attention", out[:b, 0, 0], flat.double().mean(1), f"spatial mean {what}")
            assert torch.equal(out[b:, 0, 0].cpu(), flat.max(1).values), f"spatial max {what}"
            assert np.array_equal(am.cpu().numpy(), np.argmax(flat.numpy(), 1)), f"spatial argmax {what}: not the lowest pixel index"
            assert untouched(guards)


@gpu
@pytest.mark.parametrize("hw", SPATIAL_HW)
def test_spatial_stats_bwd(ops, hw):
    h, w = _plane(hw)
    for c in ATTN_C:
        for b in (1, 3):
            gen = torch.Generator().manual_seed(c + hw + b)
            g = torch.randn((2 * b, 1, 1, c), generator=gen)
            am = torch.randint(0, hw, (b, c), generator=gen, dtype=torch.int32)
            gx = ops.spatial_stats_bwd(g.to(DEV), am.to(DEV), h, w)
            onehot = torch.nn.functional.one_hot(am.long(), hw).double().permute(0, 2, 1)      # (b, hw, c)
            ref = g[:b, 0].double() / hw + onehot * g[b:, 0].double()
            check("attention", gx, ref.reshape(b, h, w, c), f"spatial_stats_bwd C {c} B {b}")


def _scale_inputs(mode, b, h, w, c, seed):
    gen = torch.Generator().manual_seed(seed)
    v, q, gout = (torch.randn((b, h, w, c), generator=gen) for _ in range(3))
    s = torch.rand((b, h, w, 1), generator=gen) if mode == 0 else torch.randn((2 * b, 1, 1, c), generator=gen)
    return v, q, gout, s


def _scale_of(s, mode, b):
    return s if mode == 0 else (s[:b] + s[b:])


@gpu
@pytest.mark.parametrize("c", ATTN_C)
@pytest.mark.parametrize("mode", [0, 1])
def test_scale_add(ops, mode, c):
    for b, h, w in ((1, 5, 7), (3, 20, 28)):
        v, q, _, s = _scale_inputs(mode, b, h, w, c, 3 * c + b + mode)
        for with_q in (True, False):
            for view in (False, True):
                guards = []
                sd = put(s, view, guards, 0, 4) if mode == 0 else s.to(DEV)       # mode 0: channel 0 of a 4-wide tensor
                out = ops.scale_add(put(v, view, guards), sd, put(q, view, guards) if with_q else None, mode)
                ref = _scale_of(s.double(), mode, b) * v.double() + (q.double() if with_q else 0)
                check("attention", out, ref, f"scale_add B {b} q {with_q} view {view}")
                assert untouched(guards)


@gpu
@pytest.mark.parametrize("c", ATTN_C)
@pytest.mark.parametrize("mode", [0, 1])
def test_scale_add_bwd(ops, mode, c):
    for b, h, w in ((1, 5, 7), (3, 20, 28), (1, 1, 130)):
        v, _, gout, s = _scale_inputs(mode, b, h, w, c, 5 * c + b + mode)
        vr, sr = v.double().requires_grad_(True), s.double().requires_grad_(True)
        (_scale_of(sr, mode, b) * vr).backward(gout.double())
        for view in (False, True):
            guards = []
            sd = put(s, view, guards, 0, 4) if mode == 0 else s.to(DEV)
            gv, gs = ops.scale_add_bwd(put(gout, view, guards), put(v, view, guards), sd, mode)
            check("attention", gv, vr.grad, f"scale_add_bwd gv B {b} view {view}")
            check("attention", gs, sr.grad, f"scale_add_bwd gs B {b} view {view}")
            if mode == 1:       # both halves of gs are the same sum over pixels of v * gout
                assert torch.equal(gs[:b], gs[b:])
            assert untouched(guards)


# =====================================================================================================================
# 5. dilate2, channel_sum, the GRU gate gradients
@gpu
@pytest.mark.parametrize("c", [4, 96])
@pytest.mark.parametrize("odd_h,odd_w", [(True, True), (False, False), (True, False)])
def test_dilate2(ops, odd_h, odd_w, c):
    b, ho, wo = 2, 5, 7
    hd, wd = 2 * ho - int(odd_h), 2 * wo - int(odd_w)
    guards = []
    g = _data("gauss", (b, ho, wo, c), c)
    out = ops.dilate2(put(g, True, guards), hd, wd)
    ref = torch.zeros(b, hd, wd, c)
    ref[:, ::2, ::2] = g
    assert torch.equal(out.cpu(), ref) and untouched(guards)


@gpu
@pytest.mark.parametrize("c,cp,view", [(576, 576, False), (126, 128, False), (126, 128, True), (2, 4, False)])
def test_channel_sum(ops, c, cp, view):
    guards = []
    g = _data("gauss", (2, 9, 31, cp), c)              # 279 pixels a sample: two slabs of the statistics pass
    out = ops.channel_sum(put(g, view, guards), c)
    assert out.shape == (c,) and out.dtype == torch.float32
    check("small ops", out, g.double().sum((0, 1, 2))[:c], "channel_sum")
    assert untouched(guards)


@gpu
@pytest.mark.parametrize("c", [4, 128])
def test_gru_gate_backward_on_views(ops, c):
    gen = torch.Generator().manual_seed(c)
    z, r, q, h = (torch.rand((2, 5, 7, c), generator=gen) for _ in range(4))
    gy = torch.randn((2, 5, 7, c), generator=gen)
    zr, rr, qr, hr = (t.double().requires_grad_(True) for t in (z, r, q, h))
    (rr * hr).backward(gy.double())
    guards = []
    gyd, zd, rd, qd, hd = (put(t, True, guards) for t in (gy, z, r, q, h))
    dr, dh = ops.gru_rh_bwd(gyd, rd, hd)
    check("small ops", dr, rr.grad, "gru_rh_bwd dr")
    check("small ops", dh, hr.grad, "gru_rh_bwd dh")
    hr.grad = None
    ((1 - zr) * hr + zr * qr).backward(gy.double())
    dz, dq, dh = ops.gru_blend_bwd(gyd, zd, qd, hd)
    for name, a, ref in (("dz", dz, zr.grad), ("dq", dq, qr.grad), ("dh", dh, hr.grad)):
        check("small ops", a, ref, f"gru_blend_bwd {name}")
    assert untouched(guards)
