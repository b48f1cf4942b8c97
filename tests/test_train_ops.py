"""Operator tests of the kernels that exist only for the recorded update loop (csrc/train_ops.hip): ff_gru_bwd_blend,
ff_gru_bwd_rh, ff_gru_bwd_out - the gate derivatives and gradient sums between the input-gradient convolutions of a
SepConvGRU pass - and ff_sum_stack, each against a plain fp64 reference on the CPU (tests/train_ops_ref.py), called through
_hip.call exactly as train_loop.UpdateLoopFn.backward calls them.

The references come first: test_reference_chain_reproduces_autograd (no GPU) chains them in the order of the backward over a
tiny two-pass SepConvGRU and must reproduce torch autograd's d h and d motion to 1e-12 - which contribution adds where is
pinned before any kernel is compared with them.

Shapes (train_ops_ref.SHAPES): less than one block, a C of 8 whose Cm cuts a 4-vector, the loop tests' size, and 8601 pixels
(more than 1024 blocks of work: the grid-stride loop runs, its second trip ragged).  Layouts: dense; "production" (z | r and
g_z | g_r the halves of one 2C-wide buffer, as the backward holds them); "views" (every tensor in channels 4 .. 4 + C of a
SENTINEL-filled buffer C + 8 wide).  After every call the inputs' buffers must be bit-identical to what they were, the
surroundings of every output must still hold SENTINEL, and in place (as production runs) and out of place must give the
same bits.  The amax words are compared bit for bit with max|g| of the tensor the kernel wrote; masks bit for bit.  (That a word
only grows - a larger preloaded value stays, an all-zero gradient leaves zero - is held by test_amax_word_only_grows in
tests/test_pointwise_ops.py, for these three producers as for the others.)

Tolerances: `check` is that of tests/test_pointwise_ops.py (the smallest rtol = atol_rel the data would pass:
max |a - ref| / (|ref| + max|ref|)).  Largest value measured on the MI355X against fp64, and the tolerance chosen from it
(about four times the measurement; the project's convention for these groups is 3e-5):

    kernel              measured    tolerance   convention
    ff_gru_bwd_blend    6.04e-08    2.5e-07     3e-5
    ff_gru_bwd_rh       4.93e-08    2e-07       3e-5
    ff_gru_bwd_out      2.85e-08    1.2e-07     3e-5
    ff_sum_stack        1.10e-07    4.5e-07     3e-5      (T = 12; T = 1 and T = 2 are compared bit for bit)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as R
from test_pointwise_ops import DEV, SENTINEL, out_view, put, surroundings_kept, untouched, word_equals_max

gpu = pytest.mark.gpu

TOL = {                               # about 4 x the largest error measured (module docstring); the convention it replaces
    "blend": 2.5e-7,                  # 3e-5
    "rh": 2e-7,                       # 3e-5
    "out": 1.2e-7,                    # 3e-5
    "sum_stack": 4.5e-7,              # 3e-5
}
MEASURED = {}
LAYOUTS = ["dense", "production", "views"]


def check(group, a, ref, what):
    a, ref = a.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert a.shape == ref.shape, f"{what}: shape {a.shape} vs {ref.shape}"
    top = max(1e-6, float(np.abs(ref).max()))
    need = float((np.abs(a - ref) / (np.abs(ref) + top)).max())
    MEASURED[group] = max(MEASURED.get(group, 0.0), need)
    print(f"[{group}] {what}: {need:.3e}")
    assert need <= TOL[group], f"{what}: needs a tolerance of {need:.3e}, {group} allows {TOL[group]:.1e} (max|ref| {top:.3e})"


@pytest.fixture(scope="module")
def hip():
    from focusflow_official_amd import _hip
    yield _hip
    print("\nlargest error per kernel against fp64:", {k: f"{v:.3e}" for k, v in sorted(MEASURED.items())})


# =====================================================================================================================
# 1. the references themselves (no GPU)
def test_reference_chain_reproduces_autograd():
    """The three steps chained as UpdateLoopFn.backward chains them (pass 2 then pass 1, dm initialised by pass 2's rh step,
    each pass's z|r input gradient handed to the next blend step, the out step last), with fp64 F.conv2d input gradients for
    the four convolutions, over a two-pass SepConvGRU with random weights: C = 8, Cm = 6, plane 3 x 5, motion =
    cat(relu(m), flow).  Must reproduce autograd's d h_in and d m (through the ReLU) to 1e-12 of each tensor's maximum."""
    g = torch.Generator().manual_seed(11)
    b, c, cm, hh, ww = 2, 8, 6, 3, 5
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    h0 = torch.tanh(rnd(b, c, hh, ww)).requires_grad_(True)
    m = rnd(b, cm, hh, ww).requires_grad_(True)
    flow = rnd(b, c - cm, hh, ww)
    kernels = [(1, 5), (5, 1)]
    wzr = [rnd(2 * c, 2 * c, kh, kw) / (2 * c * 5) ** 0.5 for kh, kw in kernels]
    wq = [rnd(c, 2 * c, kh, kw) / (2 * c * 5) ** 0.5 for kh, kw in kernels]
    bzr, bq = [rnd(2 * c) for _ in kernels], [rnd(c) for _ in kernels]
    pads = [(kh // 2, kw // 2) for kh, kw in kernels]
    motion = torch.cat([torch.relu(m), flow], 1)
    hs, zs, rs, qs = [h0], [], [], []
    for k in range(2):                                                        # update.py:45-60
        zr = torch.sigmoid(F.conv2d(torch.cat([hs[k], motion], 1), wzr[k], bzr[k], padding=pads[k]))
        z, r = zr[:, :c], zr[:, c:]
        q = torch.tanh(F.conv2d(torch.cat([r * hs[k], motion], 1), wq[k], bq[k], padding=pads[k]))
        hs.append((1 - z) * hs[k] + z * q)
        zs.append(z), rs.append(r), qs.append(q)
    dout = rnd(b, c, hh, ww)
    want_dh, want_dm = torch.autograd.grad(hs[2], [h0, m], dout)

    last = lambda t: t.detach().permute(0, 2, 3, 1)                          # noqa: E731  NCHW -> channels last
    first = lambda t: t.permute(0, 3, 1, 2)                                   # noqa: E731

    def dgrad(w, gout, pad):                                                  # [d first input | d motion], channels last
        return last(torch.nn.grad.conv2d_input((b, 2 * c, hh, ww), w, first(gout).contiguous(), padding=pad))

    dh = last(dout)
    dm = torch.full((b, hh, ww, c), float("nan"), dtype=torch.float64)       # never read before pass 2's rh step sets it
    later_zc = None
    for k in (1, 0):
        hprev, z, r, q = last(hs[k]), last(zs[k]), last(rs[k]), last(qs[k])
        g_z, g_q, dh, dm = R.blend(dh, z, q, hprev, later_zc, dm)
        dqc = dgrad(wq[k], g_q, pads[k])
        g_r, dh, dm = R.rh(dqc, r, hprev, dh, dm, dm_init=(k == 1))
        later_zc = dgrad(wzr[k], torch.cat([g_z, g_r], -1), pads[k])
    dh, g_m = R.out(dh, later_zc, dm, last(motion), cm)
    for name, got, want in (("d h_in", first(dh), want_dh), ("d m", first(g_m)[:, :cm], want_dm)):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"{name}: {err:.2e} of the maximum")
        assert err <= 1e-12, f"{name}: {err:.2e} of the maximum"
    assert bool((g_m[..., cm:] == 0).all()), "the flow channels carry no gradient"
    assert bool((want_dm == 0).any()), "the case has no masked element"


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_cases_can_tell_the_two_words_of_blend_apart(shape):
    """No GPU: max|g_z| and max|g_q| of every case differ by more than 2 x (a swap of the two words would show), and about
    half the motion mask is exact zeros."""
    x = R.case(shape)
    for key in ("blend", "blend_dzc"):
        g_z, g_q = x["ref"][key][:2]
        mz, mq = float(g_z.abs().max()), float(g_q.abs().max())
        assert max(mz, mq) > 2 * min(mz, mq), f"{key}: max|g_z| {mz:.3f}, max|g_q| {mq:.3f}"
    share = float((x["motion"] == 0).double().mean())
    assert 0.3 < share < 0.7, share


# =====================================================================================================================
# 2. the three gate-gradient kernels
class Bufs:
    """The device tensors of one call in one layout, with what must hold afterwards: read-only inputs unchanged (buffers
    included), the surroundings of written views still SENTINEL."""

    def __init__(self, layout):
        self.views, self.prod = layout == "views", layout == "production"
        self.guards, self.kept = [], []

    def inp(self, t):
        if self.views:
            return put(t, True, self.guards)
        d = t.to(DEV)
        self.guards.append((d, d.clone()))
        return d

    def inp_pair(self, a, b):
        """Two read-only tensors; in the production layout the halves of ONE buffer (z | r after the conv-by-conv forward)."""
        if not self.prod:
            return self.inp(a), self.inp(b)
        c = a.shape[-1]
        buf = torch.cat([a, b], -1).to(DEV)
        self.guards.append((buf, buf.clone()))
        return buf[..., :c], buf[..., c:]

    def out(self, shape):
        if not self.views:
            return torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)
        buf, v = out_view(shape)
        self.kept.append((buf, shape[-1]))
        return v

    def io(self, t):
        """A tensor the call reads and writes."""
        v = self.out(tuple(t.shape))
        v.copy_(t)
        return v

    def out_pair(self, shape):
        """Two outputs; in the production layout the halves of ONE SENTINEL-filled buffer (g_z | g_r)."""
        if not self.prod:
            return self.out(shape), self.out(shape)
        c = shape[-1]
        buf = torch.full((*shape[:-1], 2 * c), SENTINEL, dtype=torch.float32, device=DEV)
        return buf[..., :c], buf[..., c:]

    def intact(self):
        return untouched(self.guards) and all(surroundings_kept(buf, 4, c) for buf, c in self.kept)


def zero_word():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def all_sentinel(t):
    return bool((t == SENTINEL).all())


def _ld(t, fallback=0):
    from focusflow_official_amd import ops
    return ops._ld(t) if t is not None else fallback


def call_blend(hip, dh_in, dzc, dm, z, q, h, gz, gq, dh_out, wz, wq, npix=None, c=None, ld=None):
    """ff_gru_bwd_blend as train_loop.py calls it; `ld`: {argument name: leading dimension} overrides (refusal tests)."""
    from focusflow_official_amd import ops
    p, st = ops._p, ops._stream
    c = z.shape[-1] if c is None else c
    npix = z.numel() // z.shape[-1] if npix is None else npix
    L = dict(dh_in=_ld(dh_in), dzc=_ld(dzc), dm=_ld(dm, c), z=_ld(z), q=_ld(q), h=_ld(h), gz=_ld(gz), gq=_ld(gq), dh_out=_ld(dh_out))
    L.update(ld or {})
    hip.call("ff_gru_bwd_blend", p(dh_in), L["dh_in"], p(dzc), L["dzc"], p(dm), L["dm"], p(z), L["z"], p(q), L["q"], p(h), L["h"],
             p(gz), L["gz"], p(gq), L["gq"], p(dh_out), L["dh_out"], p(wz), p(wq), npix, c, st())


def call_rh(hip, dqc, r, h, gr, dh, dm, dm_init, wz, npix=None, c=None, ld=None):
    from focusflow_official_amd import ops
    p, st = ops._p, ops._stream
    c = r.shape[-1] if c is None else c
    npix = r.numel() // r.shape[-1] if npix is None else npix
    L = dict(dqc=_ld(dqc), r=_ld(r), h=_ld(h), gr=_ld(gr), dh=_ld(dh), dm=_ld(dm))
    L.update(ld or {})
    hip.call("ff_gru_bwd_rh", p(dqc), L["dqc"], p(r), L["r"], p(h), L["h"], p(gr), L["gr"], p(dh), L["dh"], p(dm), L["dm"], dm_init, p(wz),
             npix, c, st())


def call_out(hip, dh, dzc, dm, motion, dh_out, gm, cm, wm, npix=None, c=None, ld=None):
    from focusflow_official_amd import ops
    p, st = ops._p, ops._stream
    c = motion.shape[-1] if c is None else c
    npix = motion.numel() // motion.shape[-1] if npix is None else npix
    L = dict(dh=_ld(dh), dzc=_ld(dzc), dm=_ld(dm), motion=_ld(motion), dh_out=_ld(dh_out), gm=_ld(gm))
    L.update(ld or {})
    hip.call("ff_gru_bwd_out", p(dh), L["dh"], p(dzc), L["dzc"], p(dm), L["dm"], p(motion), L["motion"], p(dh_out), L["dh_out"], p(gm), L["gm"],
             cm, p(wm), npix, c, st())


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_gru_bwd_blend(hip, shape, layout):
    x = R.case(shape)
    full = tuple(x["z"].shape)
    for with_dzc in (False, True):
        ref_gz, ref_gq, ref_dh, ref_dm = x["ref"]["blend_dzc" if with_dzc else "blend"]
        runs = []
        for inplace in (True, False):
            what = f"dzc {with_dzc} in place {inplace}"
            B = Bufs(layout)
            z, _r = B.inp_pair(x["z"], x["r"])
            q, h = B.inp(x["q"]), B.inp(x["h"])
            dzc = B.inp(x["dzc"]) if with_dzc else None
            if with_dzc:
                dm = B.io(x["dm"])
            else:                     # without dzc the kernel has no business with dm: no pointer at all, or one it must not follow
                dm = None if inplace else B.out(full)
            dh_in = B.io(x["dh"]) if inplace else B.inp(x["dh"])
            dh_out = dh_in if inplace else B.out(full)
            gz, gr_half = B.out_pair(full)
            gq = B.out(full)
            wz, wq = zero_word(), zero_word()
            call_blend(hip, dh_in, dzc, dm, z, q, h, gz, gq, dh_out, wz, wq)
            check("blend", gz, ref_gz, f"g_z {what}")
            check("blend", gq, ref_gq, f"g_q {what}")
            check("blend", dh_out, ref_dh, f"dh_out {what}")
            if with_dzc:
                check("blend", dm, ref_dm, f"dm += {what}")
            elif dm is not None:
                assert all_sentinel(dm), f"{what}: dm written without a dzc"
            assert all_sentinel(gr_half), f"{what}: the g_r half of the buffer was written"
            assert word_equals_max(wz, gz), f"{what}: the first word is not the bits of max|g_z|"
            assert word_equals_max(wq, gq), f"{what}: the second word is not the bits of max|g_q|"
            assert B.intact(), f"{what}: an input buffer or the surroundings of an output were written"
            runs.append([t.clone() for t in (gz, gq, dh_out)] + ([dm.clone()] if with_dzc else []) + [wz, wq])
        assert all(torch.equal(a, b) for a, b in zip(*runs)), f"dzc {with_dzc}: in place and out of place differ"


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_gru_bwd_rh(hip, shape, layout):
    x = R.case(shape)
    full = tuple(x["z"].shape)
    for dm_init in (1, 0):
        ref_gr, ref_dh, ref_dm = x["ref"]["rh_init" if dm_init else "rh_add"]
        what = f"dm_init {dm_init}"
        B = Bufs(layout)
        _z, r = B.inp_pair(x["z"], x["r"])
        h, dqc = B.inp(x["h"]), B.inp(x["dqc"])
        dh = B.io(x["dh"])
        dm = B.io(torch.full(full, float("nan")) if dm_init else x["dm"])       # dm_init: whatever dm holds is overwritten, unread
        gz_half, gr = B.out_pair(full)
        wz = zero_word()
        call_rh(hip, dqc, r, h, gr, dh, dm, dm_init, wz)
        check("rh", gr, ref_gr, f"g_r {what}")
        check("rh", dh, ref_dh, f"dh {what}")
        if dm_init:                                                               # a copy of the q input gradient's second half
            assert torch.equal(dm.cpu(), x["dqc"][..., full[-1]:]), f"{what}: dm is not the motion half of dqc"
        check("rh", dm, ref_dm, f"dm {what}")
        assert all_sentinel(gz_half), f"{what}: the g_z half of the buffer was written"
        assert word_equals_max(wz, gr), f"{what}: the word is not the bits of max|g_r|"
        assert B.intact(), f"{what}: an input buffer or the surroundings of an output were written"


def _run_out(hip, x, layout, inplace, cm):
    full = tuple(x["z"].shape)
    B = Bufs(layout)
    dzc, dm, motion = B.inp(x["dzc"]), B.inp(x["dm"]), B.inp(x["motion"])       # dm is only read here
    dh_in = B.io(x["dh"]) if inplace else B.inp(x["dh"])
    dh_out = dh_in if inplace else B.out(full)
    gm = B.out(full)
    wm = zero_word()
    call_out(hip, dh_in, dzc, dm, motion, dh_out, gm, cm, wm)
    return B, dh_out, gm, wm


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_gru_bwd_out(hip, shape, layout):
    x = R.case(shape)
    ref_dh, ref_gm = x["ref"]["out"]
    runs = []
    for inplace in (True, False):
        what = f"in place {inplace}"
        B, dh_out, gm, wm = _run_out(hip, x, layout, inplace, x["cm"])
        check("out", dh_out, ref_dh, f"dh_out {what}")
        check("out", gm, ref_gm, f"g_m {what}")
        assert torch.equal(gm.cpu() != 0, ref_gm != 0), f"{what}: the mask (channel < Cm and motion > 0) differs"
        assert word_equals_max(wm, gm), f"{what}: the word is not the bits of max|g_m|"
        assert B.intact(), f"{what}: an input buffer (dm among them) or the surroundings of an output were written"
        runs.append([dh_out.clone(), gm.clone(), wm])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "in place and out of place differ"


@gpu
@pytest.mark.parametrize("cm", ["C", 0])
def test_gru_bwd_out_with_every_and_with_no_motion_channel(hip, cm):
    shape = R.SHAPES[1]
    cm = shape[3] if cm == "C" else 0
    x = R.case(shape, cm)
    ref_dh, ref_gm = x["ref"]["out"]
    B, dh_out, gm, wm = _run_out(hip, x, "views", True, cm)
    check("out", dh_out, ref_dh, "dh_out")
    check("out", gm, ref_gm, "g_m")
    assert torch.equal(gm.cpu() != 0, ref_gm != 0) and bool((ref_gm != 0).any()) == (cm > 0)
    assert (wm.item() == 0) == (cm == 0) and word_equals_max(wm, gm) and B.intact()


@gpu
@pytest.mark.parametrize("scale", [4.0, 0.25], ids=["g_r-larger", "g_z-larger"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_blend_then_rh_leave_the_larger_maximum_in_their_shared_word(hip, shape, scale):
    """W_ZR1 / W_ZR2 of the backward: the blend step and the rh step write the two halves of G_zr and the same word, which the
    z|r input gradient then scales all 2C channels by."""
    x = R.case(shape)
    full = tuple(x["z"].shape)
    B = Bufs("production")
    z, r = B.inp_pair(x["z"], x["r"])
    q, h, dqc = B.inp(x["q"]), B.inp(x["h"]), B.inp(x["dqc"] * scale)
    dh, dm = B.io(x["dh"]), B.out(full)
    gz, gr = B.out_pair(full)
    gq = B.out(full)
    wz, wq = zero_word(), zero_word()
    call_blend(hip, dh, None, None, z, q, h, gz, gq, dh, wz, wq)
    after_blend = wz.clone()
    call_rh(hip, dqc, r, h, gr, dh, dm, 1, wz)
    mz, mr = gz.abs().max().item(), gr.abs().max().item()
    assert (mr > mz) == (scale > 1), f"max|g_z| {mz}, max|g_r| {mr}: the case does not do what its name says"
    assert word_equals_max(after_blend, gz)
    assert word_equals_max(wz, torch.cat([gz, gr], -1)), "the shared word is not max(max|g_z|, max|g_r|)"
    assert word_equals_max(wq, gq) and B.intact()


# =====================================================================================================================
# 3. ff_sum_stack: 2048 blocks of 256 lanes of 4 floats = 2097152 elements in one trip of its grid-stride loop
SUM_N = [4, 2048 * 256 * 4 + 4 * 259]
_SUM_SRC = {}


def _sum_src(n):
    if n not in _SUM_SRC:
        _SUM_SRC[n] = torch.randn((12, n), generator=torch.Generator().manual_seed(n % 1000))
    return _SUM_SRC[n]


@gpu
@pytest.mark.parametrize("n", SUM_N)
@pytest.mark.parametrize("T", [1, 2, 12])
def test_sum_stack(hip, T, n):
    from focusflow_official_amd import ops
    src = _sum_src(n)[:T].contiguous()
    sbuf = torch.full((T * n + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    sbuf[4:4 + T * n] = src.reshape(-1).to(DEV)
    snap = sbuf.clone()
    dbuf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    hip.call("ff_sum_stack", ops._p(sbuf[4:]), T, n, ops._p(dbuf[4:]), ops._stream())
    got = dbuf[4:4 + n].cpu()
    check("sum_stack", got, R.sum_stack(src.double()), f"T {T} n {n}")
    if T == 1:
        assert torch.equal(got, src[0]), "T = 1 is a copy"
    if T == 2:
        assert torch.equal(got, src[0] + src[1]), "T = 2 is one fp32 addition"
    assert torch.equal(sbuf, snap), "src was written"
    assert all_sentinel(dbuf[:4]) and all_sentinel(dbuf[4 + n:]), "dst was written outside its n elements"


# =====================================================================================================================
# 4. refusals: non-zero return (FocusFlowHipError through _hip.call) with the entry's message, and nothing written
def _refused(hip, message, fn, outputs, words):
    with pytest.raises(hip.FocusFlowHipError, match=message):
        fn()
    torch.cuda.synchronize()
    assert all(all_sentinel(t) for t in outputs), f"{message}: a refused call wrote an output"
    assert all(w.item() == 0 for w in words), f"{message}: a refused call wrote a word"


def _off_by_one_float(t):
    """The same shape and leading dimension, four bytes further on: not 16-byte aligned."""
    buf = torch.zeros((*t.shape[:-1], t.shape[-1] + 8), dtype=torch.float32, device=DEV)
    return buf[..., 1:1 + t.shape[-1]]


@gpu
def test_gate_gradient_entries_refuse_what_they_cannot_run(hip):
    x = R.case(R.SHAPES[1])
    c, cm = R.SHAPES[1][3:]
    full = tuple(x["z"].shape)
    B = Bufs("dense")
    t = {k: B.inp(x[k]) for k in ("z", "r", "q", "h", "motion", "dh", "dm", "dzc", "dqc")}
    o = {k: B.out(full) for k in ("gz", "gq", "gr", "gm", "dh_out", "dh_io", "dm_io")}
    wz, wq = zero_word(), zero_word()
    outs, words = list(o.values()), [wz, wq]
    BAD, ALIGN = ": bad argument", ": 16-byte aligned NHWC tensors, lds % 4 == 0"

    def blend(ld=None, **kw):
        a = dict(dh_in=t["dh"], dzc=t["dzc"], dm=o["dm_io"], z=t["z"], q=t["q"], h=t["h"], gz=o["gz"], gq=o["gq"], dh_out=o["dh_out"], wz=wz, wq=wq)
        extra = {k: kw.pop(k) for k in ("c", "npix") if k in kw}
        a.update(kw)
        return lambda: call_blend(hip, ld=ld, **a, **extra)

    def rh(ld=None, **kw):
        a = dict(dqc=t["dqc"], r=t["r"], h=t["h"], gr=o["gr"], dh=o["dh_io"], dm=o["dm_io"], dm_init=0, wz=wz)
        extra = {k: kw.pop(k) for k in ("c", "npix") if k in kw}
        a.update(kw)
        return lambda: call_rh(hip, ld=ld, **a, **extra)

    def out(ld=None, **kw):
        a = dict(dh=t["dh"], dzc=t["dzc"], dm=t["dm"], motion=t["motion"], dh_out=o["dh_out"], gm=o["gm"], cm=cm, wm=wz)
        extra = {k: kw.pop(k) for k in ("c", "npix") if k in kw}
        a.update(kw)
        return lambda: call_out(hip, ld=ld, **a, **extra)

    # C % 4 != 0
    _refused(hip, "ff_gru_bwd_blend" + BAD, blend(c=6), outs, words)
    _refused(hip, "ff_gru_bwd_rh" + BAD, rh(c=6), outs, words)
    _refused(hip, "ff_gru_bwd_out" + BAD, out(c=6), outs, words)
    # Cm > C
    _refused(hip, "ff_gru_bwd_out" + BAD, out(cm=c + 1), outs, words)
    # the [d h | d motion] tensor narrower than 2C
    _refused(hip, "ff_gru_bwd_blend" + ALIGN, blend(ld=dict(dzc=2 * c - 4)), outs, words)
    _refused(hip, "ff_gru_bwd_rh" + BAD, rh(ld=dict(dqc=2 * c - 4)), outs, words)
    _refused(hip, "ff_gru_bwd_out" + BAD, out(ld=dict(dzc=2 * c - 4)), outs, words)
    # a leading dimension that is no multiple of 4, a pointer that is not 16-byte aligned: every tensor argument in turn
    for entry, make, names in (("ff_gru_bwd_blend", blend, ("dh_in", "dzc", "dm", "z", "q", "h", "gz", "gq", "dh_out")),
                               ("ff_gru_bwd_rh", rh, ("dqc", "r", "h", "gr", "dh", "dm")),
                               ("ff_gru_bwd_out", out, ("dh", "dzc", "dm", "motion", "dh_out", "gm"))):
        for name in names:
            wide = name in ("dzc", "dqc")
            _refused(hip, entry + ALIGN, make(ld={name: (2 * c if wide else c) + 2}), outs, words)
            like = t["dzc"] if wide else t["z"]
            _refused(hip, entry + ALIGN, make(**{name: _off_by_one_float(like)}), outs, words)
    # no word to write the maximum to
    _refused(hip, "ff_gru_bwd_blend" + BAD, blend(wq=None), outs, words)
    _refused(hip, "ff_gru_bwd_rh" + BAD, rh(wz=None), outs, words)
    _refused(hip, "ff_gru_bwd_out" + BAD, out(wm=None), outs, words)
    assert B.intact()


@gpu
def test_sum_stack_refuses_what_it_cannot_run(hip):
    from focusflow_official_amd import ops
    src = torch.full((2 * 8 + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    dst = torch.full((8 + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    p, st = ops._p, ops._stream
    for args in ((p(src), 2, 6, p(dst)),                      # n % 4 != 0
                 (p(src[1:]), 2, 8, p(dst)),                   # src not 16-byte aligned
                 (p(src), 2, 8, p(dst[1:])),                   # dst
                 (p(src), 0, 8, p(dst)), (p(src), 2, 0, p(dst)), (p(None), 2, 8, p(dst)), (p(src), 2, 8, p(None))):
        _refused(hip, "ff_sum_stack: bad argument", lambda a=args: hip.call("ff_sum_stack", *a, st()), [src, dst], [])
