"""The on-the-fly correlation (corr_block.AlternateCorrBlock, csrc/corr_alt.hip) behind RAFT's alternate_corr.

Against an fp64 restatement of the reference's AlternateCorrBlock (grid_sample of the pooled fmap2 at coords / 2^l + delta,
dotted with fmap1, / 16) and against CorrBlock (the materialised fp32 pyramid): the alternate block's error is at most twice
CorrBlock's own + 1e-6 max|ref|, its taps are CorrBlock's bit for bit.  Measured spreads (MI355X), max|alt - fp64| /
max|CorrBlock - fp64| per coordinate case: 1.00 in 94 of the 108 (shape, batch, case) triples of the default f16x3 precision
(both errors are then the fp32 sampler's own against fp64: 2e-7 - 7e-6 of max|ref|), 0.81 - 2.14 in the rest, all of them
cases with tiny errors (far_outside, discontinuous: 2e-7 - 2e-6 of max|ref|); exact fp32: 0.75 - 1.59.  Whole network: alternate_corr=True against False and against the CPU oracle to
1e-3 px (the north-star tolerance); a 1088x1920 pair in fp32 - refused by the materialised pyramid - against the oracle.
"""
import os
import shutil
import sys
import time
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import ffraft_ref as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = [(48, 64), (46, 62), (16, 24), (17, 19), (68, 120)]


def _cfg():
    from argparse import Namespace
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"),
                     MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))


def _model(sd, alternate_corr=False):
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg(), alternate_corr=alternate_corr)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def _pooled(f2):
    """NCHW fmap2 -> its four levels (avg_pool2d(2, 2), floor semantics)."""
    lv = [f2]
    for _ in range(3):
        lv.append(F.avg_pool2d(lv[-1], 2, stride=2))
    return lv


def alt_lookup_ref(f1, f2_levels, coords, chunk=9):
    """The reference's AlternateCorrBlock, restated: f1 (B, C, H, W), f2_levels [(B, C, h_l, w_l)], coords (B, 2, H, W) [x, y]
    -> (B, 324, H, W) in the dtype of the inputs; channel k = level*81 + a*9 + b (a: x offset).  The 81 offsets go through
    grid_sample `chunk` at a time, so that no temporary grows with more than B*Q*chunk*C elements."""
    b, c, h, w = f1.shape
    q = h * w
    pts = coords.permute(0, 2, 3, 1).reshape(b, q, 1, 2)
    off = torch.linspace(-4, 4, 9, dtype=coords.dtype)
    delta = torch.stack(torch.meshgrid(off, off, indexing="ij"), -1).view(1, 1, 81, 2)
    f1q = f1.reshape(b, c, q)
    outs = []
    for lvl, f2 in enumerate(f2_levels):
        hl, wl = f2.shape[-2:]
        res = []
        for k0 in range(0, 81, chunk):
            cc = pts / 2 ** lvl + delta[:, :, k0:k0 + chunk]                      # (B, Q, n, 2)
            g = torch.cat([2 * cc[..., 0:1] / (wl - 1) - 1, 2 * cc[..., 1:2] / (hl - 1) - 1], -1)
            s = F.grid_sample(f2, g, align_corners=True)                           # (B, C, Q, n)
            res.append(torch.einsum("bcq,bcqn->bqn", f1q, s) / c ** 0.5)
        outs.append(torch.cat(res, -1))
    return torch.cat(outs, -1).permute(0, 2, 1).reshape(b, 324, h, w)


def _coord_cases(b, h, w, g):
    base = orc.coords_grid(b, h, w)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    checker = (((xs + ys) % 2) * 2 - 1).float()                 # +1 / -1 between 4-neighbours
    rows = ((ys % 2) * 2 - 1).float()
    return {
        "integer": base.clone(),
        "random": base + (torch.rand(base.shape, generator=g) * 16 - 8),
        "halves": base + 0.5, "eighths": base * 1.125,
        "far_outside": base + torch.tensor([w + 20.0, -h - 20.0]).view(1, 2, 1, 1),
        "edge": base + torch.tensor([-4.0, 4.0]).view(1, 2, 1, 1),
        # neighbouring queries 80 px apart: no tile, no row of a tile has a union that fits - single queries everywhere
        "discontinuous": base + 40.0 * checker.view(1, 1, h, w),
        # rows of the tile 24 px apart vertically: the tile's union does not fit, its rows' do
        "row_split": base + torch.stack([torch.zeros(h, w), 12.0 * rows]).view(1, 2, h, w),
        # every query on its own (uniform +-60 px): single queries, windows partly outside the plane
        "one_query": base + (torch.rand(base.shape, generator=g) * 120 - 60),
    }


def _dev_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _lookup_errors(b, h, w, precision="f16x3", seed=0):
    from focusflow_official_amd import ops
    from focusflow_official_amd.corr_block import AlternateCorrBlock, CorrBlock
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    f1, f2 = torch.randn(b, 256, h, w, generator=g), torch.randn(b, 256, h, w, generator=g)
    lv64 = _pooled(f2.double())
    prev = ops.conv_precision()
    ops.set_conv_precision(precision)
    try:
        with torch.no_grad():
            cb = CorrBlock(_dev_nhwc(f1), _dev_nhwc(f2), pyramid_dtype="fp32")
            alt = AlternateCorrBlock(_dev_nhwc(f1), _dev_nhwc(f2))
            assert alt.pyr is None
            out = {}
            for name, c in _coord_cases(b, h, w, g).items():
                cd = _dev_nhwc(c)
                o_cb, t_cb = cb(cd, want_taps=True)
                o_alt, t_alt = alt(cd, want_taps=True)
                assert torch.equal(t_alt, t_cb), f"{name}: taps differ from CorrBlock's in {(t_alt != t_cb).sum().item()} places"
                ref = alt_lookup_ref(f1.double(), lv64, c.double()).permute(0, 2, 3, 1)
                e_cb = (o_cb.cpu().double() - ref).abs().max().item()
                e_alt = (o_alt.cpu().double() - ref).abs().max().item()
                out[name] = (e_alt, e_cb, ref.abs().max().item())
    finally:
        ops.set_conv_precision(prev)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", SHAPES)
def test_alt_lookup_parity_and_taps(h, w, b):
    """Values against fp64 (bounded by CorrBlock's own error) and taps against CorrBlock, every coordinate case."""
    errs = _lookup_errors(b, h, w)
    print(f"\nspread {h}x{w} b{b}: " + ", ".join(f"{k} {e_a / max(e_c, 1e-30):.2f} ({e_a / max(m, 1e-30):.1e})" for k, (e_a, e_c, m) in errs.items()))
    for name, (e_alt, e_cb, m) in errs.items():
        assert e_alt <= 2 * e_cb + 1e-6 * m, f"{name}: alternate error {e_alt:.3e} vs CorrBlock's {e_cb:.3e} (max|ref| {m:.3e})"


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(46, 62), (17, 19)])
def test_alt_lookup_exact_fp32_precision(h, w):
    """FF_CONV_PRECISION=fp32: the exact fp32 products (32x32x2 fp32 MFMA) against fp64, bounded by CorrBlock's own error on
    its exact-fp32 route (fp32 summation of 256 products: ~3e-6 max|ref| either way)."""
    errs = _lookup_errors(3, h, w, precision="fp32")
    print(f"\nspread fp32 {h}x{w} b3: " + ", ".join(f"{k} {e_a / max(e_c, 1e-30):.2f} ({e_a / max(m, 1e-30):.1e})" for k, (e_a, e_c, m) in errs.items()))
    for name, (e_alt, e_cb, m) in errs.items():
        assert e_alt <= 2 * e_cb + 1e-6 * m, f"{name}: alternate error {e_alt:.3e} vs CorrBlock's {e_cb:.3e} (max|ref| {m:.3e})"


@pytest.mark.gpu
def test_alt_buffer_contract():
    """Inference: the shared 352-channel buffer, pad channels zero across calls.  Grad mode: a fresh tensor per call."""
    from focusflow_official_amd.corr_block import AlternateCorrBlock
    g = torch.Generator().manual_seed(3)
    b, h, w = 2, 17, 19
    f1, f2 = (_dev_nhwc(torch.randn(b, 256, h, w, generator=g)) for _ in range(2))
    c1 = _dev_nhwc(orc.coords_grid(b, h, w) + torch.rand(b, 2, h, w, generator=g) * 6 - 3)
    c2 = _dev_nhwc(orc.coords_grid(b, h, w) + torch.rand(b, 2, h, w, generator=g) * 6 - 3)
    with torch.no_grad():
        blk = AlternateCorrBlock(f1, f2)
        o1 = blk(c1)
        assert o1.shape == (b, h, w, 352)
        assert torch.count_nonzero(o1[..., 324:]).item() == 0
        v1 = o1[..., :324].clone()
        o2 = blk(c2)
        assert o2.data_ptr() == o1.data_ptr() and torch.count_nonzero(o2[..., 324:]).item() == 0
        assert not torch.equal(o2[..., :324], v1)
        assert torch.equal(blk(c1)[..., :324], v1)
    with torch.enable_grad():
        a, bb = blk(c1), blk(c1)
        assert a.data_ptr() != bb.data_ptr() and torch.equal(a, bb) and a.shape == (b, h, w, 324)
        assert torch.equal(a, v1)


@pytest.mark.gpu
def test_alt_memory_is_linear_in_the_image_area():
    """68 x 120, b = 4: bytes held after construction and one call, the 352-channel output buffer left out."""
    from focusflow_official_amd.corr_block import AlternateCorrBlock, CorrBlock
    g = torch.Generator().manual_seed(5)
    b, h, w = 4, 68, 120
    f1, f2 = (_dev_nhwc(torch.randn(b, 256, h, w, generator=g)) for _ in range(2))
    coords = _dev_nhwc(orc.coords_grid(b, h, w))
    out_bytes = b * h * w * 352 * 4
    f2_bytes = f2.numel() * 4

    def held(make):
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        with torch.no_grad():
            blk = make()
            blk(coords)
        torch.cuda.synchronize()
        n = torch.cuda.memory_allocated() - m0 - out_bytes
        del blk
        return n

    alt, cb = held(lambda: AlternateCorrBlock(f1, f2)), held(lambda: CorrBlock(f1, f2, pyramid_dtype="fp32"))
    assert 0 < alt <= 4 * f2_bytes, (alt, f2_bytes)
    assert cb >= 20 * f2_bytes, (cb, f2_bytes)


@pytest.mark.gpu
def test_corr_block_refuses_a_pyramid_beyond_the_resource_before_allocating_it():
    """1088 x 1920 (136 x 240 at 1/8): one pair's fp32 pyramid passes the lookup's 4 GB resource - refused up front, nothing
    allocated, and the message names alternate_corr=True and the fp16 pyramid (which fits)."""
    from focusflow_official_amd import _hip
    from focusflow_official_amd.corr_block import CorrBlock, pyramid_span
    f = torch.zeros(1, 136, 240, 256, device=DEV)
    assert pyramid_span(136, 240, False) >= 0xfff00000 > pyramid_span(136, 240, True)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    with torch.no_grad(), pytest.raises(_hip.FocusFlowHipError, match="alternate_corr=True") as ei:
        CorrBlock(f, f, pyramid_dtype="fp32")
    assert 'corr_pyramid_dtype="fp16"' in str(ei.value)
    assert torch.cuda.memory_allocated() == m0


@pytest.mark.gpu
def test_whole_network_alternate_vs_materialised_and_oracle(det_sd):
    """384 x 512, B = 2, 12 iterations: test_mode and the list output under no_grad, and one case with flow_init."""
    inp = [t.to(DEV) for t in orc.shifted_pair(2, 384, 512, seed=71)]
    m_ref, m_alt = _model(det_sd), _model(det_sd, alternate_corr=True)
    ys, xs = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    fi = torch.stack([3 * torch.sin(xs / 11) + 1.5, 2 * torch.cos(ys / 7) - 1]).expand(2, 2, 48, 64).contiguous()   # smooth
    with torch.no_grad():
        lo_r, up_r = m_ref(*inp, raft_iters=12, test_mode=True)
        lo_a, up_a = m_alt(*inp, raft_iters=12, test_mode=True)
        preds_r = m_ref(*inp, raft_iters=12)
        preds_a = m_alt(*inp, raft_iters=12)
        lo_fr, up_fr = m_ref(*inp, raft_iters=12, flow_init=fi.to(DEV), test_mode=True)
        lo_fa, up_fa = m_alt(*inp, raft_iters=12, flow_init=fi.to(DEV), test_mode=True)
        cpu = [t.cpu() for t in inp]
        o_lo, o_up = orc.ffraft_forward(det_sd, *cpu, raft_iters=12, test_mode=True)
        o_flo, o_fup = orc.ffraft_forward(det_sd, *cpu, raft_iters=12, flow_init=fi, test_mode=True)
    d = lambda x, y: (x.cpu() - y.cpu()).abs().max().item()     # noqa: E731
    assert d(lo_a, lo_r) <= 1e-3 and d(up_a, up_r) <= 1e-3, (d(lo_a, lo_r), d(up_a, up_r))
    assert d(lo_a, o_lo) <= 1e-3 and d(up_a, o_up) <= 1e-3, (d(lo_a, o_lo), d(up_a, o_up))
    assert len(preds_a) == 12 and max(d(x, y) for x, y in zip(preds_a, preds_r)) <= 1e-3
    assert d(preds_a[-1], o_up) <= 1e-3
    # (flow_up is in full-resolution pixels, 8x flow_low's scale: with this flow_init the materialised forward itself lands at
    # 0.94e-3 from the oracle there - measured - so the alternate one is held to 1.5x that)
    errs = (d(lo_fa, lo_fr), d(lo_fa, o_flo), d(up_fa, o_fup), d(lo_fr, o_flo), d(up_fr, o_fup))
    assert max(errs[:2]) <= 1e-3 and errs[2] <= max(1e-3, 1.5 * errs[4]), \
        f"flow_init: alt vs materialised, alt vs oracle (low, up); materialised vs oracle (low, up): {errs}"


@pytest.mark.gpu
def test_alt_graph_replay(det_sd):
    """A captured forward of an alternate_corr model matches eager (2e-4, as test_hipgraph_replay_matches_eager) and replays
    bit-identically."""
    from focusflow_official_amd.graph import GraphedForward
    m = _model(det_sd, alternate_corr=True)
    a = [t.to(DEV) for t in orc.shifted_pair(1, 128, 192, seed=31)]
    b = [t.to(DEV) for t in orc.shifted_pair(1, 128, 192, seed=32)]
    with torch.no_grad():
        ea = [t.clone() for t in m(*a, raft_iters=4, test_mode=True)]
    gf = GraphedForward(m, a, raft_iters=4)
    ga = [t.clone() for t in gf(*a)]
    gb = [t.clone() for t in gf(*b)]
    ga2 = [t.clone() for t in gf(*a)]
    torch.cuda.synchronize()
    for x, y in zip(ea, ga):
        assert (x - y).abs().max().item() <= 2e-4
    for x, y in zip(ga, ga2):
        assert torch.equal(x, y)
    assert not torch.equal(ga[1], gb[1])


def _recorded_pass(m, inp, w):
    for p in m.parameters():
        p.grad = None
    preds = m(*inp, raft_iters=3)
    sum((p * x).sum() for p, x in zip(preds, w)).backward()
    torch.cuda.synchronize()
    return [p.detach().clone() for p in preds], {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _grads_agree(ga, gb, gb2, rel):
    """Every gradient within rel x its max of the other setting's - or within 4x the spread of two passes of that setting
    (tensors whose gradient is accumulation noise: fp32 atomics make repeated backward passes differ; one pair of passes is a
    rough estimate of that spread - 2.2x it was measured between two runs of one and the same route)."""
    assert ga.keys() == gb.keys() == gb2.keys() and ga
    bad = {}
    for k in ga:
        diff, noise = (ga[k] - gb[k]).abs().max().item(), (gb2[k] - gb[k]).abs().max().item()
        if diff > max(rel * gb[k].abs().max().item(), 4 * noise):
            bad[k] = (diff, gb[k].abs().max().item(), noise)
    assert not bad, f"gradients apart (diff, max, spread of two passes of one setting): {bad}"


@pytest.mark.gpu
def test_recorded_passes_keep_the_materialised_pyramid(det_sd):
    """Trained encoders: alternate_corr=True records the materialised pyramid - outputs equal to alternate_corr=False, gradients
    within 2e-6 of each tensor's max (two backward passes of one setting differ by up to 7.1e-7), one warning per model.
    Frozen encoders, trained update block: the on-the-fly block runs on the per-operation tape; against the materialised pyramid
    on that same tape (train_loop.ENABLED off) the flows agree to 1e-3 px and the update-block gradients within 1e-2 of each
    tensor's max.  (Measured: 5.5e-3 on mask.0.bias, 1.2e-3 on the GRU's q convolutions, 5e-4 on convc1 - the same against the
    fused node.  The two blocks' correlation values differ by rounding only, ~1e-6 relative, but every ReLU / gate of the
    update block that the perturbation flips changes the weight gradient at that pixel by O(1): two passes of ONE setting
    differ by < 1e-6 relative.)"""
    from focusflow_official_amd import train_loop
    inp = [t.to(DEV) for t in orc.shifted_pair(1, 128, 192, seed=5)]
    g = torch.Generator().manual_seed(11)
    w = [torch.randn(1, 2, 128, 192, generator=g).to(DEV) for _ in range(3)]
    m_ref, m_alt = _model(det_sd), _model(det_sd, alternate_corr=True)
    out_r, gr = _recorded_pass(m_ref, inp, w)
    _, gr2 = _recorded_pass(m_ref, inp, w)
    with pytest.warns(UserWarning, match="alternate_corr"):
        out_a, ga = _recorded_pass(m_alt, inp, w)
    for x, y in zip(out_a, out_r):
        assert torch.equal(x, y)
    _grads_agree(ga, gr, gr2, 2e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _recorded_pass(m_alt, inp, w)                  # (once per model)

    for m in (m_ref, m_alt):
        for k, p in m.named_parameters():
            p.requires_grad_(".update_block." in k)
    out_a, ga = _recorded_pass(m_alt, inp, w)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(train_loop, "ENABLED", False)
        out_r, gr = _recorded_pass(m_ref, inp, w)
        _, gr2 = _recorded_pass(m_ref, inp, w)
    assert all(".update_block." in k for k in ga) and ga.keys() == gr.keys()
    _grads_agree(ga, gr, gr2, 1e-2)
    assert max((x - y).abs().max().item() for x, y in zip(out_a, out_r)) <= 1e-3


@pytest.mark.gpu
def test_1080p_pair_in_fp32_against_the_oracle(det_sd, monkeypatch):
    """1088 x 1920, B = 1, fp32 (pyramid and products), alternate_corr=True, 3 iterations: the materialised pyramid of this
    pair (5.7 GB) is refused; the on-the-fly block runs it, flow_low within 1e-3 px of the CPU oracle - its encoders and
    update loop, the lookup replaced by the on-the-fly restatement (no Q^2 volume on the host).  Under FF_CONV_PRECISION=fp32:
    at this plane (136 x 240) the update block's split-format convolutions write NaN into a corner of the first iteration's
    output for some inputs, with either correlation block - a defect of its own.  38 s on the GPU box's 16 host cores."""
    from focusflow_official_amd import ops
    t0 = time.time()
    inp = orc.shifted_pair(1, 1088, 1920, seed=13)
    m = _model(det_sd, alternate_corr=True)
    prev = ops.conv_precision()
    ops.set_conv_precision("fp32")
    try:
        with torch.no_grad():
            lo, _ = m(*[t.to(DEV) for t in inp], raft_iters=3, test_mode=True)
    finally:
        ops.set_conv_precision(prev)
    lo = lo.cpu()
    del m
    torch.cuda.empty_cache()
    sd, p = det_sd, "flow_net."
    with torch.no_grad():
        i1, i2, m1, m2 = orc.prepare_inputs(*inp)
        f1 = orc.cce_encoder(sd, p + "fnet", i1, m1, "instance", False, "1x1conv")
        f2 = orc.cce_encoder(sd, p + "fnet", i2, m2, "instance", False, "1x1conv")
        cnet = orc.cce_encoder(sd, p + "cnet", i1, m1, "batch", False, "1x1conv")
        net, ctx = torch.split(cnet, [128, 128], dim=1)
        net, ctx = torch.tanh(net), torch.relu(ctx)
        lv = _pooled(f2)
        monkeypatch.setattr(orc, "corr_lookup", lambda pyr, coords, radius=4: alt_lookup_ref(f1, lv, coords).float())
        c0 = orc.coords_grid(1, 136, 240)
        _, c1 = orc.update_loop(sd, p + "update_block", None, net, ctx, c0, c0.clone(), 3)
    ref = c1 - c0
    assert torch.isfinite(lo).all() and torch.isfinite(ref).all(), (torch.isfinite(lo).all().item(), torch.isfinite(ref).all().item())
    err = (lo - ref).abs().max().item()
    assert err <= 1e-3, err
    print(f"1080p alternate_corr vs oracle: {err:.2e} px, {time.time() - t0:.0f} s")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_alt_corr_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "corr_alt.hip"))
    assert len(kernels) >= 4, kernels
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"corr_alt.hip: kernels with scratch (bytes per lane): {spilled}"
