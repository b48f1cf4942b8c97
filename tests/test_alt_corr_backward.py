"""The backward of the on-the-fly correlation (csrc/corr_alt_bwd.hip, ops.corr_alt_lookup_bwd) in recorded passes:
corr_block.AlternateCorrBlock behind the token pair fn.CorrBuildFn / LookupFn, the fused update-loop node on that block
(train_loop.UpdateLoopFn) and RAFT's route for alternate_corr=True when a recorded batch's pyramid passes
corr_block._MAX_PYRAMID_BYTES.

The lookup is bilinear in (fmap1, fmap2) and its coefficients depend on the coordinates and upstream gradients only, so
channel c of d fmap1 depends on channel c of fmap2 alone (and vice versa): the fp64 references below run CPU autograd through
test_alt_corr.alt_lookup_ref on a few channels and scale the result to the 256-channel block's 1/16.

Bounds:
  * kernel vs fp64, per tensor: max|alt - fp64| <= 2 x max|materialised - fp64| + 1e-6 x max|fp64| (the materialised route:
    CorrBlock recorded, fn.CorrBuildFn / LookupFn, on identical inputs);
  * 1088 x 1920 plane: max|alt - fp64| <= 1e-5 x max|fp64|;
  * update loop: test_update_loop.py's bounds (fp64, fused vs tape at 2e-5) on the forced on-the-fly route, and that route
    against the materialised one on identical inputs at 1e-4 x max;
  * memory: 4x the plane area -> <= 4.5x the peak; a recorded 1088 x 1920 pass completes with finite gradients and flows
    within 1e-3 px of inference.
Measured on an MI355X:
  * kernel vs fp64: max|alt - fp64| / max|materialised - fp64| 1.05 - 1.36 per (shape, batch, precision), 2.22 once (46x62, b 1:
    both errors tiny there); max|alt - fp64| 7e-7 - 6.5e-6 of max|fp64| (the backward is exact fp32 in both precisions);
  * 1088 x 1920 plane: 7.3e-6 (d fmap1), 6.8e-6 (d fmap2) of max;
  * update loop, largest over all tensors as a fraction of max:   fused - fp64   tape - fp64   fused - tape   on-the-fly - materialised
        default (b 2, 16x24, T 3)                                  1.25e-5        1.25e-5       6.4e-7         3.8e-6
        douts middle missing / first only                          1.25e-5 / 1.85e-5 (tape alike)  7.6e-7 / 7.1e-7   4.3e-6 / 4.8e-6
        17x19, b 3, flow_init up to 12 px                          3.3e-6         3.3e-6        9.6e-7         1.4e-6
        T = 33: fused vs tape 1.8e-6; fused - fp64 1.12e-2 (d fmap1), the materialised route's own error the same
  * kernel level beyond one launch (17x19, b 2; 33 and 69 lookups with a gradient: two and three launches): alt - fp64
    1.0e-6 - 2.0e-6 of max, materialised 4.9e-7 - 8.7e-7, both precisions;
  * memory: peak 0.35 -> 1.36 GB from 32x48 to 64x96 (3.89x); the recorded 1088 x 1920 pass: 2.3e-4 px from inference.
"""
import os
import shutil
import sys

import pytest
import torch

from oracle import ffraft_ref as orc

from test_alt_corr import SHAPES, _coord_cases, _dev_nhwc, _model, _pooled, alt_lookup_ref
from test_update_loop import _cfg, _inputs, _keys, _oracle, _run, _vs, _vs_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CHANS = [0, 37, 101, 128, 200, 255]        # the channels the fp64 references compute


def _ref_grads(f1, f2, coords_list, douts, chans=CHANS):
    """fp64 d fmap1, d fmap2 (NCHW, channels `chans`) of sum_t <dout_t, lookup_t> through alt_lookup_ref."""
    a = f1[:, chans].double().requires_grad_(True)
    b = f2[:, chans].double().requires_grad_(True)
    lv = _pooled(b)
    loss = 0
    for c, d in zip(coords_list, douts):
        if d is not None:
            loss = loss + (alt_lookup_ref(a, lv, c.double()) * d.double()).sum()
    (loss * (len(chans) ** 0.5 / 16.0)).backward()          # alt_lookup_ref divides by sqrt(len(chans)): the block's 1 / 16
    return a.grad, b.grad


def _hip_grads(block_cls, f1, f2, coords_list, douts, **kw):
    """d fmap1, d fmap2 (NCHW CPU) of a recorded block: every lookup called, the gradient of the present ones."""
    a, b = _dev_nhwc(f1).requires_grad_(True), _dev_nhwc(f2).requires_grad_(True)
    blk = block_cls(a, b, **kw)
    outs = [blk(_dev_nhwc(c)) for c in coords_list]
    used = [(o, _dev_nhwc(d)) for o, d in zip(outs, douts) if d is not None]
    torch.autograd.backward([o for o, _ in used], [d for _, d in used])
    torch.cuda.synchronize()
    return a.grad.permute(0, 3, 1, 2).cpu(), b.grad.permute(0, 3, 1, 2).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", SHAPES)
def test_alt_backward_against_fp64_and_the_materialised_route(h, w, b, precision):
    """Every coordinate case of test_alt_corr, T = 1 and T = 3 with the middle dout absent."""
    from focusflow_official_amd import ops
    from focusflow_official_amd.corr_block import AlternateCorrBlock, CorrBlock
    g = torch.Generator().manual_seed(7000 + 100 * h + w + b)
    f1, f2 = torch.randn(b, 256, h, w, generator=g), torch.randn(b, 256, h, w, generator=g)
    prev = ops.conv_precision()
    ops.set_conv_precision(precision)
    spread = []
    try:
        for name, c in _coord_cases(b, h, w, g).items():
            for T in (1, 3):
                cl = [c + (torch.rand(c.shape, generator=g) - 0.5) * 2 * t for t in range(T)]     # (lookup 0: the case itself)
                douts = [torch.randn(b, 324, h, w, generator=g) for _ in range(T)]
                if T == 3:
                    douts[1] = None
                r1, r2 = _ref_grads(f1, f2, cl, douts)
                alt = _hip_grads(AlternateCorrBlock, f1, f2, cl, douts)
                mat = _hip_grads(CorrBlock, f1, f2, cl, douts, pyramid_dtype="fp32")
                for what, ref, ga, gm in (("d fmap1", r1, alt[0], mat[0]), ("d fmap2", r2, alt[1], mat[1])):
                    ga, gm = ga[:, CHANS].double(), gm[:, CHANS].double()
                    m = ref.abs().max().item()
                    e_a, e_m = (ga - ref).abs().max().item(), (gm - ref).abs().max().item()
                    spread.append((e_a / max(e_m, 1e-30), e_a / max(m, 1e-30)))
                    assert e_a <= 2 * e_m + 1e-6 * m, f"{name} T={T} {what}: alt {e_a:.3e} vs materialised {e_m:.3e} (max {m:.3e})"
    finally:
        ops.set_conv_precision(prev)
    print(f"\n{precision} {h}x{w} b{b}: alt / materialised error up to {max(s[0] for s in spread):.2f}, "
          f"alt error up to {max(s[1] for s in spread):.1e} of max")


@pytest.mark.gpu
def test_alt_backward_on_a_1088x1920_plane():
    """136 x 240 at 1/8, B = 1, two lookups of a smooth flow plus noise: d fmap1 and d fmap2 of six channels against fp64."""
    from focusflow_official_amd import ops
    from focusflow_official_amd.corr_block import AlternateCorrBlock
    g = torch.Generator().manual_seed(17)
    b, h, w = 1, 136, 240
    f1, f2 = torch.randn(b, 256, h, w, generator=g), torch.randn(b, 256, h, w, generator=g)
    base = orc.coords_grid(b, h, w)
    cl = [base + 6 * torch.sin(base / 17) + torch.rand(base.shape, generator=g) * s for s in (0.5, 2.0)]
    douts = [torch.randn(b, 324, h, w, generator=g) for _ in cl]
    r1, r2 = _ref_grads(f1, f2, cl, douts)
    prev = ops.conv_precision()
    ops.set_conv_precision("fp32")
    try:
        a1, a2 = _hip_grads(AlternateCorrBlock, f1, f2, cl, douts)
    finally:
        ops.set_conv_precision(prev)
    for what, ref, got in (("d fmap1", r1, a1), ("d fmap2", r2, a2)):
        err, m = (got[:, CHANS].double() - ref).abs().max().item(), ref.abs().max().item()
        print(f"1088x1920 {what}: {err / m:.2e} of max")
        assert err <= 1e-5 * m, (what, err, m)


@pytest.fixture(scope="module")
def raft_alt(det_sd):
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg(), alternate_corr=True)
    m.load_state_dict(det_sd, strict=True)
    return m.to(DEV).train().flow_net


def _forced(monkeypatch):
    """Force the on-the-fly route of recorded passes; returns the list of blocks RAFT builds."""
    from focusflow_official_amd import corr_block, raft_net
    made = []

    class Spy(corr_block.AlternateCorrBlock):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(raft_net, "AlternateCorrBlock", Spy)
    monkeypatch.setattr(corr_block, "_MAX_PYRAMID_BYTES", 1)
    return made


UPDATE_CASES = {
    "default": {},
    "douts_middle_missing": {"present": [True, False, True]},
    "douts_first_only": {"present": [True, False, False]},
    "odd_planes_b3_flow_init": {"b": 3, "h": 17, "w": 19, "seed": 7, "flow_init": 12.0},
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_update_loop_on_the_fly_against_fp64_tape_and_materialised(raft_alt, det_sd, case, monkeypatch):
    """RAFT._update_loop on the forced on-the-fly route: the fused node and the per-operation tape against fp64, against
    each other, and the fused node against the materialised route on the same inputs."""
    import warnings
    from focusflow_official_amd import train_loop
    spec = UPDATE_CASES[case]
    ins = _inputs(**spec)
    key = ("alt",) + tuple(sorted((k, str(v)) for k, v in spec.items()))
    r64, r32 = _oracle(det_sd, key, ins, torch.float64), _oracle(det_sd, key, ins, torch.float32)
    keys = _keys(raft_alt, ins["T"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mat, route = _run(raft_alt, ins)                          # (the batch's pyramid fits: the materialised route)
    assert route == "UpdateLoopFnBackward"
    with monkeypatch.context() as mp:
        made = _forced(mp)
        fused, route = _run(raft_alt, ins)
        assert route == "UpdateLoopFnBackward" and len(made) == 1 and made[0]._token is None, (route, len(made))
        mp.setattr(train_loop, "ENABLED", False)
        tape, route_t = _run(raft_alt, ins)
        assert route_t != route and len(made) == 2 and made[1]._token is not None
    _vs_fp64(fused, r32, r64, keys, f"{case}: fused node, on-the-fly")
    _vs_fp64(tape, r32, r64, keys, f"{case}: tape, on-the-fly")
    _vs(fused, tape, keys, f"{case}: fused node vs tape, on-the-fly")
    _vs(fused, mat, keys, f"{case}: on-the-fly vs materialised", tol=1e-4)


@pytest.mark.gpu
def test_update_loop_on_the_fly_t33(raft_alt, det_sd, monkeypatch):
    """T = 33 (ff_corr_alt_lookup_bwd: two launches, the second adding into d fmap1 and the level planes): the fused node on
    the forced route against the tape on that route, and against fp64 (ffraft_ref.update_loop) - within test_update_loop's
    bound or within 2x the materialised route's own fp64 error on the same inputs, whichever is larger.  (Over 33 iterations
    the loop is no longer well conditioned: correlation values that differ by rounding flip ReLUs of the motion encoder, and
    both routes land 1.12e-2 of max from fp64 on d fmap1 - measured - and 3.1e-3 from each other.  The launch split itself is
    checked tightly at the kernel level: test_alt_backward_beyond_one_launch_against_fp64.)"""
    import warnings
    from focusflow_official_amd import train_loop
    T = 33
    ins = _inputs(T=T, seed=3)
    keys = _keys(raft_alt, T)
    r64, r32 = _oracle(det_sd, ("alt", "T33"), ins, torch.float64), _oracle(det_sd, ("alt", "T33"), ins, torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mat, route = _run(raft_alt, ins)
    assert route == "UpdateLoopFnBackward"
    made = _forced(monkeypatch)
    fused, route = _run(raft_alt, ins)
    assert route == "UpdateLoopFnBackward" and made
    monkeypatch.setattr(train_loop, "ENABLED", False)
    tape, _ = _run(raft_alt, ins)
    _vs(fused, tape, keys, f"T={T}: fused node vs tape, on-the-fly")
    mat_err = {k: float((mat[k].double() - r64[k].double()).abs().max()) for k in keys}
    print(f"T={T}: materialised max |hip - fp64| / max|fp64| = "
          f"{max(e / max(float(r64[k].abs().max()), 1e-30) for k, e in mat_err.items()):.2e}")
    _vs_fp64(fused, r32, r64, keys, f"T={T}: fused node, on-the-fly", loose={k: 2 * e for k, e in mat_err.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_alt_backward_beyond_one_launch_against_fp64(precision):
    """Kernel level, beyond the 32 lookups of one ff_corr_alt_lookup_bwd launch: every 7th lookup without a gradient (the host
    passes only the others), 38 lookups -> 33 with a gradient (two launches, the last lookup alone in the second) and 80 -> 69
    (three launches).  d fmap1 and d fmap2 against fp64 and against the materialised route."""
    from focusflow_official_amd import ops
    from focusflow_official_amd.corr_block import AlternateCorrBlock, CorrBlock
    g = torch.Generator().manual_seed(33)
    b, h, w = 2, 17, 19
    f1, f2 = torch.randn(b, 256, h, w, generator=g), torch.randn(b, 256, h, w, generator=g)
    base = orc.coords_grid(b, h, w)
    prev = ops.conv_precision()
    ops.set_conv_precision(precision)
    try:
        for T in (38, 80):
            cl = [base + (torch.rand(base.shape, generator=g) - 0.5) * 12 for _ in range(T)]
            douts = [torch.randn(b, 324, h, w, generator=g) if t % 7 != 3 else None for t in range(T)]
            r1, r2 = _ref_grads(f1, f2, cl, douts)
            alt = _hip_grads(AlternateCorrBlock, f1, f2, cl, douts)
            mat = _hip_grads(CorrBlock, f1, f2, cl, douts, pyramid_dtype="fp32")
            for what, ref, ga, gm in (("d fmap1", r1, alt[0], mat[0]), ("d fmap2", r2, alt[1], mat[1])):
                ga, gm = ga[:, CHANS].double(), gm[:, CHANS].double()
                m = ref.abs().max().item()
                e_a, e_m = (ga - ref).abs().max().item(), (gm - ref).abs().max().item()
                print(f"{precision} T={T} {what}: alt {e_a / m:.1e}, materialised {e_m / m:.1e} of max")
                assert e_a <= 2 * e_m + 1e-6 * m, f"T={T} {what}: alt {e_a:.3e} vs materialised {e_m:.3e} (max {m:.3e})"
    finally:
        ops.set_conv_precision(prev)


@pytest.mark.gpu
def test_update_loop_on_the_fly_memory_is_linear(raft_alt, monkeypatch):
    """Peak memory of a recorded update loop (forward + backward) on the forced route at 32 x 48 and 64 x 96 (4x the area):
    it grows at most 4.5x (the pyramid would grow 16x)."""
    made = _forced(monkeypatch)
    peaks = []
    for h, w in ((32, 48), (64, 96)):
        ins = _inputs(b=2, h=h, w=w, T=3, seed=9)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        m0 = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _run(raft_alt, ins)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - m0)
    assert len(made) == 2
    print(f"peak bytes {peaks}, ratio {peaks[1] / peaks[0]:.2f}")
    assert peaks[1] <= 4.5 * peaks[0], peaks


@pytest.mark.gpu
def test_recorded_1080p_pass_with_alternate_corr(det_sd):
    """FF_RAFT_FUSION(alternate_corr=True), one 1088 x 1920 pair, FF_CONV_PRECISION=fp32, 3 iterations, trained encoders:
    the materialised pyramid (5.7 GB, beyond the lookup's resource) is not an option, the on-the-fly block and its backward
    run the pass.  Every parameter gradient finite; the recorded flows within 1e-3 px of inference's."""
    import warnings
    from focusflow_official_amd import ops
    inp = [t.to(DEV) for t in orc.shifted_pair(1, 1088, 1920, seed=13)]
    m = _model(det_sd, alternate_corr=True)
    prev = ops.conv_precision()
    ops.set_conv_precision("fp32")
    try:
        with torch.no_grad():
            ref = [p.clone() for p in m(*inp, raft_iters=3)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            preds = m(*inp, raft_iters=3)
        g = torch.Generator().manual_seed(3)
        w = [torch.randn(p.shape, generator=g).to(DEV) for p in preds]
        sum((p * x).sum() for p, x in zip(preds, w)).backward()
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision(prev)
    grads = {k: p.grad for k, p in m.named_parameters() if p.requires_grad}
    assert grads and all(v is not None for v in grads.values()), [k for k, v in grads.items() if v is None][:5]
    bad = [k for k, v in grads.items() if not torch.isfinite(v).all()]
    assert not bad, bad[:5]
    fnet = [v.abs().max().item() for k, v in grads.items() if ".fnet." in k]
    assert fnet and max(fnet) > 0          # (the feature encoder's gradient comes through the correlation alone)
    err = max((p.detach() - r).abs().max().item() for p, r in zip(preds, ref))
    print(f"1080p recorded vs inference: {err:.2e} px")
    assert err <= 1e-3, err


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_alt_corr_backward_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "corr_alt_bwd.hip"))
    assert len(kernels) >= 2, kernels
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"corr_alt_bwd.hip: kernels with scratch (bytes per lane): {spilled}"
