"""Operator tests of the kernels at the two ends of a pass, each against a plain fp64 reference on the CPU:

  B  csrc/loss.hip       FF-RAFT's fused sequence loss (prepare / accumulate / epe_metric)  vs oracle.ffraft_ref.sequence_loss
  C  csrc/pwc_loss.hip   FF-PWC's multi-scale losses (mask / scale / scale_sparse / epe_mean[_sparse])
                                                                                      vs oracle.pwc_ref.pwc_multiscale_loss
  D  csrc/update_ops.hip ff_resize_bilinear, ff_resize_to_nhwc4 vs F.interpolate in fp64; ff_nchw_to_nhwc4, ff_nhwc_to_nchw
                         bit for bit vs permute
  E  csrc/mask_modes.hip ff_mask_prepare vs oracle.ffraft_ref.init_mask plus the input scaling

at odd sizes, at level sizes that do not divide the target (overlapping adaptive windows, bilinear source coordinates that
are not k + 0.5) and once per kernel past the grid cap, where the grid-stride loops take a second trip (2048 blocks of 256
in the two loss files, 4096 in the other two).  Inputs are drawn in fp32 and the same fp32 values go to both sides.

Where a result is thresholded it is compared exactly.  That covers the resized key-point mask: the source coordinate
(d + 0.5) * scale - 0.5 of the bilinear resize is one fma in ATen; rounding the product first moves it across an integer at
a few size pairs (MASK_PARITY_CASES), and a key point in the single source row or column below the crossing then turns an
output pixel on or off.  test_mask_parity_cases_discriminate shows on the CPU that the expected maps of those cases differ
from the maps of the separately rounded coordinate, so the GPU tests on them fail if the kernels' coordinate arithmetic
changes.

Tolerances are those of tests/test_hip_losses.py for the losses and of test_hip_parity.py::test_mask_modes for
ff_mask_prepare; RESIZE_TOL is measured (see there).

Largest error seen on the MI355X against fp64: loss and 'epe' of both loss families 1.3e-07 relative (2e-5 allowed); the
two resize kernels 2.81e-06 of max|src| (1.12e-05 allowed) - that is ATen's own fp32 distance from fp64, the source
coordinates being the same fp32 numbers; neighborG 1.4e-07 on the [-1, 1] output (2e-5 allowed).

Finding: update_ops.hip is compiled with contraction off, so ff_resize_bilinear and ff_resize_to_nhwc4 used to round the
source coordinate twice; test_resize_bilinear_mask_parity and test_resize_to_nhwc4_mask_parity fail on that form.  All
three resize kernels now spell the coordinate as one __fmaf_rn.
"""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ffraft_ref as orc
from oracle import pwc_ref
from test_oracle_golden import pwc_loss_tag

gpu = pytest.mark.gpu
DEV = "cuda:0"
MAX_FLOW = 400.0
BELOW_MAX_FLOW = float(np.nextafter(np.float32(MAX_FLOW), np.float32(0)))
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))


@pytest.fixture(scope="module")
def hip():
    from focusflow_official_amd import _hip, losses, model, ops, pwc_losses
    return Namespace(call=_hip.call, Error=_hip.FocusFlowHipError, ops=ops, p=ops._p, stream=ops._stream, losses=losses,
                     pwc_losses=pwc_losses, model=model)


# =====================================================================================================================
# B. FF-RAFT sequence loss
SEQ_KINDS = {"EPELoss": {}, "CPCL_k1": dict(kernel_size=1, sigma=0.01), "CPCL_k5": dict(kernel_size=5, sigma=1.7),
             "CPCL_k7": dict(kernel_size=7, sigma=2.0), "MixLoss_k1": dict(kernel_size=1, sigma=0.01, lamda=1.0),
             "MixLoss_k5": dict(kernel_size=5, sigma=1.7, lamda=0.8), "MixLoss_k7": dict(kernel_size=7, sigma=2.0, lamda=0.8)}
# the marked pixels of sample 0 (y, x); each carries a key point so that CPCL, whose weight is the mask term alone, sees it
PIX_VALID_HALF, PIX_VALID_BELOW_HALF = (3, 3), (3, 9)
PIX_AT_MAX_FLOW, PIX_BELOW_MAX_FLOW = (6, 2), (6, 8)
EQUAL_BLOCK = (slice(None), slice(None), slice(20, 24), slice(10, 14))      # pred == gt here, in every prediction


@functools.lru_cache(maxsize=None)
def seq_case(b, h, w, n, seed=0):
    """(preds, gt, valid, mask) on the CPU in fp32, with every edge of the loss in it (test_sequence_case_holds_its_edges)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(b, 2, h, w, generator=g) * 4
    valid = (torch.rand(b, h, w, generator=g) > 0.1).float()
    values = torch.tensor([255.0, 1.0, 1e-3])[torch.randint(0, 3, (b, 1, h, w), generator=g)]      # the threshold is > 0
    mask = (torch.rand(b, 1, h, w, generator=g) < 0.03).float() * values
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):       # the zero padding of the Gaussian box
        mask[:, 0, y, x] = 255.0
    mask[0, 0, h - 1, 5:12] = 1.0
    mask[0, 0, 4:9, 0] = 1e-3
    for y, x in (PIX_VALID_HALF, PIX_VALID_BELOW_HALF, PIX_AT_MAX_FLOW, PIX_BELOW_MAX_FLOW):
        mask[0, 0, y, x], valid[0, y, x] = 255.0, 1.0
    valid[0][PIX_VALID_HALF] = 0.5                     # kept: the test is >=
    valid[0][PIX_VALID_BELOW_HALF] = BELOW_HALF        # dropped
    gt[0, :, PIX_AT_MAX_FLOW[0], PIX_AT_MAX_FLOW[1]] = torch.tensor([MAX_FLOW, 0.0])              # dropped: the test is <
    gt[0, :, PIX_BELOW_MAX_FLOW[0], PIX_BELOW_MAX_FLOW[1]] = torch.tensor([BELOW_MAX_FLOW, 0.0])  # kept
    if b > 1:
        valid[1] = 0.0                                 # a whole sample invalid
    preds = [gt + torch.randn(b, 2, h, w, generator=g) * (n - i) for i in range(n)]
    valid[0, 20:24, 10:14] = 1.0
    mask[0, 0, 21, 11] = 255.0
    for p in preds:
        p[EQUAL_BLOCK] = gt[EQUAL_BLOCK]
    return preds, gt, valid, mask


def test_sequence_case_holds_its_edges():
    """No GPU: the inputs of the sequence-loss tests contain what the tests are about."""
    for b, h, w in ((1, 37, 53), (3, 45, 70)):
        preds, gt, valid, mask = seq_case(b, h, w, 3)
        assert all(float(mask[i, 0, y, x]) > 0 for i in range(b) for y in (0, h - 1) for x in (0, w - 1))
        assert bool((mask[0, 0, h - 1, 5:12] > 0).all()) and bool((mask[0, 0, 4:9, 0] > 0).all())
        assert {1.0, float(np.float32(1e-3)), 255.0} <= set(mask.unique().tolist())
        assert float(valid[0][PIX_VALID_HALF]) == 0.5 and 0.49 < float(valid[0][PIX_VALID_BELOW_HALF]) < 0.5
        mag = gt.double().pow(2).sum(1).sqrt()
        assert float(mag[0][PIX_AT_MAX_FLOW]) == MAX_FLOW and MAX_FLOW - 1e-4 < float(mag[0][PIX_BELOW_MAX_FLOW]) < MAX_FLOW
        assert b == 1 or not bool(valid[1].any())
        assert all(torch.equal(p[EQUAL_BLOCK], gt[EQUAL_BLOCK]) for p in preds) and bool((valid[:1, 20:24, 10:14] == 1).all())
        ok = (valid >= 0.5) & (mag < MAX_FLOW)
        assert bool(ok[0][PIX_VALID_HALF]) and not bool(ok[0][PIX_VALID_BELOW_HALF])
        assert bool(ok[0][PIX_BELOW_MAX_FLOW]) and not bool(ok[0][PIX_AT_MAX_FLOW])


def seq_reference(kind, preds, gt, valid, mask, upstream=1.0, gamma=0.8, grad=None):
    """fp64 loss, 'epe' and d(upstream * loss)/d(pred_i) (None where grad[i] is False)."""
    ps = [p.double().requires_grad_(grad is None or grad[i]) for i, p in enumerate(preds)]
    loss, metrics = orc.sequence_loss(kind.split("_")[0], ps, gt.double(), valid, mask, gamma=gamma, max_flow=MAX_FLOW, **SEQ_KINDS[kind])
    if torch.isfinite(loss):
        (loss * upstream).backward()
    return float(loss.detach()), metrics["epe"], [p.grad for p in ps]


def seq_criterion(hip, kind, gamma=0.8):
    return hip.losses.build_losses(kind.split("_")[0], gamma=gamma, max_flow=MAX_FLOW, **SEQ_KINDS[kind])


def seq_compare(kind, got_loss, got_metrics, got_grads, want):
    want_loss, want_epe, want_grads = want
    print(f"[{kind}] loss {got_loss:.9g} vs {want_loss:.9g} (rel {abs(got_loss - want_loss) / max(1.0, abs(want_loss)):.2e}), "
          f"epe {got_metrics['epe']:.7g} vs {want_epe:.7g}")
    assert abs(got_loss - want_loss) < 2e-5 * max(1.0, abs(want_loss)), (got_loss, want_loss)
    assert abs(got_metrics["epe"] - want_epe) < 1e-4, (got_metrics["epe"], want_epe)
    assert abs(got_metrics["loss"] - got_loss) < 1e-6
    for i, (a, r) in enumerate(zip(got_grads, want_grads)):
        assert (a is None) == (r is None), f"prediction {i}"
        if r is not None:
            np.testing.assert_allclose(a.cpu().double().numpy(), r.numpy(), rtol=2e-5, atol=1e-9, err_msg=f"{kind}: gradient of prediction {i}")


@gpu
@pytest.mark.parametrize("b,h,w", [(1, 37, 53), (3, 45, 70)])
@pytest.mark.parametrize("kind", list(SEQ_KINDS))
def test_sequence_loss(hip, kind, b, h, w):
    """Three predictions, the first a non-contiguous view, an upstream gradient of 2; then the marked pixels one by one."""
    preds, gt, valid, mask = seq_case(b, h, w, 3)
    want = seq_reference(kind, preds, gt, valid, mask, upstream=2.0)
    base = preds[0].permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)      # NHWC storage
    pd = [base.permute(0, 3, 1, 2)] + [p.to(DEV).requires_grad_(True) for p in preds[1:]]
    assert not pd[0].is_contiguous()
    loss, metrics = seq_criterion(hip, kind)(pd, gt.to(DEV), valid.to(DEV), mask.to(DEV))
    (loss * 2.0).backward()
    grads = [base.grad.permute(0, 3, 1, 2)] + [p.grad for p in pd[1:]]
    seq_compare(kind, loss.item(), metrics, grads, want)
    for g in grads:
        g = g.cpu()
        assert bool((g[0, :, PIX_VALID_HALF[0], PIX_VALID_HALF[1]] != 0).all()), "valid == 0.5 is kept (>=)"
        assert bool((g[0, :, PIX_VALID_BELOW_HALF[0], PIX_VALID_BELOW_HALF[1]] == 0).all()), "valid just below 0.5 is dropped"
        assert bool((g[0, :, PIX_AT_MAX_FLOW[0], PIX_AT_MAX_FLOW[1]] == 0).all()), "|gt| == max_flow is dropped (<)"
        assert bool((g[0, :, PIX_BELOW_MAX_FLOW[0], PIX_BELOW_MAX_FLOW[1]] != 0).all()), "|gt| one ulp below max_flow is kept"
        assert bool((g[EQUAL_BLOCK] == 0).all()), "pred == gt: the gradient is exactly 0"
        assert b == 1 or bool((g[1] == 0).all()), "a sample without a valid pixel has no gradient"


@gpu
@pytest.mark.parametrize("kind", ["EPELoss", "MixLoss_k5"])
def test_sequence_loss_past_the_grid_cap(hip, kind):
    """3 x 384 x 512 = 589,824 pixels > 2048 * 256: prepare, accumulate and epe_metric all take a second trip."""
    preds, gt, valid, mask = seq_case(3, 384, 512, 2)
    want = seq_reference(kind, preds, gt, valid, mask)
    pd = [p.to(DEV).requires_grad_(True) for p in preds]
    loss, metrics = seq_criterion(hip, kind)(pd, gt.to(DEV), valid.to(DEV), mask.to(DEV))
    loss.backward()
    seq_compare(kind, loss.item(), metrics, [p.grad for p in pd], want)


@gpu
@pytest.mark.parametrize("kind", ["EPELoss", "CPCL_k5", "MixLoss_k5"])
def test_sequence_loss_prediction_without_grad(hip, kind):
    """The middle prediction does not require grad: it gets none, the others get theirs."""
    preds, gt, valid, mask = seq_case(1, 37, 53, 3)
    need = [True, False, True]
    want = seq_reference(kind, preds, gt, valid, mask, grad=need)
    pd = [p.to(DEV).requires_grad_(r) for p, r in zip(preds, need)]
    loss, metrics = seq_criterion(hip, kind)(pd, gt.to(DEV), valid.to(DEV), mask.to(DEV))
    loss.backward()
    assert pd[1].grad is None
    seq_compare(kind, loss.item(), metrics, [p.grad for p in pd], want)


@gpu
@pytest.mark.parametrize("n", [1, 12])
@pytest.mark.parametrize("kind", ["EPELoss", "CPCL_k5", "MixLoss_k5"])
def test_sequence_loss_one_and_twelve_predictions(hip, kind, n):
    """gamma = 0.8: the weights run from 0.8^11 = 0.086 to 1."""
    preds, gt, valid, mask = seq_case(1, 37, 53, n)
    want = seq_reference(kind, preds, gt, valid, mask)
    pd = [p.to(DEV).requires_grad_(True) for p in preds]
    loss, metrics = seq_criterion(hip, kind)(pd, gt.to(DEV), valid.to(DEV), mask.to(DEV))
    loss.backward()
    seq_compare(kind, loss.item(), metrics, [p.grad for p in pd], want)


@gpu
@pytest.mark.parametrize("kind", ["EPELoss", "CPCL_k5", "MixLoss_k5"])
def test_sequence_loss_degenerate_inputs(hip, kind):
    """Pinned to the reference: an empty mask makes CPCL and MixLoss 0/0; no valid pixel gives loss 0 and 'epe' NaN."""
    preds, gt, valid, mask = seq_case(3, 45, 70, 3)
    crit = seq_criterion(hip, kind)
    empty = torch.zeros_like(mask)
    ref_loss, ref_epe, _ = seq_reference(kind, preds, gt, valid, empty)
    loss, metrics = crit([p.to(DEV).requires_grad_(True) for p in preds], gt.to(DEV), valid.to(DEV), empty.to(DEV))
    if kind == "EPELoss":
        assert np.isfinite(ref_loss) and abs(loss.item() - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    else:
        assert not np.isfinite(ref_loss) and not np.isfinite(loss.item())
    assert abs(metrics["epe"] - ref_epe) < 1e-4
    nowhere = torch.zeros_like(valid)
    ref_loss, ref_epe, _ = seq_reference(kind, preds, gt, nowhere, mask)
    pd = [p.to(DEV).requires_grad_(True) for p in preds]
    loss, metrics = crit(pd, gt.to(DEV), nowhere.to(DEV), mask.to(DEV))
    loss.backward()
    assert ref_loss == 0.0 and np.isnan(ref_epe)
    assert loss.item() == 0.0 and np.isnan(metrics["epe"])
    assert all(bool((p.grad == 0).all()) for p in pd)


# =====================================================================================================================
# C. FF-PWC multi-scale losses
PWC_WEIGHTS = pwc_ref.PWC_LOSS_WEIGHTS
PWC_SHAPES = {            # name: (B, (H, W), level sizes, key-point density, seed)
    "45x70": (3, (45, 70), ((12, 18), (6, 9), (3, 5), (2, 3), (1, 2)), 0.03, 5),
    "37x53": (1, (37, 53), ((10, 14), (5, 7), (37, 53)), 0.03, 5),      # the last level is the target's size: one-pixel windows, identity resize
    "45x70 sparse mask": (3, (45, 70), ((12, 18), (6, 9), (3, 5), (2, 3), (1, 2)), 0.002, 0),     # empty maps from (6, 9) down
}
PWC_TAGS = ["EPELoss_pretrain_k1", "EPELoss_finetune_k1", "CPCL_pretrain_k1", "CPCL_pretrain_k3", "CPCL_pretrain_k5", "CPCL_finetune_k1",
            "CPCL_finetune_k3", "CPCL_finetune_k5", "MixLoss_pretrain_k1", "MixLoss_pretrain_k3", "MixLoss_pretrain_k5", "MixLoss_finetune_k1",
            "MixLoss_finetune_k3", "MixLoss_finetune_k5", "sparse_EPELoss_pretrain_k1", "sparse_EPELoss_finetune_k1",
            "sparse_MixLoss_pretrain_k1", "sparse_MixLoss_pretrain_k5", "sparse_MixLoss_finetune_k3", "sparse_MixLoss_finetune_k5"]
# level-0 pixels (y, x) of the 45x70 shapes whose window of the sparse target is (0, 0) throughout / holds maxima that cancel
PIX_ZERO_WINDOW, PIX_CANCEL_WINDOW = (2, 3), (5, 7)


def adaptive_window(i, n_in, n_out):
    """[floor(i * n_in / n_out), ceil((i + 1) * n_in / n_out))."""
    return (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)


@functools.lru_cache(maxsize=None)
def pwc_case(name):
    b, (hh, ww), sizes, density, seed = PWC_SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    target = torch.randn(b, 2, hh, ww, generator=g) * 3
    mask = (torch.rand(b, 1, hh, ww, generator=g) < density).float() * 255
    preds = [torch.randn(b, 2, h, w, generator=g) for h, w in sizes]
    sparse = torch.where(torch.rand(b, 1, hh, ww, generator=g) < 0.35, torch.zeros_like(target), target)
    if (hh, ww) == (45, 70):
        h, w = sizes[0]
        (y0, y1), (x0, x1) = adaptive_window(PIX_ZERO_WINDOW[0], hh, h), adaptive_window(PIX_ZERO_WINDOW[1], ww, w)
        sparse[:, :, y0:y1, x0:x1] = 0.0
        (y0, y1), (x0, x1) = adaptive_window(PIX_CANCEL_WINDOW[0], hh, h), adaptive_window(PIX_CANCEL_WINDOW[1], ww, w)
        sparse[:, :, y0:y1, x0:x1] = 0.0
        sparse[:, 0, y0 + 1, x0 + 1], sparse[:, 0, y1 - 2, x1 - 2] = 2.5, -2.5       # positive and negative maximum cancel
        sparse[:, 1, y0 + 2, x0 + 2], sparse[:, 1, y0, x1 - 1] = 1.25, -1.25
        if density > 0.01:           # a key point inside each, so that the mask term would count there
            mask[:, 0, 9, 13] = 255.0
            mask[:, 0, 20, 29] = 255.0
    maps = [F.interpolate(mask, s, mode="bilinear", align_corners=False) > 0 for s in sizes]      # ATen in fp32, as the reference runs it
    return Namespace(b=b, target=target, sparse_target=sparse, mask=mask, preds=preds, maps=maps, sizes=sizes, weights=PWC_WEIGHTS[:len(sizes)])


def test_pwc_cases_hold_their_edges():
    """No GPU: overlapping windows, the two invalid windows of the sparse target, the levels with an empty mask map."""
    c = pwc_case("45x70")
    h, w = c.sizes[0]
    assert adaptive_window(1, 45, h)[0] < adaptive_window(0, 45, h)[1]          # windows overlap: 45 / 12 is no integer
    pooled = pwc_ref.pwc_sparse_max_pool(c.sparse_target, (h, w))
    for y, x in (PIX_ZERO_WINDOW, PIX_CANCEL_WINDOW):
        assert bool((pooled[:, :, y, x] == 0).all()) and bool(c.maps[0][:, 0, y, x].all())
    (y0, y1), (x0, x1) = adaptive_window(PIX_CANCEL_WINDOW[0], 45, h), adaptive_window(PIX_CANCEL_WINDOW[1], 70, w)
    assert float(c.sparse_target[:, :, y0:y1, x0:x1].abs().max()) == 2.5
    e = pwc_case("45x70 sparse mask")
    assert bool(e.maps[0].any()) and not any(bool(m.any()) for m in e.maps[1:])


def pwc_cfg(tag, weights):
    sparse, kw = pwc_loss_tag(tag)
    return sparse, kw, Namespace(TRAIN=Namespace(LOSS_TYPE=kw["kind"], LOSS_MODE=kw["mode"], LOSS_WEIGHTS=list(weights), LOSS_Q=kw["q"],
                                                 LOSS_EPSILON=kw["eps"], LOSS_KERNEL_SIZE=kw["kernel_size"], LOSS_SIGMA=kw["sigma"],
                                                 LOSS_LAMDA=kw["lamda"]))


def pwc_run(hip, c, tag, backward=True):
    """-> (loss, epe, gradients) of the HIP path and of the fp64 oracle fed with the fp32 boolean mask maps."""
    sparse, kw, cfg = pwc_cfg(tag, c.weights)
    target = c.sparse_target if sparse else c.target
    ps = [p.double().requires_grad_(True) for p in c.preds]
    ref_loss, ref = pwc_ref.pwc_multiscale_loss(preds=ps, target=target.double(), sparse=sparse, weights=c.weights, mask_maps=c.maps, **kw)
    if backward and torch.isfinite(ref_loss):
        ref_loss.backward()
    crit = hip.pwc_losses.build_losses(cfg)
    pd = [p.to(DEV).requires_grad_(True) for p in c.preds]
    args = (pd, target.to(DEV)) + (() if kw["kind"] == "EPELoss" else (c.mask.to(DEV),)) + (sparse,)
    loss, res = crit(*args)
    if backward and torch.isfinite(loss):
        loss.backward()
    return (loss.item(), float(res["epe"]), [p.grad for p in pd]), (float(ref_loss), float(ref["epe"]), [p.grad for p in ps])


def pwc_compare(tag, got, want):
    (loss, epe, grads), (want_loss, want_epe, want_grads) = got, want
    print(f"[{tag}] loss {loss:.9g} vs {want_loss:.9g} (rel {abs(loss / want_loss - 1):.2e}), epe {epe:.7g} vs {want_epe:.7g} (rel {abs(epe / want_epe - 1):.2e})")
    assert abs(loss - want_loss) < 2e-5 * abs(want_loss), (loss, want_loss)
    assert abs(epe - want_epe) < 2e-5 * abs(want_epe), (epe, want_epe)
    for i, (a, r) in enumerate(zip(grads, want_grads)):
        r = r.numpy()
        np.testing.assert_allclose(a.cpu().double().numpy(), r, rtol=2e-4, atol=2e-6 * float(np.abs(r).max()), err_msg=f"{tag}: level {i}")


@gpu
@pytest.mark.parametrize("shape", ["45x70", "37x53"])
@pytest.mark.parametrize("tag", PWC_TAGS)
def test_pwc_losses(hip, tag, shape):
    """Loss, 'epe' and every level's gradient at level sizes that do not divide the target."""
    got, want = pwc_run(hip, pwc_case(shape), tag)
    pwc_compare(tag, got, want)


@gpu
@pytest.mark.parametrize("tag", ["sparse_EPELoss_pretrain_k1", "sparse_MixLoss_pretrain_k5"])
def test_pwc_sparse_invalid_windows(hip, tag):
    """A window that is (0, 0) throughout and one whose positive and negative maxima cancel pool to (0, 0): invalid.  Such a
    pixel counts for nothing in EPELoss and for the plain term only in MixLoss, although a key point lies in it."""
    c = pwc_case("45x70")
    got, want = pwc_run(hip, c, tag)
    pwc_compare(tag, got, want)
    g0, out = got[2][0].cpu(), c.preds[0]
    for y, x in (PIX_ZERO_WINDOW, PIX_CANCEL_WINDOW):
        if "EPELoss" in tag:
            assert bool((g0[:, :, y, x] == 0).all())
        else:                 # d/d(out) of weight * |0 - out|_2, and nothing from the mask term
            plain = c.weights[0] * out[:, :, y, x] / out[:, :, y, x].norm(dim=1, keepdim=True)
            np.testing.assert_allclose(g0[:, :, y, x].numpy(), plain.numpy(), rtol=2e-4)
            gmask, _ = hip_mask_map(hip, c.mask, c.sizes[0], 5, 1.7)
            assert bool((gmask[:, y, x] > 0).all())


def hip_mask_map(hip, mask, size, ks=1, sigma=0.01):
    """ff_pwc_loss_mask -> (gmask (B,h,w) on the CPU, msum)."""
    b, _, hh, ww = mask.shape
    m = mask.to(DEV).contiguous()
    gauss = hip.model.gaussian_table(ks, sigma).to(DEV)
    gmask = torch.full((b, *size), float("nan"), dtype=torch.float32, device=DEV)
    msum = torch.zeros(1, dtype=torch.float64, device=DEV)
    hip.call("ff_pwc_loss_mask", hip.p(m), hip.p(gauss), ks, hip.p(gmask), hip.p(msum), b, hh, ww, size[0], size[1], hip.stream())
    return gmask.cpu(), float(msum.item())


# (source size, level size, the source row / column just below the crossing, the output index that it decides)
MASK_PARITY_CASES = [(33, 13, 15, 6), (39, 15, 31, 12), (52, 20, 31, 12)]


def parity_mask(n, r):
    """n x n mask: one key point in row r, one in column r - with the fused coordinate output index i touches them with a
    weight of ~1e-6, with the separately rounded one it does not - and one in row r + 1, where both forms agree."""
    m = torch.zeros(1, 1, n, n)
    m[0, 0, r, 4] = 255.0
    m[0, 0, 4, r] = 255.0
    m[0, 0, r + 1, 27] = 255.0         # column 27 is read by output column 10 at all three size pairs
    return m


def resized_on(mask2d, size, fused):
    """numpy restatement of '(bilinear resize, align_corners=False) > 0' in fp32 with the source coordinate rounded once
    (fused: the product of two fp32 numbers is exact in fp64) or twice."""
    def taps(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        d = np.arange(n_out, dtype=np.float32) + np.float32(0.5)
        s = (d.astype(np.float64) * np.float64(scale) - 0.5).astype(np.float32) if fused else d * scale - np.float32(0.5)
        s = np.maximum(s, np.float32(0))
        i0 = s.astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0.astype(np.float32)
    m = np.asarray(mask2d, np.float32)
    (y0, y1, ly), (x0, x1, lx) = taps(m.shape[0], size[0]), taps(m.shape[1], size[1])
    one = np.float32(1)
    top = (one - lx) * m[y0][:, x0] + lx * m[y0][:, x1]
    bot = (one - lx) * m[y1][:, x0] + lx * m[y1][:, x1]
    return ((one - ly)[:, None] * top + ly[:, None] * bot) > 0


@pytest.mark.parametrize("n,s,r,i", MASK_PARITY_CASES)
def test_mask_parity_cases_discriminate(n, s, r, i):
    """No GPU: ATen's thresholded map - what the GPU tests below expect - is the map of the once-rounded coordinate and
    differs from the map of the separately rounded one, in output row i and output column i and nowhere else."""
    m = parity_mask(n, r)
    aten = (F.interpolate(m, (s, s), mode="bilinear", align_corners=False) > 0)[0, 0].numpy()
    fused, unfused = resized_on(m[0, 0].numpy(), (s, s), True), resized_on(m[0, 0].numpy(), (s, s), False)
    assert np.array_equal(aten, fused)
    ys, xs = np.nonzero(fused != unfused)
    assert len(ys) >= 2 and bool(((ys == i) | (xs == i)).all()) and (ys == i).any() and (xs == i).any()
    assert bool(fused[ys, xs].all())                         # the fused form turns them on
    assert unfused[i].any() and fused[i].any()               # row r + 1 is seen by both


@gpu
@pytest.mark.parametrize("n,s,r,i", MASK_PARITY_CASES)
def test_pwc_mask_map_parity(hip, n, s, r, i):
    """ff_pwc_loss_mask with k = 1: gmask > 0 equals ATen's thresholded fp32 map exactly, msum is its count."""
    m = parity_mask(n, r)
    aten = (F.interpolate(m, (s, s), mode="bilinear", align_corners=False) > 0)[:, 0]
    gmask, msum = hip_mask_map(hip, m, (s, s))
    assert torch.equal(gmask > 0, aten), f"differs at {torch.nonzero((gmask > 0) != aten).tolist()}"
    assert torch.equal(gmask, aten.float()) and msum == float(aten.sum())


@gpu
@pytest.mark.parametrize("shape", list(PWC_SHAPES))
def test_pwc_mask_map_and_its_sum(hip, shape):
    """Every level of every shape: k = 1 gives ATen's thresholded map exactly; k = 5 the zero-padded Gaussian of it; msum is
    the sum of the map."""
    c = pwc_case(shape)
    box = orc.gaussian_box(5, 1.7).double()
    for size, on in zip(c.sizes, c.maps):
        gmask, msum = hip_mask_map(hip, c.mask, size)
        assert torch.equal(gmask, on[:, 0].float()) and msum == float(on.sum())
        gmask, msum = hip_mask_map(hip, c.mask, size, 5, 1.7)
        want = F.conv2d(F.pad(on.double(), [2, 2, 2, 2]), box)[:, 0]
        np.testing.assert_allclose(gmask.double().numpy(), want.numpy(), rtol=0, atol=1e-6)
        assert abs(msum - float(gmask.double().sum())) <= 1e-12 * max(1.0, msum)


@gpu
@pytest.mark.parametrize("tag", ["MixLoss_pretrain_k5", "MixLoss_finetune_k1", "sparse_MixLoss_pretrain_k5", "CPCL_pretrain_k5"])
def test_pwc_empty_mask_level(hip, tag):
    """Density 0.002: the resized mask of the coarse levels is empty.  MixLoss drops the term there and stays finite and
    equal to the oracle; CPCL is 0/0, as the reference is."""
    c = pwc_case("45x70 sparse mask")
    assert any(not bool(m.any()) for m in c.maps)
    got, want = pwc_run(hip, c, tag)
    if "CPCL" in tag:
        assert not np.isfinite(want[0]) and not np.isfinite(got[0])
        return
    assert np.isfinite(got[0]) and all(bool(torch.isfinite(g).all()) for g in got[2])
    pwc_compare(tag, got, want)


@gpu
def test_pwc_real_epe_past_the_grid_cap(hip):
    """realEPE at 3 x 2 x 384 x 512 from a 96 x 128 flow: 589,824 pixels > 2048 * 256 in ff_pwc_epe_mean[_sparse], 1,179,648
    outputs > 4096 * 256 in ff_resize_bilinear."""
    g = torch.Generator().manual_seed(9)
    flow = torch.randn(3, 2, 96, 128, generator=g) * 3
    target = torch.randn(3, 2, 384, 512, generator=g) * 3
    sparse_target = torch.where(torch.rand(3, 1, 384, 512, generator=g) < 0.35, torch.zeros_like(target), target)
    for mode in ("pretrain", "finetune"):
        _, kw, cfg = pwc_cfg(f"EPELoss_{mode}_k1", PWC_WEIGHTS)
        crit = hip.pwc_losses.build_losses(cfg)
        for sparse, t in ((False, target), (True, sparse_target)):
            want = float(pwc_ref.pwc_real_epe(flow.double(), t.double(), sparse, mode, kw["eps"], kw["q"]))
            got = float(crit.realEPE(flow.to(DEV), t.to(DEV), sparse))
            print(f"realEPE {mode} sparse={sparse}: {got:.8g} vs {want:.8g} (rel {abs(got / want - 1):.2e})")
            assert abs(got - want) < 2e-5 * abs(want), (mode, sparse, got, want)


@gpu
def test_pwc_losses_refuse_bad_sizes(hip):
    c = pwc_case("45x70")
    _, _, cfg = pwc_cfg("EPELoss_pretrain_k1", [1.0])
    with pytest.raises(hip.Error):          # a level larger than the target
        hip.pwc_losses.build_losses(cfg)([torch.zeros(3, 2, 50, 70, device=DEV)], c.target.to(DEV), False)
    _, _, cfg = pwc_cfg("CPCL_pretrain_k5", [1.0])
    cfg.TRAIN.LOSS_KERNEL_SIZE = 4          # an even kernel size
    with pytest.raises(hip.Error):
        hip.pwc_losses.build_losses(cfg)([c.preds[0].to(DEV)], c.target.to(DEV), c.mask.to(DEV), False)


# =====================================================================================================================
# D. resize and layout kernels
# Largest |fp32 F.interpolate - fp64 F.interpolate| / max|src| over RESIZE_CASES and NHWC4_CASES on the CPU - the reference
# against itself - is RESIZE_MEASURED; the kernels blend in another order, so they get four times that.
RESIZE_MEASURED = 2.81e-6        # measured: 2.805e-06, at 24x40 -> 45x70; the 33/39/52 pairs reach 2.2e-06, the large cases 9e-08
RESIZE_TOL = 4 * RESIZE_MEASURED
SENTINEL = 3.0e4
# (B, C, (Hi, Wi), (Ho, Wo), ld or None, (mul0, mul1))
RESIZE_CASES = [
    (2, 2, (13, 21), (100, 180), None, (1.0, 1.0)),              # up
    (2, 1, (100, 180), (64, 96), None, (1.0, 1.0)),              # down: the mask path of FF_PWCNET
    (1, 2, (17, 19), (17, 19), None, (1.0, 1.0)),                # identity
    (2, 2, (1, 1), (5, 7), None, (1.0, 1.0)),                    # a source of one row and one column
    (1, 1, (1, 9), (4, 20), None, (1.0, 1.0)),
    (1, 2, (33, 39), (13, 15), None, (1.0, 1.0)),                # the pairs of MASK_PARITY_CASES
    (1, 1, (52, 33), (20, 13), None, (1.0, 1.0)),
    (2, 2, (13, 21), (37, 53), 7, (1.0, 1.0)),                   # an ld != C view of a wider buffer
    (2, 2, (24, 40), (45, 70), 4, (70 / 40, 45 / 24)),           # mul0, mul1: FF_PWCNET's test_mode output
    (1, 1, (13, 21), (30, 50), None, (-2.5, 7.0)),
    (3, 2, (96, 128), (384, 512), None, (1.0, 1.0)),             # 1,179,648 outputs > 4096 * 256
]
# (B, C, (Hi, Wi), (Ho, Wo))
NHWC4_CASES = [
    (2, 3, (37, 53), (64, 64)),
    (2, 1, (37, 53), (64, 64)),
    (1, 3, (100, 180), (64, 128)),
    (1, 1, (33, 39), (13, 15)),
    (1, 3, (52, 52), (20, 20)),
    (5, 1, (64, 64), (512, 512)),                                # 1,310,720 pixels > 4096 * 256
]


def resize_source(b, c, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, c, *size, generator=g) * 50 + torch.rand(b, c, 1, 1, generator=g) * 100


def interpolate(src, size):
    return F.interpolate(src, size, mode="bilinear", align_corners=False)


def measure_resize_reference():
    """max |fp32 - fp64| / max|src| of F.interpolate over the cases (RESIZE_MEASURED)."""
    worst = 0.0
    for n, (b, c, si, so, *_) in enumerate(RESIZE_CASES + NHWC4_CASES):
        src = resize_source(b, c, si, n)
        worst = max(worst, float((interpolate(src, so).double() - interpolate(src.double(), so)).abs().max() / src.abs().max()))
    return worst


def test_resize_tolerance_is_the_measured_one():
    """No GPU: RESIZE_MEASURED is what F.interpolate in fp32 is off from itself in fp64 on these cases (a CPU whose ATen
    blends in another order may come out a little lower)."""
    assert 0.5 * RESIZE_MEASURED <= measure_resize_reference() <= RESIZE_MEASURED


def hip_resize(hip, src, size, ld=None, mul=(1.0, 1.0)):
    b, c, hi, wi = src.shape
    nhwc = src.permute(0, 2, 3, 1).contiguous().to(DEV)
    buf = None
    if ld is not None:
        buf = torch.full((b, hi, wi, ld), SENTINEL, dtype=torch.float32, device=DEV)
        buf[..., 1:1 + c] = nhwc
        nhwc = buf[..., 1:1 + c]
    dst = torch.full((b, c, *size), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("ff_resize_bilinear", hip.p(nhwc), ld or c, c, hi, wi, hip.p(dst), b, size[0], size[1], float(mul[0]), float(mul[1]), hip.stream())
    if buf is not None:
        assert bool((buf[..., :1] == SENTINEL).all()) and bool((buf[..., 1 + c:] == SENTINEL).all())
    return dst.cpu()


@gpu
@pytest.mark.parametrize("n", range(len(RESIZE_CASES)))
def test_resize_bilinear(hip, n):
    b, c, si, so, ld, mul = RESIZE_CASES[n]
    src = resize_source(b, c, si, n)
    got = hip_resize(hip, src, so, ld, mul)
    want = interpolate(src.double(), so) * torch.tensor(mul[:c], dtype=torch.float64).view(1, c, 1, 1)
    err = float((got.double() - want).abs().max())
    scale = float(src.abs().max()) * max(abs(m) for m in mul[:c])
    print(f"resize_bilinear {RESIZE_CASES[n]}: max err {err:.3e} = {err / scale:.3e} of max|src * mul| (allowed {RESIZE_TOL:.1e})")
    assert err <= RESIZE_TOL * scale
    if si == so:
        assert torch.equal(got, src)


@gpu
@pytest.mark.parametrize("n,s,r,i", MASK_PARITY_CASES)
def test_resize_bilinear_mask_parity(hip, n, s, r, i):
    """FF_PWCNET resizes the key-point mask with ff_resize_bilinear and thresholds it downstream: the resized mask is
    non-zero exactly where ATen's fp32 resize is."""
    m = parity_mask(n, r)
    got = hip_resize(hip, m, (s, s))
    aten = interpolate(m, (s, s))
    assert torch.equal(got > 0, aten > 0), f"differs at {torch.nonzero((got > 0) != (aten > 0)).tolist()}"


def hip_resize_to_nhwc4(hip, src, size):
    b, c, hi, wi = src.shape
    dst = torch.full((b, *size, 4), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("ff_resize_to_nhwc4", hip.p(src.to(DEV).contiguous()), c, hi, wi, hip.p(dst), b, size[0], size[1], hip.stream())
    return dst.cpu()


@gpu
@pytest.mark.parametrize("n", range(len(NHWC4_CASES)))
def test_resize_to_nhwc4(hip, n):
    b, c, si, so = NHWC4_CASES[n]
    src = resize_source(b, c, si, len(RESIZE_CASES) + n)
    got = hip_resize_to_nhwc4(hip, src, so)
    want = interpolate(src.double(), so).expand(b, 3, *so).permute(0, 2, 3, 1)
    err = float((got[..., :3].double() - want).abs().max())
    print(f"resize_to_nhwc4 {NHWC4_CASES[n]}: max err {err:.3e} = {err / float(src.abs().max()):.3e} of max|src| (allowed {RESIZE_TOL:.1e})")
    assert err <= RESIZE_TOL * float(src.abs().max())
    assert bool((got[..., 3] == 0).all())                                        # exactly 0
    if c == 1:                                                                   # repeated bit for bit
        assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])


@gpu
@pytest.mark.parametrize("n,s,r,i", MASK_PARITY_CASES)
def test_resize_to_nhwc4_mask_parity(hip, n, s, r, i):
    m = parity_mask(n, r)
    got = hip_resize_to_nhwc4(hip, m, (s, s))[..., 0]
    aten = interpolate(m, (s, s))[:, 0]
    assert torch.equal(got > 0, aten > 0), f"differs at {torch.nonzero((got > 0) != (aten > 0)).tolist()}"


@gpu
def test_nchw_to_nhwc4(hip):
    """Bit exact: 1 channel repeated, 3 channels, a constant fill without a source; channel 3 is 0; src_c = 2 is refused."""
    def run(src, c, fill, b, h, w):
        dst = torch.full((b, h, w, 4), float("nan"), dtype=torch.float32, device=DEV)
        hip.call("ff_nchw_to_nhwc4", hip.p(src.to(DEV).contiguous() if src is not None else None), c, float(fill), hip.p(dst), b, h, w, hip.stream())
        return dst.cpu()

    g = torch.Generator().manual_seed(3)
    for b, c, h, w in ((2, 3, 17, 19), (2, 1, 17, 19), (1, 3, 1, 1), (5, 1, 512, 513)):      # the last: 1,313,280 pixels > 4096 * 256
        src = torch.randn(b, c, h, w, generator=g) * 100
        want = torch.cat([src.expand(b, 3, h, w), torch.zeros(b, 1, h, w)], 1).permute(0, 2, 3, 1)
        assert torch.equal(run(src, c, -1.0, b, h, w), want), (b, c, h, w)
    got = run(None, 0, 255.0, 2, 17, 19)
    assert torch.equal(got, torch.tensor([255.0, 255.0, 255.0, 0.0]).expand(2, 17, 19, 4))
    with pytest.raises(hip.Error):
        run(torch.zeros(1, 2, 8, 8), 2, 0.0, 1, 8, 8)


@gpu
@pytest.mark.parametrize("b,h,w,c,ld", [(2, 17, 19, 2, None), (2, 17, 19, 5, None), (1, 9, 7, 128, None), (2, 17, 19, 2, 4), (3, 5, 7, 5, 16),
                                        (1, 9, 7, 128, 136), (2, 64, 65, 128, None), (3, 301, 233, 5, 8)])
def test_nhwc_to_nchw(hip, b, h, w, c, ld):
    """ops.nhwc_to_nchw is bit exact against permute: C in {2, 5, 128}, odd planes, ld != C views, and two cases past
    4096 * 256 elements (2 x 64 x 65 x 128 = 1,064,960; 3 x 301 x 233 x 5 = 1,051,995 from a view)."""
    g = torch.Generator().manual_seed(b * h + c)
    x = torch.randn(b, h, w, c, generator=g)
    if ld is None:
        view = x.to(DEV)
    else:
        buf = torch.full((b, h, w, ld), SENTINEL, dtype=torch.float32, device=DEV)
        buf[..., 1:1 + c] = x.to(DEV)
        view = buf[..., 1:1 + c]
    got = hip.ops.nhwc_to_nchw(view)
    assert got.shape == (b, c, h, w) and got.is_contiguous()
    assert torch.equal(got.cpu(), x.permute(0, 3, 1, 2))


# =====================================================================================================================
# E. ff_mask_prepare
MASK_SIGMA = {1: 0.01, 3: 0.8, 31: 5.0}
MASK_ATOL = 2e-5             # on the [-1, 1] output (test_hip_parity.py::test_mask_modes); x 127.5 on the raw [0, 255] output


@functools.lru_cache(maxsize=None)
def mask_case(b, h, w, seed=2):
    """Key points in the corners, values other than 255, and for b > 1 the brightest cluster in sample 1 only."""
    g = torch.Generator().manual_seed(seed)
    image = torch.randint(0, 256, (b, 3, h, w), generator=g).float()
    values = torch.tensor([100.0, 1.0, 1e-3])[torch.randint(0, 3, (b, 1, h, w), generator=g)]
    mask = (torch.rand(b, 1, h, w, generator=g) < 0.02).float() * values
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        mask[:, 0, y, x] = 100.0
    s = min(1, b - 1)
    mask[s, 0, h // 2, w // 2 - 1:w // 2 + 2] = 255.0      # three neighbours at 255: the maximum of neighborG lies here
    return image, mask


def mask_reference(modal, image, mask, k, raw):
    """orc.init_mask (+ the [0,255] -> [-1,1] scaling) -> (B,3,H,W): fp64 for neighborG, which is continuous; fp32 for the
    thresholded modes, where sums of non-negative terms cannot flip the decision."""
    dt = torch.float64 if modal == "neighborG" else torch.float32
    m1, _ = orc.init_mask(image.to(dt), image.to(dt), mask.to(dt), modal, dilate=k, kernel_size=k, kernel_sigma=MASK_SIGMA[k])
    return m1 if raw else 2 * (m1 / 255.0) - 1.0


def hip_mask_prepare(hip, modal, image, mask, k, raw, image_nhwc4=False):
    table = (hip.model.gaussian_table(k, MASK_SIGMA[k]) if modal == "neighborG" else hip.model.ellipse_table(k)).to(DEV)
    img = image.to(DEV)
    if image_nhwc4:
        img = torch.cat([img, torch.zeros_like(img[:, :1])], 1).permute(0, 2, 3, 1).contiguous()
    out = hip.ops.mask_prepare(hip.model.MASK_MODES[modal], mask.to(DEV), img, table, raw=raw, image_nhwc4=image_nhwc4).cpu()
    assert bool((out[..., 3] == 0).all())
    return out[..., :3].permute(0, 3, 1, 2)


def mask_compare(modal, got, want, raw, what):
    if modal == "neighborG":
        err = float((got.double() - want).abs().max())
        print(f"{what}: max err {err:.3e}")
        assert err <= MASK_ATOL * (127.5 if raw else 1.0), what
    elif modal == "neighborE" or raw:
        assert torch.equal(got, want.float()), what          # exact: 255 or 0 (1 or -1), the image or 0
    else:                                                    # context, scaled: the decision is exact, the scaling is rounded
        assert torch.equal(got > -1.0, want > -1.0) and float((got - want).abs().max()) <= MASK_ATOL, what


@gpu
@pytest.mark.parametrize("k", [1, 3, 31])
@pytest.mark.parametrize("modal", ["neighborG", "neighborE", "context"])
def test_mask_prepare(hip, modal, k):
    """9x40 is smaller than the 31-tap kernel; at 3 x 24 x 33 the maximum that neighborG divides by lies in one sample."""
    for b, h, w in ((1, 9, 40), (2, 17, 19), (3, 24, 33)):
        image, mask = mask_case(b, h, w)
        for raw in (False, True):
            want = mask_reference(modal, image, mask, k, raw)
            mask_compare(modal, hip_mask_prepare(hip, modal, image, mask, k, raw), want, raw, f"{modal} k={k} {b}x{h}x{w} raw={raw}")
            if modal == "context":
                mask_compare(modal, hip_mask_prepare(hip, modal, image, mask, k, raw, image_nhwc4=True), want, raw,
                             f"{modal} k={k} {b}x{h}x{w} raw={raw} NHWC4 image")


def test_mask_case_maximum_lies_in_one_sample():
    """No GPU: dividing by a per-sample maximum would give another neighborG tensor."""
    image, mask = mask_case(3, 24, 33)
    for k in (1, 3, 31):
        m = F.conv2d(mask.double(), orc.gaussian_box(k, MASK_SIGMA[k]).double(), padding=k // 2)
        per_sample = m.amax(dim=(1, 2, 3))
        assert float(per_sample[1]) > 1.5 * float(per_sample[0]) and float(per_sample[1]) > 1.5 * float(per_sample[2])


@gpu
def test_mask_prepare_past_the_grid_cap(hip):
    """5 x 512 x 512 = 1,310,720 pixels > 4096 * 256, neighborG: both passes take a second trip, the maximum is global."""
    image, mask = mask_case(5, 512, 512)
    want = mask_reference("neighborG", image, mask, 3, False)
    got = hip_mask_prepare(hip, "neighborG", image, mask, 3, False)
    mask_compare("neighborG", got, want, False, "neighborG k=3 5x512x512")


@gpu
def test_mask_prepare_empty_mask(hip):
    """neighborE and context give finite all-background output; neighborG is 0 * 255 / 0 = NaN, as the reference's
    m * 255 / m.max()."""
    image, mask = mask_case(2, 17, 19)
    empty = torch.zeros_like(mask)
    for raw in (False, True):
        background = 0.0 if raw else -1.0
        for modal in ("neighborE", "context"):
            got = hip_mask_prepare(hip, modal, image, empty, 3, raw)
            assert torch.equal(got, mask_reference(modal, image, empty, 3, raw).float()) and bool((got == background).all())
        assert bool(torch.isnan(mask_reference("neighborG", image, empty, 3, raw)).all())
        assert bool(torch.isnan(hip_mask_prepare(hip, "neighborG", image, empty, 3, raw)).all())
