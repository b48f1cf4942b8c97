"""Plain RAFT (FF_RAFT_FUSION(use_fusion=None), ff_raft.py:124-132) and the fuse_cnet=False build (raft.py:98-101) on the
HIP path, against fixtures written by tests/golden/make_golden_plain.py from the reference's own RAFT."""
import os
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import golden_spec, load_golden
from oracle import ffraft_ref as orc
from oracle.weights import det_tensor
from plain_raft_ref import normalise, plain_raft_forward

DEV = "cuda:0"
GOLDEN_THREADS = 8      # the thread count the fixtures were written at (see test_oracle_golden.py)

FWD = {
    "plain_fwd_rand_128x192_b2_it12": (lambda: orc.synthetic_inputs(2, 128, 192, seed=0), 12),
    "plain_fwd_shift_128x192_b2_it12": (lambda: orc.shifted_pair(2, 128, 192, seed=1), 12),
}


def _cfg(**model):
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"),
                     MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False, **model))


def _spec_sd(name):
    return {k: det_tensor(k, s) for k, s, _ in golden_spec(name)}


@pytest.fixture(scope="module")
def sd_plain():
    return _spec_sd("state_dict_spec_plain")


@pytest.fixture(scope="module")
def sd_fcf():
    return _spec_sd("state_dict_spec_fuse_cnet_false")


def _plain(sd=None, **kw):
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion=None, **kw)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m


def _loaded(sd):
    """What loading `sd` leaves in the model: norm3 and downsample.1 are one module, and downsample.1 is loaded last."""
    return {k: sd[k.replace(".norm3.", ".downsample.1.")] for k in sd}


def crc(t):
    return zlib.crc32(t.contiguous().numpy().tobytes())


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("spec,n_keys,n_params", [("state_dict_spec_plain", 179, 5257536),
                                                   ("state_dict_spec_fuse_cnet_false", 229, 6458464)])
def test_state_dict_matches_the_reference(spec, n_keys, n_params):
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.cce import BasicEncoder
    if spec == "state_dict_spec_plain":
        m = FF_RAFT_FUSION(use_fusion=None, fusion_channels=64, abandon_fnet=True, fuse_cnet=True, freeze_flownet=True,
                           cfg=_cfg())      # (ignored by the reference for use_fusion=None)
        encoders = (m.flow_net.fnet, m.flow_net.cnet)
    else:
        m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=False, cfg=_cfg())
        encoders = (m.flow_net.cnet,)
    got = [(k, tuple(v.shape), str(v.dtype)) for k, v in m.state_dict().items()]
    assert got == golden_spec(spec)
    assert len(got) == n_keys and sum(p.numel() for p in m.parameters()) == n_params
    assert m.fusion_layer is None
    for enc in encoders:
        assert type(enc) is BasicEncoder
        for blk in (enc.layer2[0], enc.layer3[0]):
            assert blk.norm3 is blk.downsample[1]
    if spec == "state_dict_spec_plain":
        assert m.flow_net.inside_fusion is None and m.flow_net.cfg is None
        assert all(p.requires_grad for p in m.parameters())       # freeze_flownet is not read for use_fusion=None
        m.freeze_self()
        assert all(p.requires_grad for p in m.parameters())
        m.train()
        m.flow_net.freeze_bn()
        bns = [x for x in m.modules() if isinstance(x, torch.nn.BatchNorm2d)]
        assert bns and not any(x.training for x in bns)
        assert m.flow_net.fnet.norm_fn == "instance" and m.flow_net.cnet.norm_fn == "batch"


@pytest.mark.parametrize("name", list(FWD))
def test_plain_restatement_matches_reference(name, sd_plain):
    """The restated plain forward (oracle pieces) against the reference's vectors, at near bit equality."""
    g = load_golden(name)
    make, iters = FWD[name]
    image1, image2, mask1, _ = make()
    assert [crc(image1), crc(image2), crc(mask1)] == g["in_crc"].tolist(), "synthetic inputs drifted"
    prev = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)
    try:
        taps = {}
        with torch.no_grad():
            i1, i2 = normalise(image1), normalise(image2)
            flow_low, flow_up = plain_raft_forward(sd_plain, i1, i2, iters, test_mode=True, taps=taps)
            preds = plain_raft_forward(sd_plain, i1, i2, iters)
    finally:
        torch.set_num_threads(prev)
    tol = dict(rtol=2e-6, atol=2e-5)
    for k in ("fmap1", "fmap2", "cnet"):
        np.testing.assert_allclose(taps[k][:, ::8].numpy(), g[k], **tol, err_msg=k)
    np.testing.assert_allclose(flow_low.numpy(), g["flow_low"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(flow_up[:, :, ::2, ::2].numpy(), g["flow_up_sub"], rtol=0, atol=1e-4)
    assert len(preds) == int(g["n_preds"][0])
    np.testing.assert_allclose(np.stack([p[:, :, ::8, ::8].numpy() for p in preds]), g["preds_sub"], rtol=0, atol=1e-4)


def test_load_model_round_trips_a_public_raft_checkpoint(tmp_path, sd_plain):
    """RAFT.load_model(flag='all') with cfg=None: a 'module.'-prefixed checkpoint in RAFT's own layout (the public
    raft-things.pth / raft-chairs.pth), strict; a missing key raises."""
    from focusflow_official_amd.raft_net import RAFT
    ckpt = {"module." + k[len("flow_net."):]: v for k, v in sd_plain.items()}
    path = os.path.join(tmp_path, "raft-things.pth")
    torch.save(ckpt, path)
    net = RAFT(in_channels=3)
    assert net.cfg is None
    net.load_model(path, flag="all")
    got = net.state_dict()
    assert list(got) == [k[len("module."):] for k in ckpt]
    assert all(torch.equal(got[k[len("module."):]], v) for k, v in _loaded(ckpt).items())
    # through the wrapper (raft_CTS: load_raft), and pretrain (raft_CTK: the wrapper's own keys)
    m = _plain(load_raft=path)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in _loaded(sd_plain).items())
    wrapper_path = os.path.join(tmp_path, "raft_sintel_new.pth")
    torch.save(sd_plain, wrapper_path)
    m = _plain(pretrain=wrapper_path)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in _loaded(sd_plain).items())
    del ckpt["module.update_block.mask.2.bias"]
    torch.save(ckpt, path)
    with pytest.raises(RuntimeError, match="mask.2.bias"):
        RAFT(in_channels=3).load_model(path, flag="all")


def test_unbuilt_plain_configurations_still_raise():
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.cce import BasicEncoder
    from focusflow_official_amd.raft_net import RAFT
    with pytest.raises(NotImplementedError, match="inside_fusion=None"):
        FF_RAFT_FUSION(use_fusion=None, raft_small=True)
    with pytest.raises(NotImplementedError, match="dropout"):
        FF_RAFT_FUSION(use_fusion=None, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        BasicEncoder(3, 256, "instance", dropout=0.2)
    with pytest.raises(NotImplementedError, match="plain RAFT"):
        RAFT(in_channels=256, abandon_fnet=True, inside_fusion="parallel", fuse_cnet=True, cfg=_cfg())
    for front_end in ("attention", "conv"):
        with pytest.raises(NotImplementedError):
            FF_RAFT_FUSION(use_fusion=front_end, cfg=_cfg())


def test_shim_exports_the_encoder():
    from FF_RAFT_Core.extractor import BasicEncoder, ResidualBlock
    from focusflow_official_amd import cce
    assert BasicEncoder is cce.BasicEncoder and ResidualBlock is cce.ResidualBlock


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def _close(a, b, atol, what):
    err = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    assert err <= atol, f"{what}: max |diff| {err:.3e} > {atol:.3e}"


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FWD))
def test_plain_forward_matches_reference(name, sd_plain):
    from focusflow_official_amd import ops
    g = load_golden(name)
    make, iters = FWD[name]
    inp = [t.to(DEV) for t in make()]
    m = _plain(sd_plain).to(DEV).eval()
    net = m.flow_net
    with torch.no_grad():
        b, _, h, w = inp[0].shape
        i1, i2 = ops.prep_input(inp[0], b, h, w, inp[0]), ops.prep_input(inp[1], b, h, w, inp[0])
        for what, got in (("fmap1", net.fnet(i1)), ("fmap2", net.fnet(i2)), ("cnet", net.cnet(i1))):
            ref = g[what]
            # (the parity tests' bound: fp32 error relative to the tensor's scale)
            err = np.abs(_nchw(got)[:, ::8].numpy().astype(np.float64) - ref) - 2e-5 * np.abs(ref)
            assert err.max() <= 1e-5 * float(np.abs(ref).max()), f"{what}: {err.max():.3e}"
        flow_low, flow_up = m(*inp, raft_iters=iters, test_mode=True)
        preds = m(*inp, raft_iters=iters)
        # masks are never read: None gives the same flows, bit for bit
        lo_n, up_n = m(inp[0], inp[1], None, None, raft_iters=iters, test_mode=True)
    assert torch.equal(lo_n, flow_low) and torch.equal(up_n, flow_up)
    assert isinstance(preds, list) and len(preds) == int(g["n_preds"][0])
    _close(flow_low.cpu(), g["flow_low"], 1e-3, "flow_low")
    _close(flow_up.cpu()[:, :, ::2, ::2], g["flow_up_sub"], 1e-3, "flow_up")
    _close(np.stack([p.cpu()[:, :, ::8, ::8].numpy() for p in preds]), g["preds_sub"], 1e-3, "per-iteration flows")


@pytest.mark.gpu
def test_plain_384x512_matches_reference(sd_plain):
    g = load_golden("plain_fwd_shift_384x512_b1_it12")
    inp = [t.to(DEV) for t in orc.shifted_pair(1, 384, 512, seed=6)]
    m = _plain(sd_plain).to(DEV).eval()
    with torch.no_grad():
        flow_low, flow_up = m(*inp, raft_iters=12, test_mode=True)
        preds = m(inp[0], inp[1], raft_iters=12)
    _close(flow_low.cpu(), g["flow_low"], 1e-3, "384x512 flow_low")
    _close(flow_up.cpu()[:, :, ::4, ::4], g["flow_up_sub"], 1e-3, "384x512 flow_up")
    _close(np.stack([p.cpu()[:, :, ::8, ::8].numpy() for p in preds]), g["preds_sub"], 1e-3, "384x512 per-iteration flows")


@pytest.mark.gpu
def test_plain_forward_issues_no_mask_launches(sd_plain, monkeypatch):
    """mask1 / mask2 given or None: no mask preparation, no mask tensor reaches the encoders."""
    from focusflow_official_amd import ops
    calls = []
    real_prep, real_mask = ops.prep_input, ops.mask_prepare
    monkeypatch.setattr(ops, "prep_input", lambda src, *a, **k: (calls.append(src), real_prep(src, *a, **k))[1])
    monkeypatch.setattr(ops, "mask_prepare", lambda *a, **k: (calls.append("mask_prepare"), real_mask(*a, **k))[1])
    m = _plain(sd_plain).to(DEV).eval()
    seen = []
    m.flow_net.fnet.register_forward_pre_hook(lambda mod, args: seen.append(args[1:]))
    inp = [t.to(DEV) for t in orc.shifted_pair(1, 128, 128, seed=3)]
    with torch.no_grad():
        m(*inp, raft_iters=2, test_mode=True)
    assert len(calls) == 2 and calls[0] is inp[0] and calls[1] is inp[1]
    assert seen == [(None,)]


@pytest.mark.gpu
def test_plain_fuse_cnet_false_forward_matches_reference(sd_fcf):
    from focusflow_official_amd import FF_RAFT_FUSION
    g = load_golden("fuse_cnet_false_fwd_shift_128x160_b1_it4")
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=False, cfg=_cfg())
    m.load_state_dict(sd_fcf, strict=True)
    m = m.to(DEV).eval()
    inp = [t.to(DEV) for t in orc.shifted_pair(1, 128, 160, seed=8)]
    with torch.no_grad():
        flow_low, flow_up = m(*inp, raft_iters=4, test_mode=True)
        preds = m(*inp, raft_iters=4)
    _close(flow_low.cpu(), g["flow_low"], 1e-3, "fuse_cnet=False flow_low")
    _close(flow_up.cpu()[:, :, ::2, ::2], g["flow_up_sub"], 1e-3, "fuse_cnet=False flow_up")
    _close(np.stack([p.cpu()[:, :, ::8, ::8].numpy() for p in preds]), g["preds_sub"], 1e-3, "fuse_cnet=False per-iteration flows")


def _train_step(sd, g_in=None):
    m = _plain(sd).to(DEV).train()
    image1, image2, _, _ = orc.shifted_pair(2, 128, 128, seed=4)
    gen = torch.Generator().manual_seed(5)
    flow_gt = (torch.randn(2, 2, 128, 128, generator=gen) * 5).clamp(-400, 400).to(DEV)
    valid = torch.ones(2, 128, 128, device=DEV)
    preds = m(image1.to(DEV), image2.to(DEV), None, None, raft_iters=3)
    loss, _ = orc.sequence_l1(preds, flow_gt, valid)
    loss.backward()
    torch.cuda.synchronize()
    return m, preds, loss


@pytest.mark.gpu
def test_plain_train_step_matches_reference(sd_plain, monkeypatch):
    """test_hip_backward.py::test_train_step_matches_reference's bounds on the plain network."""
    from focusflow_official_amd import train_loop
    g = load_golden("train_plain_shift_128x128_b2_it3")
    g64 = load_golden("train_plain_shift_128x128_b2_it3_fp64")
    m, preds, loss = _train_step(sd_plain)
    assert type(preds[-1].grad_fn).__name__ == "UpdateLoopFnBackward"
    assert abs(loss.item() - g["loss"][0]) < 2e-4 * max(1.0, abs(g["loss"][0]))
    _close(preds[-1].detach().cpu()[:, :, ::2, ::2], g["pred_last_sub"], 1e-3, "pred_last")
    params = dict(m.named_parameters(remove_duplicate=False))
    missing = [k for k, p in params.items() if p.grad is None]
    assert not missing, f"parameters without gradient: {missing[:5]}"
    for key in [k for k in g if k.startswith("grad:")]:
        name = "flow_net." + key[5:]
        gk = params[name].grad
        got = gk.flatten()[:: max(1, gk.numel() // 512)].cpu().numpy().astype(np.float64)
        gn = float(g["gnorm:" + key[5:]][0])
        assert abs(gk.norm().item() - gn) < 2e-3 * max(gn, 1e-3), f"{name}: |grad| {gk.norm().item():.6g} vs {gn:.6g}"
        want64 = g64["grad64:" + key[5:]]
        scale = float(np.abs(want64).max())
        ref_spread = float(np.abs(g[key].astype(np.float64) - want64).max())
        hip_spread = float(np.abs(got - want64).max())
        bound = 1e-4 * scale if ("flow_head.conv2" in name or "mask.2" in name) else max(8 * ref_spread, 5e-3 * scale)
        assert hip_spread <= bound, f"{name}: |hip - fp64| {hip_spread / scale:.2e} of max vs reference spread {ref_spread / scale:.2e}"
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters())).item()
    assert abs(total - g["grad_total_norm"][0]) < 2e-3 * g["grad_total_norm"][0]
    sd = m.state_dict()
    for key in [k for k in g if k.startswith("buf:")]:
        np.testing.assert_allclose(sd["flow_net." + key[4:]].cpu().numpy(), g[key], rtol=1e-4, atol=1e-5)
    # the same step on the per-operation tape
    fused = {k: p.grad.clone() for k, p in params.items()}
    monkeypatch.setattr(train_loop, "ENABLED", False)
    m2, preds2, _ = _train_step(sd_plain)
    assert type(preds2[-1].grad_fn).__name__ != "UpdateLoopFnBackward"
    for k, p in m2.named_parameters(remove_duplicate=False):
        scale = float(fused[k].abs().max())
        err = float((p.grad - fused[k]).abs().max())
        assert err <= 1e-5 * max(scale, 1e-12) + 1e-7, f"{k}: fused node vs tape {err:.3e} (max {scale:.3e})"


@pytest.mark.gpu
def test_plain_frozen_bn_step(sd_plain):
    """raft_CTK: freeze_bn() inside a training step - running statistics fixed, gamma / beta still trained; the
    gradients against the restatement in fp64 (BatchNorm in eval mode)."""
    m = _plain(sd_plain).to(DEV).train()
    m.flow_net.freeze_bn()
    bufs = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    inp = orc.shifted_pair(1, 128, 128, seed=9)
    preds = m(*[t.to(DEV) for t in inp], raft_iters=2)
    preds[-1].abs().mean().backward()
    torch.cuda.synchronize()
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in bufs.items())
    params = dict(m.named_parameters(remove_duplicate=False))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())

    def ref(dtype):
        sd = {k: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k
                  else v.to(dtype) if v.is_floating_point() else v) for k, v in sd_plain.items()}
        out = plain_raft_forward(sd, normalise(inp[0]).to(dtype), normalise(inp[1]).to(dtype), iters=2, training=False)
        out[-1].abs().mean().backward()
        return out[-1].detach(), sd

    last32, r32 = ref(torch.float32)
    _, r64 = ref(torch.float64)
    _close(preds[-1].detach().cpu(), last32, 2e-4 * float(last32.abs().max()), "frozen-BN pred")
    for name in ["flow_net.cnet.norm1.weight", "flow_net.cnet.layer2.0.downsample.1.bias", "flow_net.cnet.conv1.weight",
                 "flow_net.fnet.layer1.1.conv2.weight", "flow_net.update_block.gru.convq1.weight"]:
        got, g32, g64 = params[name].grad.cpu().double(), r32[name].grad.double(), r64[name].grad
        scale = float(g64.abs().max())
        bound = max(8 * float((g32 - g64).abs().max()), 5e-3 * scale)
        assert float((got - g64).abs().max()) <= bound, name


@pytest.mark.gpu
def test_plain_alternate_corr_inference(sd_plain):
    """alternate_corr=True: the same plain inference as the materialised block (test_alt_corr.py's whole-network bound)."""
    inp = [t.to(DEV) for t in orc.shifted_pair(2, 384, 512, seed=71)]
    m_ref, m_alt = _plain(sd_plain).to(DEV).eval(), _plain(sd_plain, alternate_corr=True).to(DEV).eval()
    with torch.no_grad():
        lo_r, up_r = m_ref(*inp, raft_iters=12, test_mode=True)
        lo_a, up_a = m_alt(*inp, raft_iters=12, test_mode=True)
        preds_r, preds_a = m_ref(*inp, raft_iters=12), m_alt(*inp, raft_iters=12)
    _close(lo_a.cpu(), lo_r.cpu(), 1e-3, "alt flow_low")
    _close(up_a.cpu(), up_r.cpu(), 1e-3, "alt flow_up")
    assert len(preds_a) == 12 and max(float((x - y).abs().max()) for x, y in zip(preds_a, preds_r)) <= 1e-3


@pytest.mark.gpu
def test_plain_graph_replay(sd_plain):
    """A captured plain eval forward replays bit-identically to eager on a second input.  (B = 6 at 384 x 512: above
    ops.conv2d's small-plane bound, so the capture takes no K split the eager forward does not: same arithmetic.)"""
    from focusflow_official_amd.graph import GraphedForward
    m = _plain(sd_plain).to(DEV).eval()
    a = [t.to(DEV) for t in orc.shifted_pair(6, 384, 512, seed=31)[:2]] + [None, None]
    b = [t.to(DEV) for t in orc.shifted_pair(6, 384, 512, seed=32)[:2]] + [None, None]
    gf = GraphedForward(m, a, raft_iters=4)
    ga = [t.clone() for t in gf(*a)]
    gb = [t.clone() for t in gf(*b)]
    with torch.no_grad():
        eb = [t.clone() for t in m(*b, raft_iters=4, test_mode=True)]
    torch.cuda.synchronize()
    for x, y in zip(eb, gb):
        assert torch.equal(x, y), f"graph vs eager: max |diff| {float((x - y).abs().max()):.3e}"
    assert not torch.equal(ga[1], gb[1])


# the three plain-RAFT configs' MODEL / TRAIN settings (config/experiment/raft_CTS.yaml, raft_CTK.yaml,
# config/ablation/train/raft_start.yaml); shapes cut to 2 x 128 x 160 for the test
CONFIGS = {
    "raft_CTS": dict(STAGE="sintel", LOSS_TYPE="EPELoss", MASK_MODAL="point", LOSS_GAMMA=0.85, PRETRAIN=None, LOAD_MODULE="raft-things.pth", LR=1e-4),
    "raft_CTK": dict(STAGE="kitti", LOSS_TYPE="EPELoss", MASK_MODAL="point", LOSS_GAMMA=0.85, PRETRAIN="raft_sintel_new.pth", LOAD_MODULE=None, LR=1e-4),
    "raft_start": dict(STAGE="chairs", LOSS_TYPE="MixLoss", MASK_MODAL="context", LOSS_GAMMA=0.8, PRETRAIN=None, LOAD_MODULE=None, LR=4e-4),
}


@pytest.fixture(scope="module")
def rccl_group():
    """world_size 1 over RCCL, on a port of this module's own."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29583", HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_plain_configs_train_py_call_sequence(name, sd_plain, tmp_path, rccl_group):
    """train.py's call sequence through the shim (test_shim_dropin.py) with each plain config's settings: constructor,
    freeze_bn outside 'chairs', weights by PRETRAIN / LOAD_MODULE (public RAFT layout, 'module.' keys) or a restored
    checkpoint, DDP(find_unused_parameters=False), two steps with the config's loss, then evaluate.py's test_mode call."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    from FF_RAFT_Core.ff_raft import FF_RAFT_FUSION
    from focusflow_official_amd.losses import build_losses
    c = CONFIGS[name]
    torch.save(sd_plain, os.path.join(tmp_path, "raft_sintel_new.pth"))
    torch.save({"module." + k[len("flow_net."):]: v for k, v in sd_plain.items()}, os.path.join(tmp_path, "raft-things.pth"))
    cfg = Namespace(TRAIN=Namespace(STAGE=c["STAGE"], MASK_MODAL=c["MASK_MODAL"], MASK_CHANNEL=3, MASK_DILATE=31, KERNEL_SIZE=31,
                                    KERNEL_SIGMA=5, CLIP=1.0, LOSS_TYPE=c["LOSS_TYPE"], LOSS_GAMMA=c["LOSS_GAMMA"], MAX_FLOW=400,
                                    LOSS_KERNEL_SIZE=1, LOSS_SIGMA=0.01, LOSS_LAMDA=1),
                    MODEL=Namespace(FUSION=None, FUSION_TYPE=None, FUSION_CHANNEL=256, PRETRAIN=c["PRETRAIN"], LOAD_MODULE=c["LOAD_MODULE"],
                                    FREEZE_MODULE=False, SMALL=False, ABANDON_FNET=False, FUSE_CNET=True, ITERS=3, DROPOUT=0.0,
                                    ALT_CORR=False, LOAD_MODULE_TO_BRANCH=False))
    path = lambda f: os.path.join(tmp_path, f) if f else None      # noqa: E731
    model = FF_RAFT_FUSION(pretrain=path(cfg.MODEL.PRETRAIN), load_raft=path(cfg.MODEL.LOAD_MODULE), use_fusion=cfg.MODEL.FUSION,
                           fusion_channels=cfg.MODEL.FUSION_CHANNEL, raft_small=cfg.MODEL.SMALL, dropout=cfg.MODEL.DROPOUT,
                           alternate_corr=cfg.MODEL.ALT_CORR, abandon_fnet=cfg.MODEL.ABANDON_FNET, fuse_cnet=cfg.MODEL.FUSE_CNET,
                           freeze_flownet=cfg.MODEL.FREEZE_MODULE, cfg=cfg)
    if cfg.TRAIN.STAGE != "chairs":
        model.flow_net.freeze_bn()
    if cfg.MODEL.PRETRAIN is None and cfg.MODEL.LOAD_MODULE is None:
        model.load_state_dict(sd_plain, strict=True)             # train.py:199 (RESTORE_CHECKPOINT)
    assert all(torch.equal(model.state_dict()[k], v) for k, v in _loaded(sd_plain).items())
    model.to(DEV)
    optimizer = torch.optim.AdamW(filter(lambda p: p.requires_grad, model.parameters()), lr=c["LR"], weight_decay=1e-5, eps=1e-8)
    model = DDP(model, device_ids=[0], output_device=0, find_unused_parameters=False)
    loss_function = build_losses(cfg.TRAIN.LOSS_TYPE, gamma=cfg.TRAIN.LOSS_GAMMA, max_flow=400, kernel_size=1, sigma=0.01, lamda=1)
    image1, image2, mask1, mask2 = [x.to(DEV) for x in orc.shifted_pair(2, 128, 160, seed=5)]
    flow = torch.randn(2, 2, 128, 160, generator=torch.Generator().manual_seed(1)).to(DEV) * 3
    valid = torch.ones(2, 128, 160, device=DEV)
    bufs = {k: v.clone() for k, v in model.module.state_dict().items() if "running_" in k}
    model.train()
    if cfg.TRAIN.STAGE != "chairs":
        model.module.flow_net.freeze_bn()
    losses = []
    for _ in range(2):
        before = {k: v.detach().clone() for k, v in model.module.named_parameters()}
        optimizer.zero_grad()
        flow_predictions = model(image1, image2, mask1, mask2, raft_iters=cfg.MODEL.ITERS)
        loss, metrics = loss_function(flow_predictions, flow, valid, mask1)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.TRAIN.CLIP)
        optimizer.step()
        assert torch.isfinite(loss) and "epe" in metrics
        losses.append(loss.item())
        moved = [k for k, v in model.module.named_parameters() if not torch.equal(v, before[k])]
        assert len(moved) > 0.9 * len(before), f"{len(moved)} of {len(before)} parameters moved"
    after = model.module.state_dict()
    frozen_bn = cfg.TRAIN.STAGE != "chairs"
    assert all(torch.equal(after[k], v) == frozen_bn for k, v in bufs.items())
    model.eval()
    with torch.no_grad():
        flow_low, flow_up = model.module(image1, image2, mask1, mask2, raft_iters=2, test_mode=True)
    assert flow_low.shape == (2, 2, 16, 20) and flow_up.shape == (2, 2, 128, 160)
    assert bool(torch.isfinite(flow_up).all())
