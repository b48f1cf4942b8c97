#!/usr/bin/env python
"""Generate the plain-RAFT fixtures (use_fusion=None, ff_raft.py:124-132) by RUNNING THE REFERENCE (authoring container
only), in the style of make_golden.py: the reference's own ``RAFT(in_channels=3)`` (raft.py imports no cv2) and its
``inside_fusion='parallel', fuse_cnet=False`` build, filled with the name-hashed weights of ``oracle/weights.py``.
Only data is written: state_dict specs, input checksums and sampled outputs.

The training step's fp64 companion is computed by tests/plain_raft_ref.py, a restatement of plain RAFT from the oracle's
own pieces, in double - as make_golden_train64.py does for the CCE; its fp32 run is first held to the reference's
gradients here.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plain.py
"""
import json
import os
import sys
import zlib
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference/core/models/ff-raft")
sys.dont_write_bytecode = True

from FF_RAFT_Core.raft import RAFT  # noqa: E402  (reference)

from oracle import ffraft_ref as orc  # noqa: E402
from oracle.weights import det_tensor  # noqa: E402
from plain_raft_ref import normalise, plain_raft_forward  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)

TRAIN_KEYS = ["fnet.conv1.weight", "fnet.layer1.0.conv1.weight", "fnet.layer2.0.downsample.0.weight", "fnet.conv2.bias",
              "cnet.conv1.weight", "cnet.layer3.1.conv2.weight", "cnet.norm1.weight", "cnet.layer2.0.norm3.bias",
              "update_block.encoder.convc1.weight", "update_block.gru.convq2.weight", "update_block.gru.convz1.bias",
              "update_block.flow_head.conv2.weight", "update_block.mask.2.weight", "update_block.encoder.convf1.weight"]
TRAIN_BUFS = ["cnet.norm1.running_mean", "cnet.norm1.running_var", "cnet.layer2.0.downsample.1.running_var",
              "cnet.layer3.1.norm2.running_mean"]


def crc(t: torch.Tensor) -> int:
    return zlib.crc32(t.contiguous().numpy().tobytes())


def np32(t):
    return t.detach().float().contiguous().numpy()


def cfg():
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"),
                     MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))


def filled(net):
    sd = net.state_dict()
    net.load_state_dict({k: det_tensor("flow_net." + k, v.shape) for k, v in sd.items()}, strict=True)
    return net


def build_plain():
    """RAFT exactly as FF_RAFT_FUSION(use_fusion=None) builds it (ff_raft.py:125)."""
    return filled(RAFT(in_channels=3, small=False, dropout=0.0, alternate_corr=False))


def build_fuse_cnet_false():
    return filled(RAFT(in_channels=256, small=False, dropout=0.0, alternate_corr=False, abandon_fnet=False,
                       inside_fusion="parallel", fuse_cnet=False, cfg=cfg()))


def write_spec(net, name):
    spec = [["flow_net." + k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, name + ".json"), "w") as f:
        json.dump(spec, f)
    print(name, len(spec), "keys,", sum(p.numel() for p in net.parameters()), "parameters")


def case_forward(net, name, inputs, iters, fuse_cnet_false=False, full=True):
    """Eval-mode forward: sampled encoder outputs, flow_low / flow_up (test_mode) and every iteration's up-sampled flow
    of the train-mode list (sub-sampled)."""
    image1, image2, mask1, mask2 = inputs
    net.eval()
    if fuse_cnet_false:
        i1, i2, m1, m2 = orc.prepare_inputs(image1, image2, mask1, mask2, 3)
        args = (i1, i2, m1, m2)
    else:
        i1, i2 = normalise(image1), normalise(image2)
        args = (i1, i2)
    with torch.no_grad():
        if fuse_cnet_false:
            fmap1, fmap2 = net.fnet(i1, m1), net.fnet(i2, m2)
            cnet = net.cnet(i1)
        else:
            fmap1, fmap2 = net.fnet([i1, i2])
            cnet = net.cnet(i1)
        flow_low, flow_up = net(*args, iters=iters, test_mode=True)
        preds = net(*args, iters=iters)
    rec = dict(in_crc=np.array([crc(image1), crc(image2), crc(mask1)], dtype=np.int64),
               flow_low=np32(flow_low), n_preds=np.array([len(preds)]),
               preds_sub=np.stack([np32(p[:, :, ::8, ::8]) for p in preds]))
    if full:
        rec.update(fmap1=np32(fmap1[:, ::8]), fmap2=np32(fmap2[:, ::8]), cnet=np32(cnet[:, ::8]),
                   flow_up_sub=np32(flow_up[:, :, ::2, ::2]), pred_last_sub=np32(preds[-1][:, :, ::2, ::2]))
    else:
        rec.update(flow_up_sub=np32(flow_up[:, :, ::4, ::4]),
                   flow_up_stats=np.array([flow_up.mean().item(), flow_up.abs().max().item()], dtype=np.float64))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
    print(name, "max|flow_up|", float(flow_up.abs().max()))


def train_inputs():
    image1, image2, _, _ = orc.shifted_pair(2, 128, 128, seed=4)
    g = torch.Generator().manual_seed(5)
    flow_gt = (torch.randn(2, 2, 128, 128, generator=g) * 5).clamp(-400, 400)
    return image1, image2, flow_gt, torch.ones(2, 128, 128)


def case_train(net, name):
    """Train-mode forward (BatchNorm batch statistics) + sequence L1 (losses.py:18-47) + backward."""
    image1, image2, flow_gt, valid = train_inputs()
    net.train()
    net.zero_grad()
    preds = net(normalise(image1), normalise(image2), iters=3)
    loss, _ = orc.sequence_l1(preds, flow_gt, valid)
    loss.backward()
    params = dict(net.named_parameters())
    rec = dict(loss=np.array([loss.item()], dtype=np.float64), pred_last_sub=np32(preds[-1][:, :, ::2, ::2]),
               flow_gt_crc=np.array([crc(flow_gt)], dtype=np.int64))
    for k in TRAIN_KEYS:
        gk = params[k].grad
        rec["grad:" + k] = np32(gk.flatten()[:: max(1, gk.numel() // 512)])
        rec["gnorm:" + k] = np.array([gk.norm().item()], dtype=np.float64)
    total = torch.sqrt(sum((p.grad ** 2).sum() for p in net.parameters()))
    rec["grad_total_norm"] = np.array([total.item()], dtype=np.float64)
    sd = net.state_dict()
    for k in TRAIN_BUFS:
        rec["buf:" + k] = np32(sd[k])
    assert all(p.grad is not None for p in net.parameters())
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
    print(name, "loss", loss.item(), "gradnorm", total.item())
    net.zero_grad()
    return rec


def case_train64(spec_name, ref, name):
    """The same step in fp32 and fp64 through the restatement; fp32 is held to the reference's fixture first."""
    with open(os.path.join(HERE, spec_name + ".json")) as f:
        sd0 = {k: det_tensor(k, s) for k, s, _ in json.load(f)}
    image1, image2, flow_gt, valid = train_inputs()

    def step(dtype):
        sd = {k: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k
                  else v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        preds = plain_raft_forward(sd, normalise(image1).to(dtype), normalise(image2).to(dtype), iters=3, training=True)
        loss, _ = orc.sequence_l1(preds, flow_gt.to(dtype), valid.to(dtype))
        loss.backward()
        return loss, sd

    l32, sd32 = step(torch.float32)
    l64, sd64 = step(torch.float64)
    assert abs(l32.item() - ref["loss"][0]) < 1e-6 * max(1.0, abs(ref["loss"][0])), (l32.item(), ref["loss"][0])
    rec = {"loss64": np.array([l64.item()])}
    for k in TRAIN_KEYS:
        key = "flow_net." + k
        if sd32[key].grad is None:      # norm3 and downsample.1 are ONE module in the reference (two state_dict keys)
            key = key.replace(".norm3.", ".downsample.1.")
        g32, g64 = sd32[key].grad, sd64[key].grad
        s32 = g32.flatten()[:: max(1, g32.numel() // 512)].numpy()
        s64 = g64.flatten()[:: max(1, g64.numel() // 512)].numpy()
        want = ref["grad:" + k]
        np.testing.assert_allclose(s32, want, rtol=0, atol=2e-5 * float(np.abs(want).max()), err_msg=key)
        rec["grad64:" + k] = s64
        rec["gnorm64:" + k] = np.array([g64.norm().item()])
        spread = np.abs(want.astype(np.float64) - s64).max() / np.abs(s64).max()
        print(f"{key:60s} |fp32ref - fp64| / max = {spread:.2e}")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
    print(name, "loss fp32", l32.item(), "fp64", l64.item())


def main():
    net = build_plain()
    write_spec(net, "state_dict_spec_plain")
    case_forward(net, "plain_fwd_rand_128x192_b2_it12", orc.synthetic_inputs(2, 128, 192, seed=0), 12)
    case_forward(net, "plain_fwd_shift_128x192_b2_it12", orc.shifted_pair(2, 128, 192, seed=1), 12)
    case_forward(net, "plain_fwd_shift_384x512_b1_it12", orc.shifted_pair(1, 384, 512, seed=6), 12, full=False)
    ref = case_train(net, "train_plain_shift_128x128_b2_it3")
    case_train64("state_dict_spec_plain", ref, "train_plain_shift_128x128_b2_it3_fp64")

    net = build_fuse_cnet_false()
    write_spec(net, "state_dict_spec_fuse_cnet_false")
    case_forward(net, "fuse_cnet_false_fwd_shift_128x160_b1_it4", orc.shifted_pair(1, 128, 160, seed=8), 4, fuse_cnet_false=True)


if __name__ == "__main__":
    main()
