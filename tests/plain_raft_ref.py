"""Plain RAFT (raft.py:92-95, :185-236 with inside_fusion=None) and the fuse_cnet=False build (raft.py:98-101, :204)
restated from the oracle's own pieces: BasicEncoder (extractor.py:118-192) is the CCE's frame branch without the mask
branch and the fusion units.  Test infrastructure, shared by tests/test_plain_raft.py and
tests/golden/make_golden_plain.py (which pins it to the reference and writes its fp64 companion)."""
import torch

from oracle import ffraft_ref as orc


def basic_encoder(sd, p, x, kind, training=False):
    """BasicEncoder.forward (extractor.py:168-192) on one tensor."""
    x = torch.relu(orc._norm(sd, p + ".norm1", orc._conv(sd, p + ".conv1", x, 2, 3), kind, training))
    x = orc._stage(sd, p + ".layer1", x, kind, 1, training)
    x = orc._stage(sd, p + ".layer2", x, kind, 2, training)
    x = orc._stage(sd, p + ".layer3", x, kind, 2, training)
    return orc._conv(sd, p + ".conv2", x)


def normalise(image):
    """ff_raft.py:147-148: [0, 255] -> [-1, 1]."""
    return 2 * (image.contiguous() / 255.0) - 1.0


def plain_raft_forward(sd, i1, i2, iters=12, flow_init=None, test_mode=False, training=False, prefix="flow_net.",
                       masks=None, taps=None):
    """RAFT.forward on normalised images.  masks=None: plain RAFT - fnet runs on [i1, i2] as one batch of 2B
    (raft.py:186).  masks=(m1, m2): the fuse_cnet=False build - the CCE fnet per frame (raft.py:188-189) with a
    BasicEncoder cnet.  Returns the list of up-sampled flows, or (flow_low, flow_up) in test_mode."""
    p = prefix
    b = i1.shape[0]
    if masks is None:
        fmap1, fmap2 = basic_encoder(sd, p + "fnet", torch.cat([i1, i2], 0), "instance", training).split([b, b], 0)
    else:
        fmap1 = orc.cce_encoder(sd, p + "fnet", i1, masks[0], "instance", training)
        fmap2 = orc.cce_encoder(sd, p + "fnet", i2, masks[1], "instance", training)
    if fmap1.dtype != torch.float64:      # raft.py:191-193; fp64 is kept for noise studies
        fmap1, fmap2 = fmap1.float(), fmap2.float()
    pyramid = orc.corr_pyramid(orc.corr_volume(fmap1, fmap2))
    cnet = basic_encoder(sd, p + "cnet", i1, "batch", training)
    net, inp = torch.split(cnet, [128, 128], dim=1)
    net, inp = torch.tanh(net), torch.relu(inp)
    _, _, hh, ww = i1.shape
    coords0 = orc.coords_grid(b, hh // 8, ww // 8, i1.dtype)
    coords1 = coords0.clone()
    if flow_init is not None:
        coords1 = coords1 + flow_init
    if taps is not None:
        taps.update(fmap1=fmap1, fmap2=fmap2, cnet=cnet)
    preds, coords1 = orc.update_loop(sd, p + "update_block", pyramid, net, inp, coords0, coords1, iters)
    if test_mode:
        return coords1 - coords0, preds[-1]
    return preds
