"""Plain RAFT (FF_RAFT_FUSION(use_fusion=None)) against FF-RAFT (use_fusion='parallel', the CCE encoders), same process.

    python tools/bench_plain_raft.py [--rounds 5] [--reps 20]

Legs, each alternating the two models round by round (median of the rounds):
  forward    pairs/s at 8 x 384 x 512, 12 iterations, test_mode: eager forwards and captured ones (GraphedForward)
  train      ms per training step (forward + EPELoss + backward, 12 iterations): 8 x 368 x 496 with BatchNorm in
             train mode (raft_start's stage), and plain RAFT alone at raft_CTK's 6 x 288 x 960 with freeze_bn()
Progress goes to stderr; stdout gets one JSON line.
"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def _model(kind):
    from focusflow_official_amd import FF_RAFT_FUSION
    from oracle.weights import det_tensor
    spec = "state_dict_spec_plain" if kind == "plain" else "state_dict_spec"
    with open(os.path.join(ROOT, "tests", "golden", spec + ".json")) as f:
        sd = {k: det_tensor(k, s) for k, s, _ in json.load(f)}
    if kind == "plain":
        m = FF_RAFT_FUSION(use_fusion=None)
    else:
        cfg = Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))
        m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def _inputs(b, h, w):
    from oracle import ffraft_ref as orc
    return [t.to(DEV) for t in orc.shifted_pair(b, h, w, seed=3)]


def _alternate(fns, rounds, reps, per_call):
    """{name: median over `rounds` of per_call(seconds per call)}, the callables timed in alternation."""
    per = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            per[k].append(per_call((time.perf_counter() - t0) / reps))
    return {k: sorted(v)[len(v) // 2] for k, v in per.items()}, per


def forward(rounds, reps):
    from focusflow_official_amd.graph import GraphedForward
    b, h, w, iters = 8, 384, 512, 12
    inp = _inputs(b, h, w)
    models = {k: _model(k) for k in ("plain", "ffraft")}

    def eager(m):
        def run():
            with torch.no_grad():
                m(*inp, raft_iters=iters, test_mode=True)
        return run

    med_e, all_e = _alternate({k: eager(m) for k, m in models.items()}, rounds, reps, lambda s: b / s)
    graphs = {k: GraphedForward(m, inp, raft_iters=iters) for k, m in models.items()}
    med_g, all_g = _alternate({k: (lambda g=g: g(*inp)) for k, g in graphs.items()}, rounds, reps, lambda s: b / s)
    print(f"forward {b}x{h}x{w} it{iters} pairs/s eager {med_e}  graph {med_g}  (all: {all_e} / {all_g})", file=sys.stderr)
    del graphs, models
    torch.cuda.empty_cache()
    return {"forward_8x384x512_it12_pairs_per_s": {"eager": med_e, "graph": med_g}}


def _step(m, inp, loss_fn, flow, valid, iters):
    for p in m.parameters():
        p.grad = None
    preds = m(*inp, raft_iters=iters)
    loss, _ = loss_fn(preds, flow, valid, inp[2])
    loss.backward()


def train(rounds, reps):
    from focusflow_official_amd.losses import build_losses
    loss_fn = build_losses("EPELoss", gamma=0.8, max_flow=400)
    out = {}
    iters = 12
    # 8 x 368 x 496, BatchNorm in train mode: plain vs FF-RAFT
    b, h, w = 8, 368, 496
    inp = _inputs(b, h, w)
    g = torch.Generator().manual_seed(5)
    flow = (torch.randn(b, 2, h, w, generator=g) * 5).to(DEV)
    valid = torch.ones(b, h, w, device=DEV)
    models = {k: _model(k).train() for k in ("plain", "ffraft")}
    med, per = _alternate({k: (lambda m=m: _step(m, inp, loss_fn, flow, valid, iters)) for k, m in models.items()},
                          rounds, max(2, reps // 2), lambda s: s * 1e3)
    print(f"train {b}x{h}x{w} it{iters} ms/step {med}  (all: {per})", file=sys.stderr)
    out["train_8x368x496_it12_ms"] = med
    del models, inp, flow, valid
    torch.cuda.empty_cache()
    # raft_CTK: 6 x 288 x 960, freeze_bn()
    b, h, w = 6, 288, 960
    inp = _inputs(b, h, w)
    flow = (torch.randn(b, 2, h, w, generator=g) * 5).to(DEV)
    valid = torch.ones(b, h, w, device=DEV)
    m = _model("plain").train()
    m.flow_net.freeze_bn()
    med, per = _alternate({"plain": lambda: _step(m, inp, loss_fn, flow, valid, iters)}, rounds, max(2, reps // 2), lambda s: s * 1e3)
    print(f"train {b}x{h}x{w} it{iters} freeze_bn ms/step {med}  (all: {per})", file=sys.stderr)
    out["train_6x288x960_it12_freeze_bn_ms"] = med
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--legs", default="forward,train")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps}
    legs = a.legs.split(",")
    if "forward" in legs:
        res.update(forward(a.rounds, a.reps))
    if "train" in legs:
        res.update(train(a.rounds, a.reps))
    print(json.dumps(res))
