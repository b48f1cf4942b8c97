"""The recorded update loop on its own: train_loop.UpdateLoopFn (one autograd node for all iterations, the default training
route) and the per-operation tape of fn.py (FF_TRAIN_LOOP=0, FF_CONV_PRECISION=fp32, chunked pyramids), driven through the
dispatch RAFT.forward uses (RAFT._update_loop) and compared with CPU autograd over the oracle's loop (ffraft_ref.update_loop)
in float64 and float32, on well-conditioned inputs.

The whole-network gradient tests in test_hip_backward.py cannot be tight (their context features drive the gates to ~1000,
see the note above _check_grad_spread there).  Here the loop's inputs are on the scales of the single-step test
(test_update_block_step_backward_against_fp64: net0 = tanh(randn), inp = relu(randn), correlation values O(1)), where the
loop is as well conditioned as one step - so a systematic error of 1e-3 of a tensor's maximum (one iteration's share missing
from a weight gradient, a wrong mask scale, a slab scaled by the wrong max|g| word) fails.

Bounds, per tensor (every prediction, d net0, d inp, d fmap1, d fmap2, every trainable parameter of the update block):
  * against fp64:      max|hip - fp64| <= max(8 x max|oracle fp32 - fp64|, 1e-4 x max|fp64|);
  * fused node vs tape on identical inputs: max|fused - tape| <= 2e-5 x max|tape|;
  * W_F16 (plain fp16 operands): max|hip - fp64| <= 3 x the tape's own error under W_F16 (or the bound above).
Measured on an MI355X, largest over all tensors of a case, as a fraction of that tensor's maximum:
                                                       fused - fp64   tape - fp64   fused - tape
  default (f16x3, fused forward, gate, side stream,
           WCHUNK 4; b 2, 16x24, T 3)                    1.25e-5       1.24e-5       5.8e-7
  conv-by-conv forward (FUSED_FWD=0)                     1.24e-5       1.24e-5       6.1e-7
  ungated / one stream                                   1.25e-5       1.24e-5       5.9e-7 / 6.0e-7
  WCHUNK 1 / 2 / 12                                      1.25e-5       1.24e-5       5.7e-7 / 6.4e-7 / 5.8e-7
  douts spread over 1e2, WCHUNK 4 / 2                    1.79e-5       1.79e-5       8.4e-7 / 7.6e-7
  douts last-only / first-only / middle missing          1.25e-5 / 1.72e-5 / 1.25e-5 (tape alike)   5.8e-7 / 8.3e-7 / 6.9e-7
  freeze_self("parallel")                                1.25e-5       1.24e-5       6.4e-7
  fmaps without gradient                                 1.25e-5       1.24e-5       5.5e-7
  per-iteration lookup backward                          1.25e-5       1.24e-5       7.5e-7
  17x19 planes, b 3, flow_init up to 12 px               3.7e-6        3.8e-6        5.7e-7
  the tape under W_F32                                   -             1.37e-5       -
  douts x 2^-30 / x 2^20 against x 1 (grads / s; the predictions bit-identical): fused node 5.8e-7 / 6.2e-7, tape 6.9e-7 / 5.2e-7
  W_F16: fused and tape both 7.5e-2 (d fmap1); T = 33 (tape only): fused - tape 1.4e-6
(The largest fp64 errors are in the predictions and the mask head, where the CPU fp32 oracle shows the same.)
Seeds: a ReLU output within rounding of zero flips its mask and moves single gradient entries by 1e-3 .. 3e-2 of the
maximum - no arithmetic defect, just a discontinuous derivative.  Over seeds 4 .. 13 of the odd-plane case six put some
element there (the HIP run or the CPU fp32 oracle on the other side of fp64); the seeds below are free of such elements.
If a kernel change ever moves one across, the fused-vs-tape comparison (same forward, same masks) stays tight and tells a
flip from a defect.
"""
import contextlib

import pytest
import torch

from oracle import ffraft_ref as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRE = "flow_net.update_block"
GRAD_INPUTS = ("dnet0", "dinp", "dfmap1", "dfmap2")
_ORACLE = {}


def _cfg():
    from argparse import Namespace
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"),
                     MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))


@pytest.fixture(scope="module")
def raft(det_sd):
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg())
    m.load_state_dict(det_sd, strict=True)
    return m.to(DEV).train().flow_net


def _inputs(b=2, h=16, w=24, T=3, seed=1, spread=1.0, present=None, flow_init=0.0):
    """NCHW CPU tensors: net0, inp, fmap1, fmap2 (randn: the correlation values <f1, f2> / 16 are ~N(0, 1)), flow_init or
    None, and the T upstream gradients - dout_t scaled by spread^((T-1-t)/(T-1)) (the first iteration's the largest), None
    where present[t] is False."""
    g = torch.Generator().manual_seed(seed)
    net0 = torch.tanh(torch.randn(b, 128, h, w, generator=g))
    inp = torch.randn(b, 128, h, w, generator=g).relu()
    f1, f2 = torch.randn(b, 256, h, w, generator=g), torch.randn(b, 256, h, w, generator=g)
    fi = (torch.rand(b, 2, h, w, generator=g) * 2 - 1) * flow_init if flow_init else None
    douts = [torch.randn(b, 2, 8 * h, 8 * w, generator=g) * spread ** ((T - 1 - t) / max(1, T - 1)) for t in range(T)]
    if present is not None:
        douts = [d if keep else None for d, keep in zip(douts, present)]
    return dict(net0=net0, inp=inp, fmap1=f1, fmap2=f2, flow_init=fi, douts=douts, T=T)


def _oracle(det_sd, key, ins, dtype):
    """CPU autograd through ffraft_ref: corr_volume -> corr_pyramid -> update_loop, loss sum_t <dout_t, pred_t>."""
    if (key, dtype) in _ORACLE:
        return _ORACLE[key, dtype]
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in det_sd.items() if k.startswith(PRE + ".")}
    net0, inp, f1, f2 = (ins[k].to(dtype).clone().requires_grad_(True) for k in ("net0", "inp", "fmap1", "fmap2"))
    b, _, h, w = net0.shape
    pyr = orc.corr_pyramid(orc.corr_volume(f1, f2))
    c0 = orc.coords_grid(b, h, w, dtype)
    c1 = c0 + ins["flow_init"].to(dtype) if ins["flow_init"] is not None else c0.clone()
    preds, _ = orc.update_loop(sd, PRE, pyr, net0, inp, c0, c1, ins["T"])
    sum((p * d.to(dtype)).sum() for p, d in zip(preds, ins["douts"]) if d is not None).backward()
    out = {f"flow_up[{t}]": p.detach() for t, p in enumerate(preds)}
    out.update(dnet0=net0.grad, dinp=inp.grad, dfmap1=f1.grad, dfmap2=f2.grad)
    out.update({k[len(PRE) + 1:]: v.grad for k, v in sd.items()})
    _ORACLE[key, dtype] = out
    return out


def _run(raft, ins, grad_fmaps=True, grad_of=None):
    """One recorded pass of the loop on the HIP path, set up as RAFT.forward sets it up (norm-statistics arena, weight-gradient
    scope, one-launch weight packing, the LoopParamGate created before the loop), then the gradient of sum_t <dout_t, pred_t>:
    by .backward(), or - grad_of = list of names - by torch.autograd.grad over those leaves only.
    -> ({name: CPU tensor}, the type name of the predictions' autograd node)."""
    from focusflow_official_amd import cce, fn, ops
    ub = raft.update_block

    def dev(t, grad=True):
        return t.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(grad)

    leaves = dict(net0=dev(ins["net0"]), inp=dev(ins["inp"]), fmap1=dev(ins["fmap1"], grad_fmaps), fmap2=dev(ins["fmap2"], grad_fmaps))
    b, h, w, _ = leaves["net0"].shape
    for p in ub.parameters():
        p.grad = None
    ops.begin_forward(DEV)
    fn.begin_graph(DEV)
    cce.prepack(raft, DEV)
    try:
        gate = raft._loop_gate(raft._fused_train())
        fi = ins["flow_init"]
        coords1 = ops.coords_init(b, h, w, leaves["net0"], fi.to(DEV) if fi is not None else None)
        preds = raft._update_loop(leaves["net0"], leaves["inp"], leaves["fmap1"], leaves["fmap2"], coords1, ins["T"], gate)
    finally:
        fn.end_graph()
    assert len(preds) == ins["T"]
    route = type(preds[0].grad_fn).__name__
    used = [(p, d.to(DEV)) for p, d in zip(preds, ins["douts"]) if d is not None]
    out = {f"flow_up[{t}]": p.detach().cpu() for t, p in enumerate(preds)}
    params = dict(ub.named_parameters())
    if grad_of is None:
        torch.autograd.backward([p for p, _ in used], [d for _, d in used])
        torch.cuda.synchronize()
        grads = {"d" + k: v.grad for k, v in leaves.items()}
        grads.update({k: p.grad for k, p in params.items() if p.requires_grad})
    else:
        wrt = [leaves[k[1:]] if k in GRAD_INPUTS else params[k] for k in grad_of]
        loss = sum((p * d).sum() for p, d in used)
        grads = dict(zip(grad_of, torch.autograd.grad(loss, wrt)))
        torch.cuda.synchronize()
        assert all(p.grad is None for p in params.values()), "torch.autograd.grad must not write .grad"
    for k, v in grads.items():
        if v is not None:
            out[k] = v.permute(0, 3, 1, 2).cpu() if k in GRAD_INPUTS else v.cpu()
    return out, route


def _keys(raft, T, grad_fmaps=True):
    return ([f"flow_up[{t}]" for t in range(T)] + ["dnet0", "dinp"] + (["dfmap1", "dfmap2"] if grad_fmaps else [])
            + [k for k, p in raft.update_block.named_parameters() if p.requires_grad])


def _vs_fp64(got, r32, r64, keys, what, loose=None):
    """Every tensor within max(8 x the oracle's own fp32 spread, 1e-4 of its maximum) of fp64 - or within loose[k]
    (absolute) where given.  Returns the largest |got - fp64| / max|fp64|."""
    bad, worst = [], (0.0, None)
    for k in keys:
        assert got.get(k) is not None, f"{what}: no {k}"
        want = r64[k].double()
        scale = float(want.abs().max())       # (0: convf1's weights when only iteration 0, whose flow is zero, is reached)
        err = float((got[k].double() - want).abs().max())
        bound = max(8 * float((r32[k].double() - want).abs().max()), 1e-4 * scale)
        if loose is not None:
            bound = max(bound, loose[k])
        if err >= worst[0] * max(scale, 1e-30):
            worst = (err / max(scale, 1e-30), k)
        if not err <= bound:
            bad.append(f"{k}: |hip - fp64| {err / scale:.2e} of max, bound {bound / scale:.2e}")
    print(f"{what}: max |hip - fp64| / max|fp64| = {worst[0]:.2e} ({worst[1]})")
    assert not bad, f"{what}:\n  " + "\n  ".join(bad)
    return worst


def _vs(got, ref, keys, what, tol=2e-5):
    """Every tensor within tol of its maximum of `ref` (the same inputs through another route)."""
    bad, worst = [], (0.0, None)
    for k in keys:
        assert got.get(k) is not None and ref.get(k) is not None, f"{what}: no {k}"
        scale = float(ref[k].abs().max())
        err = float((got[k] - ref[k]).abs().max())
        if err >= worst[0] * max(scale, 1e-30):
            worst = (err / max(scale, 1e-30), k)
        if not err <= tol * scale:
            bad.append(f"{k}: {err / max(scale, 1e-30):.2e} of max (bound {tol:.0e})")
    print(f"{what}: max |a - b| / max|b| = {worst[0]:.2e} ({worst[1]})")
    assert not bad, f"{what}:\n  " + "\n  ".join(bad)
    return worst


@contextlib.contextmanager
def _precision(name):
    from focusflow_official_amd import ops
    prev = ops.conv_precision()
    ops.set_conv_precision(name)
    try:
        yield
    finally:
        ops.set_conv_precision(prev)


@contextlib.contextmanager
def _frozen(raft, on):
    try:
        if on:
            raft.update_block.freeze_self("parallel")
        yield
    finally:
        for p in raft.update_block.parameters():
            p.requires_grad_(True)


# name: (switches of train_loop / fn, _inputs arguments, fmaps differentiated, freeze_self("parallel") on the update block)
CASES = {
    "default": ({}, {}, True, False),
    "conv_by_conv_forward": ({"FUSED_FWD": False}, {}, True, False),
    "ungated": ({"DEFER_PARAM_GRADS": False}, {}, True, False),
    "one_stream": ({"WGRAD_SIDE_STREAM": False}, {}, True, False),
    "wchunk1": ({"WCHUNK": 1}, {}, True, False),
    "wchunk2": ({"WCHUNK": 2}, {}, True, False),
    "wchunk12": ({"WCHUNK": 12}, {}, True, False),
    "douts_spread_1e2": ({}, {"spread": 100.0}, True, False),
    "douts_spread_1e2_wchunk2": ({"WCHUNK": 2}, {"spread": 100.0}, True, False),
    "douts_last_only": ({}, {"present": [False, False, True]}, True, False),
    "douts_first_only": ({}, {"present": [True, False, False]}, True, False),
    "douts_middle_missing": ({}, {"present": [True, False, True]}, True, False),
    "frozen_encoder_and_gru": ({}, {}, True, True),
    "fmaps_without_grad": ({}, {}, False, False),
    "lookup_bwd_per_iteration": ({"_LOOKUP_BWD_ALL": False}, {}, True, False),
    "odd_planes_b3_flow_init": ({}, {"b": 3, "h": 17, "w": 19, "seed": 7, "flow_init": 12.0}, True, False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_update_loop_against_fp64_and_the_tape(raft, det_sd, case, monkeypatch):
    """The fused node under one switch setting against fp64, and against the per-operation tape on the same inputs; the
    tape against fp64 too."""
    from focusflow_official_amd import corr_block, train_loop
    switches, spec, grad_fmaps, frozen = CASES[case]
    for k, v in switches.items():
        monkeypatch.setattr(corr_block if k == "_LOOKUP_BWD_ALL" else train_loop, k, v)
    ins = _inputs(**spec)
    key = tuple(sorted((k, str(v)) for k, v in spec.items()))
    r64, r32 = _oracle(det_sd, key, ins, torch.float64), _oracle(det_sd, key, ins, torch.float32)
    with _frozen(raft, frozen):
        keys = _keys(raft, ins["T"], grad_fmaps)
        fused, route = _run(raft, ins, grad_fmaps)
        assert route == "UpdateLoopFnBackward", route
        if frozen:
            assert all(p.grad is None for p in raft.update_block.parameters() if not p.requires_grad)
            assert not any(k.startswith(("encoder.", "gru.")) for k in keys) and len(keys) > ins["T"] + 4
        with monkeypatch.context() as mp:
            mp.setattr(train_loop, "ENABLED", False)
            tape, route_t = _run(raft, ins, grad_fmaps)
        assert route_t != route
    _vs_fp64(fused, r32, r64, keys, f"{case}: fused node")
    _vs_fp64(tape, r32, r64, keys, f"{case}: tape")
    _vs(fused, tape, keys, f"{case}: fused node vs tape")


def test_update_loop_split_formats(raft, det_sd, monkeypatch):
    """W_F16 (plain fp16 operands: the node takes its conv-by-conv forward) within 3 x the tape's own error under W_F16;
    the tape under W_F32 (the route FF_CONV_PRECISION=fp32 trains on: the fused node does not take it) against fp64."""
    from focusflow_official_amd import train_loop
    ins = _inputs(seed=2)
    r64, r32 = _oracle(det_sd, "seed2", ins, torch.float64), _oracle(det_sd, "seed2", ins, torch.float32)
    keys = _keys(raft, ins["T"])
    with _precision("f16"):
        fused, route = _run(raft, ins)
        assert route == "UpdateLoopFnBackward", route
        monkeypatch.setattr(train_loop, "ENABLED", False)
        tape, _ = _run(raft, ins)
    monkeypatch.setattr(train_loop, "ENABLED", True)
    tape_err = {k: float((tape[k].double() - r64[k].double()).abs().max()) for k in keys}
    _vs_fp64(fused, r32, r64, keys, "W_F16: fused node", loose={k: 3 * e for k, e in tape_err.items()})
    print("W_F16: the tape's own max |tape - fp64| / max|fp64| = "
          f"{max(e / float(r64[k].abs().max()) for k, e in tape_err.items()):.2e}")
    with _precision("fp32"):
        tape32, route = _run(raft, ins)
    assert route != "UpdateLoopFnBackward"
    _vs_fp64(tape32, r32, r64, keys, "W_F32: tape")


def test_update_loop_at_the_gradient_scales_it_trains_at(raft, monkeypatch):
    """Every dout times 2^-30 (below the 2^-22 an element of a mean loss over a batch of eight 368 x 496 crops carries) and
    times 2^20: the backward is linear in the douts and the factor a power of two, so grads / s must equal the run at s = 1
    up to the atomics' summation order - 2e-5 of each tensor's maximum, the module's bound for two routes over identical
    inputs - and the predictions are the same bits.  Everything between the convolutions' gradient kernels rests on the
    max|g| words for this: a word that is never written (zero: scale one) or written from the wrong tensor passes at
    gradients near 2^0 and flushes the split halves to zero, or overflows them, here.  The fused node and the tape."""
    from focusflow_official_amd import train_loop
    base = _inputs()
    preds = [f"flow_up[{t}]" for t in range(base["T"])]
    gkeys = [k for k in _keys(raft, base["T"]) if k not in preds]
    for enabled in (True, False):
        monkeypatch.setattr(train_loop, "ENABLED", enabled)
        one, route = _run(raft, base)
        assert (route == "UpdateLoopFnBackward") == enabled, route
        for e in (-30, 20):
            s = 2.0 ** e
            got, _ = _run(raft, dict(base, douts=[d * s for d in base["douts"]]))
            assert all(torch.equal(got[k], one[k]) for k in preds), f"the predictions depend on the douts (2^{e})"
            assert all(got.get(k) is not None and bool(torch.isfinite(got[k]).all()) for k in gkeys), f"2^{e}: a gradient is missing or not finite"
            _vs({k: got[k] / s for k in gkeys}, one, gkeys, f"{'fused node' if enabled else 'tape'}: douts x 2^{e} vs x 1")


def test_update_loop_beyond_the_one_launch_lookup_backward(raft, monkeypatch):
    """T = 33 > ops.LOOKUP_BWD_ALL_MAX: the node scatters the lookup gradients iteration by iteration; against the tape."""
    from focusflow_official_amd import ops, train_loop
    T = ops.LOOKUP_BWD_ALL_MAX + 1
    ins = _inputs(T=T, seed=3)
    keys = _keys(raft, T)
    fused, route = _run(raft, ins)
    assert route == "UpdateLoopFnBackward", route
    monkeypatch.setattr(train_loop, "ENABLED", False)
    tape, _ = _run(raft, ins)
    _vs(fused, tape, keys, f"T={T}: fused node vs tape")


def test_chunked_corr_block_under_grad_mode(raft, monkeypatch):
    """Frozen feature encoder and a pyramid beyond corr_block._MAX_PYRAMID_BYTES: the block is built in batch chunks, the
    fused node declines it (no single pyramid) and the tape runs the loop.  Every lookup must hand convc1 a tensor of its own
    (the tape keeps it for the weight gradient): the gradients equal those of the unchunked block's run."""
    from focusflow_official_amd import corr_block, raft_net
    ins = _inputs(seed=5)
    keys = _keys(raft, ins["T"], grad_fmaps=False)
    made = []

    class Spy(corr_block.CorrBlock):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(raft_net, "CorrBlock", Spy)
    whole, route = _run(raft, ins, grad_fmaps=False)
    assert route == "UpdateLoopFnBackward" and made[-1]._chunks is None
    monkeypatch.setattr(corr_block, "_MAX_PYRAMID_BYTES", 1)      # one pair per chunk
    chunked, route = _run(raft, ins, grad_fmaps=False)
    assert route != "UpdateLoopFnBackward" and [(lo, hi) for lo, hi, _ in made[-1]._chunks] == [(0, 1), (1, 2)]
    _vs(chunked, whole, keys, "chunked pyramid (tape) vs one pyramid")


def test_autograd_grad_over_subsets_of_the_leaves(raft):
    """torch.autograd.grad over the update block's parameters only, over the encoder-side leaves only (the engine then prunes
    the LoopParamGate: nothing joins the weight-gradient side stream, its buffers are guarded by record_stream) and over
    everything: the same values as one .backward().  (This checks the values; it cannot show that the side stream's reads
    are race-free.)"""
    ins = _inputs(seed=6)
    params = [k for k, _ in raft.update_block.named_parameters()]
    full, _ = _run(raft, ins)
    for subset in (params, ["dinp", "dfmap1", "dfmap2"], list(GRAD_INPUTS) + params):
        got, route = _run(raft, ins, grad_of=subset)
        assert route == "UpdateLoopFnBackward"
        # (2e-6: two .backward() passes on identical inputs differ by up to 7.1e-7 of max - d fmap1; measured for autograd.grad
        # over these subsets: up to 8.8e-7)
        _vs(got, full, subset, f"autograd.grad over {len(subset)} leaves", tol=2e-6)
