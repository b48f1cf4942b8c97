"""Warm-start video inference: forward_interpolate on the device (csrc/warm_start.hip, ops.forward_interpolate), the
flow_init input of graph.GraphedForward and the session API warm_start.FlowSequence.

The reference is core/utils/utils.py:26-54 (scipy.griddata 'nearest'), recorded in tests/golden/warm_start.npz by
tests/golden/make_golden_warm_start.py.  For fresh inputs the tests use `brute_force_interpolate`, an fp64 brute force
that the generator showed equal to the reference on all 20 fixture cases (0 differing, 0 tied pixels of 71 680); scipy is
not needed on the GPU machine.  Exactness is bit equality: the output holds copies of input floats."""
import ctypes
import os
import re
import shutil
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_spec, load_golden

DEV = "cuda:0"
PLANES = [(14, 18), (46, 62), (48, 64), (68, 120)]
FLOWS = ["randn2", "randn8", "smooth6", "const", "zero"]
CASES = [f"{h}x{w}_{k}" for h, w in PLANES for k in FLOWS]
GRAPH_VS_EAGER = 2e-4      # px: test_hip_parity.test_hipgraph_replay_matches_eager (a captured single pair takes K splits)
HIP_VS_ORACLE = 1e-3       # px: the project's parity bound (test_hip_parity.test_model_matches_reference_vectors, flow_init case)


def brute_force_interpolate(flow, pixels=None):
    """utils.py:26-54 restated: fp64 landing points (int64 + float32, as numpy promotes), strict bounds, and for every grid
    pixel the kept vector with the smallest fp64 squared distance, the lowest source index on a tie.  Nothing lands: zeros
    (the reference: NaN).  flow (2,H,W) float32 -> (out (2,H,W), tied (H,W) bool: the minimum is attained more than once);
    with `pixels` (flat indices) only those: (2,P), (P,)."""
    flow = np.asarray(flow, np.float32)
    _, h, w = flow.shape
    y0, x0 = np.mgrid[0:h, 0:w]
    x1, y1 = (x0 + flow[0]).reshape(-1), (y0 + flow[1]).reshape(-1)      # float64
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h))
    pix = np.arange(h * w) if pixels is None else np.asarray(pixels)
    src, tied = np.zeros(pix.size, np.int64), np.zeros(pix.size, bool)
    for lo in range(0, pix.size if keep.size else 0, 512):
        q = pix[lo:lo + 512]
        dx, dy = (q % w)[:, None] - x1[keep][None], (q // w)[:, None] - y1[keep][None]
        d2 = dx * dx + dy * dy
        src[lo:lo + 512] = keep[d2.argmin(axis=1)]      # (argmin: the first = lowest source index)
        tied[lo:lo + 512] = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1
    out = flow.reshape(2, -1)[:, src] if keep.size else np.zeros((2, pix.size), np.float32)
    return (out.reshape(2, h, w), tied.reshape(h, w)) if pixels is None else (out, tied)


@pytest.fixture(scope="module")
def vectors():
    return load_golden("warm_start")


# ----------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    from focusflow_official_amd import _hip, build
    hdr = open(os.path.join(ROOT, "include", "focusflow_hip.h")).read()
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ("ff_forward_interpolate", "ff_forward_interpolate_ws"):
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), f"{name} is not declared in focusflow_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.EXPORTS
    assert "ff_forward_interpolate" in _hip._SIGS
    lib.ff_abi_version.restype = ctypes.c_int
    assert lib.ff_abi_version() == _hip.ABI_VERSION == 7 and "#define FF_ABI_VERSION 7" in hdr
    ws = _hip.load().ff_forward_interpolate_ws
    assert ws(1, 48, 64) > 0 and ws(8, 48, 64) == 8 * ws(1, 48, 64) and ws(1, 0, 64) == 0 and ws(1, 40000, 8) == 0


def test_cpu_tensor_raises():
    from focusflow_official_amd import ops, warm_start
    from focusflow_official_amd._hip import FocusFlowHipError
    assert warm_start.forward_interpolate is ops.forward_interpolate
    with pytest.raises(FocusFlowHipError):
        ops.forward_interpolate(torch.zeros(2, 6, 8))


def test_flow_sequence_refuses_training_mode():
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.warm_start import FlowSequence
    m = FF_RAFT_FUSION(use_fusion=None)
    m.train()
    with pytest.raises(ValueError):
        FlowSequence(m)
    seq = FlowSequence(m.eval(), graph=False)
    m.train()
    with pytest.raises(ValueError):
        seq(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_vectors(case, vectors):
    out, tied = brute_force_interpolate(vectors[case + "_in"])
    assert np.array_equal(out, vectors[case + "_out"]) and not tied.any()


def test_restatement_reproduces_the_older_fixture():
    g = load_golden("utils_padder")
    assert np.array_equal(brute_force_interpolate(g["fi_in"])[0], g["fi_out"])


@pytest.mark.parametrize("case", CASES)
def test_host_version_still_equals_reference_vectors(case, vectors):
    pytest.importorskip("scipy")
    from focusflow_official_amd.utils import forward_interpolate
    out = forward_interpolate(torch.from_numpy(vectors[case + "_in"]))
    assert out.device.type == "cpu" and np.array_equal(out.numpy(), vectors[case + "_out"])


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_warm_start_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "warm_start.hip"))
    assert len(kernels) >= 5, kernels
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"warm_start.hip: kernels with scratch (bytes per lane): {spilled}"


# ----------------------------------------------------------------------------
# 1-3: the kernel
# ----------------------------------------------------------------------------
def _fi(flow_np, **kw):
    from focusflow_official_amd import ops
    return ops.forward_interpolate(torch.from_numpy(np.ascontiguousarray(flow_np)).to(DEV), **kw).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_kernel_equals_reference_vectors(case, vectors):
    fin, ref = vectors[case + "_in"], vectors[case + "_out"]
    assert np.array_equal(_fi(fin), ref)                       # (2,H,W)
    assert np.array_equal(_fi(fin[None])[0], ref)              # (1,2,H,W)


@pytest.mark.gpu
@pytest.mark.parametrize("plane", PLANES)
def test_kernel_batch_is_per_sample(plane, vectors):
    from focusflow_official_amd import ops
    names = [f"{plane[0]}x{plane[1]}_{k}" for k in FLOWS]
    fin = torch.from_numpy(np.stack([vectors[n + "_in"] for n in names])).to(DEV)
    ref = np.stack([vectors[n + "_out"] for n in names])
    assert np.array_equal(ops.forward_interpolate(fin).cpu().numpy(), ref)
    # a non-contiguous view: the batch reversed and every sample inside a wider buffer
    wide = torch.full((len(names), 2, plane[0] + 3, plane[1] + 5), 7.0, device=DEV)
    wide[:, :, 1:-2, 2:-3] = fin
    view = wide.flip(0)[:, :, 1:-2, 2:-3]
    assert not view.is_contiguous()
    assert np.array_equal(ops.forward_interpolate(view).cpu().numpy(), ref[::-1])
    # out=: a given buffer, and in place
    out = torch.empty_like(fin)
    assert ops.forward_interpolate(fin, out=out) is out and np.array_equal(out.cpu().numpy(), ref)
    ops.forward_interpolate(fin, out=fin)
    assert np.array_equal(fin.cpu().numpy(), ref)


@pytest.mark.gpu
def test_kernel_known_answers():
    from focusflow_official_amd import ops
    h, w = 6, 8
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)

    def to(px, py):      # the flow that sends every pixel to (px, py): far out of frame by default
        return np.stack([px - xs, py - ys]).astype(np.float32)

    # nothing lands: zeros (the reference: NaN everywhere)
    assert np.array_equal(_fi(np.full((2, h, w), 1000.0, np.float32)), np.zeros((2, h, w), np.float32))
    # exactly one vector lands: the whole plane holds it
    f = to(-50.0, -50.0)
    f[:, 2, 3] = (1.25, -0.5)
    got = _fi(f)
    assert (got[0] == 1.25).all() and (got[1] == -0.5).all()
    # landing exactly on x1 == 0 or y1 == H is dropped, just inside is kept
    f = to(-50.0, -50.0)
    f[:, 1, 2] = (-2.0, 1.0)        # x1 = 0: dropped
    f[:, 4, 5] = (0.5, 2.0)         # y1 = 6 = H: dropped
    f[:, 3, 3] = (2.0, 0.25)        # lands at (5, 3.25)
    got = _fi(f)
    assert (got[0] == 2.0).all() and (got[1] == 0.25).all()
    # NaN / inf components are dropped, the rest of the plane is filled from the others
    rng = np.random.default_rng(5)
    f = (rng.standard_normal((2, 14, 18)) * 2).astype(np.float32)
    f[0, 3, 4], f[1, 5, 6], f[0, 7, 8], f[1, 9, 1] = np.nan, np.inf, -np.inf, np.nan
    ref, tied = brute_force_interpolate(f)
    got = _fi(f)
    assert not tied.any() and np.isfinite(got).all() and np.array_equal(got, ref)
    # an exact tie: sources (1,1) and (6,4) land at (2.5, 3) and (3.5, 3); from pixel (3, 3) both are 0.25 away (squared),
    # as from every pixel of column 3: the lower source index wins - five launches in a row and inside a replayed graph
    f = to(-50.0, -50.0)
    f[:, 4, 6] = (3.5 - 6.0, 3.0 - 4.0)
    f[:, 1, 1] = (2.5 - 1.0, 3.0 - 1.0)
    ref, tied = brute_force_interpolate(f)
    assert tied[:, 3].all() and tied.sum() == h and (ref[0, :, 3] == 1.5).all() and (ref[1, :, 3] == 2.0).all()
    assert (ref[0, :, 4:] == -2.5).all() and (ref[0, :, :3] == 1.5).all()
    dev = torch.from_numpy(f).to(DEV)
    for _ in range(5):
        assert np.array_equal(ops.forward_interpolate(dev).cpu().numpy(), ref)
    # ... and with the two sources exchanged, so that the winner is not "the one scattered first / last"
    f2 = to(-50.0, -50.0)
    f2[:, 1, 1] = (3.5 - 1.0, 3.0 - 1.0)
    f2[:, 4, 6] = (2.5 - 6.0, 3.0 - 4.0)
    ref2, _ = brute_force_interpolate(f2)
    assert (ref2[0, :, 3] == 2.5).all() and np.array_equal(_fi(f2), ref2)
    out = torch.empty_like(dev)
    ops.forward_interpolate(dev, out=out)      # (loads the kernels before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.forward_interpolate(dev, out=out)
    for _ in range(3):
        out.fill_(-1.0)
        graph.replay()
        assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.gpu
def test_kernel_large_planes():
    g = torch.Generator().manual_seed(77)
    f = (torch.randn(2, 136, 240, generator=g) * 4).numpy()
    ref, tied = brute_force_interpolate(f)
    assert not tied.any() and np.array_equal(_fi(f), ref)
    f = (torch.randn(2, 270, 480, generator=g) * 4).numpy()
    pix = np.random.default_rng(78).choice(270 * 480, size=2000, replace=False)
    ref, tied = brute_force_interpolate(f, pix)
    assert not tied.any() and np.array_equal(_fi(f).reshape(2, -1)[:, pix], ref)
    # few landed points, far apart: the search has to walk many rows (30 of 32 640 vectors stay in frame)
    f = np.full((2, 136, 240), 5000.0, np.float32)
    idx = np.random.default_rng(79).choice(136 * 240, size=30, replace=False)
    f.reshape(2, -1)[:, idx] = (torch.randn(2, 30, generator=g) * 3).numpy()
    ref, tied = brute_force_interpolate(f)
    assert not tied.any() and np.array_equal(_fi(f), ref)


# ----------------------------------------------------------------------------
# 4-6: the graph input, the session API, the oracle
# ----------------------------------------------------------------------------
def _cfg():
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))


def _ffraft(sd):
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg())
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def plain_model():
    from focusflow_official_amd import FF_RAFT_FUSION
    from oracle.weights import det_tensor
    m = FF_RAFT_FUSION(use_fusion=None)
    m.load_state_dict({k: det_tensor(k, s) for k, s, _ in golden_spec("state_dict_spec_plain")}, strict=True)
    return m.to(DEV).eval()


def _sequence(b, h, w, frames=4, seed=0, shift=(3, -5), n_points=500, smooth=4):
    """`frames` frames of one low-pass-filtered random image that moves by a further `shift` px per frame, plus noise
    (oracle.ffraft_ref.shifted_pair builds one pair this way), and a key-point mask per frame.  CPU tensors."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(b, 3, h // smooth + 2, w // smooth + 2, generator=g), size=(h, w), mode="bilinear", align_corners=False) * 255
    imgs, masks = [], []
    for k in range(frames):
        img = torch.roll(base, shifts=(shift[0] * k, shift[1] * k), dims=(2, 3))
        if k:
            img = img + torch.randn(b, 3, h, w, generator=g) * 2
        imgs.append(img.clamp(0, 255).contiguous())
        masks.append((torch.rand(b, 1, h, w, generator=g) < n_points / (h * w)).float() * 255)
    return imgs, masks


def _clone(pair):
    return [t.clone() for t in pair]


def _assert_equal(a, b, what):
    for x, y, n in zip(a, b, ("flow_low", "flow_up")):
        assert torch.equal(x, y), f"{what}: {n} max |diff| {float((x - y).abs().max()):.3e}"


def _assert_close(a, b, atol, what):
    for x, y, n in zip(a, b, ("flow_low", "flow_up")):
        err = float((x.double().cpu() - y.double().cpu()).abs().max())
        print(f"{what}: {n} max |diff| {err:.3e} (bound {atol:g})")
        assert err <= atol, f"{what}: {n} max |diff| {err:.3e} > {atol:g}"


@pytest.mark.gpu
def test_graph_flow_init_plain_bit_exact(plain_model):
    """B = 6 at 384 x 512 (test_plain_raft.test_plain_graph_replay): capture and eager run the same arithmetic."""
    from focusflow_official_amd.graph import GraphedForward
    from oracle import ffraft_ref as orc
    m = plain_model
    a = [t.to(DEV) for t in orc.shifted_pair(6, 384, 512, seed=31)[:2]] + [None, None]
    b = [t.to(DEV) for t in orc.shifted_pair(6, 384, 512, seed=32)[:2]] + [None, None]
    finit = (torch.randn(6, 2, 48, 64, generator=torch.Generator().manual_seed(33)) * 2).to(DEV)
    cold = GraphedForward(m, a, raft_iters=4)
    warm = GraphedForward(m, a, raft_iters=4, flow_init=True)
    assert cold.flow_init is None and warm.flow_init.shape == (6, 2, 48, 64) and not warm.flow_init.any()
    with pytest.raises(ValueError):
        cold(*b, flow_init=finit)
    cb = _clone(cold(*b))
    _assert_equal(cb, warm(*b), "zero flow_init buffer vs no flow_init")
    gi = _clone(warm(*b, flow_init=finit))
    with torch.no_grad():
        ei = m(*b, raft_iters=4, flow_init=finit, test_mode=True)
    _assert_equal(ei, gi, "graph vs eager, explicit flow_init")
    assert not torch.equal(gi[1], cb[1])
    _assert_equal(gi, warm(*b), "the buffer keeps its contents between replays")
    warm.reset()
    _assert_equal(cb, warm(*b), "after reset()")


@pytest.mark.gpu
def test_graph_flow_init_ffraft(det_sd):
    from focusflow_official_amd.graph import GraphedForward
    from oracle import ffraft_ref as orc
    m = _ffraft(det_sd)
    a = [t.to(DEV) for t in orc.shifted_pair(1, 128, 192, seed=31)]
    b = [t.to(DEV) for t in orc.shifted_pair(1, 128, 192, seed=32)]
    finit = (torch.randn(1, 2, 16, 24, generator=torch.Generator().manual_seed(34)) * 2).to(DEV)
    cold = GraphedForward(m, a, raft_iters=4)
    warm = GraphedForward(m, a, raft_iters=4, flow_init=True)
    _assert_equal(_clone(cold(*b)), warm(*b), "zero flow_init buffer vs no flow_init")
    gi = _clone(warm(*b, flow_init=finit))
    with torch.no_grad():
        ei = m(*b, raft_iters=4, flow_init=finit, test_mode=True)
    _assert_close(gi, ei, GRAPH_VS_EAGER, "graph vs eager, explicit flow_init")


@pytest.mark.gpu
def test_chain_plain_three_ways(plain_model):
    from focusflow_official_amd import ops
    from focusflow_official_amd.warm_start import FlowSequence
    m = plain_model
    imgs, _ = _sequence(6, 384, 512, seed=41)
    imgs = [t.to(DEV) for t in imgs]
    pairs = list(zip(imgs[:-1], imgs[1:]))

    def run(seq):
        return [_clone(seq(i1, i2)) for i1, i2 in pairs]

    graphed = FlowSequence(m, raft_iters=4, graph=True)
    first = run(graphed)
    graphed.reset()
    _assert_equal(first[0], graphed(*pairs[0]), "frame 0 after reset()")
    graphed.reset()
    again = run(graphed)
    eager = FlowSequence(m, raft_iters=4, graph=False)
    stepwise = run(eager)
    by_hand, finit = [], None
    with torch.no_grad():
        for i1, i2 in pairs:
            low, up = m(i1, i2, None, None, raft_iters=4, flow_init=finit, test_mode=True)
            finit = ops.forward_interpolate(low)
            by_hand.append([low.clone(), up.clone()])
    cold = FlowSequence(m, raft_iters=4, warm_start=False, graph=True)
    for t in range(len(pairs)):
        _assert_equal(by_hand[t], first[t], f"frame {t}: FlowSequence(graph=True) vs the hand-written loop")
        _assert_equal(by_hand[t], stepwise[t], f"frame {t}: FlowSequence(graph=False) vs the hand-written loop")
        _assert_equal(first[t], again[t], f"frame {t}: the sequence replayed a second time")
        c = cold(*pairs[t])
        assert torch.equal(c[1], first[t][1]) == (t == 0), f"frame {t}: a warm start changes every frame but the first"
    # a new shape: the graph is rebuilt and the sequence starts cold
    small = [t[:2, :, :128, :192].contiguous() for t in pairs[0]]
    got = _clone(graphed(*small))
    assert got[1].shape == (2, 2, 128, 192) and not graphed.flow_init.eq(0).all()
    _assert_equal(got, FlowSequence(m, raft_iters=4, graph=True)(*small), "rebuilt for 2 x 128 x 192 vs a new session")
    _assert_equal(first[0], graphed(*pairs[0]), "back at 6 x 384 x 512: frame 0 of a new sequence")


@pytest.mark.gpu
def test_chain_ffraft_point_frame_by_frame(det_sd):
    """A captured single pair takes K splits the eager forward does not, and a nearest-neighbour fill is discontinuous:
    every replay is compared against an eager forward given the very flow_init the graph's buffer held before it."""
    from focusflow_official_amd import ops
    from focusflow_official_amd.warm_start import FlowSequence
    m = _ffraft(det_sd)
    imgs, masks = _sequence(1, 128, 192, seed=42)
    imgs, masks = [t.to(DEV) for t in imgs], [t.to(DEV) for t in masks]
    pairs = [(imgs[k], imgs[k + 1], masks[k], masks[k + 1]) for k in range(3)]
    graphed = FlowSequence(m, raft_iters=4, graph=True)
    stepwise = FlowSequence(m, raft_iters=4, graph=False)
    finit = None
    for t, pair in enumerate(pairs):
        held = graphed.flow_init.clone() if t else None       # (the graph does not exist before the first call)
        got = _clone(graphed(*pair))
        with torch.no_grad():
            ref = m(*pair, raft_iters=4, flow_init=held, test_mode=True)
        _assert_close(got, ref, GRAPH_VS_EAGER, f"frame {t}: replay vs eager with the same flow_init")
        assert torch.equal(graphed.flow_init, ops.forward_interpolate(got[0])), f"frame {t}: the buffer holds the next initialisation"
        with torch.no_grad():
            low, up = m(*pair, raft_iters=4, flow_init=finit, test_mode=True)
            finit = ops.forward_interpolate(low)
        _assert_equal([low, up], stepwise(*pair), f"frame {t}: FlowSequence(graph=False) vs the hand-written loop")
        assert torch.equal(stepwise.flow_init, finit)
    assert float(held.abs().max()) > 1.0      # the initialisation is a real flow (the sequence moves by (3,-5) px per frame)


@pytest.mark.gpu
def test_chain_against_oracle_frame_by_frame(det_sd):
    """No compounding: per frame, (a) the kernel's output equals the brute force of the same HIP flow_low except where the
    brute force itself reports an exactly tied minimum (at most 0.1 % of the plane), (b) the oracle given that flow_init
    agrees with the HIP forward given the same flow_init within the parity bound."""
    from focusflow_official_amd import ops
    from oracle import ffraft_ref as orc
    m = _ffraft(det_sd)
    imgs, masks = _sequence(1, 128, 192, seed=43)
    finit = None
    for t in range(3):
        inp = (imgs[t], imgs[t + 1], masks[t], masks[t + 1])
        with torch.no_grad():
            low, up = m(*[x.to(DEV) for x in inp], raft_iters=4, flow_init=finit, test_mode=True)
            ref_low, ref_up = orc.ffraft_forward(det_sd, *inp, raft_iters=4, flow_init=None if finit is None else finit.cpu(), test_mode=True)
        _assert_close([low, up], [ref_low, ref_up], HIP_VS_ORACLE, f"frame {t}: HIP vs oracle with the same flow_init")
        finit = ops.forward_interpolate(low)
        ref, tied = brute_force_interpolate(low[0].cpu().numpy())
        got = finit[0].cpu().numpy()
        print(f"frame {t}: {int(tied.sum())} tied pixels of {tied.size}, {int((got != ref).any(axis=0).sum())} differ")
        assert tied.mean() <= 1e-3, f"frame {t}: {int(tied.sum())} tied pixels of {tied.size}"
        assert np.array_equal(got[:, ~tied], ref[:, ~tied]), f"frame {t}: kernel vs brute force outside ties"
