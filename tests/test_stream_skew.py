"""The hand-made stream forks and joins of the product under skewed timing (tests/stream_skew.py): every case runs once on ONE
stream (ops.policy.single_stream, WGRAD_SIDE_STREAM off, FF_TRAIN_STREAMS=0: the same kernels at the same launch shapes) and
once with its streams on while a delay sits behind every fork (side_late), behind every event recorded on the main stream
(main_late) or in front of the backward nodes autograd replays on the side streams (replay_late).  At these sizes a step is
host-bound: without the delays every kernel has finished before the next is enqueued and no event matters.

Before every skewed run the same pass runs unskewed on other inputs (with the hooks counting: that is where the number of
delays, and from it their length, comes from), so a buffer read before it is written holds another pair's values.  Every
skewed run asserts that it took at least the reference's time plus half of all queued delays.

Bounds.  Inference: the single-stream reference run twice on the same inputs (A, B, A) is bit-identical -> torch.equal; were
it not, 4 x that spread, at most 1e-4 px (test_hip_split.py's bound for two routes of one arithmetic).  Update loop alone:
2e-5 x max|ref| per tensor (test_update_loop.py's fused-vs-tape bound).  Whole step: per tensor max(4 x d0, 2e-6) x max|ref|,
d0 that tensor's own spread between two reference runs (step 1: reference runs from the skewed run's own parameters).

Measured on an MI355X (delays: number x length; "on main": elapsed on the main stream, reference -> skewed):
  self-test: with every wait right in all three modes; join wait left out under side_late: the stale fill; fork wait left
    out under main_late: round 1's value in round 2.  WITHOUT delays both omissions read the right values - the premise.
  inference (reference run twice: bit-identical; every skewed run torch.equal to it):
    FF-RAFT f16x3      side_late 16 x 3.8 ms (cce.py:810 x8, cce.py:816 x4, update_block.py:179 x3, raft_net.py:121), 3.8 -> 59.7 ms;
                       main_late  9 x 3.8 ms, 3.8 -> 36.2 ms;   f16 side_late 16 x 3.4 ms, 3.3 -> 52.5 ms
    alternate_corr     side_late 16 x 3.9 ms, 3.9 -> 60.7 ms;   main_late 9 x 3.9 ms, -> 37.2 ms
    plain RAFT         side_late  4 x 2.3 ms, 2.3 -> 10.6 ms;   main_late 5 x 2.3 ms, -> 13.0 ms
    two forwards       side_late 32 x 6.4 ms, 6.4 -> 195.8 ms;  main_late 18 x 6.4 ms, -> 118.3 ms
  update loop alone (fraction of each tensor's maximum, largest over all keys; bound 2e-5):
    gated WCHUNK 4     side_late 1 x 8.2 ms 5.5e-7;  main_late 2 x 8.2 ms 6.4e-7       ungated  5.8e-7 / 6.4e-7
    WCHUNK 1           side_late 3 x 8.2 ms 6.1e-7;  main_late 4 x 8.2 ms 6.2e-7       tape: main_late 1 x 8.2 ms 6.4e-7 (side_late:
    douts, middle missing  7.6e-7 / 6.1e-7                                              the tape forks nothing - asserted)
    pruned gate        side_late 1 x 6.2 ms, 44 canaries (70.7 MB, largest 5.3 MB) untouched, d net0 / d inp 3.3e-7
  whole step, two steps (516 tensors; 87 - 110 ms on one stream):
    side_late, encoder stream only 228 x 7.9 ms -> 1837 ms; branch streams only 198 x 9.1 ms -> 1839 ms (fn.py:95 and :76, the
    zero arena's and the max|.| words' ready event, are 180 - 224 of them); main_late 15 x 20 ms -> 339 ms; replay_late 6 x 20 ms
    -> 178 ms.  With every stream live side_late queued 342 x 5.3 ms and main saw 856 ms of the 988 ms it needed (two chains
    side by side): hence the two variants.
    Step 0 (against the two one-stream runs of the whole pass) is within max(4 x d0, 2e-6) in every variant.  Step 1 is
    compared with the one-stream step from the parameters the skewed run's own step 1 started from (_against_one_stream):
    against the shared reference it cannot be, because every run's step-0 gradients differ in their last bits (254 of 258
    tensors between two one-stream runs: the weight-gradient atomics), the update carries single last-bit differences into the
    parameters, and the test weights turn those into discrete jumps - pred[0] of step 1 lands 0, 5.3e-7, 2.1e-6, 2.2e-6,
    5.0e-6 or 5.12e-6 of its maximum away, between two ONE-STREAM runs as between any two configurations (measured over seven
    configurations run twice each).  A race reads another batch's values, O(1) of a tensor's maximum: the largest d0 of a
    tensor with a gradient that is not noise around zero is 1.2e-5, five decades below.  (The biases in front of an
    InstanceNorm have a zero gradient in exact arithmetic: theirs is all noise, d0 up to 2.0 of their maximum, and
    the bound follows it.)
  a caller's stream, the default stream held (three streams: see _on_own_stream): FF-RAFT 11 x 3.9 ms, held 94 ms, pass 45 ms, equal bits; the training step 21 x 15 ms, held 830 ms, pass 366 ms; FF-PWC forks
    nothing, equal bits; video session 32 x 7.5 ms, held 492 ms, pass 242 ms, equal bits, the detector's second workspace made.
"""
import contextlib
from argparse import Namespace

import pytest
import torch

import stream_skew as ss
from oracle import ffraft_ref as orc

gpu = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, ITERS = 2, 128, 192, 3
PAIR_A, PAIR_B, PAIR_WARM = dict(seed=21, shift=(3, -5)), dict(seed=22, shift=(-4, 2)), dict(seed=23, shift=(2, 6))
PAIR_WARM2 = dict(seed=24, shift=(1, -7))
LR = 1e-4
PX_CAP = 1e-4
_REF = {}       # references, computed once and left unchanged

# ----------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------
def test_harness_installs_and_removes_its_hooks(monkeypatch):
    before = (torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream, torch.cuda.Event.record)
    with ss.Skew(monkeypatch, None, "count") as sk:
        inside = (torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream, torch.cuda.Event.record)
        assert all(a is not b for a, b in zip(before, inside))
        assert ss._orig(torch.cuda.Stream, "wait_event") is before[0] and ss._orig(torch.cuda.Event, "record") is before[2]
    assert (torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream, torch.cuda.Event.record) == before
    assert sk.count == sk.records == sk.refused == 0
    with pytest.raises(AssertionError):
        ss.Skew(monkeypatch, None, "side_late", delay_ms=ss.MAX_MS + 1)
    with pytest.raises(AssertionError):
        ss.Skew(monkeypatch, None, "sideways")


def test_delay_clamp_and_budget():
    assert ss.clamp_delay(0.3) == ss.MIN_MS and ss.clamp_delay(7.5) == 7.5 and ss.clamp_delay(300.0) == ss.MAX_MS
    assert ss.clamp_delay(300.0, n=12) == ss.MAX_MS                     # a dozen forks: 240 ms
    assert ss.clamp_delay(300.0, n=300) == pytest.approx(0.9 * ss.BUDGET_MS / 300)
    assert ss.clamp_delay(300.0, n=5000) == ss.MIN_MS                   # (the run then refuses what goes beyond the budget)
    assert 300 * ss.clamp_delay(300.0, n=300) <= ss.BUDGET_MS


# ----------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------
def _cfg():
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))


def _pair(seed, shift, b=B):
    return [t.to(DEV) for t in orc.shifted_pair(b, H, W, seed=seed, shift=shift)]


@contextlib.contextmanager
def _one_stream():
    from focusflow_official_amd import ops
    prev, ops.policy.single_stream = ops.policy.single_stream, True
    try:
        yield
    finally:
        ops.policy.single_stream = prev


@contextlib.contextmanager
def _precision(name):
    from focusflow_official_amd import ops
    prev = ops.conv_precision()
    ops.set_conv_precision(name)
    try:
        yield
    finally:
        ops.set_conv_precision(prev)


def _skewed(monkeypatch, mode, run, warm, ref_gpu_ms, ref_wall_ms, what):
    """warm(c) unskewed on the current stream with the hooks counting, then run(sk) under `mode` -> (run's result, the Skew);
    (None, the counting Skew) where the pass has nothing that `mode` delays."""
    main = torch.cuda.current_stream()
    with ss.Skew(monkeypatch, main, "count") as c:
        warm(c)
    torch.cuda.synchronize()
    n = {"side_late": c.count, "main_late": c.records, "replay_late": c.replays}[mode]
    if n == 0:
        return None, c
    d = ss.clamp_delay(ref_wall_ms, n)
    with ss.Skew(monkeypatch, main, mode, d) as sk, ss.Timed(main) as t:
        out = run(sk)
    ss.assert_skewed(sk, t.gpu_ms, ref_gpu_ms, what)
    return out, sk


def _same_or_within(got, ref, ref_again, what):
    """Lists of CPU tensors.  Bit-identical reference runs -> torch.equal; else 4 x their spread, at most PX_CAP."""
    spread = max(float((a.double() - b.double()).abs().max()) for a, b in zip(ref, ref_again))
    diff = max(float((a.double() - b.double()).abs().max()) for a, b in zip(got, ref))
    print(f"{what}: reference spread {spread:.3e}, skewed - reference {diff:.3e}")
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(got, ref)) and len(got) == len(ref)
    if spread == 0.0:
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), f"{what}: differs from the one-stream run by {diff:.3e} (whose two runs are bit-identical)"
    else:
        assert diff <= min(4 * spread, PX_CAP), f"{what}: {diff:.3e} against a reference spread of {spread:.3e}"


# ----------------------------------------------------------------------------
# 2. the harness itself: plain torch ops, both outcomes
# ----------------------------------------------------------------------------
STALE, ROUNDS, N_EL = -1.0, 2, 1 << 20


def _fork_join(side, fork_wait=True, join_wait=True, sk=None):
    """ROUNDS times: main fills src with the round's number, forks; side copies src into x, main joins and copies x.
    -> (min, max) of what main's copy holds, per round."""
    main = torch.cuda.current_stream()
    src = torch.full((N_EL,), STALE, device=DEV)
    x = torch.full((N_EL,), STALE, device=DEV)
    torch.cuda.synchronize()
    if sk is not None and sk.mode in ("replay_late", "count"):
        sk.replay_late([side])
    outs = []
    for r in range(1, ROUNDS + 1):
        src.fill_(float(r))
        fork = torch.cuda.Event()
        fork.record(main)
        with torch.cuda.stream(side):
            if fork_wait:
                side.wait_event(fork)
            x.copy_(src)
            join = torch.cuda.Event()
            join.record(side)
        if join_wait:
            main.wait_event(join)
        outs.append(x.clone())
    torch.cuda.synchronize()
    return [(float(o.min()), float(o.max())) for o in outs]


@gpu
def test_harness_delays_create_the_skew_they_claim(monkeypatch):
    side = torch.cuda.Stream()
    _fork_join(side)      # (warm: the fill / copy kernels are loaded)
    with ss.Timed() as ref:
        assert _fork_join(side) == [(1.0, 1.0), (2.0, 2.0)]
    want = [(float(r), float(r)) for r in range(1, ROUNDS + 1)]
    for mode in ("side_late", "main_late", "replay_late"):
        got, sk = _skewed(monkeypatch, mode, lambda sk: _fork_join(side, sk=sk), lambda c: _fork_join(side, sk=c), ref.gpu_ms, 5.0, f"self-test {mode}")
        assert got == want, f"{mode} with every wait in place: {got}"
        assert sk.count == (1 if mode == "replay_late" else ROUNDS), sk.report()
        assert all(s == "replay_late" or s.startswith("test_stream_skew.py:") for s in sk.sites), sk.report()      # the per-site label
    # the join wait left out of THIS test's code: under side_late main copies x before the late side stream has written it
    with ss.Skew(monkeypatch, torch.cuda.current_stream(), "side_late", 5.0) as sk:
        got = _fork_join(side, join_wait=False)
    assert sk.count == ROUNDS and got == [(STALE, STALE)] * ROUNDS, got
    # the fork wait left out: under main_late the side stream copies src before main, held up behind round 1's record, has
    # written round 2's value (round 1's fill has no delay in front of it: not asserted)
    with ss.Skew(monkeypatch, torch.cuda.current_stream(), "main_late", 5.0) as sk:
        got = _fork_join(side, fork_wait=False)
    assert sk.count == ROUNDS and got[1] != (2.0, 2.0), got
    # and neither omission shows without the delays on an idle card - which is why the other tests of this module need them
    print("self-test without delays, join / fork wait left out:", _fork_join(side, join_wait=False), _fork_join(side, fork_wait=False))


# ----------------------------------------------------------------------------
# 3. inference
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(det_sd):
    import test_alt_corr
    import test_hip_parity
    from conftest import golden_spec
    from focusflow_official_amd import FF_RAFT_FUSION
    from oracle.weights import det_tensor
    plain = FF_RAFT_FUSION(use_fusion=None)
    plain.load_state_dict({k: det_tensor(k, s) for k, s, _ in golden_spec("state_dict_spec_plain")}, strict=True)
    return {"ffraft": test_hip_parity._model(det_sd), "alt_corr": test_alt_corr._model(det_sd, alternate_corr=True), "plain": plain.to(DEV).eval()}


def _forwards(model, pairs):
    """The forwards back to back, nothing synchronised between them; then the copies -> [flow_low, flow_up, ...] on the CPU."""
    with torch.no_grad():
        outs = [model(*p, raft_iters=ITERS, test_mode=True) for p in pairs]
    return [t.cpu() for o in outs for t in o]


def _infer_ref(models, kind, precision):
    key = ("infer", kind, precision)
    if key not in _REF:
        m = models[kind]
        a, b = _pair(**PAIR_A), _pair(**PAIR_B)
        with _one_stream(), _precision(precision):
            _forwards(m, [a])        # (the first forward on these weights reads its range words on the host; kernels load)
            with ss.Timed() as t:
                ra = _forwards(m, [a])
            rb = _forwards(m, [b])
            ra2 = _forwards(m, [a])
            with ss.Timed() as t2:
                _forwards(m, [a, b])
        _REF[key] = dict(a=ra, b=rb, a2=ra2, one=(t.gpu_ms, t.wall_ms), two=(t2.gpu_ms, t2.wall_ms))
    return _REF[key]


INFER_CASES = [(k, p, m) for k, p in (("ffraft", "f16x3"), ("alt_corr", "f16x3"), ("plain", "f16x3"), ("ffraft_twice", "f16x3"))
               for m in ("side_late", "main_late")] + [("ffraft", "f16", "side_late")]
FORK_FILES = {"ffraft": {"raft_net.py", "cce.py", "update_block.py"}, "alt_corr": {"raft_net.py", "cce.py", "update_block.py"},
              "plain": {"raft_net.py", "update_block.py"}}


@gpu
@pytest.mark.parametrize("kind,precision,mode", INFER_CASES, ids=lambda v: str(v))
def test_inference_under_skew(models, kind, precision, mode, monkeypatch):
    from focusflow_official_amd import raft_net
    monkeypatch.setattr(raft_net, "_STREAMS_MIN_PIXELS", 0)
    twice = kind.endswith("_twice")
    net = kind.split("_twice")[0]
    m, ref = models[net], _infer_ref(models, net, precision)
    pairs = [_pair(**PAIR_A), _pair(**PAIR_B)] if twice else [_pair(**PAIR_A)]
    warm = [_pair(**PAIR_WARM), _pair(**PAIR_WARM2)] if twice else [_pair(**PAIR_WARM)]      # (never a pair the skewed pass expects)
    gpu_ms, wall_ms = ref["two" if twice else "one"]
    what = f"inference {kind} {precision} {mode}"
    with _precision(precision):
        got, sk = _skewed(monkeypatch, mode, lambda sk: _forwards(m, pairs), lambda c: _forwards(m, warm), gpu_ms, wall_ms, what)
    files = {s.split(":")[0] for s in sk.sites}
    assert FORK_FILES[net] <= files, f"{what}: no delay at a fork of {FORK_FILES[net] - files}"
    _same_or_within(got, ref["a"] + (ref["b"] if twice else []), ref["a2"] + (ref["b"] if twice else []), what)


# ----------------------------------------------------------------------------
# 4a / 4b. the recorded update loop alone
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raft(det_sd):
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg())
    m.load_state_dict(det_sd, strict=True)
    return m.to(DEV).train().flow_net


LOOP_INPUTS = {"all": {}, "middle_missing": {"present": [True, False, True]}}
# name: (switches of train_loop, inputs)
LOOP_CASES = {
    "gated_wchunk4": ({"WCHUNK": 4}, "all"),
    "ungated": ({"DEFER_PARAM_GRADS": False}, "all"),
    "wchunk1": ({"WCHUNK": 1}, "all"),
    "tape": ({"ENABLED": False}, "all"),
    "douts_middle_missing": ({}, "middle_missing"),
}


def _loop_ref(raft, which, monkeypatch, grad_of=None):
    import test_update_loop as ul
    from focusflow_official_amd import train_loop
    key = ("loop", which, tuple(grad_of or ()))
    if key not in _REF:
        ins = ul._inputs(**LOOP_INPUTS[which])
        warm = ul._inputs(seed=8, **LOOP_INPUTS[which])
        with monkeypatch.context() as mp:
            mp.setattr(train_loop, "WGRAD_SIDE_STREAM", False)
            ul._run(raft, ins, grad_of=grad_of)
            with ss.Timed() as t:
                out, route = ul._run(raft, ins, grad_of=grad_of)
        assert route == "UpdateLoopFnBackward"
        _REF[key] = dict(ins=ins, warm=warm, out=out, gpu_ms=t.gpu_ms, wall_ms=t.wall_ms)
    return _REF[key]


@gpu
@pytest.mark.parametrize("mode", ["side_late", "main_late"])
@pytest.mark.parametrize("case", list(LOOP_CASES))
def test_update_loop_under_skew(raft, case, mode, monkeypatch):
    import test_update_loop as ul
    from focusflow_official_amd import train_loop
    switches, which = LOOP_CASES[case]
    ref = _loop_ref(raft, which, monkeypatch)
    for k, v in switches.items():
        monkeypatch.setattr(train_loop, k, v)
    assert train_loop.WGRAD_SIDE_STREAM
    what = f"update loop {case} {mode}"
    got, sk = _skewed(monkeypatch, mode, lambda sk: ul._run(raft, ref["ins"]), lambda c: ul._run(raft, ref["warm"]), ref["gpu_ms"], ref["wall_ms"], what)
    if got is None:
        # the per-operation tape forks nothing in a pass without encoders: there is no wait on a side stream to delay
        assert (case, mode) == ("tape", "side_late"), f"{what}: nothing to delay ({sk.report()})"
        return
    out, route = got
    assert (route == "UpdateLoopFnBackward") == (case != "tape")
    if case != "tape":
        assert any(s.startswith("train_loop.py:") for s in sk.sites), sk.report()
    ul._vs(out, ref["out"], ul._keys(raft, ref["ins"]["T"]), what)


def _run_pruned(raft, ins, sizes):
    """test_update_loop._run for torch.autograd.grad over net0 and inp only, as RAFT.forward leaves things: nothing outside the
    graph holds the gate's mailbox, so the graph's end frees the slabs' buffers - and BEFORE any synchronisation canaries of
    the sizes in `sizes` (filled in by the spy on train_loop._tensors) are allocated on the main stream and painted.
    -> ({dnet0, dinp} on the CPU, the canaries that changed)."""
    from focusflow_official_amd import cce, fn, ops

    def dev(t, grad):
        return t.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(grad)

    net0, inp, f1, f2 = dev(ins["net0"], True), dev(ins["inp"], True), dev(ins["fmap1"], False), dev(ins["fmap2"], False)
    b, h, w, _ = net0.shape
    douts = [d.to(DEV) for d in ins["douts"]]
    for p in raft.update_block.parameters():
        p.grad = None
    ops.begin_forward(DEV)
    fn.begin_graph(DEV)
    cce.prepack(raft, DEV)
    try:
        gate = raft._loop_gate(raft._fused_train())
        assert gate is not None
        coords1 = ops.coords_init(b, h, w, net0, None)
        preds = raft._update_loop(net0, inp, f1, f2, coords1, ins["T"], gate)
    finally:
        fn.end_graph()
    del gate
    assert type(preds[0].grad_fn).__name__ == "UpdateLoopFnBackward"
    loss = sum((p * d).sum() for p, d in zip(preds, douts))
    del sizes[:]
    torch.cuda.synchronize()
    dnet0, dinp = torch.autograd.grad(loss, [net0, inp])
    del preds, loss           # the graph, the node and the mailbox go; the side stream has not started on the slabs yet
    canaries = [torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV) for n in sizes]
    assert canaries, "the spy saw no buffers: the gated branch of UpdateLoopFn.backward was not taken"
    torch.cuda.synchronize()
    changed = [i for i, c in enumerate(canaries) if not bool((c == 0xA5).all())]
    return {"dnet0": dnet0.permute(0, 3, 1, 2).cpu(), "dinp": dinp.permute(0, 3, 1, 2).cpu()}, changed


@gpu
def test_pruned_gate_leaves_the_slabs_their_buffers(raft, monkeypatch):
    """torch.autograd.grad over net0 and inp prunes the LoopParamGate: nobody waits for the weight-gradient slabs, which start
    late here (side_late).  Their stacks, gradient stacks, max|g| words and sums (every storage train_loop._tensors hands to
    record_stream, sizes taken by a spy) must not be handed out again while the side stream works: canaries of exactly those
    sizes, allocated on the main stream right behind the backward, stay as painted, and d net0 / d inp equal the one-stream
    run's.  (Whether the allocator WOULD hand those blocks back without the record_stream calls is its best-fit choice among
    the blocks just freed - same sizes, same stream, nothing else free of those sizes in a warmed process: likely, not
    guaranteed.  The gradient comparison does not depend on it.)"""
    import test_update_loop as ul
    from focusflow_official_amd import train_loop
    keys = ["dnet0", "dinp"]
    ref = _loop_ref(raft, "all", monkeypatch, grad_of=keys)
    sizes, inner = [], train_loop._tensors

    def spy(obj):
        out = inner(obj)
        sizes.extend(t.numel() * t.element_size() for t in out)
        return out

    monkeypatch.setattr(train_loop, "_tensors", spy)
    main = torch.cuda.current_stream()
    with ss.Skew(monkeypatch, main, "count") as c:
        _run_pruned(raft, ref["warm"], sizes)
    assert c.count > 0
    d = ss.clamp_delay(ref["wall_ms"], c.count)
    with ss.Skew(monkeypatch, main, "side_late", d) as sk, ss.Timed(main, before_end=sk.join_delayed) as t:
        got, changed = _run_pruned(raft, ref["ins"], sizes)
    # (the clock on main stops behind a join of the test's own: the product joins nobody here, which is the point)
    ss.assert_skewed(sk, t.gpu_ms, ref["gpu_ms"], "pruned gate side_late")
    print(f"pruned gate: {len(sizes)} canaries, {sum(sizes) / 1e6:.1f} MB, largest {max(sizes) / 1e6:.2f} MB")
    assert len(sizes) >= 4 and not changed, f"canaries {changed} of sizes {[sizes[i] for i in changed]} were written by a late slab"
    ul._vs(got, ref["out"], keys, "pruned gate side_late")


# ----------------------------------------------------------------------------
# 4c. the whole training step
# ----------------------------------------------------------------------------
def _gt(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 2, H, W, generator=g) * 5).to(DEV)


def _train_model(det_sd):
    from focusflow_official_amd import FF_RAFT_FUSION
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg())
    m.load_state_dict(det_sd, strict=True)
    m = m.to(DEV).train()
    m.flow_net.freeze_bn()
    return m


def _train_steps(m, batches, before_backward=None, first=0):
    """A step per batch with an SGD update behind each -> {name: CPU tensor}: the loss, every prediction and every
    parameter's gradient of every step, numbered from `first`, and under "after{step}:" the model's state behind the update
    (copied on the running stream, nothing synchronised)."""
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    valid = torch.ones(B, H, W, device=DEV)
    keep = {}
    for step, (pair, flow_gt) in enumerate(batches, first):
        preds = m(*pair, raft_iters=ITERS)
        loss, _ = orc.sequence_l1(preds, flow_gt, valid)
        opt.zero_grad(set_to_none=True)
        if before_backward is not None:
            before_backward(m)
        loss.backward()
        keep[f"step{step}.loss"] = loss.detach()
        keep.update({f"step{step}.pred[{i}]": p.detach() for i, p in enumerate(preds)})
        missing = [k for k, p in m.named_parameters() if p.grad is None]
        assert not missing, missing[:4]
        keep.update({f"step{step}.grad:{k}": p.grad.clone() for k, p in m.named_parameters()})
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)      # (as test_two_training_steps_...: the test weights' gradients are large)
        opt.step()
        keep.update({f"after{step}:{k}": v.detach().clone() for k, v in m.state_dict().items()})
    return {k: v.cpu() for k, v in keep.items()}


def _against_one_stream(det_sd, got, ref, monkeypatch, what):
    """Step 0 against the two one-stream runs of _train_ref.  Step 1 against the one-stream step FROM THE PARAMETERS `got`'s
    own step 1 started from (its state behind the first update, loaded into a fresh model; run twice for d0): every run's
    step-0 gradients differ from every other's in their last bits - the weight-gradient atomics, two one-stream runs alike -
    and behind the update the ill-conditioned test weights turn single last-bit differences of parameters into steps of
    5e-7 .. 5e-6 of a prediction's maximum and 1e-4 of a gradient's.  Two one-stream runs land 0 to 5.1e-6 apart in
    pred[0] of step 1, in a handful of discrete values, so one pair's spread says nothing about the next run's distance.
    From equal parameters step 1 is what step 0 is: the same kernels on the same operands, up to the atomics' order."""
    from focusflow_official_amd import train_loop
    start = {k[len("after0:"):]: v for k, v in got.items() if k.startswith("after0:")}
    assert set(start) == set(det_sd)
    moved = max(float((start[k] - det_sd[k]).abs().max()) for k in start if start[k].dtype.is_floating_point)
    assert moved > 0, "the update between the steps moved no parameter"
    _first_update(start, got, ref, what)
    with monkeypatch.context() as mp, _one_stream():
        mp.setenv("FF_TRAIN_STREAMS", "0")
        mp.setattr(train_loop, "WGRAD_SIDE_STREAM", False)
        one, again = (_train_steps(_train_model(start), _batches()[1:], first=1) for _ in range(2))
    plain = lambda d: {k: v for k, v in d.items() if not k.startswith("after")}      # noqa: E731
    step0 = lambda d: {k: v for k, v in plain(d).items() if k.startswith("step0.")}      # noqa: E731
    step1 = {k: v for k, v in plain(got).items() if k.startswith("step1.")}
    assert len(step1) == len(step0(got)) == len(plain(one)) > 250
    _vs_own_spread(step0(got), step0(ref["out"]), step0(ref["again"]), what + ", step 0")
    _vs_own_spread(step1, plain(one), plain(again), what + ", step 1 from its own parameters")
    # the parameters behind the second update, too: the optimiser read what the backward wrote
    after = lambda d: {k: v for k, v in d.items() if k.startswith("after1:") and v.dtype.is_floating_point}      # noqa: E731
    _vs_own_spread(after(got), after(one), after(again), what + ", parameters behind step 1")


def _batches(warm=False):
    if warm:
        return [(_pair(**PAIR_WARM), _gt(33)), (_pair(**PAIR_WARM2), _gt(34))]
    return [(_pair(**PAIR_A), _gt(31)), (_pair(**PAIR_B), _gt(32))]


def _train_ref(det_sd, monkeypatch):
    from focusflow_official_amd import train_loop
    if "train" not in _REF:
        with monkeypatch.context() as mp, _one_stream():
            mp.setenv("FF_TRAIN_STREAMS", "0")
            mp.setattr(train_loop, "WGRAD_SIDE_STREAM", False)
            r0 = _train_steps(_train_model(det_sd), _batches())
            m = _train_model(det_sd)
            with ss.Timed() as t:
                r1 = _train_steps(m, _batches())
        _REF["train"] = dict(out=r1, again=r0, gpu_ms=t.gpu_ms, wall_ms=t.wall_ms, init={k: v.clone() for k, v in det_sd.items()})
    return _REF["train"]


def _first_update(start, got, ref, what):
    """The parameters behind the FIRST update (what step 1 starts from) against the one-stream run's.  p' = p - LR c g with the
    clip factor c = min(1, 1 / |all g|) <= 1, so two runs' p' differ by LR |c g - c' g'| <= LR (|g - g'| + |c - c'| |g'|), and
    |c - c'| <= the relative difference of the norms <= the gradients' own relative bound: at most
    2 LR max(4 x d0, 2e-6) max|g_ref| for gradients within their bound of step 0 (d0: that gradient's spread between the two
    one-stream runs), plus one fp32 rounding of the subtraction on either side, 2^-23 max|p|.  Buffers must be equal."""
    bad, informative, n = [], 0, 0
    for k, p in start.items():
        want = ref["out"]["after0:" + k]
        if "step0.grad:" + k not in ref["out"]:
            # a buffer - or the second name of a module that has two (its parameters are compared under the first)
            if torch.equal(want, ref["init"][k]):
                assert torch.equal(p, want), f"{what}: the buffer {k} changed"
            continue
        g, g2 = ref["out"]["step0.grad:" + k], ref["again"]["step0.grad:" + k]
        gmax = float(g.abs().max())
        d0 = float((g2 - g).abs().max()) / gmax if gmax else 0.0
        tol = 2 * LR * max(4 * d0, 2e-6) * gmax + 2.0 ** -23 * float(want.abs().max())
        err = float((p - want).abs().max())
        n += 1
        informative += float((want - ref["init"][k]).abs().max()) > 4 * tol      # an update left out would show here
        if not err <= tol:
            bad.append(f"{k}: {err:.2e}, bound {tol:.2e}")
    print(f"{what}, parameters behind step 0: {n} tensors, in {informative} of them the update itself is above 4 x the bound")
    assert informative >= 1 and not bad, f"{what}: {len(bad)} parameters behind the first update\n  " + "\n  ".join(bad[:12])


def _vs_own_spread(got, ref, again, what):
    """Every tensor within max(4 x d0, 2e-6) of its maximum, d0 its own spread between the two reference runs."""
    bad, worst_d0, worst = [], 0.0, (0.0, None)
    quiet = [0.0, 0.0, 0]        # over the tensors whose d0 is below 1e-3 (not noise around a zero gradient): largest d0, largest error, how many
    assert set(got) == set(ref)
    for k, want in ref.items():
        scale = float(want.abs().max())
        if scale == 0.0:
            assert not got[k].any(), f"{what}: {k} is zero on one stream"
            continue
        d0 = float((again[k] - want).abs().max()) / scale
        err = float((got[k] - want).abs().max()) / scale
        worst_d0 = max(worst_d0, d0)
        if d0 < 1e-3:
            quiet = [max(quiet[0], d0), max(quiet[1], err), quiet[2] + 1]
        if err > worst[0]:
            worst = (err, k)
        if not err <= max(4 * d0, 2e-6):
            bad.append(f"{k}: {err:.2e} of max, its own spread {d0:.2e}")
    print(f"{what}: {len(ref)} tensors, largest spread between two reference runs {worst_d0:.2e} of max, largest skewed - reference {worst[0]:.2e} ({worst[1]}); "
          f"over the {quiet[2]} tensors with a spread below 1e-3: spread {quiet[0]:.2e}, skewed - reference {quiet[1]:.2e}")
    assert not bad, f"{what}: {len(bad)} tensors\n  " + "\n  ".join(bad[:12])


# side_late with every stream live does not meet the skew check: the delays of the context encoder's chain (its own stream and
# its mask branch's) and those of the feature encoder's mask branch run side by side, and main sees the longer chain only
# (measured: 342 delays of 5.3 ms, 856 ms on main where 988 ms were needed).  So side_late runs twice with fewer live side
# streams - the encoder stream alone, the branch stream alone; main_late and replay_late run with all of them.
# variant: (mode, switches, the branch streams a step makes, files with a delayed fork)
TRAIN_VARIANTS = {
    "side_late-encoder_stream": ("side_late", {"cce._BRANCH_STREAMS": False}, 0, {"raft_net.py", "fn.py", "train_loop.py"}),
    "side_late-branch_streams": ("side_late", {"raft_net._ENC_STREAMS": False}, 1, {"cce.py", "fn.py", "train_loop.py"}),
    "main_late": ("main_late", {}, 2, {"raft_net.py", "cce.py", "fn.py", "train_loop.py"}),
    "replay_late": ("replay_late", {}, 2, set()),
}


@gpu
@pytest.mark.parametrize("variant", list(TRAIN_VARIANTS))
def test_training_step_under_skew(det_sd, variant, monkeypatch):
    from focusflow_official_amd import cce, raft_net
    mode, switches, n_branch, fork_files = TRAIN_VARIANTS[variant]
    ref = _train_ref(det_sd, monkeypatch)
    monkeypatch.setenv("FF_TRAIN_STREAMS", "1")
    monkeypatch.setattr(raft_net, "_STREAMS_MIN_PIXELS", 0)
    monkeypatch.setattr(cce, "_branch_streams", {})      # every stream in it is then one of this test's passes
    for k, v in switches.items():
        monkeypatch.setattr({"cce": cce, "raft_net": raft_net}[k.split(".")[0]], k.split(".")[1], v)

    def late(sk):
        def hook(m):
            if sk.mode in ("replay_late", "count"):
                enc = getattr(m.flow_net, "_enc_stream", None)
                sk.replay_late(([enc] if enc is not None else []) + list(cce._branch_streams.values()))
        return hook

    def run(sk):
        cce._branch_streams.clear()       # (the warm model's encoder stream had its own entry)
        return _train_steps(m, _batches(), late(sk))

    what = f"training step {variant}"
    m_warm, m = _train_model(det_sd), _train_model(det_sd)
    got, sk = _skewed(monkeypatch, mode, run, lambda c: _train_steps(m_warm, _batches(True), late(c)), ref["gpu_ms"], ref["wall_ms"], what)
    assert len(cce._branch_streams) == n_branch, "the mask branches of fnet (keyed by main) and of cnet (keyed by the encoder stream)"
    files = {s.split(":")[0] for s in sk.sites}
    assert fork_files <= files, sk.report()
    _against_one_stream(det_sd, got, ref, monkeypatch, what)


# ----------------------------------------------------------------------------
# 5. a caller's own stream, the default stream held
# ----------------------------------------------------------------------------
def _fresh_streams(monkeypatch, *models):
    """The product's stream caches start empty and the context encoder stays on the caller's stream (monkeypatch puts all of it
    back): the pass makes its side streams anew, for the caller's stream, two of them (see _on_own_stream)."""
    from focusflow_official_amd import cce, raft_net, train_loop, update_block
    monkeypatch.setattr(raft_net, "_ENC_STREAMS", False)
    monkeypatch.setattr(cce, "_branch_streams", {})
    monkeypatch.setattr(update_block, "_side_streams", {})
    monkeypatch.setattr(train_loop, "_side_streams", {})
    for m in models:
        monkeypatch.setattr(m.flow_net, "_enc_stream", None, raising=False)


def _on_own_stream(monkeypatch, mode, run, warm, ref_gpu_ms, ref_wall_ms, what):
    """run() on a stream of the caller's with the hooks on (main = that stream) while ONE bounded sleep holds the default
    stream: anything that lands on the default stream finishes after the results were read.  -> run's result.
    A process has 4 hardware queues here and more streams than that: a stream that shares the default stream's queue waits
    for the sleep without any launch having gone astray (measured: with five streams in the pass one of them always did).
    So the callers keep the pass to three streams - its own, the branch stream and the motion encoder's or the weight
    gradients' side stream; the context encoder's stream is off - and empty the product's stream caches, the three are drawn
    right behind a stream that shares the default stream's queue (ss.draw_until_shared), and every stream the counting pass
    saw is checked for sharing it before the sleep is queued."""
    dflt = torch.cuda.default_stream()
    drawn = ss.draw_until_shared(dflt)
    s = torch.cuda.Stream()
    ss._orig(torch.cuda.Stream, "wait_stream")(s, dflt)        # the inputs were made on the default stream
    held = {}

    def hold(n, d):
        # twice the pass (its measured wall time plus the delays it is about to get), at most 1 s
        ms = min(1000.0, 2.0 * (ref_wall_ms + n * d))
        torch.cuda.synchronize()
        ss.sleep_on(dflt, ms)
        held["ev"], held["ms"] = torch.cuda.Event(), ms
        ss._orig(torch.cuda.Event, "record")(held["ev"], dflt)

    with torch.cuda.stream(s):
        with ss.Skew(monkeypatch, s, "count") as c:
            warm(c)
        s.synchronize()
        shared = [x for x in [s] + c.streams if x != dflt and ss.shares_queue(x, dflt)]
        assert not shared, (f"{what}: {len(shared)} of the pass's {len(c.streams)} streams share the default stream's hardware queue "
                            f"(drawn behind the {drawn}th stream of the pool): holding the default stream would hold them")
        n = {"side_late": c.count, "main_late": c.records}[mode]
        budget = max(n * ss.MIN_MS, 450.0 - ref_wall_ms)         # so that pass + delays stay inside half of the 1 s the sleep may last
        d = ss.clamp_delay(ref_wall_ms, n, budget) if n else ss.MIN_MS
        hold(n, d)
        with ss.Skew(monkeypatch, s, mode, d, max(budget, d)) as sk, ss.Timed(s, sync=s.synchronize) as t:
            out = run(sk)
        still_held = not held["ev"].query()
    torch.cuda.synchronize()
    print(f"{what}: the default stream was held for {held['ms']:.0f} ms; the pass on its own stream took {t.wall_ms:.0f} ms")
    assert still_held, f"{what}: the default stream's sleep ({held['ms']:.0f} ms) was over when the pass had finished ({t.wall_ms:.0f} ms): something waited for the default stream"
    if n:
        ss.assert_skewed(sk, t.gpu_ms, ref_gpu_ms, what)
    else:
        print(f"{what}: the pass forks nothing ({c.report()})")
    return out


@gpu
def test_inference_on_a_callers_stream(models, monkeypatch):
    from focusflow_official_amd import raft_net
    monkeypatch.setattr(raft_net, "_STREAMS_MIN_PIXELS", 0)
    m, ref = models["ffraft"], _infer_ref(models, "ffraft", "f16x3")
    a, warm = _pair(**PAIR_A), _pair(**PAIR_WARM)
    _fresh_streams(monkeypatch, m)
    with _precision("f16x3"):
        got = _on_own_stream(monkeypatch, "side_late", lambda sk: _forwards(m, [a]), lambda c: _forwards(m, [warm]), *ref["one"], "FF-RAFT on a caller's stream")
    _same_or_within(got, ref["a"], ref["a2"], "FF-RAFT on a caller's stream")


@gpu
def test_training_step_on_a_callers_stream(det_sd, monkeypatch):
    from focusflow_official_amd import raft_net
    ref = _train_ref(det_sd, monkeypatch)
    monkeypatch.setenv("FF_TRAIN_STREAMS", "1")
    monkeypatch.setattr(raft_net, "_STREAMS_MIN_PIXELS", 0)
    m_warm, m = _train_model(det_sd), _train_model(det_sd)
    batches, warm = _batches(), _batches(True)
    _fresh_streams(monkeypatch)
    got = _on_own_stream(monkeypatch, "main_late", lambda sk: _train_steps(m, batches), lambda c: _train_steps(m_warm, warm), ref["gpu_ms"], ref["wall_ms"],
                         "training step on a caller's stream")
    _against_one_stream(det_sd, got, ref, monkeypatch, "training step on a caller's stream")


@gpu
def test_ffpwc_on_a_callers_stream(monkeypatch):
    import test_hip_pwc
    from focusflow_official_amd.pwcnet import FF_PWCNET
    cfg = Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION="parallel", FUSION_TYPE="1x1conv"))
    m = FF_PWCNET(cfg)
    m.load_state_dict(test_hip_pwc._pwc_weights(), strict=True)
    m = m.to(DEV).eval()

    def inputs(seed):
        i1, i2, m1, _ = orc.shifted_pair(1, H, W, seed=seed, shift=(2, -3))
        return [i1.to(DEV), i2.to(DEV), m1.to(DEV), torch.zeros_like(m1).to(DEV)]

    def fwd(x):
        with torch.no_grad():
            outs = m(*x), m(*x, test_mode=True)
        return [t.cpu() for t in outs[0]] + [outs[1].cpu()]

    a, warm = inputs(41), inputs(42)
    with _precision("f16x3"):
        fwd(a)
        with ss.Timed() as t:
            ref = fwd(a)
        fwd(warm)
        again = fwd(a)
        got = _on_own_stream(monkeypatch, "side_late", lambda sk: fwd(a), lambda c: fwd(warm), t.gpu_ms, t.wall_ms, "FF-PWC on a caller's stream")
    assert float(ref[-1].abs().max()) > 0.05
    _same_or_within(got, ref, again, "FF-PWC on a caller's stream")


@gpu
def test_video_session_on_a_callers_stream(models, monkeypatch):
    import test_tracks
    from focusflow_official_amd import raft_net
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    monkeypatch.setattr(raft_net, "_STREAMS_MIN_PIXELS", 0)
    det = GoodFeatures()         # one detector for every session: its workspace is kept per stream

    def session(frames):
        seq = FrameSequence(models["ffraft"], raft_iters=ITERS, graph=False, keypoints=det, tracks=True)
        assert seq.push(frames[0]) is None
        res = [seq.push(f) for f in frames[1:]]
        out = []
        for r in res:
            out += [r.flow_low, r.flow_up, r.matches, r.valid, r.count, r.tracks.ids, r.tracks.age, r.tracks.born]
        return [t.cpu() for t in out]

    _fresh_streams(monkeypatch, models["ffraft"])
    frames = test_tracks._u8_frames(1, 125, 157, 3, seed=61, shift=(3, -5))
    other = test_tracks._u8_frames(1, 125, 157, 3, seed=62, shift=(-2, 4))
    with _precision("f16x3"):
        session(frames)
        with ss.Timed() as t:
            ref = session(frames)
        session(other)
        again = session(frames)
        got = _on_own_stream(monkeypatch, "side_late", lambda sk: session(frames), lambda c: session(other), t.gpu_ms, t.wall_ms, "video session on a caller's stream")
    assert len(det._ws) >= 2, "the detector's workspace is kept per stream"
    assert bool((ref[5] >= 0).any()), "no live tracks: the session tracked nothing"
    _same_or_within(got, ref, again, "video session on a caller's stream")
