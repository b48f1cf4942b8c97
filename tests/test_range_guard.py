"""The always-on range guard, every route to a refusal: ff_range_probe (the two numbers it rests on), the host-side state machine
(ops.guard_*, graph.CapturedStep) driven without a model, and the model-level cases in which a flow computed by split
convolutions on out-of-range context features used to come back with no error.

Closes the ADVICE.md (round 5) finding on `raft_net.py`: "The range guard has a hole once `_exact_ctx` is set" - a recorded
pass after an inference forward armed the flag - and its sibling, the replay of a hipGraph captured before the flag was armed.
Both had one root: the verdict on a finished forward used the owner's PRESENT flag, not the route that forward took.

1. ff_range_probe does no arithmetic, so the expected word is bit-exact: the int32 bits of max|x| in fp32, 0x7f800000 for a NaN
   or an infinity anywhere, and never less than the word held before (range_guard_ref.probe_word).  groups = npix * C / 4,
   grid = min(ceil(groups / 1024), 512) blocks of 256: the sizes walk one group, the wave and block edges, the second block,
   and the block cap with one more grid-stride trip.  Layouts: dense, and a channel slice (ld = C + 8 from channel 4) of a buffer
   filled with a SENTINEL above every finite value inside - a read outside the slice changes the word.
2. The state machine over a stub owner and two small tensors whose contents the test sets, eager and through
   CapturedStep.capture / replay, against the table of range_guard_ref.verdict_table; the same table on the CPU against the
   pure ops.guard_verdict.
3. Two model-level tests at 1 x 128 x 160, raft_iters=2: a recorded pass after arming, and replays after arming.

Scales of part 3 and the levels measured with them on the MI355X (synthetic test weights, orc.shifted_pair seed 3):
   recorded pass after arming: cnet.conv2 weight and bias x 50 -> max|ctx| = 20 352.7;
   replay after arming: unscaled level 700.767 -> cnet.conv2 x 16: max|ctx| = 6 586.39 at capture (inside [X_LIMIT/4, X_LIMIT));
   normalised input x 8 -> max|ctx| = 25 340.9, max|fmap| = 34.4986 in the replay (the premise the test asserts).  The context
   output is not linear in the input (the folded BatchNorm shifts and the biases stay put): x 4 gives 13 710.7, still inside.
No tolerance but the 1e-3 px of the eager exact-route test; everything else is bit-exact or raised / not raised."""
import ctypes
import math
import threading
import types
import warnings

import numpy as np
import pytest
import torch

import range_guard_ref as ref

gpu = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 3.0e4                      # above every finite value the probe tests plant (X_LIMIT = 16 376 is the largest)
X_LIMIT = ref.X_LIMIT


@pytest.fixture()
def hip():
    from focusflow_official_amd import _hip, ops
    assert ops.X_LIMIT == X_LIMIT

    def clean():                        # (nothing of one test is left for the next: a forward that raised keeps its words)
        st = ops._guard_state()
        st["words"], st["capture_words"] = None, None
        st["pending"].clear()

    clean()
    yield types.SimpleNamespace(_hip=_hip, ops=ops, Error=_hip.FocusFlowHipError)
    clean()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. ff_range_probe
# ---------------------------------------------------------------------------------------------------------------------------------
def _word(held=0):
    return torch.tensor([held], dtype=torch.int32, device=DEV)


def _probe(hip, x, word):
    b, h, w, c = x.shape
    hip._hip.call("ff_range_probe", hip.ops._p(x), hip.ops._ld(x), b * h * w, c, hip.ops._p(word), hip.ops._stream())


class Plane:
    """An fp32 (1, 1, npix, C) tensor on the device - dense, or channels [4, 4 + C) of a SENTINEL-filled buffer C + 8 wide - with
    its host copy; elements are set by flat index into the LOGICAL tensor, as bits, so that a NaN keeps its sign and payload."""

    def __init__(self, npix, c, view, fill=None, seed=0):
        self.npix, self.c = npix, c
        if fill is None:
            self.host = np.random.default_rng(seed).uniform(-1.0, 1.0, (npix, c)).astype(np.float32)
        else:
            self.host = np.full((npix, c), fill, np.float32)
        t = torch.from_numpy(self.host).view(1, 1, npix, c)
        if view:
            self.buf = torch.full((1, 1, npix, c + 8), SENTINEL, dtype=torch.float32, device=DEV)
            self.buf[..., 4:4 + c] = t.to(DEV)
            self.x = self.buf[..., 4:4 + c]
        else:
            self.buf = self.x = t.to(DEV)
        self.snap = self.buf.clone()

    def set_bits(self, idx, b):
        self.host.reshape(-1).view(np.int32)[idx] = np.int32(b)
        self.x.view(torch.int32)[0, 0, idx // self.c, idx % self.c] = int(np.int32(b))
        self.snap = self.buf.clone()

    def set(self, idx, v):
        self.set_bits(idx, ref.bits(v))

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.snap.view(torch.int32))


def _s32(u):
    """A 32-bit pattern as the int32 it is stored as."""
    return u - (1 << 32) if u >= 1 << 31 else u


# (npix, C): groups = npix * C / 4
PROBE_SIZES = [(1, 4), (255, 4), (256, 4), (257, 4), (1024, 4), (1025, 4), (512 * 1024 + 1, 4),
               (8, 128), (33, 128), (4, 256), (17, 256), (3, 324), (13, 324), (6473, 324)]      # 6473 x 81 = 524 313 groups: past the cap at C = 324


@gpu
@pytest.mark.parametrize("view", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("npix,c", PROBE_SIZES, ids=lambda v: str(v))
def test_probe_finds_the_maximum_wherever_it_sits(hip, npix, c, view):
    """The maximum planted at the first element, the last one, each of the four lanes of a float4, the first lane of the last
    group of the last grid-stride trip - positive and negative - over values in [-1, 1]: the word is the bits of its magnitude,
    and the input buffer is bit-identical afterwards."""
    p = Plane(npix, c, view, seed=npix + c)
    n = npix * c
    mid = (n // 4 // 2) * 4
    spots = [0, n - 1, mid, min(mid + 1, n - 1), min(mid + 2, n - 1), min(mid + 3, n - 1), n - 4]
    word = _word()
    _probe(hip, p.x, word)
    assert int(word) == ref.probe_word(p.host) and int(word) <= ref.bits(1.0), "no planted value"
    for k, idx in enumerate(spots):
        keep = p.host.reshape(-1).view(np.int32)[idx]
        p.set(idx, (2.5 + 0.125 * k) * (-1.0 if k % 2 else 1.0))
        word = _word()
        _probe(hip, p.x, word)
        assert int(word) == ref.probe_word(p.host) == ref.bits(2.5 + 0.125 * k), f"maximum at flat index {idx} of {n}"
        assert p.untouched()
        p.set_bits(idx, int(keep))


@gpu
@pytest.mark.parametrize("view", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("npix,c", [(257, 4), (1025, 4), (13, 324)], ids=lambda v: str(v))
def test_probe_values_at_the_edges_of_the_format(hip, npix, c, view):
    """-0.0 only and all zeros (the word keeps what it held), a subnormal maximum, X_LIMIT exactly and the fp32 below it; and
    0x7f800000 for +inf, -inf, a quiet NaN and a NaN with the sign bit set, in the middle and alone at the last element."""
    n = npix * c
    for fill in (-0.0, 0.0):
        p = Plane(npix, c, view, fill=fill)
        for held in (0, ref.bits(5.0), 1):
            word = _word(held)
            _probe(hip, p.x, word)
            assert int(word) == held == ref.probe_word(p.host, held), f"fill {fill!r}, word held {held:#x}"
    p = Plane(npix, c, view, fill=0.0)                  # subnormals: 1e-40 among smaller ones of both signs
    for idx, v in ((n // 2, 1e-40), (0, -1e-41), (n - 1, 1e-45)):
        p.set(idx, v)
    word = _word()
    _probe(hip, p.x, word)
    assert int(word) == ref.probe_word(p.host) == ref.bits(1e-40) and 0 < int(word) < 0x00800000
    p = Plane(npix, c, view, seed=5)
    for v in (ref.BELOW, X_LIMIT, -ref.BELOW, -X_LIMIT):
        p.set(n // 3, v)
        word = _word()
        _probe(hip, p.x, word)
        assert int(word) == ref.probe_word(p.host) == ref.bits(abs(v))
        got = float(word.view(torch.float32))
        assert (got < X_LIMIT) == (abs(v) < X_LIMIT)      # (the comparison the guard makes with it)
    for pattern in (0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF):
        for idx in (n // 2 + 1, n - 1):
            p = Plane(npix, c, view, seed=6)
            p.set_bits(idx, _s32(pattern))
            for held in (0, ref.bits(3.0e38)):
                word = _word(held)
                _probe(hip, p.x, word)
                assert int(word) == ref.INF_WORD == ref.probe_word(p.host, held), f"{pattern:#x} at {idx} of {n}"
            assert p.untouched()


@gpu
@pytest.mark.parametrize("view", [False, True], ids=["dense", "slice"])
def test_probe_accumulates_into_the_word(hip, view):
    """A word holding more stays, one holding less is replaced, two probes into one word leave the maximum of both; through
    ops.guard_probe, slot 1 of a pair leaves slot 0 as it was and the other way round."""
    ops = hip.ops
    a, b = Plane(257, 4, view, seed=1), Plane(13, 324, view, seed=2)
    a.set(700, -3.0)
    b.set(4000, 9.0)
    word = _word(ref.bits(4.0))
    _probe(hip, a.x, word)
    assert int(word) == ref.bits(4.0)
    word = _word(ref.bits(2.0))
    _probe(hip, a.x, word)
    assert int(word) == ref.bits(3.0)
    for first, second in ((a, b), (b, a)):
        word = _word()
        _probe(hip, first.x, word)
        _probe(hip, second.x, word)
        assert int(word) == ref.bits(9.0)
    mark = ref.bits(7.0)
    st = ops._guard_state()
    for slot, other in ((0, 1), (1, 0)):
        pair = torch.tensor([mark, mark], dtype=torch.int32, device=DEV)
        pair[slot] = 0
        st["words"] = pair
        ops.guard_probe(a.x, slot)
        ops.guard_probe(b.x, slot)
        assert pair.tolist()[slot] == ref.bits(9.0) and pair.tolist()[other] == mark
    st["words"] = None
    ops.guard_probe(a.x, 0)                              # (no forward running: nothing to write into)
    assert a.untouched() and b.untouched()


@gpu
def test_probe_refuses_what_it_cannot_read(hip):
    """C % 4 != 0, ld < C, ld % 4 != 0, npix == 0 and a pointer off 16 bytes: an error through ff_last_error, the word as it was."""
    ops, _hip = hip.ops, hip._hip
    x = torch.full((64,), SENTINEL, dtype=torch.float32, device=DEV)
    held = ref.bits(3.0)
    word = _word(held)
    cases = {"C % 4": (x.data_ptr(), 8, 2, 6), "ld < C": (x.data_ptr(), 4, 2, 8), "ld % 4": (x.data_ptr(), 6, 2, 4),
             "npix == 0": (x.data_ptr(), 4, 0, 4), "pointer off 16 bytes": (x.data_ptr() + 4, 4, 2, 4),
             "C == 0": (x.data_ptr(), 4, 2, 0)}
    for what, (ptr, ld, npix, c) in cases.items():
        with pytest.raises(hip.Error, match="ff_range_probe: bad argument"):
            _hip.call("ff_range_probe", ctypes.c_void_p(ptr), ld, npix, c, ops._p(word), ops._stream())
        assert b"ff_range_probe: bad argument" in _hip.load().ff_last_error(), what
        torch.cuda.synchronize()
        assert int(word) == held, what
    _hip.call("ff_range_probe", ctypes.c_void_p(x.data_ptr()), 4, 2, 4, ops._p(word), ops._stream())     # (the same call, well-formed)
    assert int(word) == ref.bits(SENTINEL)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the state machine, without a model
# ---------------------------------------------------------------------------------------------------------------------------------
def _owner(**kw):
    return types.SimpleNamespace(**{"_guard_hist": False, "_guard_level": 0.0, "_exact_ctx": False, **kw})


class Rig:
    """A stub forward: two static NHWC tensors whose contents the test sets, and step() = guard_begin, two probes, guard_end
    with the route the 'forward' took."""

    def __init__(self, ops, owner, what="stub forward"):
        self.ops, self.owner, self.what = ops, owner, what
        self.ctx = torch.zeros(1, 2, 3, 8, device=DEV)
        self.fmap = torch.zeros(2, 2, 3, 4, device=DEV)
        self.exact = self.recorded = False

    def put(self, m_ctx, m_fmap):
        self.ctx.fill_(0.5)
        self.fmap.fill_(-0.25)
        self.ctx[0, 1, 2, 7] = -m_ctx if m_ctx == m_ctx else m_ctx
        self.fmap[1, 0, 1, 2] = m_fmap

    def step(self):
        self.ops.guard_begin(torch.device(DEV))
        self.ops.guard_probe(self.ctx, 0)
        self.ops.guard_probe(self.fmap, 1)
        self.ops.guard_end(self.what, owner=self.owner, exact_ctx=self.exact, recorded=self.recorded)


def _outcome(ops, Error, owner):
    """guard_check(sync=True) -> (raised, armed, message)."""
    try:
        ops.guard_check(sync=True)
    except Error as e:
        return True, owner._exact_ctx, str(e)
    return False, owner._exact_ctx, ""


def _judge(hip, owner, got, row, label, flag_before):
    """One look's outcome against its row; flag_before: the owner's `_exact_ctx` when the look began."""
    m_ctx, m_fmap, route, (refuses, arms, tail) = row
    raised, armed, msg = got
    where = f"m_ctx {m_ctx!r}, m_fmap {m_fmap!r}, route {route}, flag {flag_before}"
    assert raised == refuses, where
    assert armed == (flag_before or arms), where
    if refuses:
        assert msg.startswith(label + ":") and "16376" in msg and "not valid" in msg, f"{where}: {msg}"
        if tail == ref.TAIL_RECORDED:
            assert tail in msg, f"{where}: {msg}"
        else:
            assert msg.endswith(tail) and ref.TAIL_RECORDED not in msg, f"{where}: {msg}"
    assert owner._guard_hist and owner._guard_level == ref.level_after(m_ctx, m_fmap), where
    assert hip.ops._guard_state()["pending"] == [], where
    hip.ops.guard_check(sync=True)                      # after a refusal (or none) the next look is quiet


def test_verdict_table_pure():
    """ops.guard_verdict against the written-down table (no GPU)."""
    from focusflow_official_amd import ops
    rows = ref.verdict_table()
    assert len(rows) == 3 * 11 + 6
    for m_ctx, m_fmap, route, (refuses, arms, tail) in rows:
        got = ops.guard_verdict(m_ctx, m_fmap, route == "exact", route == "recorded")
        where = f"m_ctx {m_ctx!r}, m_fmap {m_fmap!r}, route {route}: {got}"
        assert got[:2] == (refuses, arms), where
        assert (got[2] == "") == (not refuses) and tail in got[2], where
        # an armed flag changes nothing for a recorded pass
        assert ops.guard_verdict(m_ctx, m_fmap, True, True) == ops.guard_verdict(m_ctx, m_fmap, False, True)


@gpu
def test_guard_verdicts_eager(hip):
    """Every row of the table through an eager stub forward whose words are looked at afterwards (ops.guard_check): raised or
    not, armed or not, the tail of the message, the owner's level, nothing left pending.  The owner's flag at the time of the
    look is the OPPOSITE of the route the forward took, where that can differ: the verdict follows the route."""
    ops = hip.ops
    # the owner's flag when the look happens - split: not armed (armed is the exact route's case); exact: armed, or cleared since;
    # recorded: not armed, or armed since by an inference forward
    flags = {"split": (False,), "exact": (True, False), "recorded": (False, True)}
    for row in ref.verdict_table():
        m_ctx, m_fmap, route, _ = row
        for flag in flags[route]:
            owner = _owner()
            rig = Rig(ops, owner)
            rig.exact, rig.recorded = route == "exact", route == "recorded"
            rig.put(m_ctx, m_fmap)
            rig.step()
            owner._exact_ctx = flag
            _judge(hip, owner, _outcome(ops, hip.Error, owner), row, "stub forward", flag)


@gpu
def test_guard_verdicts_through_a_captured_step(hip):
    """The same table, the stub forward captured once per route (graph.CapturedStep) and replayed on each row's values: a replay
    is judged by the owner's flag as it stood at CAPTURE.  After the first refusal of a finite context output arms the flag,
    the same replay is refused again, and again."""
    from focusflow_official_amd.graph import CapturedStep
    ops = hip.ops
    for route in ("split", "exact"):
        owner = _owner(_exact_ctx=route == "exact")
        rig = Rig(ops, owner)
        rig.put(1.0, 1.0)
        cs = CapturedStep(torch.device(DEV), ("stub replay",), owner)
        cs.capture(rig.step, lambda: None, warmup=1)
        assert owner._guard_level == 1.0                # (the warm-up step was looked at before the capture)
        for row in ref.verdict_table():
            m_ctx, m_fmap, r, (refuses, arms, _) = row
            if r != route:
                continue
            owner._guard_hist, owner._guard_level, owner._exact_ctx = False, 0.0, route == "exact"
            rig.put(m_ctx, m_fmap)
            cs.replay()
            _judge(hip, owner, _outcome(ops, hip.Error, owner), row, "stub replay", route == "exact")
            torch.cuda.synchronize()
            assert cs._words[0].tolist() == [ref.probe_word(np.float32([m_ctx, 0.5])), ref.probe_word(np.float32([m_fmap, 0.25]))]
            for _ in range(2):                          # the flag as it stands now (armed by the refusal) does not excuse the graph
                cs.replay()
                raised, _, msg = _outcome(ops, hip.Error, owner)
                assert raised == refuses and (not raised or msg.startswith("stub replay:")), row
            owner._exact_ctx = not owner._exact_ctx     # ... nor does any other value of it
            cs.replay()
            assert _outcome(ops, hip.Error, owner)[0] == refuses, row


@gpu
def test_captured_words_are_zeroed_per_replay_and_labelled_per_forward(hip):
    """A CapturedStep with two labels (a video session's forward / backward pair): the k-th forward's words are reported under
    the k-th label.  Every replay starts its words from zero: an in-range replay after an out-of-range one is clean once the
    refusal is taken."""
    from focusflow_official_amd.graph import CapturedStep
    ops = hip.ops
    owner = _owner()
    one, two = Rig(ops, owner), Rig(ops, owner)
    cs = CapturedStep(torch.device(DEV), ("pair forward", "pair backward"), owner)

    def step():
        one.step()
        with cs.guard(1):
            two.step()

    one.put(1.0, 2.0)
    two.put(3.0, 4.0)
    cs.capture(step, lambda: None, warmup=1)
    words = lambda: [[float(np.int32(w).view(np.float32)) for w in pair.tolist()] for pair in cs._words]     # noqa: E731
    cs.replay()
    ops.guard_check(sync=True)
    assert words() == [[1.0, 2.0], [3.0, 4.0]]
    for bad, good, label in ((two, one, "pair backward"), (one, two, "pair forward")):
        bad.put(2 * X_LIMIT, 2.0)
        cs.replay()
        raised, armed, msg = _outcome(ops, hip.Error, owner)
        assert raised and armed and msg.startswith(label + ":") and ops._guard_state()["pending"] == [], msg
        bad.put(0.75, 0.5)
        good.put(0.75, 0.5)
        cs.replay()
        ops.guard_check(sync=True)                      # clean: nothing of the replay before is left in the words
        assert words() == [[0.75, 0.5], [0.75, 0.5]] and ops._guard_state()["pending"] == []
        bad.put(X_LIMIT, 0.5)                           # armed since - and still the split route in the graph
        cs.replay()
        with pytest.raises(hip.Error, match=label):
            ops.guard_check(sync=True)
        bad.put(0.75, 0.5)
        owner._exact_ctx = False


@gpu
def test_guard_careful(hip, monkeypatch):
    """ops.guard_careful: True without history; True at level * GUARD_MARGIN == X_LIMIT exactly, False one ulp below; False with
    no words (no forward running, RANGE_GUARD off) and while a hipGraph is being captured."""
    ops = hip.ops
    at = X_LIMIT / ops.GUARD_MARGIN
    assert at * ops.GUARD_MARGIN == X_LIMIT
    fresh, edge, below = _owner(), _owner(_guard_hist=True, _guard_level=at), _owner(_guard_hist=True, _guard_level=math.nextafter(at, 0.0))
    assert not ops.guard_careful(fresh)                 # no forward running
    ops.guard_begin(torch.device(DEV))
    assert ops.guard_careful(fresh) and ops.guard_careful(edge) and not ops.guard_careful(below)
    assert ops.guard_careful(types.SimpleNamespace())   # (an owner that never heard of the guard)
    ops.guard_end("careful", owner=fresh, handled=True)
    assert not ops.guard_careful(fresh) and ops._guard_state()["pending"] == []
    monkeypatch.setattr(ops, "RANGE_GUARD", False)
    ops.guard_begin(torch.device(DEV))
    assert not ops.guard_careful(fresh) and not ops.guard_careful(edge)
    ops.guard_end("careful", owner=fresh)
    monkeypatch.setattr(ops, "RANGE_GUARD", True)
    words = torch.zeros(2, dtype=torch.int32, device=DEV)
    seen = []
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.guard_capture(words), torch.cuda.graph(g):
        ops.guard_begin(torch.device(DEV))
        seen.append((ops._guard_state()["words"] is words, ops.guard_careful(fresh), ops.guard_careful(edge)))
        ops.guard_end("careful", owner=fresh)
    assert seen == [(True, False, False)] and ops._guard_state()["pending"] == []


def test_guard_capture_restores_the_outer_words_when_the_block_raises():
    """ops.guard_capture nests; the outer value is back after the inner block, also when it raises (no GPU)."""
    from focusflow_official_amd import ops
    st = ops._guard_state()
    a, b = object(), object()
    assert st["capture_words"] is None
    with ops.guard_capture(a):
        with pytest.raises(RuntimeError, match="inner"), ops.guard_capture(b):
            assert st["capture_words"] is b
            raise RuntimeError("inner")
        assert st["capture_words"] is a
        with ops.guard_capture(b), ops.guard_capture(None):
            assert st["capture_words"] is None
        assert st["capture_words"] is a
    assert st["capture_words"] is None


def test_guard_state_is_per_thread():
    """ops._guard_state() in a second thread is a different dict with a pending list of its own (no GPU)."""
    from focusflow_official_amd import ops
    mine, box = ops._guard_state(), {}
    assert ops._guard_state() is mine

    def other():
        st = ops._guard_state()
        st["pending"].append("theirs")
        box["st"], box["again"] = st, ops._guard_state()

    before = list(mine["pending"])
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert box["st"] is box["again"] and box["st"] is not mine
    assert box["st"]["pending"] == ["theirs"] and box["st"]["pending"] is not mine["pending"] and mine["pending"] == before


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the two holes, on the model
# ---------------------------------------------------------------------------------------------------------------------------------
def _scaled_sd(det_sd, k):
    sd = {key: v.clone() for key, v in det_sd.items()}
    for key in ("flow_net.cnet.conv2.weight", "flow_net.cnet.conv2.bias"):
        sd[key] *= k
    return sd


@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused-node", "tape"])
def test_recorded_pass_after_arming_is_refused(hip, det_sd, fused, monkeypatch):
    """The weights of the exact-route test (cnet.conv2 x 50: |ctx| ~ 35 000).  A torch.no_grad() forward - a validation pass in
    the middle of training, no train() / eval() in between - warns and arms the exact route; the next forward of the same module
    with grad enabled is recorded, has no exact route, and must raise instead of running the split convolutions on those
    context features.  Fused update-loop node and per-operation tape."""
    from focusflow_official_amd import train_loop
    from oracle import ffraft_ref as orc
    from test_hip_parity import _model
    monkeypatch.setattr(train_loop, "ENABLED", fused)
    m = _model(_scaled_sd(det_sd, 50.0))
    inp = [t.to(DEV) for t in orc.shifted_pair(1, 128, 160, seed=3)]
    with torch.no_grad(), pytest.warns(UserWarning, match="exact-fp32"):
        m(*inp, raft_iters=2, test_mode=True)
    net = m.flow_net
    print(f"armed by the no_grad forward: max|ctx| = {net._guard_level:.6g}")
    assert net._exact_ctx and X_LIMIT <= net._guard_level < math.inf          # the premise: finite, beyond the limit, armed
    assert torch.is_grad_enabled() and any(q.requires_grad for q in net.cnet.parameters())
    with pytest.raises(hip.Error, match="RECORDED"):
        m(*inp, raft_iters=2)
    assert net._exact_ctx                               # (the inference route stays armed)
    m.check_range()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")
        m(*inp, raft_iters=2, test_mode=True)           # inference goes on, on the exact route
    m.check_range()


@gpu
def test_replays_after_arming_are_refused_until_the_graph_is_captured_again(hip, det_sd):
    """cnet.conv2 scaled by the power of two that puts the example pair's context maximum into [X_LIMIT/4, X_LIMIT); a
    GraphedForward captured there holds the split route.  A replay on the pair with its NORMALISED input 2x/255 - 1 times 8
    lifts the context output past the limit and keeps it finite (the feature encoder is instance-normalised and stays put):
    asserted from the capture's words.  The first check_range() raises and arms; a second and a third replay on the same inputs
    are refused again under the capture's label (they used to pass: the armed flag excused the graph's split route).  A
    GraphedForward captured now takes the exact route, passes, and its flow meets the CPU oracle at 1e-3 px."""
    from focusflow_official_amd.graph import GraphedForward
    from oracle import ffraft_ref as orc
    from test_hip_parity import _model, close
    inp = orc.shifted_pair(1, 128, 160, seed=3)
    dev = lambda ts: [t.to(DEV) for t in ts]            # noqa: E731
    m0 = _model(det_sd)
    with torch.no_grad():
        m0(*dev(inp), raft_iters=2, test_mode=True)
    m0.check_range()
    level0 = m0.flow_net._guard_level
    k = 2.0 ** math.floor(math.log2(ref.BELOW / level0))
    in_scale = 8.0
    sd = _scaled_sd(det_sd, k)
    m = _model(sd)
    gf = GraphedForward(m, dev(inp), raft_iters=2)
    gf(*dev(inp))
    gf.check_range()
    level = m.flow_net._guard_level
    print(f"unscaled level {level0:.6g}: cnet.conv2 x {k:g} -> level {level:.6g} at capture; normalised input x {in_scale:g}")
    assert X_LIMIT / 4 <= level < X_LIMIT and not m.flow_net._exact_ctx
    # images whose normalised form is in_scale times the pair's: 2 x'/255 - 1 = s (2 x/255 - 1)
    big = [(in_scale * (2 * inp[0] / 255.0 - 1.0) + 1.0) * 127.5, (in_scale * (2 * inp[1] / 255.0 - 1.0) + 1.0) * 127.5, inp[2], inp[3]]
    gf(*dev(big))
    torch.cuda.synchronize()
    m_ctx, m_fmap = gf._captured._words[0].view(torch.float32).tolist()
    print(f"replay on the scaled pair: max|ctx| = {m_ctx:.6g}, max|fmap| = {m_fmap:.6g}")
    assert X_LIMIT <= m_ctx < math.inf and m_fmap < X_LIMIT                   # the premise
    with pytest.raises(hip.Error, match="GraphedForward replay.*from now on"):
        gf.check_range()
    assert m.flow_net._exact_ctx
    for nth in ("second", "third"):
        gf(*dev(big))
        with pytest.raises(hip.Error, match="GraphedForward replay"):
            gf.check_range()
        assert hip.ops._guard_state()["pending"] == [], nth
    gf(*dev(inp))                                       # (in range: the same graph is still good for what it can compute)
    gf.check_range()
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter("always")
        gf2 = GraphedForward(m, dev(big), raft_iters=2)
    assert not [w for w in said if "exact-fp32" in str(w.message)]           # armed already: nothing new to say
    assert gf2._captured._exact_ctx
    lo, up = gf2(*dev(big))
    gf2.check_range()
    m_ctx2, m_fmap2 = gf2._captured._words[0].view(torch.float32).tolist()
    assert X_LIMIT <= m_ctx2 < math.inf and m_fmap2 < X_LIMIT                 # (the same inputs, accepted on this route)
    ref_lo, ref_up = orc.ffraft_forward(sd, *big, raft_iters=2, test_mode=True)
    close(up.cpu(), ref_up, rtol=0, atol=1e-3, what="flow_up of the graph captured on the exact route")
    close(lo.cpu(), ref_lo, rtol=0, atol=1e-3, what="flow_low of the graph captured on the exact route")
    gf(*dev(big))                                       # the old graph beside it: still the split route, still refused
    with pytest.raises(hip.Error, match="GraphedForward replay"):
        gf.check_range()
