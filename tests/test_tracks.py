"""Key-point tracks: csrc/tracks.hip (ff_tracks_replenish, ff_tracks_mask, ff_tracks_advance), their ops wrappers,
tracks.TrackTable and frames.FrameSequence(tracks=...).

Every step is exact by definition (include/focusflow_hip.h), so the kernels and the session are held to the numpy restatement
of tests/tracks_ref.py with equality; the only bound here is GRAPH_VS_EAGER, the project's bound between a replayed and an
eagerly issued forward, for the flow of the first pair against the session without tracks."""
import ctypes
import os
import re
import shutil
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_spec
import tracks_ref as R

DEV = "cuda:0"
GRAPH_VS_EAGER = 2e-4      # px: test_warm_start.py / test_frame_sequence.py
ENTRY_POINTS = ("ff_tracks_replenish", "ff_tracks_mask", "ff_tracks_advance")
H, W = 125, 157
F32 = np.float32


# ----------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    from focusflow_official_amd import _hip, build
    hdr = open(os.path.join(ROOT, "include", "focusflow_hip.h")).read()
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), f"{name} is not declared in focusflow_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.EXPORTS and name in _hip._SIGS
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_hip._SIGS[name]), f"{name}: {len(_hip._SIGS[name])} bound arguments, the header declares {len(decl.split(','))}"
    history = hdr.split("#define FF_ABI_VERSION")[0]
    assert "7 (unchanged): entry points only: ff_tracks_replenish, ff_tracks_mask, ff_tracks_advance" in history
    lib.ff_abi_version.restype = ctypes.c_int
    assert lib.ff_abi_version() == int(re.search(r"#define FF_ABI_VERSION (\d+)", hdr).group(1)) == _hip.ABI_VERSION == 7


def test_wrappers_raise_on_cpu_tensors():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    tb = {k: torch.from_numpy(v) for k, v in R.empty_table(1, 4).items()}
    points, count = torch.zeros(1, 4, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(FocusFlowHipError, match="pos"):
        ops.tracks_replenish(tb["pos"], tb["ids"], tb["age"], tb["next_id"], points, count, 5, 7, 10)
    with pytest.raises(FocusFlowHipError, match="pos"):
        ops.tracks_mask(tb["pos"], tb["ids"], 5, 7)
    with pytest.raises(FocusFlowHipError, match="pos"):
        ops.tracks_advance(tb["pos"], tb["ids"], tb["age"], torch.zeros(1, 2, 8, 8), 0, 1, 5, 7)


def _table(b, n, live, next_id=0):
    """live: {(sample, slot): (x, y, id, age)}."""
    tb = R.empty_table(b, n, next_id)
    for (bi, s), (x, y, i, a) in live.items():
        tb["pos"][bi, s], tb["ids"][bi, s], tb["age"][bi, s] = (x, y), i, a
    return tb


def _points(rows, m):
    """rows: one list of (x, y) per sample -> (points (B,m,2) int32 with -1 beyond the count, count (B) int32)."""
    pts = np.full((len(rows), m, 2), -1, np.int32)
    for bi, r in enumerate(rows):
        pts[bi, :len(r)] = np.asarray(r, np.int32).reshape(-1, 2)
    return pts, np.asarray([len(r) for r in rows], np.int32)


def test_restatement_of_replenish_known_answers():
    tb = _table(1, 4, {(0, 1): (20.0, 30.0, 7, 3)}, next_id=100)
    # exactly min_distance away (same row; a 6-8-10 triangle): not blocked.  min_distance - 1 on the same row: blocked
    pts, cnt = _points([[(30, 30), (29, 30), (26, 38), (20, 30)]], 6)
    assert R.blocked(tb, pts, cnt, 64, 64, 10)[0].tolist() == [False, True, False, True, False, False]
    out, born, live = R.replenish(tb, pts, cnt, 64, 64, 10)
    assert out["ids"][0].tolist() == [100, 7, 101, -1] and born.tolist() == [2] and live.tolist() == [3] and out["next_id"].tolist() == [102]
    assert out["pos"][0].tolist() == [[30, 30], [20, 30], [26, 38], [-1, -1]] and out["age"][0].tolist() == [0, 3, 0, 0]
    assert tb["ids"][0].tolist() == [-1, 7, -1, -1]      # (the argument is left alone)
    # min_distance 0 blocks nothing, not even a detection on the track
    assert not R.blocked(tb, pts, cnt, 64, 64, 0).any()
    # more unblocked detections than free slots: the strongest (first) are taken, lowest slots first; ids continue across calls
    pts, cnt = _points([[(50, 50), (5, 5), (60, 10), (40, 40), (10, 60)]], 5)
    out2, born, live = R.replenish(out, pts, cnt, 64, 64, 10)
    assert born.tolist() == [1] and live.tolist() == [4] and out2["ids"][0].tolist() == [100, 7, 101, 102] and out2["pos"][0, 3].tolist() == [50, 50]
    assert out2["next_id"].tolist() == [103]
    # a full table: no births, nothing changes
    out3, born, live = R.replenish(out2, pts, cnt, 64, 64, 10)
    assert born.tolist() == [0] and live.tolist() == [4] and all(np.array_equal(out3[k], out2[k]) for k in out2)
    # count = 0, and a detection outside the frame is passed over
    out4, born, _ = R.replenish(tb, pts, np.zeros(1, np.int32), 64, 64, 10)
    assert born.tolist() == [0] and all(np.array_equal(out4[k], tb[k]) for k in tb)
    pts, cnt = _points([[(64, 5), (5, 5)]], 2)
    out5, born, _ = R.replenish(tb, pts, cnt, 64, 64, 10)
    assert born.tolist() == [1] and out5["pos"][0, 0].tolist() == [5, 5]


def _known_mask_advance_case():
    """Six slots on a 5 x 7 frame that lies at left 0, top 1 of an 8 x 8 field: -> (table, flow_up)."""
    tb = _table(1, 6, {(0, 0): (6.0, 2.0, 10, 0),        # on x = W - 1: x1 = x0, the flow of the last column
                       (0, 1): (1.5, 1.25, 11, 4),       # sub-pixel
                       (0, 2): (3.0, 3.0, 12, 1),        # pushed out of the frame
                       (0, 4): (2.0, 0.0, 13, 2),        # a NaN
                       (0, 5): (1.5, 1.25, 14, 0)})      # the same pixel as slot 1
    flow = np.zeros((1, 2, 8, 8), F32)
    flow[0, 0, 1 + 2, 6], flow[0, 1, 1 + 2, 6] = -0.5, 1.0
    flow[0, 0, 1 + 1, 1:3], flow[0, 0, 1 + 2, 1:3] = (1.0, 3.0), (5.0, 7.0)      # u = 0.75 (0.5 1 + 0.5 3) + 0.25 (0.5 5 + 0.5 7) = 3
    flow[0, 1, 1 + 3, 3] = 1.25                # 3 + 1.25 > H - 1
    flow[0, 0, 1 + 0, 2] = np.nan
    flow[0, :, 0, :] = 99.0                    # the padding row: never read
    return tb, flow


def _assert_known_mask_advance(m, out, mt, valid, ids, age):
    """The answers worked out by hand, for whoever computed them (numpy arrays)."""
    assert m.shape == (1, 1, 5, 7) and m.sum() == 4 * 255      # five tracks on four pixels
    assert m[0, 0, 2, 6] == 255 and m[0, 0, 1, 2] == 255 and m[0, 0, 3, 3] == 255 and m[0, 0, 0, 2] == 255      # (1.5 + 0.5 -> 2, 1.25 + 0.5 -> 1)
    assert mt[0, 0].tolist() == [6, 2, 5.5, 3] and mt[0, 1].tolist() == [1.5, 1.25, 4.5, 1.25] and mt[0, 2].tolist() == [3, 3, 3, 4.25]
    assert mt[0, 3].tolist() == [-1, -1, -1, -1] and np.isnan(mt[0, 4, 2]) and mt[0, 4, :2].tolist() == [2, 0]
    assert valid[0].tolist() == [1, 1, 0, 0, 0, 1] and ids[0].tolist() == [10, 11, 12, -1, 13, 14] and age[0].tolist() == [0, 4, 1, 0, 2, 0]
    assert out["ids"][0].tolist() == [10, 11, -1, -1, -1, 14] and out["age"][0].tolist() == [1, 5, 0, 0, 0, 1]
    assert out["pos"][0].tolist() == [[5.5, 3], [4.5, 1.25], [-1, -1], [-1, -1], [-1, -1], [4.5, 1.25]]
    assert out["next_id"].tolist() == [0]


def test_restatement_of_mask_and_advance_known_answers():
    tb, flow = _known_mask_advance_case()
    _assert_known_mask_advance(R.mask(tb, 5, 7), *R.advance(tb, flow, 0, 1, 5, 7))


def test_frame_result_copies_and_pickles():
    """Without tracks a result is the five-item named tuple it was; with tracks it has a sixth item.  Both survive copy, deepcopy
    (the way to keep a result past the next push: its tensors are the session's static buffers) and pickle, and keep the
    helpers of a NamedTuple."""
    import copy
    import pickle
    from focusflow_official_amd.frames import FrameResult
    from focusflow_official_amd.tracks import TrackResult
    five = FrameResult(torch.ones(2), torch.zeros(3), None, None, None)
    six = FrameResult(torch.ones(2), torch.zeros(3), torch.ones(1, 4, 4), torch.ones(1, 4, dtype=torch.uint8), torch.tensor([4], dtype=torch.int32),
                      TrackResult(torch.arange(4)[None], torch.zeros(1, 4, dtype=torch.int32), torch.tensor([4], dtype=torch.int32)))

    def same(a, b):
        if isinstance(a, tuple):
            return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))

    for res, n in ((five, 5), (six, 6)):
        assert len(res) == n and len(res._fields) == n and isinstance(res, FrameResult) and list(res._asdict()) == list(res._fields)
        assert res._fields[:5] == ("flow_low", "flow_up", "matches", "valid", "count") and all(getattr(res, f) is v for f, v in zip(res._fields, res))
        for clone in (copy.copy(res), copy.deepcopy(res), pickle.loads(pickle.dumps(res)), FrameResult._make(res), res._replace()):
            assert clone is not res and same(clone, res), type(clone)
        assert copy.copy(res)[0] is res[0] and copy.deepcopy(res)[0] is not res[0]
        moved = res._replace(count=7)
        assert moved.count == 7 and len(moved) == n and moved.flow_low is res.flow_low and (moved.tracks is res.tracks)
        with pytest.raises(ValueError):
            res._replace(flow=1)
    assert five.tracks is None and six.tracks is six[5] and six._fields[5] == "tracks" and "tracks" not in five._asdict()
    assert len(five._replace(tracks=six.tracks)) == 6 and len(six._replace(tracks=None)) == 5


def test_session_with_tracks_needs_a_detector():
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.frames import FrameResult, FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    from focusflow_official_amd.tracks import TrackResult, TrackTable
    plain = FF_RAFT_FUSION(use_fusion=None).eval()
    with pytest.raises(ValueError, match="tracks"):
        FrameSequence(plain, tracks=True)
    with pytest.raises(ValueError, match="tracks"):
        FrameSequence(plain, tracks=64)
    with pytest.raises(ValueError, match="tracks"):
        FrameSequence(plain, keypoints=GoodFeatures(), tracks=4097)
    with pytest.raises(ValueError, match="tracks"):
        FrameSequence(plain, keypoints=GoodFeatures(), tracks=0)
    assert FrameSequence(plain, keypoints=GoodFeatures(), tracks=True)._slots == 500 and FrameSequence(plain, keypoints=GoodFeatures(100), tracks=64)._slots == 64
    assert FrameSequence(plain, keypoints=GoodFeatures()).tracks is None and FrameSequence(plain, keypoints=GoodFeatures(), tracks=False)._slots == 0
    # the result: five items as ever without tracks, a trailing sixth with them
    a, b = FrameResult(1, 2, 3, 4, 5), FrameResult(1, 2, 3, 4, 5, TrackResult(6, 7, 8))
    assert tuple(a) == (1, 2, 3, 4, 5) and a.tracks is None and (a.flow_low, a.flow_up, a.matches, a.valid, a.count) == (1, 2, 3, 4, 5)
    assert len(b) == 6 and b[-1] is b.tracks and b.tracks.ids == 6 and b.tracks.age == 7 and b.tracks.born == 8 and b.count == 5
    tb = TrackTable(2, 8, "cpu")
    assert tb.pos.shape == (2, 8, 2) and (tb.pos == -1).all() and (tb.ids == -1).all() and tb.ids.dtype == torch.int64
    assert tb.age.dtype == torch.int32 and not tb.age.any() and tb.next_id.tolist() == [0, 0] and not tb.live.any()
    saved = tb.state()
    tb.ids[0, 1], tb.age[0, 1], tb.next_id[0] = 5, 2, 6
    tb.pos[0, 1] = 3.5
    tb.reset()
    assert (tb.ids == -1).all() and (tb.pos == -1).all() and not tb.age.any() and tb.next_id.tolist() == [6, 0]      # ids go on counting
    tb.load_state(saved)
    assert tb.next_id.tolist() == [0, 0]


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_tracks_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "tracks.hip"))
    assert len(kernels) >= 4, kernels      # replenish, zero, scatter, advance
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"tracks.hip: kernels with scratch (bytes per lane): {spilled}"
    lds = max(int(k.get("LDS", "0")) for k in kernels)
    assert 32768 <= lds <= 65536, f"replenish keeps 4096 positions in LDS and fits the 64 KB a block may have: {lds}"


# ----------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------
def _dev(tb):
    return {k: torch.from_numpy(v).to(DEV) for k, v in tb.items()}


def _same(got, want, what):
    """Equal as values, a NaN equal to a NaN."""
    got, want = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.detach().cpu() for t in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    same = (got == want) | ((got != got) & (want != want)) if got.is_floating_point() else got == want
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} values differ"


def _same_table(got, want, what):
    for k in ("pos", "ids", "age", "next_id"):
        _same(got[k], want[k], f"{what}: {k}")


def _replenish_on_device(tb, pts, cnt, h, w, md):
    from focusflow_official_amd import ops
    d = _dev(tb)
    born, live = ops.tracks_replenish(d["pos"], d["ids"], d["age"], d["next_id"], torch.from_numpy(pts).to(DEV), torch.from_numpy(cnt).to(DEV), h, w, md)
    return d, born, live


def _check_replenish(tb, pts, cnt, h, w, md, what):
    want, born, live = R.replenish(tb, pts, cnt, h, w, md)
    got, gborn, glive = _replenish_on_device(tb, pts, cnt, h, w, md)
    _same_table(got, want, what)
    _same(gborn, born, what + ": born")
    _same(glive, live, what + ": live")
    return want, born, live


@pytest.mark.gpu
def test_replenish_hand_made():
    """B = 2, N = 8, M = 16 on a 64 x 64 frame."""
    full = {(1, s): (8.0 * s + 0.5, 40.25, 50 + s, s) for s in range(8)}
    some = {(0, 1): (20.0, 30.0, 7, 3), (0, 6): (50.5, 9.75, 9, 1)}
    dets = [(30, 30), (29, 30), (26, 38), (20, 30), (50, 0), (41, 10), (5, 5), (60, 60), (10, 50), (33, 55), (45, 45)]
    # an empty (all dead) table beside a full one
    pts, cnt = _points([dets, dets], 16)
    want, born, live = _check_replenish(_table(2, 8, full, next_id=3), pts, cnt, 64, 64, 10, "empty and full")
    assert born.tolist() == [8, 0] and live.tolist() == [8, 8] and want["ids"][0].tolist() == list(range(3, 11)) and want["ids"][1].tolist() == list(range(50, 58))
    # a table with two tracks (blocked detections, more open ones than free slots) beside count = 0
    pts, cnt = _points([dets, []], 16)
    want, born, live = _check_replenish(_table(2, 8, {**some, **full}, next_id=1 << 33), pts, cnt, 64, 64, 10, "two tracks and count 0")
    assert born.tolist() == [6, 0] and live.tolist() == [8, 8] and want["next_id"].tolist() == [(1 << 33) + 6, 1 << 33]      # seven open, six free
    assert R.blocked(_table(2, 8, some), pts, cnt, 64, 64, 10)[0, :11].tolist() == [False, True, False, True, True, True] + [False] * 5
    # fewer open detections than free slots, M = 1, min_distance = 0
    pts, cnt = _points([dets[:4], dets[:1]], 16)
    want, born, live = _check_replenish(_table(2, 8, some), pts, cnt, 64, 64, 10, "slots to spare")
    assert born.tolist() == [2, 1] and live.tolist() == [4, 1]
    _check_replenish(_table(2, 8, some), pts, cnt, 64, 64, 0, "min_distance 0")
    pts, cnt = _points([[(20, 31)], [(0, 0)]], 1)
    want, born, _ = _check_replenish(_table(2, 8, some), pts, cnt, 64, 64, 10, "M = 1")
    assert born.tolist() == [0, 1]
    # count beyond M is read as M; a detection outside the frame is passed over
    pts, _ = _points([dets[:10], [(64, 5), (5, 64), (5, 5)] + dets[:7]], 10)
    _check_replenish(_table(2, 8, some), pts, np.asarray([77, 10], np.int32), 64, 64, 10, "count beyond M, points outside the frame")


def _big_replenish_case(md):
    """B = 3, N = 700, M = 500 on 125 x 157.  Random tracks at sub-pixel positions right of x = 70; the strip left of it holds
    planted track / detection pairs at exactly min_distance and just inside or outside it."""
    rng = np.random.default_rng(7)
    b, n, m = 3, 700, 500
    tb = R.empty_table(b, n)
    tb["next_id"][:] = ((1 << 31) + 5, 1 << 40, 7)
    for bi, nlive in enumerate((40, 690, 300)):
        slots = np.sort(rng.choice(np.arange(8, n), nlive, replace=False))
        tb["pos"][bi, slots, 0] = rng.uniform(70, W - 1, nlive).astype(F32)
        tb["pos"][bi, slots, 1] = rng.uniform(0, H - 1, nlive).astype(F32)
        tb["ids"][bi, slots] = rng.permutation(nlive) + 1000
        tb["age"][bi, slots] = rng.integers(0, 9, nlive)
    pts = np.stack([rng.integers(0, W, (b, m)), rng.integers(0, H, (b, m))], axis=-1).astype(np.int32)
    below, above = np.nextafter(F32(30), F32(0)), np.nextafter(F32(30), F32(99))
    planted = [((4.0, 4.0), (4 + md, 4), False),                 # exactly min_distance on a row
               ((4.0, 34.0), (4 + md - 1, 34), md > 0),          # one pixel inside
               ((above, 64.0), (30 + md, 64), md > 0),           # 2^-19 px inside
               ((below, 94.0), (30 + md, 94), False),            # 2^-19 px outside
               ((4.5, 120.0), (4, 120), md > 0)]                 # half a pixel away
    if md == 10:
        planted.append(((40.0, 20.0), (46, 28), False))          # 6-8-10: dx dx + dy dy == 100 exactly
        planted.append(((52.25, 108.0), (46, 100), False))       # 6.25, 8: 103.0625
        planted.append(((51.75, 45.0), (46, 37), True))          # 5.75, 8: 97.0625
    for bi in range(b):
        for k, (p, d, _) in enumerate(planted):
            tb["pos"][bi, k], tb["ids"][bi, k], tb["age"][bi, k] = p, 500 + k, 1
            pts[bi, 3 * k + 1] = d
    cnt = np.asarray([m, m - 13, m], np.int32)
    for bi in range(b):
        pts[bi, cnt[bi]:] = -1
    return tb, pts, cnt, planted


@pytest.mark.gpu
@pytest.mark.parametrize("md", [10, 3, 0])
def test_replenish_is_exact(md):
    tb, pts, cnt, planted = _big_replenish_case(md)
    block = R.blocked(tb, pts, cnt, H, W, md)
    for bi in range(3):
        assert [bool(block[bi, 3 * k + 1]) for k in range(len(planted))] == [want for _, _, want in planted], f"the planted pairs of sample {bi}"
    want, born, live = _check_replenish(tb, pts, cnt, H, W, md, f"min_distance {md}")
    print(f"min_distance {md}: blocked {block.sum(1).tolist()} of {cnt.tolist()}, born {born.tolist()}, live {live.tolist()}")
    assert (want["next_id"] > 1 << 31).tolist() == [True, True, False] and int(want["ids"][0].max()) == (1 << 31) + 5 + int(born[0]) - 1
    if md:
        assert 0 < block[0].sum() < cnt[0] and born[0] == cnt[0] - block[0].sum()      # slots to spare: every open detection is born
    if md == 3:
        free = 700 - 690 - len(planted)
        assert born[1] == free > 0 and live[1] == 700 and cnt[1] - block[1].sum() > free      # a few free slots for many open detections
    if md == 0:
        assert not block.any() and live.tolist() == [40 + len(planted) + 500, 700, 300 + len(planted) + 395]
    # once more on the result: ids continue, the births of the first call block their own detections
    _check_replenish(want, pts, cnt, H, W, md, f"min_distance {md}, second call")


def _mask_case():
    rng = np.random.default_rng(3)
    b, n = 2, 300
    tb = R.empty_table(b, n)
    alive = rng.random((b, n)) < 0.7
    tb["pos"][..., 0] = rng.uniform(0, W - 1, (b, n)).astype(F32)
    tb["pos"][..., 1] = rng.uniform(0, H - 1, (b, n)).astype(F32)
    fixed = [(W - 1, H - 1), (0, 0), (10.5, 20.5), (10.75, 21.25), (W - 1.5, 0.49999997), (W - 1, 0), (0, H - 1), (77.0, 33.0), (77.25, 32.5)]
    tb["pos"][0, :len(fixed)] = np.asarray(fixed, F32)
    alive[0, :len(fixed)] = True
    tb["pos"][1, 5], alive[1, 5] = (W - 1, H - 1), True
    tb["ids"] = np.where(alive, np.arange(b * n).reshape(b, n), -1)
    tb["pos"][~alive] = -1
    return tb


@pytest.mark.gpu
def test_mask_and_advance_known_answers_on_the_device():
    """The hand-worked answers of test_restatement_of_mask_and_advance_known_answers, asked of the library."""
    from focusflow_official_amd import ops
    tb, flow = _known_mask_advance_case()
    d = _dev(tb)
    m = ops.tracks_mask(d["pos"], d["ids"], 5, 7)
    mt, valid, ids, age = ops.tracks_advance(d["pos"], d["ids"], d["age"], torch.from_numpy(flow).to(DEV), 0, 1, 5, 7)
    _assert_known_mask_advance(m.cpu().numpy(), {k: v.cpu().numpy() for k, v in d.items()}, mt.cpu().numpy(), valid.cpu().numpy(), ids.cpu().numpy(),
                               age.cpu().numpy())


@pytest.mark.gpu
def test_mask_is_exact():
    from focusflow_official_amd import ops
    tb = _mask_case()
    want = R.mask(tb, H, W)
    assert want[0, 0, H - 1, W - 1] == 255 and want[1, 0, H - 1, W - 1] == 255 and want[0, 0, 21, 11] == 255 and want[0, 0, 33, 77] == 255
    assert want[0, 0, 20, 10] == 0 and (want == 255).sum() < (tb["ids"] >= 0).sum()      # 10.5 rounds up; tracks share pixels
    d = _dev(tb)
    got = ops.tracks_mask(d["pos"], d["ids"], H, W)
    _same(got, want, "mask")
    out = torch.full((2, 1, H, W), 7.0, device=DEV)
    assert ops.tracks_mask(d["pos"], d["ids"], H, W, out=out) is out
    _same(out, want, "mask into out=")
    # an empty table, and a plane that is no multiple of four floats
    e = _dev(R.empty_table(1, 5))
    assert not ops.tracks_mask(e["pos"], e["ids"], 5, 7).any()
    one = _dev(_table(1, 5, {(0, 3): (6.0, 4.0, 1, 0)}))
    _same(ops.tracks_mask(one["pos"], one["ids"], 5, 7), R.mask(_table(1, 5, {(0, 3): (6.0, 4.0, 1, 0)}), 5, 7), "5 x 7")


def _advance_case():
    """B = 2, N = 4096 on 125 x 157 inside a 128 x 160 field: integers, the last row and column, random sub-pixels, dead slots;
    a flow of randn 6 with planted NaN and pushes out of the frame."""
    rng = np.random.default_rng(0)
    b, n = 2, 4096
    tb = R.empty_table(b, n, next_id=9)
    tb["pos"][..., 0] = rng.uniform(0, W - 1, (b, n)).astype(F32)
    tb["pos"][..., 1] = rng.uniform(0, H - 1, (b, n)).astype(F32)
    tb["pos"][:, 0:600] = np.floor(tb["pos"][:, 0:600])      # integer positions
    tb["pos"][:, 600:700, 0] = W - 1                          # the last column
    tb["pos"][:, 700:800, 1] = H - 1                          # the last row
    tb["pos"][:, 800] = (W - 1, H - 1)
    tb["pos"][:, 801] = (0, 0)
    tb["pos"][:, 802] = (np.nextafter(F32(W - 1), F32(0)), np.nextafter(F32(H - 1), F32(0)))
    alive = rng.random((b, n)) < 0.9
    alive[:, 800:803] = True
    tb["ids"] = np.where(alive, rng.permutation(b * n).reshape(b, n) + (1 << 35), -1)
    tb["age"] = np.where(alive, rng.integers(0, 50, (b, n)), 0).astype(np.int32)
    tb["pos"][~alive] = -1
    flow = (rng.standard_normal((b, 2, 128, 160)) * 6).astype(F32)
    return tb, flow


def _plant(flow, tb, left, top):
    """NaN and pushes out of the frame at the taps of some live slots; exact zeros under the corners."""
    flow = flow.copy()
    for bi in range(flow.shape[0]):
        live = np.flatnonzero(tb["ids"][bi] >= 0)
        for k, s in enumerate(live[5:45]):
            x0, y0 = int(np.floor(tb["pos"][bi, s, 0])), int(np.floor(tb["pos"][bi, s, 1]))
            flow[bi, k % 2, y0 + top, x0 + left] = np.nan if k < 20 else (400.0 if k % 4 < 2 else -400.0)
        flow[bi, :, top + H - 1, left + W - 1] = 0      # slot 800 stays on the corner: valid
        flow[bi, :, top, left] = (-0.0, 0.25)           # slot 801
    return flow


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sintel", "kitti"])
def test_advance_is_exact(mode):
    from focusflow_official_amd import ops
    left, top, hp, wp = R.pad_offsets(H, W, mode)
    assert (hp, wp) == (128, 160) and (left, top) == ((1, 1) if mode == "sintel" else (1, 0))
    tb, flow = _advance_case()
    flow = _plant(flow, tb, left, top)
    want, wm, wv, wi, wa = R.advance(tb, flow, left, top, H, W)
    # the input tells the definition from a blend whose a * b + c were contracted to FMAs
    _, fm, fv, _, _ = R.advance(tb, flow, left, top, H, W, blend=R._blend_fma)
    differ = ((wm != fm) & ~(np.isnan(wm) & np.isnan(fm))).any(-1)
    print(f"{mode}: an FMA-contracted blend differs from the definition in {int(differ.sum())} of {differ.size} rows; "
          f"{int(wv.sum())} valid of {int((tb['ids'] >= 0).sum())} live")
    assert differ.sum() > 0, "this input could not see a contracted blend"
    live = tb["ids"] >= 0
    assert 0 < wv.sum() < live.sum() and np.isnan(wm).any() and wv[:, 800].all() and (wm[:, 800, 2:] == (W - 1, H - 1)).all()
    assert (wm[:, 801] == np.asarray([0, 0, 0, 0.25], F32)).all()

    def run(field):
        d = _dev(tb)
        res = ops.tracks_advance(d["pos"], d["ids"], d["age"], field, left, top, H, W)
        _same_table(d, want, f"advance ({mode})")
        for g, w_, what in zip(res, (wm, wv, wi, wa), ("matches", "valid", "ids", "age")):
            _same(g, w_, f"advance ({mode}): {what}")
        return d

    run(torch.from_numpy(flow).to(DEV))
    # on integer positions the match is ff_keypoint_matches' as a value
    pts = torch.from_numpy(tb["pos"][:, :600].astype(np.int32)).to(DEV)
    km, kv = ops.keypoint_matches(pts, torch.full((2,), 600, dtype=torch.int32, device=DEV), torch.from_numpy(flow).to(DEV), left, top, H, W)
    rows = torch.from_numpy(live[:, :600] & ~np.isnan(wm[:, :600]).any(-1))
    assert int(rows.sum()) > 900
    _same(km.cpu()[rows], torch.from_numpy(wm[:, :600])[rows], "integer positions against keypoint_matches")
    _same(kv.cpu()[rows], torch.from_numpy(wv[:, :600])[rows], "integer positions against keypoint_matches: valid")
    # a strided flow_up: channels, rows and columns of a larger tensor; and into out=
    big = torch.zeros(2, 3, 132, 170, device=DEV)
    view = big[:, 1:, 2:130, 9:169]
    view.copy_(torch.from_numpy(flow))
    assert not view.is_contiguous()
    run(view)
    d = _dev(tb)
    outs = (torch.full((2, 4096, 4), 5.0, device=DEV), torch.full((2, 4096), 9, dtype=torch.uint8, device=DEV),
            torch.full((2, 4096), 9, dtype=torch.int64, device=DEV), torch.full((2, 4096), 9, dtype=torch.int32, device=DEV))
    res = ops.tracks_advance(d["pos"], d["ids"], d["age"], view, left, top, H, W, out=outs)
    assert all(a is b for a, b in zip(res, outs))
    _same(outs[0], wm, "out= matches")
    _same(outs[2], wi, "out= ids")


@pytest.mark.gpu
def test_wrappers_refuse_by_name():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    d = _dev(R.empty_table(1, 4))
    pos, ids, age, nid = d["pos"], d["ids"], d["age"], d["next_id"]
    pts, cnt = torch.zeros(1, 4, 2, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    flow = torch.zeros(1, 2, 8, 8, device=DEV)
    big = _dev(R.empty_table(1, 4097))
    for fn, word in ((lambda: ops.tracks_replenish(pos.double(), ids, age, nid, pts, cnt, 5, 7, 10), "pos"),
                     (lambda: ops.tracks_replenish(pos, ids.int(), age, nid, pts, cnt, 5, 7, 10), "ids"),
                     (lambda: ops.tracks_replenish(pos, ids, age.long(), nid, pts, cnt, 5, 7, 10), "age"),
                     (lambda: ops.tracks_replenish(pos, ids, age, nid.int(), pts, cnt, 5, 7, 10), "next_id"),
                     (lambda: ops.tracks_replenish(pos, ids, age, nid, pts.float(), cnt, 5, 7, 10), "points"),
                     (lambda: ops.tracks_replenish(pos, ids, age, nid, pts, cnt.long(), 5, 7, 10), "count"),
                     (lambda: ops.tracks_replenish(pos, ids, age, nid, pts, cnt, 5, 7, 33), "min_distance"),      # refused by the library
                     (lambda: ops.tracks_replenish(pos, ids, age, nid, pts, cnt, 5, 7, -1), "min_distance"),
                     (lambda: ops.tracks_replenish(pos, ids, age, nid, torch.zeros(1, 4097, 2, dtype=torch.int32, device=DEV), cnt, 5, 7, 10), "M = 4097"),
                     (lambda: ops.tracks_replenish(big["pos"], big["ids"], big["age"], big["next_id"], pts, cnt, 5, 7, 10), "N = 4097"),
                     (lambda: ops.tracks_replenish(pos, ids, age, nid, pts, cnt, 5, 7, 10, out=(cnt.long(), cnt)), "born"),
                     (lambda: ops.tracks_mask(pos[:, :, :1], ids, 5, 7), "pos"),
                     (lambda: ops.tracks_mask(big["pos"], big["ids"], 5, 7), "N = 4097"),
                     (lambda: ops.tracks_mask(pos, ids, 5, 7, out=torch.zeros(1, 1, 8, 8, device=DEV)), "out"),
                     (lambda: ops.tracks_advance(pos, ids, age, flow[:, :1], 0, 1, 5, 7), "flow_up"),
                     (lambda: ops.tracks_advance(pos, ids, age, flow, 2, 1, 5, 7), "left"),      # 2 + 7 > 8: refused by the library
                     (lambda: ops.tracks_advance(pos, ids, age, flow, 0, 4, 5, 7), "top"),
                     (lambda: ops.tracks_advance(pos, ids, age, flow, 0, 1, 5, 7, out=(flow, cnt, cnt, cnt)), "matches")):
        with pytest.raises(FocusFlowHipError, match=word):
            fn()
    _same_table(d, R.empty_table(1, 4), "a refused call leaves the table alone")


# ----------------------------------------------------------------------------
# the session
# ----------------------------------------------------------------------------
ITERS, FRAMES = 12, 6
SEED, SHIFT = 51, (3, -5)      # (what the flow of these frames does to the tracks is asserted, not assumed: _check_non_vacuous)


def _cfg():
    return Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))


@pytest.fixture(scope="module")
def models(det_sd):
    from focusflow_official_amd import FF_RAFT_FUSION
    from oracle.weights import det_tensor
    ff = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=_cfg())
    ff.load_state_dict(det_sd, strict=True)
    plain = FF_RAFT_FUSION(use_fusion=None)
    plain.load_state_dict({k: det_tensor(k, s) for k, s, _ in golden_spec("state_dict_spec_plain")}, strict=True)
    return {"ffraft": ff.to(DEV).eval(), "plain": plain.to(DEV).eval()}


def _u8_frames(b, h, w, frames, seed, shift):
    """A smooth random image that moves by `shift` per frame under a little noise, as a decoder delivers it: uint8 (B,H,W,3)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(b, 3, h // 4 + 2, w // 4 + 2, generator=g), size=(h, w), mode="bilinear", align_corners=False) * 255
    out = []
    for k in range(frames):
        img = torch.roll(base, shifts=(shift[0] * k, shift[1] * k), dims=(2, 3))
        if k:
            img = img + torch.randn(b, 3, h, w, generator=g) * 2
        out.append(img.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    return out


def _table_of(seq):
    return {k: t.detach().cpu().numpy().copy() for k, t in zip(("pos", "ids", "age", "next_id"), seq.tracks._tensors())}


_RUNS = {}


def _run(models, kind, graph, slots=True, max_corners=500):
    """One session over the six frames, every pair held to the restatement's session step (b); -> what the pairs showed.
    Cached: the tests below look at the same runs."""
    key = (kind, graph, slots, max_corners)
    if key in _RUNS:
        return _RUNS[key]
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    model, det = models[kind], GoodFeatures(max_corners=max_corners)
    frames = _u8_frames(1, H, W, FRAMES, SEED, SHIFT)
    seq = FrameSequence(model, raft_iters=ITERS, graph=graph, keypoints=det, tracks=slots)
    n = max_corners if slots is True else slots
    assert seq.tracks is None and seq.push(frames[0]) is None
    assert seq.tracks.n == n and not seq.tracks.live.any()
    ref = R.empty_table(1, n)
    pairs = []
    for t in range(FRAMES - 1):
        res = seq.push(frames[t + 1])
        what = f"{kind} graph={graph} slots={n} pair {t}"
        points, count = det.points(frames[t].to(DEV).permute(0, 3, 1, 2).float().contiguous())      # the unpadded first frame of the pair
        step = R.session_step(ref, points.cpu().numpy(), count.cpu().numpy(), res.flow_up.cpu().numpy(), H, W, det.min_distance)
        assert len(res) == 6 and res.matches.shape == (1, n, 4) and res.flow_up.shape == (1, 2, H, W)
        _same(res.matches, step["matches"], what + ": matches")
        _same(res.valid, step["valid"], what + ": valid")
        _same(res.tracks.ids, step["ids"], what + ": ids")
        _same(res.tracks.age, step["age"], what + ": age")
        _same(res.tracks.born, step["born"], what + ": born")
        _same(res.count, step["count"], what + ": count (live)")
        _same_table(_table_of(seq), step["table"], what + ": seq.tracks")
        if kind == "ffraft":
            _same(seq.mask1, step["mask1"], what + ": mask1")
        else:
            assert seq.mask1 is None
        died = int(((step["ids"] >= 0) & (step["valid"] == 0)).sum())
        free = n - (int(step["count"][0]) - int(step["born"][0]))      # before the replenish
        pairs.append({"res": [x.clone() for x in res[:5]], "mask1": None if seq.mask1 is None else seq.mask1.clone(), "born": int(step["born"][0]),
                      "live": int(step["count"][0]), "blocked": step["blocked"], "died": died, "max_age": int(step["age"].max()),
                      "detected": int(count[0]), "open": int(count[0]) - step["blocked"], "free": free, "flow_max": float(res.flow_up.abs().max())})
        print(what + ": " + ", ".join(f"{k} {v}" for k, v in pairs[-1].items() if k not in ("res", "mask1")))
        ref = step["table"]
    _RUNS[key] = {"pairs": pairs, "table": ref, "seq": seq, "det": det, "frames": frames}
    return _RUNS[key]


def _check_non_vacuous(pairs, what):
    """(d): the six frames exercise what the session is for."""
    assert max(p["max_age"] for p in pairs) >= 2, f"{what}: no track was followed over three pairs"
    assert sum(p["blocked"] for p in pairs) >= 1, f"{what}: no detection was blocked by a live track"
    assert sum(p["born"] for p in pairs[1:]) >= 1, f"{what}: no birth after the first pair"
    assert sum(p["died"] for p in pairs) >= 1, f"{what}: no track died"


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_tracks_equal_the_restatement(models, kind, graph):
    """(b) inside _run, (a) the first pair against the session without tracks, (d) non-vacuity."""
    from focusflow_official_amd.frames import FrameSequence
    run = _run(models, kind, graph)
    _check_non_vacuous(run["pairs"], f"{kind} graph={graph}")
    bare = FrameSequence(models[kind], raft_iters=ITERS, graph=graph, keypoints=run["det"])
    assert bare.push(run["frames"][0]) is None
    want = bare.push(run["frames"][1])
    assert len(want) == 5 and want.tracks is None
    flow_low, flow_up, matches, valid, count = run["pairs"][0]["res"]
    for x, y, name in ((flow_low, want.flow_low, "flow_low"), (flow_up, want.flow_up, "flow_up")):
        err = float((x.double() - y.double()).abs().max())
        print(f"{kind} graph={graph}: first pair, {name} with tracks against without: max |diff| {err:.3e}")
        assert err <= GRAPH_VS_EAGER and (graph or err == 0.0), f"{name}: {err:.3e}"
    _same(matches, want.matches.cpu(), "first pair: matches")
    _same(valid, want.valid.cpu(), "first pair: valid")
    _same(count, want.count.cpu(), "first pair: count")
    if kind == "ffraft":
        _same(run["pairs"][0]["mask1"], bare.mask1.cpu(), "first pair: mask1")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_graph_and_eager_end_with_identical_tables(models, kind):
    """(c): the capture's warm-up steps neither move tracks nor spend ids."""
    g, e = _run(models, kind, True), _run(models, kind, False)
    _same_table(g["table"], e["table"], f"{kind}: graph against eager after {FRAMES} frames")
    assert int(g["table"]["next_id"][0]) == sum(p["born"] for p in g["pairs"])      # every id was spent on a birth


@pytest.mark.gpu
def test_session_with_a_full_table(models):
    """tracks=64 under max_corners=100: more open detections than slots, so the table fills and births wait for deaths."""
    run = _run(models, "ffraft", True, slots=64, max_corners=100)
    pairs = run["pairs"]
    assert pairs[0]["open"] > 64 and pairs[0]["born"] == 64 and pairs[0]["live"] == 64      # the strongest 64 of the open detections
    assert any(p["open"] > p["free"] > 0 for p in pairs[1:]), "no later pair had more open detections than free slots"


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_session_reset_empties_the_table_and_ids_go_on(models, graph):
    """(e).  Runs last on the cached session: it moves it on."""
    run = _run(models, "plain", graph, slots=200)
    seq, det, frames = run["seq"], run["det"], run["frames"]
    spent = int(run["table"]["next_id"][0])
    assert spent > 0 and seq.tracks.live.any()
    seq.reset()
    assert not seq.tracks.live.any() and int(seq.tracks.next_id[0]) == spent and (seq.tracks.pos == -1).all() and not seq.tracks.age.any()
    assert seq.push(frames[2]) is None
    res = seq.push(frames[3])
    points, count = det.points(frames[2].to(DEV).permute(0, 3, 1, 2).float().contiguous())
    step = R.session_step(R.empty_table(1, 200, next_id=spent), points.cpu().numpy(), count.cpu().numpy(), res.flow_up.cpu().numpy(), H, W, det.min_distance)
    _same(res.matches, step["matches"], "after reset(): matches")
    _same(res.tracks.ids, step["ids"], "after reset(): ids")
    _same(res.tracks.age, step["age"], "after reset(): age")
    _same_table(_table_of(seq), step["table"], "after reset(): seq.tracks")
    born = int(res.tracks.born[0])
    live = res.tracks.ids[0][res.tracks.ids[0] >= 0]
    assert born > 0 and step["blocked"] == 0 and not res.tracks.age.any() and sorted(live.tolist()) == list(range(spent, spent + born))
    # a new shape drops the table with the other buffers
    other = _u8_frames(1, 128, 144, 2, SEED, SHIFT)
    assert seq.push(other[0]) is None and not seq.tracks.live.any() and int(seq.tracks.next_id[0]) == 0
    assert seq.push(other[1]).matches.shape == (1, 200, 4)
