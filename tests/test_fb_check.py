"""Forward-backward consistency: csrc/fb_check.hip (ff_fb_dense, ff_fb_matches), their ops wrappers and
frames.FrameSequence(fb=...).

The definition is exact (include/focusflow_hip.h), so the kernels and the session are held to the numpy restatement of
tests/fb_ref.py with equality: there are no tolerances here.  The models, frames and shapes of the session tests are those of
tests/test_tracks.py."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import fb_ref as FB
import tracks_ref as R
import test_tracks as T
from test_tracks import models      # noqa: F401  (the module-scoped fixture: FF-RAFT on det_sd and the plain spec)

DEV = T.DEV
ENTRY_POINTS = ("ff_fb_dense", "ff_fb_matches")
H, W = T.H, T.W
F32 = np.float32
INF = F32(np.inf)
_same, _dev = T._same, T._dev


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
    assert "7 (unchanged): entry points only: ff_fb_dense, ff_fb_matches" in history
    lib.ff_abi_version.restype = ctypes.c_int
    assert lib.ff_abi_version() == int(re.search(r"#define FF_ABI_VERSION (\d+)", hdr).group(1)) == _hip.ABI_VERSION == 7


def test_wrappers_raise_on_cpu_tensors():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    field = torch.zeros(1, 2, 8, 8)
    with pytest.raises(FocusFlowHipError, match="fw"):
        ops.fb_dense(field, field, 0, 1, 5, 7)
    with pytest.raises(FocusFlowHipError, match="matches"):
        ops.fb_matches(torch.zeros(1, 4, 4), torch.zeros(1, 4, dtype=torch.uint8), field, 0, 1, 5, 7)


def test_frame_result_has_four_shapes():
    """What tests/test_tracks.py::test_frame_result_copies_and_pickles holds for the results without fb, for all four shapes."""
    import copy
    import pickle
    from focusflow_official_amd.frames import FBCheck, FBResult, FrameResult
    from focusflow_official_amd.tracks import TrackResult
    tr = TrackResult(torch.arange(4)[None], torch.zeros(1, 4, dtype=torch.int32), torch.tensor([4], dtype=torch.int32))
    fbs = (FBResult(torch.ones(1, 2, 3, 3), torch.zeros(1, 1, 3, 3), torch.ones(1, 1, 3, 3, dtype=torch.uint8), torch.ones(1, 4), torch.ones(1, 4, dtype=torch.uint8)),
           FBResult(torch.ones(1, 2, 3, 3), torch.zeros(1, 1, 3, 3), torch.ones(1, 1, 3, 3, dtype=torch.uint8), None, None))
    base = (torch.ones(2), torch.zeros(3), torch.ones(1, 4, 4), torch.ones(1, 4, dtype=torch.uint8), torch.tensor([4], dtype=torch.int32))
    five, six_t = FrameResult(*base), FrameResult(*base, tr)
    six_f, seven = FrameResult(*base[:2], None, None, None, fb=fbs[1]), FrameResult(*base, tr, fbs[0])

    def same(a, b):
        if isinstance(a, tuple):
            return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))

    for res, n in ((five, 5), (six_t, 6), (six_f, 6), (seven, 7)):
        assert len(res) == n and len(res._fields) == n and isinstance(res, FrameResult) and list(res._asdict()) == list(res._fields)
        assert res._fields[:5] == ("flow_low", "flow_up", "matches", "valid", "count") and all(getattr(res, f) is v for f, v in zip(res._fields, res))
        for clone in (copy.copy(res), copy.deepcopy(res), pickle.loads(pickle.dumps(res)), FrameResult._make(res), res._replace()):
            assert clone is not res and same(clone, res), type(clone)
        assert copy.copy(res)[0] is res[0] and copy.deepcopy(res)[0] is not res[0]
        moved = res._replace(count=7)
        assert moved.count == 7 and len(moved) == n and moved.flow_low is res.flow_low and moved.tracks is res.tracks and moved.fb is res.fb
        with pytest.raises(ValueError):
            res._replace(flow=1)
    assert five.fb is None and six_t.fb is None and six_f.tracks is None and "fb" not in five._asdict() and "fb" not in six_t._asdict()
    assert six_f.fb is six_f[5] and six_f._fields[5] == "fb" and seven._fields[5:] == ("tracks", "fb") and seven.tracks is seven[5] and seven.fb is seven[6]
    assert len(five._replace(fb=fbs[1])) == 6 and len(seven._replace(fb=None)) == 6 and len(seven._replace(tracks=None, fb=None)) == 5
    assert six_f.fb.point_err2 is None and six_f.fb.status is None and FBResult._fields == ("flow_bw", "err2", "occluded", "point_err2", "status")
    assert FBCheck() == (0.01, 0.5, None, True) and FBCheck._fields == ("alpha", "beta", "iters", "warm")


def test_session_refuses_a_bad_fb():
    from focusflow_official_amd import FF_RAFT_FUSION
    from focusflow_official_amd.frames import FBCheck, FrameSequence
    plain = FF_RAFT_FUSION(use_fusion=None).eval()
    for bad in (FBCheck(alpha=-1.0), FBCheck(beta=float("nan")), FBCheck(iters=0), "yes", 0.5):
        with pytest.raises(ValueError, match="fb"):
            FrameSequence(plain, fb=bad)
    assert FrameSequence(plain).fb is None and FrameSequence(plain, fb=False).fb is None and FrameSequence(plain, fb=True).fb == FBCheck()
    seq = FrameSequence(plain, fb=FBCheck(beta=2.0, iters=6, warm=False))      # fb requires nothing else
    assert seq.fb.beta == 2.0 and seq.fb.iters == 6 and seq.fb_mask is None


def _frame_5x7(u, v):
    """A (1,2,8,8) field whose 5 x 7 frame at left 0, top 1 holds (u, v); the padding holds 99: it is never read."""
    f = np.full((1, 2, 8, 8), 99.0, F32)
    f[0, 0, 1:6, 0:7], f[0, 1, 1:6, 0:7] = u, v
    return f


def _known_shift():
    """fw = (2, -1), bw = (-2, 1): the round trip closes wherever the target is inside."""
    return _frame_5x7(2.0, -1.0), _frame_5x7(-2.0, 1.0)


def _assert_known_shift(err2, occ):
    left_frame = np.zeros((5, 7), bool)
    left_frame[0, :], left_frame[:, 5:] = True, True      # y - 1 < 0; x + 2 > 6
    assert err2.shape == (1, 1, 5, 7) and occ.shape == (1, 1, 5, 7) and occ.dtype == np.uint8 and err2.dtype == F32
    assert (occ[0, 0] == left_frame).all() and (err2[0, 0][left_frame] == INF).all() and (err2[0, 0][~left_frame] == 0).all()


def _known_block():
    """fw = (0.5, 0.5), so every target has four taps of weight 1/4; bw = (-0.5, -0.5) but for a 2 x 2 block at x 3..4, y 2..3,
    whose u is 4 too large: a pixel that reaches k taps of the block (its weights 1/4 each: k = 1, 2 or 4) ends k px off."""
    fw, bw = _frame_5x7(0.5, 0.5), _frame_5x7(-0.5, -0.5)
    bw[0, 0, 1 + 2:1 + 4, 3:5] = 3.5
    return fw, bw


def _assert_known_block(err2, occ):
    want = np.zeros((5, 7), F32)
    want[1:4, 2:5] = np.asarray([[1, 2, 1], [2, 4, 2], [1, 2, 1]], F32) ** 2      # taps x, x + 1 and y, y + 1: the pre-image is x 2..4, y 1..3
    want[4, :], want[:, 6] = INF, INF                                              # y + 0.5 > 4; x + 0.5 > 6
    assert (err2[0, 0] == want).all(), err2[0, 0]
    assert (occ[0, 0] == (want > 0)).all() and occ[0, 0, 1:4, 2:5].all() and occ[0, 0, :4, :6].sum() == 9


def _known_boundary():
    """alpha = 0, beta = 1.  fw = (1, 0) and bw = 0: every round trip ends exactly 1 px off, err2 == bound: consistent.  One bw
    tap of 2^-23 makes 1 + ub the next float above 1: not consistent.  The pixel x = 5 lands exactly on x' = W - 1: inside."""
    fw, bw = _frame_5x7(1.0, 0.0), _frame_5x7(0.0, 0.0)
    bw[0, 0, 1 + 2, 1] = F32(2.0 ** -23)      # the target of pixel (0, 2)
    return fw, bw


def _assert_known_boundary(err2, occ):
    above = np.nextafter(F32(1), F32(2))
    want = np.ones((5, 7), F32)
    want[:, 6] = INF                           # x + 1 = 7 > W - 1
    want[2, 0] = above * above                 # (rounded to fp32 by numpy: 1 + 2^-22)
    assert want[2, 0] > 1 and (err2[0, 0] == want).all(), err2[0, 0]
    occluded = np.zeros((5, 7), bool)
    occluded[:, 6], occluded[2, 0] = True, True
    assert (occ[0, 0] == occluded).all() and not occ[0, 0, :, 5].any()


def _known_nan():
    """A NaN in fw: the target left the frame.  A NaN in a bw tap: inconsistent, with a NaN error.  (The tap is (2, 0): targets
    have x0 >= 2 and y0 >= 0, so no other target reaches it as its x1 or y1 tap, where 0 * NaN would count as well.)"""
    fw, bw = _known_shift()
    fw[0, 0, 1 + 2, 1] = np.nan               # pixel (1, 2)
    bw[0, 1, 1 + 0, 2] = np.nan               # the target of pixel (0, 1)
    return fw, bw


def _assert_known_nan(err2, occ):
    assert err2[0, 0, 2, 1] == INF and occ[0, 0, 2, 1] == 1 and np.isnan(err2[0, 0, 1, 0]) and occ[0, 0, 1, 0] == 1
    rest = np.ones((5, 7), bool)
    rest[2, 1] = rest[1, 0] = False
    want_e, want_o = FB.dense(*_known_shift(), 0, 1, 5, 7)
    assert (err2[0, 0][rest] == want_e[0, 0][rest]).all() and (occ[0, 0][rest] == want_o[0, 0][rest]).all()


KNOWN = ((_known_shift, _assert_known_shift, (0.01, 0.5)), (_known_block, _assert_known_block, (0.01, 0.5)),
         (_known_boundary, _assert_known_boundary, (0.0, 1.0)), (_known_nan, _assert_known_nan, (0.01, 0.5)))


def _known_rows():
    """Seven rows on the boundary case's fields (alpha 0, beta 1): -> (matches, valid, table)."""
    m = np.asarray([[[-1, -1, -1, -1],            # no row
                     [3, 1, 4, 1],                # exactly 1 px off: consistent
                     [0, 2, 1, 2],                # the planted tap: inconsistent
                     [6, 3, 7, 3],                # the target left the frame
                     [5, 0, 6, 0],                # lands on x' = W - 1: inside, consistent
                     [0.5, 2, 1.5, 2],            # half of the planted tap, 1.5 + 2^-24 rounds to 1.5: consistent
                     [2, 2, np.nan, 2]]], F32)    # a NaN target: left the frame
    valid = np.asarray([[0, 1, 1, 0, 1, 1, 0]], np.uint8)
    tb = R.empty_table(1, 7, next_id=20)
    for s in (1, 2, 4, 5):                        # (the advance killed the slots of rows 3 and 6 already)
        tb["pos"][0, s], tb["ids"][0, s], tb["age"][0, s] = m[0, s, 2:], 10 + s, s
    return m, valid, tb


def _assert_known_rows(err2, status, valid, tb, had_table):
    above = np.nextafter(F32(1), F32(2))
    assert status[0].tolist() == [0, 1, 3, 2, 1, 1, 2] and valid[0].tolist() == [0, 1, 0, 0, 1, 1, 0]
    assert err2[0].tolist() == [-1, 1, above * above, INF, 1, 1, INF]
    if had_table:
        assert tb["ids"][0].tolist() == [-1, 11, -1, -1, 14, 15, -1] and tb["age"][0].tolist() == [0, 1, 0, 0, 4, 5, 0]
        assert tb["pos"][0].tolist() == [[-1, -1], [4, 1], [-1, -1], [-1, -1], [6, 0], [1.5, 2], [-1, -1]] and tb["next_id"].tolist() == [20]


def test_restatement_known_answers():
    for make, check, (alpha, beta) in KNOWN:
        fw, bw = make()
        check(*FB.dense(fw, bw, 0, 1, 5, 7, alpha, beta))
    m, valid, tb = _known_rows()
    _, bw = _known_boundary()
    e, s, v, out = FB.matches(m, valid, bw, 0, 1, 5, 7, 0.0, 1.0, table=tb)
    _assert_known_rows(e, s, v, out, True)
    assert tb["ids"][0].tolist() == [-1, 11, 12, -1, 14, 15, -1] and valid[0].tolist() == [0, 1, 1, 0, 1, 1, 0]      # (the arguments are left alone)
    e, s, v, out = FB.matches(m, valid, bw, 0, 1, 5, 7, 0.0, 1.0)
    _assert_known_rows(e, s, v, None, False)
    assert out is None


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_fb_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_spills
    kernels = scan_spills.scan(os.path.join(scan_spills.CSRC, "fb_check.hip"))
    assert len(kernels) >= 3, kernels      # dense with a 32-bit and with a 64-bit index, matches
    spilled = {k["name"]: int(k.get("ScratchSize", "0")) for k in kernels if int(k.get("ScratchSize", "0")) > 0}
    assert not spilled, f"fb_check.hip: kernels with scratch (bytes per lane): {spilled}"


# ----------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fields(left, top, fw=None):
    """B = 2, 128 x 160 fields around a 125 x 157 frame: fw, bw ~ 6 randn with
      * a region of the integer shift (3, -2) whose bw is the exact negative: consistent pixels, err2 == 0;
      * a region of the sub-pixel shift (1.25, 0.5) whose bw is the negative under noise of 1.1 px: both verdicts near the bound,
        through blends that an FMA would round differently;
      * NaN and +-400 pushes in fw, right of both regions; targets exactly on the last column, the last row and the corner."""
    rng = np.random.default_rng(11)
    if fw is None:
        fw = (rng.standard_normal((2, 2, 128, 160)) * 6).astype(F32)
    else:
        fw = fw.copy()
    bw = (rng.standard_normal((2, 2, 128, 160)) * 6).astype(F32)
    fw[:, 0, top + 20:top + 60, left + 30:left + 90], fw[:, 1, top + 20:top + 60, left + 30:left + 90] = 3.0, -2.0
    bw[:, 0, top + 10:top + 70, left + 25:left + 100], bw[:, 1, top + 10:top + 70, left + 25:left + 100] = -3.0, 2.0
    fw[:, 0, top + 75:top + 115, left + 20:left + 120], fw[:, 1, top + 75:top + 115, left + 20:left + 120] = 1.25, 0.5
    noise = (rng.standard_normal((2, 2, 50, 120)) * 1.1).astype(F32)
    bw[:, :, top + 70:top + 120, left + 15:left + 135] = np.asarray([-1.25, -0.5], F32)[None, :, None, None] + noise
    for k in range(40):
        y, x = int(rng.integers(0, H)), int(rng.integers(125, W))
        fw[k % 2, k % 2, top + y, left + x] = np.nan if k < 20 else (400.0 if k % 4 < 2 else -400.0)
    for b in range(2):
        fw[b, :, top + 5, left + 100] = (W - 1 - 100, 0)             # onto the last column
        fw[b, :, top + 100, left + 7] = (0.5, H - 1 - 100)           # onto the last row
        fw[b, :, top + 64, left + 150] = (W - 1 - 150, H - 1 - 64)   # onto the corner
        fw[b, :, top + H - 1, left + W - 1] = 0                      # stays on the corner
    return fw, bw


@pytest.fixture(scope="module", params=["sintel", "kitti"])
def dense_case(request):
    """The fields, and the restatement computed once: the definition and the FMA-contracted variant."""
    left, top, hp, wp = R.pad_offsets(H, W, request.param)
    assert (hp, wp) == (128, 160) and (left, top) == ((1, 1) if request.param == "sintel" else (1, 0))
    fw, bw = _fields(left, top)
    want = FB.dense(fw, bw, left, top, H, W)
    fma = FB.dense(fw, bw, left, top, H, W, contracted=True)
    return {"mode": request.param, "left": left, "top": top, "fw": fw, "bw": bw, "want": want, "fma": fma}


@pytest.mark.gpu
def test_dense_is_exact(dense_case):
    from focusflow_official_amd import ops
    c = dense_case
    left, top, fw, bw, (we, wo), (fe, fo) = c["left"], c["top"], c["fw"], c["bw"], c["want"], c["fma"]
    # the input tells the definition from a contracted one, and shows both verdicts, an exact zero, +inf and a NaN
    differ = (we != fe) & ~(np.isnan(we) & np.isnan(fe))
    print(f"{c['mode']}: an FMA-contracted check differs from the definition in {int(differ.sum())} of {differ.size} errors and "
          f"{int((wo != fo).sum())} verdicts; {int(wo.sum())} of {wo.size} pixels occluded")
    assert differ.sum() > 0, "this input could not see a contracted round trip"
    assert 0 < wo.sum() < wo.size and (we == 0).sum() >= 2 * 40 * 60 and np.isinf(we).any()
    assert not wo[:, 0, 20:60, 30:90].any() and 0 < wo[:, 0, 80:110, 25:115].sum() < 2 * 30 * 90      # the two planted regions
    for b in range(2):      # the targets on the last column, the last row and the corner are inside
        assert all(np.isfinite(we[b, 0, y, x]) for y, x in ((5, 100), (100, 7), (64, 150), (H - 1, W - 1)))

    def check(got, what):
        _same(got[0], we, f"dense ({c['mode']}, {what}): err2")
        _same(got[1], wo, f"dense ({c['mode']}, {what}): occluded")

    check(ops.fb_dense(_t(fw), _t(bw), left, top, H, W), "contiguous")
    # strided views of larger tensors, fw and bw strided differently: odd row strides, ...
    big_f, big_b = torch.zeros(2, 3, 132, 170, device=DEV), torch.zeros(2, 2, 130, 164, device=DEV)
    vf, vb = big_f[:, 1:, 2:130, 9:169], big_b[:, :, 1:129, 3:163]
    vf.copy_(_t(fw)), vb.copy_(_t(bw))
    assert not vf.is_contiguous() and not vb.is_contiguous() and vf.stride() != vb.stride()
    check(ops.fb_dense(vf, vb, left, top, H, W), "odd row stride")
    # ... rows of a multiple of four floats from a 16-byte aligned column, and from a column that is not
    wide = torch.zeros(2, 2, 128, 168, device=DEV)
    for c0, what in ((4, "row stride 168, aligned"), (1, "row stride 168, off alignment")):
        v = wide[:, :, :, c0:c0 + 160]
        v.copy_(_t(fw))
        check(ops.fb_dense(v, _t(bw), left, top, H, W), what)
    # ... and into out=
    outs = (torch.full((2, 1, H, W), 7.0, device=DEV), torch.full((2, 1, H, W), 9, dtype=torch.uint8, device=DEV))
    res = ops.fb_dense(_t(fw), vb, left, top, H, W, out=outs)
    assert res[0] is outs[0] and res[1] is outs[1]
    check(outs, "out=")
    # ... and into outputs that start off 16-byte / 4-byte alignment
    buf_e, buf_o = torch.full((2 * H * W + 1,), 7.0, device=DEV), torch.full((2 * H * W + 3,), 9, dtype=torch.uint8, device=DEV)
    for outs in ((buf_e[1:].view(2, 1, H, W), buf_o[:2 * H * W].view(2, 1, H, W)), (buf_e[:2 * H * W].view(2, 1, H, W), buf_o[3:].view(2, 1, H, W))):
        check(ops.fb_dense(_t(fw), _t(bw), left, top, H, W, out=outs), "out= off alignment")
    # other thresholds: nothing but the frame's edge and NaN is occluded under a huge beta; alpha alone
    for alpha, beta in ((0.0, 3e38), (0.05, 0.0)):
        want = FB.dense(fw, bw, left, top, H, W, alpha, beta)
        got = ops.fb_dense(_t(fw), _t(bw), left, top, H, W, alpha, beta)
        _same(got[0], want[0], f"alpha {alpha} beta {beta}: err2")
        _same(got[1], want[1], f"alpha {alpha} beta {beta}: occluded")


@pytest.mark.gpu
def test_dense_known_answers_on_the_device():
    """B = 1, 5 x 7 in 8 x 8: a plane of 35 elements is no multiple of any vector width.  The hand-worked answers, asked of the
    library: contiguous, as the first 7 columns of rows of 8, and in rows of 7."""
    from focusflow_official_amd import ops
    for make, check, (alpha, beta) in KNOWN:
        fw, bw = make()
        e, o = ops.fb_dense(_t(fw), _t(bw), 0, 1, 5, 7, alpha, beta)
        check(e.cpu().numpy(), o.cpu().numpy())
        e, o = ops.fb_dense(_t(fw)[..., :7], _t(bw)[..., :7], 0, 1, 5, 7, alpha, beta)
        check(e.cpu().numpy(), o.cpu().numpy())
        e, o = ops.fb_dense(_t(fw[..., :7]), _t(bw[..., :7]), 0, 1, 5, 7, alpha, beta)
        check(e.cpu().numpy(), o.cpu().numpy())
    m, valid, tb = _known_rows()
    _, bw = _known_boundary()
    for table in (True, False):
        d, v = _dev(tb), _t(valid)
        e, s = ops.fb_matches(_t(m), v, _t(bw), 0, 1, 5, 7, 0.0, 1.0, table=(d["pos"], d["ids"], d["age"]) if table else None)
        _assert_known_rows(e.cpu().numpy(), s.cpu().numpy(), v.cpu().numpy(), {k: t.cpu().numpy() for k, t in d.items()}, table)
        if not table:
            T._same_table(d, tb, "no table given: the table is left alone")


@pytest.fixture(scope="module")
def point_case():
    """N = 4096 rows as ops.tracks_advance leaves them (test_tracks' table: integers, the last row and column, sub-pixels, dead
    slots) on the fields above; the restatement computed once."""
    left, top, _, _ = R.pad_offsets(H, W, "sintel")
    tb, flow = T._advance_case()
    fw, bw = _fields(left, top, fw=T._plant(flow, tb, left, top))
    adv, m, valid, _, _ = R.advance(tb, fw, left, top, H, W)
    want = FB.matches(m, valid, bw, left, top, H, W, table=adv)
    fma = FB.matches(m, valid, bw, left, top, H, W, contracted=True)
    return {"left": left, "top": top, "tb": tb, "fw": fw, "bw": bw, "adv": adv, "m": m, "valid": valid, "want": want, "fma": fma}


@pytest.mark.gpu
def test_matches_are_exact(point_case):
    from focusflow_official_amd import ops
    c = point_case
    left, top, bw, adv, (we, ws, wv, wt) = c["left"], c["top"], c["bw"], c["adv"], c["want"]
    counts = np.bincount(ws.ravel(), minlength=4)
    differ = (we != c["fma"][0]) & ~(np.isnan(we) & np.isnan(c["fma"][0]))
    print(f"status 0 / 1 / 2 / 3: {counts.tolist()}; an FMA-contracted check differs in {int(differ.sum())} rows")
    assert (counts > 0).all() and differ.sum() > 0 and (wt["ids"] >= 0).sum() == counts[1] and (adv["ids"] >= 0).sum() == counts[1] + counts[3]
    # the rows come from the library's own advance
    d = _dev(c["tb"])
    m, valid, _, _ = ops.tracks_advance(d["pos"], d["ids"], d["age"], _t(c["fw"]), left, top, H, W)
    _same(m, c["m"], "advance: matches")
    T._same_table(d, adv, "advance")
    # with the table: status-3 slots die, all others are bit-unchanged (the restatement says which)
    m_before = m.clone()
    e, s = ops.fb_matches(m, valid, _t(bw), left, top, H, W, table=(d["pos"], d["ids"], d["age"]))
    for g, w_, what in ((e, we, "err2"), (s, ws, "status"), (valid, wv, "valid")):
        _same(g, w_, f"matches with the table: {what}")
    T._same_table(d, wt, "the culled table")
    _same(m, m_before.cpu(), "matches are not written")
    keep = torch.from_numpy(ws != FB.INCONSISTENT)
    for k in ("pos", "ids", "age"):
        assert torch.equal(d[k].cpu()[keep], torch.from_numpy(adv[k])[keep]), f"{k}: a slot whose row is not inconsistent changed"
    # without the table only `valid` changes; into out=; a strided bw
    d2, v2 = _dev(adv), _t(c["valid"])
    big = torch.zeros(2, 2, 130, 164, device=DEV)
    vb = big[:, :, 1:129, 3:163]
    vb.copy_(_t(bw))
    outs = (torch.full((2, 4096), 5.0, device=DEV), torch.full((2, 4096), 9, dtype=torch.uint8, device=DEV))
    res = ops.fb_matches(_t(c["m"]), v2, vb, left, top, H, W, out=outs)
    assert res[0] is outs[0] and res[1] is outs[1]
    for g, w_, what in ((outs[0], we, "err2"), (outs[1], ws, "status"), (v2, wv, "valid")):
        _same(g, w_, f"matches without the table: {what}")
    T._same_table(d2, adv, "no table given")
    # rows at integer positions equal fb_dense at those pixels, as values
    de, do = (t.cpu().numpy() for t in ops.fb_dense(_t(c["fw"]), _t(bw), left, top, H, W))
    pos = c["tb"]["pos"][:, :600].astype(np.int64)
    rows = (ws[:, :600] != FB.NO_ROW) & ~np.isnan(c["m"][:, :600]).any(-1)      # (a NaN beside the pixel reaches the row's blend as 0 * NaN)
    bi = np.arange(2)[:, None]
    at_e, at_o = de[bi, 0, pos[..., 1], pos[..., 0]], do[bi, 0, pos[..., 1], pos[..., 0]]
    assert rows.sum() > 900 and (c["m"][:, :600, :2][rows] == pos[rows]).all()
    _same(at_e[rows], we[:, :600][rows], "integer positions against fb_dense: err2")
    _same(at_o[rows], (ws[:, :600][rows] != FB.CONSISTENT).astype(np.uint8), "integer positions against fb_dense: the verdict")
    assert ((ws[:, :600][rows] == FB.LEFT_FRAME) == np.isinf(at_e[rows])).all()


@pytest.mark.gpu
def test_matches_of_a_detector(point_case):
    """Rows as ops.keypoint_matches writes them, count < N: the rows beyond the count are no rows."""
    from focusflow_official_amd import ops
    c = point_case
    left, top, fw, bw = c["left"], c["top"], c["fw"], c["bw"]
    rng = np.random.default_rng(5)
    n = 300
    pts = np.stack([rng.integers(0, W, (2, n)), rng.integers(0, H, (2, n))], axis=-1).astype(np.int32)
    pts[:, :40, 0], pts[:, :40, 1] = rng.integers(31, 88, (2, 40)), rng.integers(21, 58, (2, 40))      # some in the consistent region
    cnt = np.asarray([n, 187], np.int32)
    pts[1, 187:] = -1
    m, valid = ops.keypoint_matches(_t(pts), _t(cnt), _t(fw), left, top, H, W)
    want_e, want_s, want_v, _ = FB.matches(m.cpu().numpy(), valid.cpu().numpy(), bw, left, top, H, W)
    assert (want_s[1, 187:] == FB.NO_ROW).all() and (want_s[0] != FB.NO_ROW).all() and (want_s == FB.CONSISTENT).sum() >= 30
    e, s = ops.fb_matches(m, valid, _t(bw), left, top, H, W)
    for g, w_, what in ((e, want_e, "err2"), (s, want_s, "status"), (valid, want_v, "valid")):
        _same(g, w_, f"detector rows: {what}")


@pytest.mark.gpu
def test_wrappers_refuse_by_name():
    from focusflow_official_amd import ops
    from focusflow_official_amd._hip import FocusFlowHipError
    d = _dev(R.empty_table(1, 4))
    pos, ids, age = d["pos"], d["ids"], d["age"]
    flow = torch.zeros(1, 2, 8, 8, device=DEV)
    m, valid = torch.full((1, 4, 4), -1.0, device=DEV), torch.zeros(1, 4, dtype=torch.uint8, device=DEV)
    big = _dev(R.empty_table(1, 4097))
    nan = float("nan")
    for fn, word in ((lambda: ops.fb_dense(flow.double(), flow, 0, 1, 5, 7), "fw"),
                     (lambda: ops.fb_dense(flow, flow.half(), 0, 1, 5, 7), "bw"),
                     (lambda: ops.fb_dense(flow[:, :1], flow, 0, 1, 5, 7), "fw"),
                     (lambda: ops.fb_dense(flow, flow[:, :, :7], 0, 1, 5, 7), "bw"),
                     (lambda: ops.fb_dense(flow, torch.zeros(2, 2, 8, 8, device=DEV), 0, 1, 5, 7), "bw"),
                     (lambda: ops.fb_dense(flow, flow, 2, 1, 5, 7), "left"),      # 2 + 7 > 8: refused by the library
                     (lambda: ops.fb_dense(flow, flow, 0, 4, 5, 7), "top"),
                     (lambda: ops.fb_dense(flow, flow, -1, 1, 5, 7), "left"),
                     (lambda: ops.fb_dense(flow, flow, 0, 1, 0, 7), "H = 0"),
                     (lambda: ops.fb_dense(flow, flow, 0, 1, 5, 7, alpha=-0.01), "alpha"),
                     (lambda: ops.fb_dense(flow, flow, 0, 1, 5, 7, beta=-1.0), "beta"),
                     (lambda: ops.fb_dense(flow, flow, 0, 1, 5, 7, alpha=nan), "alpha"),
                     (lambda: ops.fb_dense(flow, flow, 0, 1, 5, 7, out=(torch.zeros(1, 1, 5, 7, device=DEV), torch.zeros(1, 1, 5, 7, device=DEV))), "occluded"),
                     (lambda: ops.fb_dense(flow, flow, 0, 1, 5, 7, out=(torch.zeros(1, 1, 8, 8, device=DEV), valid)), "err2"),
                     (lambda: ops.fb_matches(m.double(), valid, flow, 0, 1, 5, 7), "matches"),
                     (lambda: ops.fb_matches(m[:, :, :3], valid, flow, 0, 1, 5, 7), "matches"),
                     (lambda: ops.fb_matches(m, valid.bool(), flow, 0, 1, 5, 7), "valid"),
                     (lambda: ops.fb_matches(m, valid[:, :3], flow, 0, 1, 5, 7), "valid"),
                     (lambda: ops.fb_matches(m, valid, flow[:, :1], 0, 1, 5, 7), "bw"),
                     (lambda: ops.fb_matches(torch.zeros(1, 4097, 4, device=DEV), torch.zeros(1, 4097, dtype=torch.uint8, device=DEV), flow, 0, 1, 5, 7), "N = 4097"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 1, 5, 7, table=(pos, ids)), "table"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 1, 5, 7, table=(pos, ids, None)), "table"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 1, 5, 7, table=(pos, ids.int(), age)), "ids"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 1, 5, 7, table=(big["pos"], big["ids"], big["age"])), "table"),
                     (lambda: ops.fb_matches(m, valid, flow, 2, 1, 5, 7, table=(pos, ids, age)), "left"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 4, 5, 7, table=(pos, ids, age)), "top"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 1, 5, 7, alpha=-1.0, table=(pos, ids, age)), "alpha"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 1, 5, 7, beta=nan, table=(pos, ids, age)), "beta"),
                     (lambda: ops.fb_matches(m, valid, flow, 0, 1, 5, 7, out=(valid, valid)), "err2")):
        with pytest.raises(FocusFlowHipError, match=word):
            fn()
    T._same_table(d, R.empty_table(1, 4), "a refused call leaves the table alone")
    live = T._table(1, 4, {(0, 1): (2.0, 2.0, 7, 3)})
    d = _dev(live)
    rows = torch.tensor([[[-1, -1, -1, -1], [1, 2, 2, 2], [-1, -1, -1, -1], [-1, -1, -1, -1]]], dtype=torch.float32, device=DEV)
    with pytest.raises(FocusFlowHipError, match="alpha"):
        ops.fb_matches(rows, torch.tensor([[0, 1, 0, 0]], dtype=torch.uint8, device=DEV), flow + 3, 0, 1, 5, 7, alpha=-1.0, table=(d["pos"], d["ids"], d["age"]))
    T._same_table(d, live, "a refused call leaves a live table alone")


# ----------------------------------------------------------------------------
# the session
# ----------------------------------------------------------------------------
ITERS, FRAMES = T.ITERS, T.FRAMES
NO_CULL = (0.0, 3e38)
_RUNS = {}


def _frames():
    return T._u8_frames(1, H, W, FRAMES, T.SEED, T.SHIFT)


def _np(t):
    return t.detach().cpu().numpy()


def _check_dense(res, alpha, beta, what):
    """The dense items against the restatement fed with the pair's own flows (unpadded: the taps never leave the frame)."""
    assert res.fb.flow_bw.shape == (1, 2, H, W) and res.fb.err2.shape == (1, 1, H, W) and res.fb.occluded.dtype == torch.uint8
    we, wo = FB.dense(_np(res.flow_up), _np(res.fb.flow_bw), 0, 0, H, W, alpha, beta)
    _same(res.fb.err2, we, what + ": dense err2")
    _same(res.fb.occluded, wo, what + ": occluded")


def _run_tracks(models, kind, graph, fb, max_corners=500):
    """One tracks session over the six frames; with fb = (alpha, beta) every pair is held to tracks_ref.session_step followed by
    fb_ref.  -> what the pairs showed.  Cached."""
    key = (kind, graph, fb)
    if key in _RUNS:
        return _RUNS[key]
    from focusflow_official_amd.frames import FBCheck, FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    model, det, frames = models[kind], GoodFeatures(max_corners=max_corners), _frames()
    seq = FrameSequence(model, raft_iters=ITERS, graph=graph, keypoints=det, tracks=True, fb=None if fb is None else FBCheck(alpha=fb[0], beta=fb[1]))
    assert seq.push(frames[0]) is None and seq.fb_mask is None
    ref = R.empty_table(1, max_corners)
    pairs = []
    for t in range(FRAMES - 1):
        res = seq.push(frames[t + 1])
        what = f"{kind} graph={graph} fb={fb} pair {t}"
        pair = {"res": [x.clone() for x in res[:5]], "ids": res.tracks.ids.clone(), "age": res.tracks.age.clone(), "born": res.tracks.born.clone(),
                "table": T._table_of(seq)}
        if fb is None:
            assert len(res) == 6 and res.fb is None
        else:
            assert len(res) == 7 and res[-1] is res.fb and res._fields[-2:] == ("tracks", "fb") and res.fb.status.shape == (1, max_corners)
            points, count = det.points(frames[t].to(DEV).permute(0, 3, 1, 2).float().contiguous())
            step = R.session_step(ref, _np(points), _np(count), _np(res.flow_up), H, W, det.min_distance)
            we, ws, wv, culled = FB.matches(step["matches"], step["valid"], _np(res.fb.flow_bw), 0, 0, H, W, fb[0], fb[1], table=step["table"])
            _same(res.matches, step["matches"], what + ": matches")
            _same(res.tracks.ids, step["ids"], what + ": ids")
            _same(res.tracks.age, step["age"], what + ": age")
            _same(res.tracks.born, step["born"], what + ": born")
            _same(res.count, step["count"], what + ": count (live)")
            _same(res.fb.status, ws, what + ": status")
            _same(res.fb.point_err2, we, what + ": point_err2")
            _same(res.valid, wv, what + ": valid")
            T._same_table(pair["table"], culled, what + ": seq.tracks (the culled table)")
            _check_dense(res, fb[0], fb[1], what)
            if kind == "ffraft":
                _same(seq.mask1, step["mask1"], what + ": mask1")
                _same(seq.fb_mask, R.pad_replicate(R.mask(step["table"], H, W)), what + ": fb_mask (the advanced, unculled table)")
            else:
                assert seq.mask1 is None and seq.fb_mask is None
            ref = culled
            pair.update(status=ws, err2=we, ids_before=step["ids"], flow_bw=res.fb.flow_bw.clone())
            print(what + f": status 0 / 1 / 2 / 3 {np.bincount(ws.ravel(), minlength=4).tolist()}, born {int(step['born'][0])}, "
                  f"occluded {int(res.fb.occluded.sum())} of {H * W}")
        pairs.append(pair)
    _RUNS[key] = {"pairs": pairs, "seq": seq, "table": T._table_of(seq)}
    return _RUNS[key]


def _threshold(models, kind):
    """Non-vacuity is constructed: (1) an eager session whose check culls nothing equals the eager session without fb, item for
    item and table for table; (2, 3) the median of its first pair's finite errors over the consistent rows becomes beta.  The
    threshold is a test input, not a tolerance."""
    key = ("beta", kind)
    if key in _RUNS:
        return _RUNS[key]
    free, bare = _run_tracks(models, kind, False, NO_CULL), _run_tracks(models, kind, False, None)
    for t, (a, b) in enumerate(zip(free["pairs"], bare["pairs"])):
        for x, y, name in zip(a["res"] + [a["ids"], a["age"], a["born"]], b["res"] + [b["ids"], b["age"], b["born"]],
                              ("flow_low", "flow_up", "matches", "valid", "count", "ids", "age", "born")):
            _same(x, y.cpu(), f"{kind}: a check that culls nothing against no check, pair {t}: {name}")
        T._same_table(a["table"], b["table"], f"{kind}: a check that culls nothing against no check, pair {t}: the table")
        assert not (a["status"] == FB.INCONSISTENT).any()
    first = free["pairs"][0]
    errs = first["err2"][(first["status"] == FB.CONSISTENT) & np.isfinite(first["err2"])]
    assert len(np.unique(errs)) >= 2, f"{kind}: the first pair's round-trip errors do not differ: {np.unique(errs)}"
    beta = float(F32(np.median(errs)))
    print(f"{kind}: first pair, {len(errs)} consistent rows, err2 min {errs.min():.4g} median {beta:.6g} max {errs.max():.4g}")
    _RUNS[key] = (0.0, beta)
    return _RUNS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_equals_the_restatement(models, kind, graph):
    fb = _threshold(models, kind)
    run = _run_tracks(models, kind, graph, fb)      # (every pair is held to the restatement inside)
    pairs = run["pairs"]
    # (4) on the first pair the check kills a track and lets one live
    first = pairs[0]["status"]
    assert (first == FB.INCONSISTENT).sum() >= 1 and (first == FB.CONSISTENT).sum() >= 1, np.bincount(first.ravel(), minlength=4)
    assert (pairs[0]["table"]["ids"][first == FB.INCONSISTENT] == -1).all() and (pairs[0]["table"]["ids"][first == FB.CONSISTENT] >= 0).all()
    # (5) a slot the check freed is refilled by a later replenish, with a new id
    refilled = 0
    for t, p in enumerate(pairs[:-1]):
        for s in np.flatnonzero(p["status"][0] == FB.INCONSISTENT):
            old = int(p["ids_before"][0, s])
            refilled += any(int(q["ids_before"][0, s]) > old for q in pairs[t + 1:])
    print(f"{kind} graph={graph}: {refilled} slots freed by the check were refilled with a new id")
    assert refilled >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_graph_and_eager_end_with_identical_tables(models, kind):
    """The capture's warm-up steps (which run the check, and cull) leave no trace in the table."""
    fb = _threshold(models, kind)
    g, e = _run_tracks(models, kind, True, fb), _run_tracks(models, kind, False, fb)
    T._same_table(g["table"], e["table"], f"{kind}: graph against eager after {FRAMES} frames")
    for t, (a, b) in enumerate(zip(g["pairs"], e["pairs"])):
        assert (a["status"] == b["status"]).all(), f"{kind}: pair {t}: status of graph and eager"


def _detector_rows(points, count, flow_up):
    """What ff_keypoint_matches writes for the unpadded field: -> (matches (B,N,4) float32, valid (B,N) uint8)."""
    b, n, _ = points.shape
    m, valid = np.full((b, n, 4), -1, F32), np.zeros((b, n), np.uint8)
    for bi in range(b):
        for k in range(int(count[bi])):
            x, y = int(points[bi, k, 0]), int(points[bi, k, 1])
            tx, ty = F32(x) + flow_up[bi, 0, y, x], F32(y) + flow_up[bi, 1, y, x]
            m[bi, k] = (x, y, tx, ty)
            valid[bi, k] = 0 <= tx <= W - 1 and 0 <= ty <= H - 1
    return m, valid


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
def test_session_with_a_detector_only(models, kind, graph):
    """No table: the point items are the restatement on the detector's rows, only `valid` is gated; fb_mask is the detector on
    the newest frame."""
    from focusflow_official_amd.frames import FBCheck, FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    alpha, beta = _threshold(models, kind)
    det, frames = GoodFeatures(), _frames()
    seq = FrameSequence(models[kind], raft_iters=ITERS, graph=graph, keypoints=det, fb=FBCheck(alpha=alpha, beta=beta))
    assert seq.push(frames[0]) is None and seq.tracks is None
    for t in range(2):
        res = seq.push(frames[t + 1])
        what = f"{kind} graph={graph} detector only, pair {t}"
        assert len(res) == 6 and res.tracks is None and res[-1] is res.fb and res._fields[-1] == "fb"
        points, count = det.points(frames[t].to(DEV).permute(0, 3, 1, 2).float().contiguous())
        _same(res.count, count.cpu(), what + ": count")
        m, valid = _detector_rows(_np(points), _np(count), _np(res.flow_up))
        we, ws, wv, _ = FB.matches(m, valid, _np(res.fb.flow_bw), 0, 0, H, W, alpha, beta)
        _same(res.matches, m, what + ": matches")
        _same(res.fb.status, ws, what + ": status")
        _same(res.fb.point_err2, we, what + ": point_err2")
        _same(res.valid, wv, what + ": valid")
        _check_dense(res, alpha, beta, what)
        assert (ws == FB.NO_ROW).sum() == 500 - int(count[0]) and (ws == FB.INCONSISTENT).any() and (ws == FB.CONSISTENT).any(), np.bincount(ws.ravel())
        if kind == "ffraft":
            mask2 = det(frames[t + 1].to(DEV).permute(0, 3, 1, 2).float().contiguous())
            _same(seq.fb_mask, R.pad_replicate(_np(mask2)), what + ": fb_mask (the detector on the newest frame)")
        else:
            assert seq.fb_mask is None


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_session_with_caller_masks(models, graph):
    """FF-RAFT without a detector: the dense items, no point items; the backward pair reads the mask that came with the newest
    frame, the next forward pair reads it as mask1."""
    from focusflow_official_amd.frames import FrameSequence
    frames = _frames()
    g = torch.Generator().manual_seed(3)
    masks = [((torch.rand(1, 1, H, W, generator=g) < 0.02) * 255).to(torch.uint8) for _ in range(3)]
    seq = FrameSequence(models["ffraft"], raft_iters=ITERS, graph=graph, fb=True)
    assert seq.push(frames[0], mask=masks[0]) is None
    for t in range(2):
        res = seq.push(frames[t + 1], mask=masks[t + 1])
        what = f"caller masks graph={graph}, pair {t}"
        assert len(res) == 6 and res.matches is None and res.valid is None and res.count is None and res.fb.point_err2 is None and res.fb.status is None
        _check_dense(res, 0.01, 0.5, what)
        _same(seq.fb_mask, R.pad_replicate(masks[t + 1].float().numpy()), what + ": fb_mask")
        _same(seq.mask1, R.pad_replicate(masks[t].float().numpy()), what + ": mask1")
        assert 0 < int(res.fb.occluded.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ffraft", "plain"])
@pytest.mark.parametrize("warm_start", [True, False], ids=["warm_start", "cold_session"])
def test_session_backward_flow_is_the_models(models, kind, warm_start):
    """Eager: the backward flow equals a by-hand model(image2, image1, ...) call with the same arguments; fb.iters and
    warm=False are honoured (and with them, the session's own warm_start or its absence)."""
    from focusflow_official_amd import ops
    from focusflow_official_amd.frames import FBCheck, FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    model, frames = models[kind], _frames()
    left, top, hp, wp = ops.pad_offsets(H, W)
    for check in (FBCheck(), FBCheck(iters=5), FBCheck(warm=False), FBCheck(iters=7, warm=False)):
        seq = FrameSequence(model, raft_iters=ITERS, graph=False, warm_start=warm_start, keypoints=GoodFeatures(), tracks=True, fb=check)
        seq.push(frames[0])
        seq.push(frames[1])
        res = seq.push(frames[2])      # (the second pair: with warm_start the forward flow started from the first pair's)
        what = f"{kind} warm_start={warm_start} {check}"
        kw = {}
        if check.warm:
            start = -ops.forward_interpolate(res.flow_low)
            kw = dict(flow_init=start)
            assert start.abs().max() > 0
        with torch.no_grad():
            _, want = model(seq._img2, seq._img1, seq.fb_mask, None, raft_iters=check.iters or ITERS, test_mode=True, **kw)
        _same(res.fb.flow_bw, want[:, :, top:top + H, left:left + W].cpu(), what + ": flow_bw")
        if check.warm:
            _same(seq._fb_init, start.cpu(), what + ": the backward flow's start")
            if warm_start:
                _same(seq.flow_init, (-start).cpu(), what + ": flow_init is left as forward_interpolate wrote it")
        else:
            assert seq._fb_init is None
    # the variants differ from each other: the arguments reach the model
    flows = {}
    for check in (FBCheck(), FBCheck(iters=5), FBCheck(warm=False)):
        seq = FrameSequence(model, raft_iters=ITERS, graph=False, warm_start=warm_start, keypoints=GoodFeatures(), fb=check)
        seq.push(frames[0])
        flows[check] = seq.push(frames[1]).fb.flow_bw.clone()
    a, b, c = flows.values()
    assert not torch.equal(a, b) and not torch.equal(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_session_reset_and_a_new_shape(models, graph):
    """reset() and a change of (B,H,W) treat the new buffers like the others."""
    from focusflow_official_amd.frames import FrameSequence
    from focusflow_official_amd.keypoints import GoodFeatures
    frames = _frames()
    alpha, beta = _threshold(models, "ffraft")
    fresh = _run_tracks(models, "ffraft", graph, (alpha, beta))["pairs"][0]
    seq = _run_tracks(models, "ffraft", graph, (alpha, beta))["seq"]      # (runs last on the cached session: it moves it on)
    spent = int(seq.tracks.next_id[0])
    seq.reset()
    assert seq.fb_mask is None and not seq.tracks.live.any() and not seq._fb_init.any()
    assert seq.push(frames[0]) is None
    res = seq.push(frames[1])
    # the first pair again, from an empty table and a cold start: the same statuses, ids shifted by what was spent
    _same(res.fb.status, fresh["status"], f"graph={graph}: after reset(): status")
    _same(res.fb.point_err2, fresh["err2"], f"graph={graph}: after reset(): point_err2")
    _same(res.fb.flow_bw, fresh["flow_bw"].cpu(), f"graph={graph}: after reset(): flow_bw")
    live = fresh["ids_before"] >= 0
    assert (res.tracks.ids.cpu().numpy()[live] == fresh["ids_before"][live] + spent).all()
    other = T._u8_frames(1, 128, 144, 2, T.SEED, T.SHIFT)
    assert seq.push(other[0]) is None and not seq.tracks.live.any() and seq.fb_mask is None
    res = seq.push(other[1])
    assert res.fb.err2.shape == (1, 1, 128, 144) and res.fb.flow_bw.shape == (1, 2, 128, 144) and seq.fb_mask.shape == (1, 1, 128, 144)
    we, wo = FB.dense(_np(res.flow_up), _np(res.fb.flow_bw), 0, 0, 128, 144, alpha, beta)
    _same(res.fb.err2, we, "a new shape: dense err2")
    _same(res.fb.occluded, wo, "a new shape: occluded")
