"""Numpy restatement of csrc/fb_check.hip (ff_fb_dense, ff_fb_matches): the yardstick of tests/test_fb_check.py.  The definition
is that of include/focusflow_hip.h: fp32, every operation rounded separately (numpy rounds every array operation to the dtype of
its operands, and nothing here fuses two), the bilinear blend of tracks_ref.  Nothing calls the library.

`contracted=True` computes what a compiler that contracts a * b + c to FMAs makes of the same source: NOT the definition.  The
tests assert that their input tells the two apart."""
import numpy as np

import tracks_ref as R

F32 = np.float32
NO_ROW, CONSISTENT, LEFT_FRAME, INCONSISTENT = 0, 1, 2, 3      # status of a match row


def _sum_sq(a, b, contracted):
    """a a + b b."""
    return R._fma(a, a, b * b) if contracted else (a * a) + (b * b)


def round_trip(X, Y, xt, yt, bw, left, top, h, w, alpha, beta, contracted=False):
    """X, Y, xt, yt: (B,K) float32 start points and forward targets; bw: (B,2,Hp,Wp) float32, the frame at (left, top).
    -> (err2 (B,K) float32, inconsistent (B,K) bool).  Where the target lies outside the frame (or is a NaN) err2 = +inf and
    nothing of bw counts."""
    bw = np.asarray(bw, F32)
    alpha, beta = F32(alpha), F32(beta)
    blend = R._blend_fma if contracted else R._blend
    assert all(a.dtype == F32 for a in (X, Y, xt, yt))
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (xt >= 0) & (xt <= F32(w - 1)) & (yt >= 0) & (yt <= F32(h - 1))      # (a NaN compares false)
        x0 = np.clip(np.nan_to_num(np.floor(xt), nan=0.0, posinf=w - 1, neginf=0.0), 0, w - 1).astype(np.int64)
        y0 = np.clip(np.nan_to_num(np.floor(yt), nan=0.0, posinf=h - 1, neginf=0.0), 0, h - 1).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        fx, fy = xt - x0.astype(F32), yt - y0.astype(F32)
        bi = np.arange(bw.shape[0])[:, None]
        ub, vb = (blend(f[bi, y0 + top, x0 + left], f[bi, y0 + top, x1 + left], f[bi, y1 + top, x0 + left], f[bi, y1 + top, x1 + left], fx, fy)
                  for f in (bw[:, 0], bw[:, 1]))
        du, dv = (xt + ub) - X, (yt + vb) - Y
        err2 = _sum_sq(du, dv, contracted)
        fu, fv = xt - X, yt - Y
        mf, mb = _sum_sq(fu, fv, contracted), _sum_sq(ub, vb, contracted)
        bound = R._fma(np.full_like(mf, alpha), mf + mb, np.full_like(mf, beta)) if contracted else (alpha * (mf + mb)) + beta
        assert err2.dtype == F32 and bound.dtype == F32
        bad = ~inside | ~(err2 <= bound)                                               # (a NaN anywhere: inconsistent)
    return np.where(inside, err2, F32(np.inf)).astype(F32), bad


def dense(fw, bw, left, top, h, w, alpha=0.01, beta=0.5, contracted=False):
    """fw, bw: (B,2,Hp,Wp) float32.  -> (err2 (B,1,h,w) float32, occluded (B,1,h,w) uint8)."""
    fw = np.asarray(fw, F32)
    b = fw.shape[0]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    X = np.broadcast_to(xs.astype(F32).reshape(1, -1), (b, h * w))
    Y = np.broadcast_to(ys.astype(F32).reshape(1, -1), (b, h * w))
    with np.errstate(invalid="ignore", over="ignore"):
        xt = X + fw[:, 0, top:top + h, left:left + w].reshape(b, -1)
        yt = Y + fw[:, 1, top:top + h, left:left + w].reshape(b, -1)
    err2, bad = round_trip(X, Y, xt, yt, bw, left, top, h, w, alpha, beta, contracted)
    return err2.reshape(b, 1, h, w), bad.astype(np.uint8).reshape(b, 1, h, w)


def matches(m, valid, bw, left, top, h, w, alpha=0.01, beta=0.5, table=None, contracted=False):
    """m (B,N,4) float32 [x, y, x', y'], valid (B,N) uint8, table: None or a tracks_ref table whose slots are the rows.
    -> (err2 (B,N) float32, status (B,N) uint8, valid (B,N) uint8, table or None); the arguments are left alone."""
    m = np.asarray(m, F32)
    with np.errstate(invalid="ignore"):
        row = ~(m[..., 0] < 0)                        # a no-row holds x = -1
    err2, bad = round_trip(m[..., 0], m[..., 1], m[..., 2], m[..., 3], bw, left, top, h, w, alpha, beta, contracted)
    status = np.where(~row, NO_ROW, np.where(valid == 0, LEFT_FRAME, np.where(bad, INCONSISTENT, CONSISTENT))).astype(np.uint8)
    err2 = np.where(status == NO_ROW, F32(-1), np.where(status == LEFT_FRAME, F32(np.inf), err2)).astype(F32)
    if table is not None:
        table = R.copy_table(table)
        dead = status == INCONSISTENT
        table["pos"][dead], table["ids"][dead], table["age"][dead] = -1, -1, 0
    return err2, status, (status == CONSISTENT).astype(np.uint8), table
