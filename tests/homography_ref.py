"""Numpy restatement of csrc/homography.hip (ff_homography_ransac, ff_homography_residual) and of the hold of
ff_epipolar_ransac_hold: the yardstick of tests/test_homography.py.  The definition is that of include/focusflow_hip.h: a RANSAC
over 4-point homographies (DLT) in fp32, every operation rounded separately (numpy rounds every array operation to the dtype of
its operands, and nothing here fuses two).  What the definition shares with the epipolar check - the hash of the draws, the
frame constants, the elimination - is taken from tests/epipolar_ref.py, as the kernels take it from one header.  Nothing calls the
library."""
import numpy as np

import epipolar_ref as E
import tracks_ref as R

F32 = np.float32
U32 = np.uint32
NO_ROW, INLIER, NOT_CANDIDATE, OUTLIER, NO_VERDICT = E.NO_ROW, E.INLIER, E.NOT_CANDIDATE, E.OUTLIER, E.NO_VERDICT
MIN_SAMPLE = 4


def draws(seed, epoch, b, k, m):
    """Floyd's algorithm: the 4 distinct ranks below m >= 4 of hypotheses k (an int array (K)) -> (K,4) int64."""
    k = np.asarray(k, np.int64)
    picks = np.zeros(k.shape + (MIN_SAMPLE,), np.int64)
    for j in range(MIN_SAMPLE):
        n = m - MIN_SAMPLE + j
        t = (E.word(seed, epoch, b, MIN_SAMPLE * k + j) % U32(n + 1)).astype(np.int64)
        taken = (picks[..., :j] == t[..., None]).any(-1)
        picks[..., j] = np.where(taken, n, t)
    return picks


def system(x, y, xp, yp):
    """The rows of K samples, each (K,4) float32 -> the DLT systems (K,8,9): rows 2 j and 2 j + 1 belong to draw j."""
    K = x.shape[0]
    A = np.zeros((K, 8, 9), F32)
    one = np.ones_like(x)
    A[:, 0::2, 0], A[:, 0::2, 1], A[:, 0::2, 2] = x, y, one
    A[:, 0::2, 6], A[:, 0::2, 7], A[:, 0::2, 8] = -(xp * x), -(xp * y), -xp
    A[:, 1::2, 3], A[:, 1::2, 4], A[:, 1::2, 5] = x, y, one
    A[:, 1::2, 6], A[:, 1::2, 7], A[:, 1::2, 8] = -(yp * x), -(yp * y), -yp
    return A


def hypotheses(xn, seed, epoch, b, K):
    """xn (4,M) float32 normalised candidates, M >= 4 -> (h (K,9), good (K), picks (K,4)): the models with w > 0 on their own
    sample; not good: a pivot of 0, an unknown that is not finite, or w not strictly of one sign on the sample."""
    picks = draws(seed, epoch, b, np.arange(K), xn.shape[1])
    x, y, xp, yp = (xn[i][picks] for i in range(4))                      # (K,4)
    h, good = E.solve(system(x, y, xp, yp))
    with np.errstate(all="ignore"):
        w = (h[:, 6, None] * x + h[:, 7, None] * y) + h[:, 8, None]
    assert w.dtype == F32
    pos, neg = (w > 0).all(1), (w < 0).all(1)
    good = good & (pos | neg)
    h = np.where((good & neg)[:, None], -h, h)
    return h, good, picks


def transfer(h, x, y, xp, yp):
    """h (...,9) against rows of a broadcastable shape -> (num, den, w) float32: the one expression of the scoring pass and of
    the final flags."""
    h = [h[..., i] for i in range(9)]
    with np.errstate(all="ignore"):
        u = (h[0] * x + h[1] * y) + h[2]
        v = (h[3] * x + h[4] * y) + h[5]
        w = (h[6] * x + h[7] * y) + h[8]
        du, dv = u - xp * w, v - yp * w
        num = du * du + dv * dv
        den = w * w
    assert num.dtype == F32 and den.dtype == F32 and w.dtype == F32
    return num, den, w


def to_pixels(h, s, cx, cy):
    """The model of normalised coordinates -> H (3,3) of pixel coordinates: T^-1 Hn T, T = [[s, 0, -cx s], [0, s, -cy s], [0, 0, 1]]."""
    h = np.asarray(h, F32).reshape(3, 3)
    g = np.zeros((3, 3), F32)
    out = np.zeros((3, 3), F32)
    with np.errstate(all="ignore"):
        for i in range(3):
            g[i, 0], g[i, 1] = h[i, 0] * s, h[i, 1] * s
            g[i, 2] = h[i, 2] - (g[i, 0] * cx + g[i, 1] * cy)
        for j in range(3):
            out[0, j] = g[0, j] / s + cx * g[2, j]
            out[1, j] = g[1, j] / s + cy * g[2, j]
            out[2, j] = g[2, j]
    return out


def ransac(m, valid, h, w, threshold=1.0, hypotheses_=512, min_inliers=8, permille=500, planar_permille=900, seed=0, epoch=0, table=None, cull=False):
    """m (B,N,4) float32 [x, y, x', y'], valid (B,N) uint8, table: None or a tracks_ref table whose slots are the rows.
    -> dict(H (B,3,3), dist2 (B,N), status (B,N), inliers (B), candidates (B), ok (B), planar (B), valid (B,N), table or None,
    epoch: the epoch word after the call, best (B): the winning hypothesis or -1); the arguments are left alone."""
    m = np.asarray(m, F32)
    valid = np.asarray(valid, np.uint8)
    B, N, _ = m.shape
    K = int(hypotheses_)
    s, cx, cy, t, s2 = E.frame_constants(h, w, threshold)
    out = dict(H=np.zeros((B, 3, 3), F32), dist2=np.zeros((B, N), F32), status=np.zeros((B, N), np.uint8), inliers=np.zeros(B, np.int32),
               candidates=np.zeros(B, np.int32), ok=np.zeros(B, np.uint8), planar=np.zeros(B, np.uint8), valid=valid.copy(),
               table=None if table is None else R.copy_table(table), epoch=int(epoch) + 1, best=np.full(B, -1, np.int64))
    for b in range(B):
        with np.errstate(invalid="ignore"):
            row = ~(m[b, :, 0] < 0)                                      # a no-row holds x = -1
            finite = np.isfinite(m[b]).all(1)
            cand = row & finite & (valid[b] != 0) & (m[b, :, 0] >= 0)
            xn = np.stack([(m[b, :, 0] - cx) * s, (m[b, :, 1] - cy) * s, (m[b, :, 2] - cx) * s, (m[b, :, 3] - cy) * s])      # (4,N)
        M = int(cand.sum())
        count, best, hm = 0, -1, None
        if M >= MIN_SAMPLE:
            hs, good, _ = hypotheses(xn[:, cand], seed, epoch, b, K)
            num, den, wd = transfer(hs[:, None, :], *(xn[i, cand][None, :] for i in range(4)))      # (K,M)
            with np.errstate(all="ignore"):
                counts = np.where(good, ((wd > 0) & (num <= t * den)).sum(1), 0)
            best = int(counts.argmax())                                  # (the lowest k of equal counts)
            count, hm = int(counts[best]), hs[best]
        ok = M >= MIN_SAMPLE and count >= min_inliers and 1000 * count >= permille * M
        status = np.where(~row, NO_ROW, np.where(~cand, NOT_CANDIDATE, NO_VERDICT)).astype(np.uint8)
        dist2 = np.where(row, F32(np.inf), F32(-1)).astype(F32)
        if ok:
            num, den, wd = transfer(hm, *(xn[i] for i in range(4)))
            with np.errstate(all="ignore"):
                front = wd > 0
                inl = front & (num <= t * den)
                d = np.where(den > 0, num / den, np.where(inl, F32(0), F32(np.inf))) / s2
            status = np.where(cand, np.where(inl, INLIER, OUTLIER), status).astype(np.uint8)
            dist2 = np.where(row & finite & front, d, dist2).astype(F32)
            out["H"][b] = to_pixels(hm, s, cx, cy)
            dead = status == OUTLIER
            out["valid"][b][dead] = 0
            if out["table"] is not None and cull:
                tb = out["table"]
                tb["pos"][b][dead], tb["ids"][b][dead], tb["age"][b][dead] = -1, -1, 0
        out["status"][b], out["dist2"][b], out["ok"][b], out["candidates"][b], out["best"][b] = status, dist2, ok, M, best
        out["planar"][b] = ok and 1000 * count >= planar_permille * M
        out["inliers"][b] = count if ok else 0      # (the scoring pass and the flags share one expression: count == (status == 1).sum())
    return out


def residual(flow, H, ok):
    """flow (B,2,h,w) float32, H (B,3,3) float32, ok (B) -> (B,h,w) float32: |(x + u, y + v) - pi(H (x, y, 1))|^2, +inf where the
    map's w is not > 0, -1 over a sample without a verdict."""
    flow, H = np.asarray(flow, F32), np.asarray(H, F32)
    B, _, h, w = flow.shape
    out = np.full((B, h, w), F32(-1))
    y, x = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    for b in range(B):
        if not ok[b]:
            continue
        g = H[b].reshape(9)
        with np.errstate(all="ignore"):
            pu = (g[0] * x + g[1] * y) + g[2]
            pv = (g[3] * x + g[4] * y) + g[5]
            pw = (g[6] * x + g[7] * y) + g[8]
            dx, dy = (x + flow[b, 0]) - pu / pw, (y + flow[b, 1]) - pv / pw
            r = dx * dx + dy * dy
        assert r.dtype == F32
        out[b] = np.where(pw > 0, r, F32(np.inf))
    return out


def epipolar_hold(m, valid, h, w, hold, **kw):
    """tests/epipolar_ref.ransac under ff_epipolar_ransac_hold: a held sample gets no verdict - ok 0, F zero, candidate rows status
    4, dist2 +inf on rows, valid and the table untouched, inliers 0, candidates M -; the others are what they are unheld."""
    r = E.ransac(m, valid, h, w, **kw)
    m, valid = np.asarray(m, F32), np.asarray(valid, np.uint8)
    table = kw.get("table")
    for b in np.flatnonzero(np.asarray(hold) != 0):
        with np.errstate(invalid="ignore"):
            row = ~(m[b, :, 0] < 0)
            cand = row & np.isfinite(m[b]).all(1) & (valid[b] != 0) & (m[b, :, 0] >= 0)
        r["F"][b], r["ok"][b], r["inliers"][b], r["best"][b] = 0, 0, 0, -1
        r["status"][b] = np.where(~row, NO_ROW, np.where(~cand, NOT_CANDIDATE, NO_VERDICT))
        r["dist2"][b] = np.where(row, F32(np.inf), F32(-1))
        r["valid"][b] = valid[b]
        if table is not None:
            for k in ("pos", "ids", "age"):
                r["table"][k][b] = table[k][b]
    return r
