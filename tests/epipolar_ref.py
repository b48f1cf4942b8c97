"""Numpy restatement of csrc/epipolar.hip (ff_epipolar_ransac): the yardstick of tests/test_epipolar.py.  The definition is that
of include/focusflow_hip.h: a RANSAC over 8-point fundamental matrices in fp32, every operation rounded separately (numpy rounds
every array operation to the dtype of its operands, and nothing here fuses two); the draws come from a 32-bit integer hash with
exact wrap-around.  Nothing calls the library.

Hypotheses are carried as arrays over k, so a call costs a few dozen array operations per elimination step."""
import numpy as np

import tracks_ref as R

F32 = np.float32
U32 = np.uint32
NO_ROW, INLIER, NOT_CANDIDATE, OUTLIER, NO_VERDICT = 0, 1, 2, 3, 4      # status of a match row
MIN_SAMPLE = 8


def mix(x):
    """lowbias32 on uint32 arrays (array arithmetic wraps around silently)."""
    shape = np.shape(x)
    x = np.array(x, U32).reshape(-1)
    x ^= x >> U32(16)
    x *= U32(0x7feb352d)
    x ^= x >> U32(15)
    x *= U32(0x846ca68b)
    x ^= x >> U32(16)
    return x.reshape(shape)


def word(seed, epoch, b, counter):
    """The 32-bit word of (seed, epoch, sample, counter); counter may be an array."""
    with np.errstate(over="ignore"):
        h = mix(U32((int(seed) + 0x9e3779b9) & 0xffffffff))
        h = mix(h ^ U32(int(epoch) & 0xffffffff))
        h = mix(h ^ U32(b))
        return mix(h ^ np.asarray(counter, U32))


def draws(seed, epoch, b, k, m):
    """Floyd's algorithm: the 8 distinct ranks below m >= 8 of hypotheses k (an int array (K)) -> (K,8) int64."""
    k = np.asarray(k, np.int64)
    picks = np.zeros(k.shape + (MIN_SAMPLE,), np.int64)
    for j in range(MIN_SAMPLE):
        n = m - MIN_SAMPLE + j
        t = (word(seed, epoch, b, MIN_SAMPLE * k + j) % U32(n + 1)).astype(np.int64)
        taken = (picks[..., :j] == t[..., None]).any(-1)
        picks[..., j] = np.where(taken, n, t)
    return picks


def frame_constants(h, w, threshold):
    """-> (s, cx, cy, t, s2) as float32: made in double and rounded once, as the host side of the library does."""
    s = F32(2.0 / (h + w))
    threshold = float(F32(threshold))                  # (the C ABI takes a float)
    t = F32(threshold * threshold * float(s) * float(s))
    return s, F32((w - 1) / 2.0), F32((h - 1) / 2.0), t, F32(float(s) * float(s))


def solve(A):
    """A (K,8,9) float32: elimination with full pivoting and back-substitution with the free unknown 1.
    -> (f (K,9) float32, good (K) bool: every step met a pivot > 0 and f is finite)."""
    A = np.array(A, F32)
    K = A.shape[0]
    ar = np.arange(K)
    perm = np.tile(np.arange(9), (K, 1))
    good = np.ones(K, bool)
    with np.errstate(all="ignore"):
        for p in range(8):
            mag = np.abs(A[:, p:, p:])
            mag = np.where(np.isnan(mag), F32(-1), mag).reshape(K, -1)
            flat = mag.argmax(1)                          # (the first of equal entries in (row, column) order: a strict >)
            good &= mag[ar, flat] > 0
            pr, pc = p + flat // (9 - p), p + flat % (9 - p)
            rows_p, rows_r = A[ar, p, :].copy(), A[ar, pr, :].copy()
            A[ar, p, :], A[ar, pr, :] = rows_r, rows_p
            cols_p, cols_c = A[ar, :, p].copy(), A[ar, :, pc].copy()
            A[ar, :, p], A[ar, :, pc] = cols_c, cols_p
            a, c = perm[ar, p].copy(), perm[ar, pc].copy()
            perm[ar, p], perm[ar, pc] = c, a
            for r in range(p + 1, 8):
                factor = A[:, r, p] / A[:, p, p]
                A[:, r, p + 1:] = A[:, r, p + 1:] - factor[:, None] * A[:, p, p + 1:]
        z = np.ones((K, 9), F32)
        for i in range(7, -1, -1):
            acc = A[:, i, 8].copy()
            for c in range(i + 1, 8):
                acc = acc + A[:, i, c] * z[:, c]
            z[:, i] = (-acc) / A[:, i, i]
        f = np.zeros((K, 9), F32)
        f[ar[:, None], perm] = z
        assert f.dtype == F32 and A.dtype == F32
        good &= np.isfinite(f).all(1)
    return f, good


def sampson(f, x, y, xp, yp):
    """f (...,9) against rows x, y, xp, yp of a broadcastable shape -> (num, den) float32: the one expression of the scoring
    pass and of the final flags."""
    f = [f[..., i] for i in range(9)]
    with np.errstate(all="ignore"):
        fx0 = (f[0] * x + f[1] * y) + f[2]
        fx1 = (f[3] * x + f[4] * y) + f[5]
        fx2 = (f[6] * x + f[7] * y) + f[8]
        ft0 = (f[0] * xp + f[3] * yp) + f[6]
        ft1 = (f[1] * xp + f[4] * yp) + f[7]
        e = (xp * fx0 + yp * fx1) + fx2
        num = e * e
        den = ((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1
    assert num.dtype == F32 and den.dtype == F32
    return num, den


def to_pixels(f, s, cx, cy):
    """The model of normalised coordinates -> F (3,3) of pixel coordinates: T^t F T, T = [[s, 0, -cx s], [0, s, -cy s], [0, 0, 1]]."""
    f = np.asarray(f, F32).reshape(3, 3)
    g = np.zeros((3, 3), F32)
    for i in range(3):
        g[i, 0], g[i, 1] = f[i, 0] * s, f[i, 1] * s
        g[i, 2] = f[i, 2] - (g[i, 0] * cx + g[i, 1] * cy)
    out = np.zeros((3, 3), F32)
    for j in range(3):
        out[0, j], out[1, j] = s * g[0, j], s * g[1, j]
        out[2, j] = g[2, j] - (out[0, j] * cx + out[1, j] * cy)
    return out


def hypotheses(xn, seed, epoch, b, K):
    """xn (4,M) float32 normalised candidates, M >= 8 -> (f (K,9), good (K), picks (K,8))."""
    m = xn.shape[1]
    picks = draws(seed, epoch, b, np.arange(K), m)
    x, y, xp, yp = (xn[i][picks] for i in range(4))                      # (K,8)
    A = np.stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, np.ones_like(x)], axis=2)
    f, good = solve(A)
    return f, good, picks


def ransac(m, valid, h, w, threshold=1.0, hypotheses_=512, min_inliers=16, permille=500, seed=0, epoch=0, table=None, cull=True):
    """m (B,N,4) float32 [x, y, x', y'], valid (B,N) uint8, table: None or a tracks_ref table whose slots are the rows.
    -> dict(F (B,3,3), dist2 (B,N), status (B,N), inliers (B), candidates (B), ok (B), valid (B,N), table or None, epoch: the
    epoch word after the call, best (B): the winning hypothesis or -1); the arguments are left alone."""
    m = np.asarray(m, F32)
    valid = np.asarray(valid, np.uint8)
    B, N, _ = m.shape
    K = int(hypotheses_)
    s, cx, cy, t, s2 = frame_constants(h, w, threshold)
    out = dict(F=np.zeros((B, 3, 3), F32), dist2=np.zeros((B, N), F32), status=np.zeros((B, N), np.uint8), inliers=np.zeros(B, np.int32),
               candidates=np.zeros(B, np.int32), ok=np.zeros(B, np.uint8), valid=valid.copy(), table=None if table is None else R.copy_table(table),
               epoch=int(epoch) + 1, best=np.full(B, -1, np.int64))
    for b in range(B):
        with np.errstate(invalid="ignore"):
            row = ~(m[b, :, 0] < 0)                                      # a no-row holds x = -1
            finite = np.isfinite(m[b]).all(1)
            cand = row & finite & (valid[b] != 0) & (m[b, :, 0] >= 0)
            xn = np.stack([(m[b, :, 0] - cx) * s, (m[b, :, 1] - cy) * s, (m[b, :, 2] - cx) * s, (m[b, :, 3] - cy) * s])      # (4,N)
        M = int(cand.sum())
        count, best, f = 0, -1, None
        if M >= MIN_SAMPLE:
            fs, good, _ = hypotheses(xn[:, cand], seed, epoch, b, K)
            num, den = sampson(fs[:, None, :], *(xn[i, cand][None, :] for i in range(4)))      # (K,M)
            with np.errstate(all="ignore"):
                counts = np.where(good, (num <= t * den).sum(1), 0)
            best = int(counts.argmax())                                  # (the lowest k of equal counts)
            count, f = int(counts[best]), fs[best]
        ok = M >= MIN_SAMPLE and count >= min_inliers and 1000 * count >= permille * M
        status = np.where(~row, NO_ROW, np.where(~cand, NOT_CANDIDATE, NO_VERDICT)).astype(np.uint8)
        dist2 = np.where(row, F32(np.inf), F32(-1)).astype(F32)
        if ok:
            num, den = sampson(f, *(xn[i] for i in range(4)))
            with np.errstate(all="ignore"):
                inl = num <= t * den
                d = np.where(den > 0, num / den, np.where(inl, F32(0), F32(np.inf))) / s2
            status = np.where(cand, np.where(inl, INLIER, OUTLIER), status).astype(np.uint8)
            dist2 = np.where(row & finite, d, dist2).astype(F32)
            out["F"][b] = to_pixels(f, s, cx, cy)
            dead = status == OUTLIER
            out["valid"][b][dead] = 0
            if out["table"] is not None and cull:
                tb = out["table"]
                tb["pos"][b][dead], tb["ids"][b][dead], tb["age"][b][dead] = -1, -1, 0
        out["status"][b], out["dist2"][b], out["ok"][b], out["candidates"][b], out["best"][b] = status, dist2, ok, M, best
        out["inliers"][b] = count if ok else 0      # (the scoring pass and the flags share one expression: count == (status == 1).sum())
    return out
