"""The `goodfeature` key-point detector restated in exact integer and fp64 arithmetic: the yardstick of
tests/test_keypoints.py (csrc/keypoints.hip must equal it bit for bit: mask, points, order and count).

It restates the documented algorithm of cv.goodFeaturesToTrack(img, max_corners, quality_level, min_distance) with OpenCV's
defaults (block size 3, Sobel aperture 3, minimum eigenvalue), as scripts/maskGenerate.py calls it.  OpenCV itself is not
available where this suite runs, so agreement with OpenCV is expected, not measured: OpenCV evaluates the same quantities
in float32 with a scale factor, and its tie order is its sort's own (tests/diagnostics/keypoints_vs_opencv.py prints the
overlap for whoever has cv2).

  1 gray     channels -> np.rint (half-even), clipped to 0..255; R,G,B -> (4899 R + 9617 G + 1868 B + 8192) >> 14
  2 dx, dy   3x3 Sobel with reflect-101 borders
  3 a, b, c  3x3 sums of dx^2, dx dy, dy^2, reflect-101 applied to the three product planes
  4 lambda   ((a + c) - sqrt((a - c)^2 + 4 b^2)) / 2 in fp64 (the radicand is an exact integer below 2^53)
  5 keep     lambda > max(lambda) * quality_level
  6 maxima   kept pixels that equal the maximum of the kept values of their 3x3 neighbourhood, off the outermost ring
  7 order    descending lambda, ties by ascending y W + x
  8 greedy   accept unless an accepted point has dx^2 + dy^2 < min_distance^2; stop after max_corners
"""
import numpy as np


def gray_u8(image):
    """(C,H,W) float32, C = 1 or 3 -> (H,W) int64 in 0..255."""
    v = np.clip(np.rint(np.asarray(image, np.float32)), 0, 255).astype(np.int64)
    if v.shape[0] == 1:
        return v[0]
    assert v.shape[0] == 3
    return (4899 * v[0] + 9617 * v[1] + 1868 * v[2] + 8192) >> 14


def _box3(p):
    q = np.pad(p, 1, mode="reflect")      # numpy's 'reflect' is reflect-101
    h, w = p.shape
    return sum(q[j:j + h, i:i + w] for j in range(3) for i in range(3))


def min_eigenvalue(gray):
    """(H,W) integers -> (H,W) float64."""
    g = np.pad(np.asarray(gray, np.int64), 1, mode="reflect")
    h, w = gray.shape
    s = lambda j, i: g[j:j + h, i:i + w]      # noqa: E731
    dx = (s(0, 2) + 2 * s(1, 2) + s(2, 2)) - (s(0, 0) + 2 * s(1, 0) + s(2, 0))
    dy = (s(2, 0) + 2 * s(2, 1) + s(2, 2)) - (s(0, 0) + 2 * s(0, 1) + s(0, 2))
    a, b, c = _box3(dx * dx), _box3(dx * dy), _box3(dy * dy)
    rad = (a - c) ** 2 + 4 * b * b
    assert rad.max() < 2 ** 53
    return ((a + c).astype(np.float64) - np.sqrt(rad.astype(np.float64))) / 2.0


def candidates(lam, quality_level):
    """-> flat indices of the candidates in the walk's order (step 7)."""
    h, w = lam.shape
    t = lam.max() * np.float64(quality_level)
    kept = np.where(lam > t, lam, -np.inf)
    q = np.pad(kept, 1, constant_values=-np.inf)
    top = np.max([q[j:j + h, i:i + w] for j in range(3) for i in range(3)], axis=0)
    is_cand = (lam > t) & (kept == top)
    is_cand[[0, -1], :] = False
    is_cand[:, [0, -1]] = False
    idx = np.flatnonzero(is_cand)
    return idx[np.lexsort((idx, -lam.reshape(-1)[idx]))]


def greedy(order, h, w, max_corners, min_distance):
    """The sequential walk of step 8 over flat indices in order -> accepted flat indices, in acceptance order."""
    r = max(min_distance - 1, 0)
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    disc = (dx * dx + dy * dy) < min_distance * min_distance
    blocked = np.zeros((h + 2 * r, w + 2 * r), bool)
    out = []
    for p in order.tolist():
        y, x = divmod(p, w)
        if blocked[y + r, x + r]:
            continue
        out.append(p)
        if len(out) == max_corners:
            break
        blocked[y:y + 2 * r + 1, x:x + 2 * r + 1] |= disc
    return np.asarray(out, np.int64)


def greedy_parallel_rounds(order, lam, max_corners, min_distance):
    """Step 8 without a walk: a candidate is rejected once an accepted one is within the distance, and accepted once no
    stronger undecided one is; the cap follows from the rank among the accepted.  -> (accepted in order, rounds)."""
    h, w = lam.shape
    y, x = np.divmod(order, w)
    n = order.size
    near = ((y[:, None] - y[None]) ** 2 + (x[:, None] - x[None]) ** 2) < min_distance * min_distance
    np.fill_diagonal(near, False)
    stronger = np.arange(n)[None] < np.arange(n)[:, None]      # [i, j]: j is walked before i
    state = np.zeros(n, np.int8)                                # 0 undecided, 1 accepted, 2 rejected
    rounds = 0
    while (state == 0).any():
        rounds += 1
        rejected = (state == 0) & (near & (state == 1)[None]).any(axis=1)
        state[rejected] = 2
        accepted = (state == 0) & ~(near & stronger & (state == 0)[None]).any(axis=1)
        state[accepted] = 1
    return order[state == 1][:max_corners], rounds


def good_features_ref(image, max_corners=500, quality_level=0.01, min_distance=10, return_all=False):
    """image (C,H,W) float32 -> mask (1,H,W) float32, points (max_corners,2) int32 [x, y] (-1 beyond count), count;
    return_all: also the number accepted without the cap and the number of candidates."""
    gray = gray_u8(image)
    h, w = gray.shape
    lam = min_eigenvalue(gray)
    order = candidates(lam, quality_level) if lam.max() > 0 else np.zeros(0, np.int64)
    acc = greedy(order, h, w, max_corners, min_distance)
    mask = np.zeros((1, h, w), np.float32)
    mask.reshape(-1)[acc] = 255.0
    points = np.full((max_corners, 2), -1, np.int32)
    points[:acc.size, 0], points[:acc.size, 1] = acc % w, acc // w
    if return_all:
        return mask, points, int(acc.size), int(greedy(order, h, w, h * w, min_distance).size), int(order.size)
    return mask, points, int(acc.size)


# ---- the image generators of the tests: integers 0..255 as float32 (1,H,W) ----
def _box_mean(img, r):
    q = np.pad(img.astype(np.int64), r, mode="reflect")
    h, w = img.shape
    k = 2 * r + 1
    return np.rint(sum(q[j:j + h, i:i + w] for j in range(k) for i in range(k)) / (k * k))


def make_image(kind, h, w, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        img = np.full((h, w), 77)
    elif kind == "tiled":
        tile = rng.integers(0, 256, (16, 16))
        img = np.tile(tile, ((h + 15) // 16, (w + 15) // 16))[:h, :w]
    else:
        img = rng.integers(0, 256, (h, w))
        if kind in ("blur1", "blur3"):
            img = _box_mean(img, int(kind[4]))
        else:
            assert kind == "noise", kind
    return img.astype(np.float32)[None]
