"""Numpy restatements of csrc/tracks.hip (ff_tracks_replenish, ff_tracks_mask, ff_tracks_advance) and of one step of a
frames.FrameSequence(tracks=...) session: the yardsticks of tests/test_tracks.py.  The definitions are those of
include/focusflow_hip.h: fp64 for the distance test and fp32 for the blend, every operation rounded separately (numpy rounds
every array operation to the dtype of its operands, and nothing here fuses two).  Nothing calls the library.

A table is a dict of numpy arrays: pos (B,N,2) float32, ids (B,N) int64, age (B,N) int32, next_id (B) int64.  The functions
return new tables and leave their arguments alone."""
import numpy as np

F32 = np.float32


def empty_table(b, n, next_id=0):
    return {"pos": np.full((b, n, 2), -1, F32), "ids": np.full((b, n), -1, np.int64), "age": np.zeros((b, n), np.int32),
            "next_id": np.full((b,), next_id, np.int64)}


def copy_table(tb):
    return {k: np.array(v, copy=True) for k, v in tb.items()}


def pad_offsets(h, w, mode="sintel"):
    """(left, top, Hp, Wp) of replicate padding to multiples of 8: centred for 'sintel', rows at the bottom otherwise."""
    pad_h, pad_w = (8 - h % 8) % 8, (8 - w % 8) % 8
    return pad_w // 2, (pad_h // 2 if mode == "sintel" else 0), h + pad_h, w + pad_w


def blocked(tb, points, count, h, w, min_distance):
    """(B,M) bool: detection j lies below the count, inside the frame, and a slot that is live has
    dx dx + dy dy < min_distance^2 in fp64."""
    b, m, _ = points.shape
    out = np.zeros((b, m), bool)
    md2 = np.float64(min_distance) * np.float64(min_distance)
    for bi in range(b):
        alive = tb["ids"][bi] >= 0
        px, py = tb["pos"][bi, alive, 0].astype(np.float64), tb["pos"][bi, alive, 1].astype(np.float64)
        for j in range(min(max(int(count[bi]), 0), m)):
            x, y = int(points[bi, j, 0]), int(points[bi, j, 1])
            if not (0 <= x < w and 0 <= y < h):
                continue
            dx, dy = px - np.float64(x), py - np.float64(y)
            with np.errstate(invalid="ignore"):
                out[bi, j] = bool(((dx * dx) + (dy * dy) < md2).any())
    return out


def replenish(tb, points, count, h, w, min_distance):
    """-> (table, born (B) int32, live (B) int32)."""
    tb = copy_table(tb)
    b, m, _ = points.shape
    block = blocked(tb, points, count, h, w, min_distance)
    born, live = np.zeros(b, np.int32), np.zeros(b, np.int32)
    for bi in range(b):
        free = [s for s in range(tb["ids"].shape[1]) if tb["ids"][bi, s] < 0]      # ascending
        r = 0
        for j in range(min(max(int(count[bi]), 0), m)):      # detector order
            x, y = int(points[bi, j, 0]), int(points[bi, j, 1])
            if not (0 <= x < w and 0 <= y < h) or block[bi, j]:
                continue
            if r == len(free):
                break
            s = free[r]
            tb["ids"][bi, s] = tb["next_id"][bi] + r
            tb["pos"][bi, s] = (F32(x), F32(y))
            tb["age"][bi, s] = 0
            r += 1
        tb["next_id"][bi] += r
        born[bi] = r
        live[bi] = int((tb["ids"][bi] >= 0).sum())
    return tb, born, live


def _pixel(v, n):
    """floorf(v + 0.5f) clamped to 0 .. n - 1 (a NaN: 0)."""
    with np.errstate(invalid="ignore"):
        p = np.floor(v.astype(F32) + F32(0.5))
    return np.clip(np.nan_to_num(p, nan=0.0, posinf=n - 1, neginf=0.0), 0, n - 1).astype(np.int64)


def mask(tb, h, w):
    """(B,1,h,w) float32: 255 at the pixel nearest to every live slot."""
    b = tb["ids"].shape[0]
    out = np.zeros((b, 1, h, w), F32)
    for bi in range(b):
        alive = tb["ids"][bi] >= 0
        out[bi, 0, _pixel(tb["pos"][bi, alive, 1], h), _pixel(tb["pos"][bi, alive, 0], w)] = 255
    return out


def _blend(f00, f01, f10, f11, fx, fy):
    """The definition: fp32, each operation rounded separately, in this order."""
    wx0 = F32(1) - fx
    top = (wx0 * f00) + (fx * f01)
    bot = (wx0 * f10) + (fx * f11)
    wy0 = F32(1) - fy
    return (wy0 * top) + (fy * bot)


def _fma(a, b, c):
    """fmaf(a, b, c) for fp32 arrays: the product of two fp32 values is exact in fp64; the fp64 sum is rounded once more to fp32
    (double rounding could differ from a true FMA only in a tie of the fp64 sum, which the variant below does not care about:
    it only has to differ from the definition)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _blend_fma(f00, f01, f10, f11, fx, fy):
    """What a compiler that contracts a * b + c makes of the same source: NOT the definition.  The advance test asserts that its
    input tells the two apart."""
    wx0 = F32(1) - fx
    top = _fma(wx0, f00, fx * f01)
    bot = _fma(wx0, f10, fx * f11)
    wy0 = F32(1) - fy
    return _fma(wy0, top, fy * bot)


def advance(tb, flow_up, left, top, h, w, blend=_blend):
    """flow_up: (B,2,Hp,Wp) float32, the frame at (left, top).  -> (table, matches (B,N,4) float32, valid (B,N) uint8,
    ids_out (B,N) int64, age_out (B,N) int32)."""
    tb = copy_table(tb)
    flow_up = np.asarray(flow_up, F32)
    b, n = tb["ids"].shape
    alive = tb["ids"] >= 0
    x, y = tb["pos"][..., 0], tb["pos"][..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = np.clip(np.nan_to_num(np.floor(x), nan=0.0, posinf=w - 1, neginf=0.0), 0, w - 1).astype(np.int64)
        y0 = np.clip(np.nan_to_num(np.floor(y), nan=0.0, posinf=h - 1, neginf=0.0), 0, h - 1).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        fx, fy = x - x0.astype(F32), y - y0.astype(F32)
        bi = np.arange(b)[:, None]
        uv = []
        for c in range(2):
            f = flow_up[:, c]
            uv.append(blend(f[bi, y0 + top, x0 + left], f[bi, y0 + top, x1 + left], f[bi, y1 + top, x0 + left], f[bi, y1 + top, x1 + left], fx, fy))
        tx, ty = x + uv[0], y + uv[1]
        assert tx.dtype == F32 and ty.dtype == F32 and fx.dtype == F32
        ok = alive & (tx >= 0) & (tx <= F32(w - 1)) & (ty >= 0) & (ty <= F32(h - 1))      # (a NaN compares false)
    matches = np.where(alive[..., None], np.stack([x, y, tx, ty], axis=-1), F32(-1)).astype(F32)
    ids_out, age_out = np.where(alive, tb["ids"], -1), np.where(alive, tb["age"], 0).astype(np.int32)
    tb["pos"] = np.where(ok[..., None], np.stack([tx, ty], axis=-1), F32(-1)).astype(F32)
    tb["ids"] = np.where(ok, tb["ids"], -1)
    tb["age"] = np.where(ok, tb["age"] + 1, 0).astype(np.int32)
    return tb, matches, ok.astype(np.uint8), ids_out, age_out


def pad_replicate(plane, mode="sintel"):
    """(B,1,h,w) -> (B,1,Hp,Wp), replicate-padded as utils.InputPadder pads."""
    h, w = plane.shape[-2:]
    left, top, hp, wp = pad_offsets(h, w, mode)
    return np.pad(plane, ((0, 0), (0, 0), (top, hp - h - top), (left, wp - w - left)), mode="edge")


def session_step(tb, points, count, flow_up, h, w, min_distance, mode="sintel"):
    """One pair of a FrameSequence(tracks=...) session around a GIVEN flow: replenish from the detector's points, rasterise and
    pad the mask the model reads, advance by flow_up, the UNPADDED (B,2,h,w) field (taps never leave the frame, so the padding
    is never read).  -> dict of everything the session shows, and `blocked`, the number of detections a live track blocked."""
    n_blocked = int(blocked(tb, points, count, h, w, min_distance).sum())
    tb, born, live = replenish(tb, points, count, h, w, min_distance)
    mask1 = pad_replicate(mask(tb, h, w), mode)
    tb, matches, valid, ids_out, age_out = advance(tb, flow_up, 0, 0, h, w)
    return {"table": tb, "matches": matches, "valid": valid, "ids": ids_out, "age": age_out, "born": born, "count": live, "mask1": mask1,
            "blocked": n_blocked}
