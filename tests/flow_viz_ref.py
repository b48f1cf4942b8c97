"""Numpy restatement of csrc/flow_viz.hip (ff_flow_rad_max, ff_flow_to_image): the yardstick of tests/test_flow_viz.py.  The
definition is that of include/focusflow_hip.h, which is the dtype chain of the reference's core/utils/flow_viz.py::flow_to_image
(and of the FF-FlowFormer copy's `max_flow`): fp32 up to the wheel index, fp64 behind it, every operation rounded on its own
(numpy rounds every array operation to the dtype of its operands, and nothing here fuses two).  tests/golden/flow_viz.npz ties
it to the reference byte for byte.  Nothing calls the library.

On top of the reference: a batch (every sample has its own maximum), a frame at (left, top) of a padded field, an occlusion
plane painted over the colours, and the non-finite rule (the reference has no defined answer there)."""
import numpy as np

F32 = np.float32
NCOLS = 55


def make_colorwheel():
    """The 55 x 3 wheel of Baker et al. (ICCV 2007), float64, values 0 .. 255: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6."""
    wheel = np.zeros((NCOLS, 3))
    col = 0
    for n, rise, fall in ((15, 1, None), (6, None, 0), (4, 2, None), (11, None, 1), (13, 0, None), (6, None, 2)):
        ramp = np.floor(255 * np.arange(n) / n)
        if rise is not None:      # a channel rises while the one before it in the cycle stays at 255
            wheel[col:col + n, (rise + 2) % 3] = 255
            wheel[col:col + n, rise] = ramp
        else:                     # a channel falls while the one behind it stays at 255
            wheel[col:col + n, fall] = 255 - ramp
            wheel[col:col + n, (fall + 1) % 3] = 255
        col += n
    return wheel


def clipped(flow, clip_flow):
    """(u, v) as the magnitude and the colours see them: np.clip(flow, 0, clip_flow), which clips below to 0 as well."""
    flow = np.asarray(flow, F32)
    if clip_flow is None:
        return flow
    with np.errstate(invalid="ignore"):
        return np.minimum(np.maximum(flow, F32(0)), F32(clip_flow)).astype(F32)


def _radius(u, v):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(u * u + v * v)
    assert r.dtype == F32
    return r


def _frame(flow, left, top, h, w):
    flow = np.asarray(flow, F32)
    assert flow.ndim == 4 and flow.shape[1] == 2
    h = flow.shape[2] - top if h is None else h
    w = flow.shape[3] - left if w is None else w
    return flow[:, :, top:top + h, left:left + w]


def rad_max(flow, left=0, top=0, h=None, w=None, clip_flow=None):
    """flow (B,2,Hp,Wp) float32 -> (B) float32: the maximum of the clipped flow's magnitude over the h x w frame at (left,
    top); a vector with a non-finite component or magnitude is left out, and a frame of such vectors only gives 0."""
    raw = _frame(flow, left, top, h, w)
    f = clipped(raw, clip_flow)
    r = _radius(f[:, 0], f[:, 1])
    ok = np.isfinite(raw[:, 0]) & np.isfinite(raw[:, 1]) & np.isfinite(r)
    return np.where(ok, r, F32(0)).reshape(r.shape[0], -1).max(axis=1).astype(F32)


def flow_to_image(flow, left=0, top=0, h=None, w=None, max_flow=None, clip_flow=None, order="rgb", layout="hwc", occluded=None,
                  occluded_color=(0, 0, 0)):
    """flow (B,2,Hp,Wp) float32 -> (image uint8 (B,h,w,3) or (B,3,h,w), rad_max (B) float32).  occluded: None or (B,1,h,w) /
    (B,h,w), painted occluded_color (r, g, b) where it is non-zero."""
    raw = _frame(flow, left, top, h, w)
    b, _, h, w = raw.shape
    f = clipped(raw, clip_flow)
    u, v = f[:, 0], f[:, 1]
    r = _radius(u, v)
    ok = np.isfinite(raw[:, 0]) & np.isfinite(raw[:, 1]) & np.isfinite(r)
    m = np.where(ok, r, F32(0)).reshape(b, -1).max(axis=1).astype(F32)
    if max_flow is None:
        den = (m + F32(1e-5)).astype(F32)
    else:
        den = np.full(b, F32(float(max_flow) + 1e-5), F32)      # (the reference adds two Python floats and divides an fp32 array by the sum)
    u, v = np.where(ok, u, F32(0)), np.where(ok, v, F32(0))      # (left-out vectors are painted over below)
    with np.errstate(over="ignore", invalid="ignore"):
        un, vn = u / den[:, None, None], v / den[:, None, None]
        rad = np.sqrt(un * un + vn * vn)
        a = np.arctan2(-vn, -un) / F32(np.pi)
        fk = (a + F32(1)) / F32(2) * F32(NCOLS - 1)
    assert rad.dtype == F32 and fk.dtype == F32
    k0 = np.clip(np.floor(fk).astype(np.int32), 0, NCOLS - 1)
    k1 = k0 + 1
    k1[k1 == NCOLS] = 0
    frac = fk.astype(np.float64) - k0
    wheel = make_colorwheel()
    img = np.zeros((b, h, w, 3), np.uint8)
    for c in range(3):
        col = (1 - frac) * (wheel[k0, c] / 255.0) + frac * (wheel[k1, c] / 255.0)
        with np.errstate(over="ignore", invalid="ignore"):
            col = np.where(rad <= 1, 1 - rad.astype(np.float64) * (1 - col), col * 0.75)
        img[..., c] = np.floor(255 * col)
    img[~ok] = 0
    if occluded is not None:
        occ = np.asarray(occluded).reshape(b, h, w) != 0
        img[occ] = np.asarray(occluded_color, np.uint8)
    if order == "bgr":
        img = img[..., ::-1]
    if layout == "chw":
        img = img.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(img), m
