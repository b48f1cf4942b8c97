"""fp64 references of the materialised correlation block's kernels (torch on the CPU; no GPU, no autograd needed).

Tap indices and fractional weights always come from oracle.ffraft_ref.lookup_taps - the separately rounded fp32 chain
that tests/test_oracle_golden.py pins to ATen - so that a coordinate on an integer floors as the kernels floor it;
everything after the taps is fp64.  Coordinates are (Q, 2) float32 tensors [x, y]; planes are (Q, h_l, w_l).

The `mutate` arguments exist for the discrimination tests of tests/test_corr_kernels.py only: each names one way a kernel
could be subtly wrong, and the tests assert that the bounds they hold the kernels to would catch it.
"""
import torch

from oracle import ffraft_ref as orc

U = 2.0 ** -24          # unit roundoff of fp32


def level_sizes(h0, w0):
    return [(h0 >> l, w0 >> l) for l in range(4)]


def taps(coords, h0, w0):
    """oracle.ffraft_ref.lookup_taps for (Q, 2) coordinates: per level (x0, y0, wx, wy), each (Q, 9)."""
    q = coords.shape[0]
    return orc.lookup_taps(coords.float().t().reshape(1, 2, 1, q).contiguous(), level_sizes(h0, w0))


def _corners(x0, y0, wx, wy, hl, wl, mutate=None):
    """The four corners of every (a, b) tap pair of a level: flat plane index (Q, 81), in-plane mask, fp64 weight."""
    q = x0.shape[0]
    wx, wy = wx.double(), wy.double()
    for dy in (0, 1):
        for dx in (0, 1):
            xi = (x0 + dx).long()[:, :, None].expand(q, 9, 9)           # a-major: k = a * 9 + b
            yi = (y0 + dy).long()[:, None, :].expand(q, 9, 9)
            ok = (xi >= 0) & (xi < wl) & (yi >= 0) & (yi < hl)
            if mutate == "drop_last_row" and dy == 1:
                ok = ok & (yi != hl - 1)
            if mutate == "drop_last_col" and dx == 1:
                ok = ok & (torch.arange(9).view(1, 9, 1) != 8)
            wgt = (wx if dx else 1 - wx)[:, :, None] * (wy if dy else 1 - wy)[:, None, :]
            idx = yi.clamp(0, hl - 1) * wl + xi.clamp(0, wl - 1)
            yield idx.reshape(q, 81), ok.reshape(q, 81), wgt.reshape(q, 81)


def lookup_ref(levels64, coords32, mutate=None):
    """CorrBlock.__call__: the four-tap blend with zero padding.  levels64: four (Q, h_l, w_l) fp64 planes.
    -> (out64, absout64), both (Q, 324), channel k = level * 81 + a * 9 + b (a: x offset); absout64 is the same blend over
    |levels| (every weight is >= 0), the scale of the rounding-error bound."""
    h0, w0 = levels64[0].shape[-2:]
    q = coords32.shape[0]
    outs, absouts = [], []
    for plane, (x0, y0, wx, wy) in zip(levels64, taps(coords32, h0, w0)):
        hl, wl = plane.shape[-2:]
        if mutate == "shift_col":
            x0 = x0 + 1
        flat = plane.reshape(q, hl * wl)
        acc, aacc = torch.zeros(q, 81, dtype=torch.float64), torch.zeros(q, 81, dtype=torch.float64)
        for idx, ok, wgt in _corners(x0, y0, wx, wy, hl, wl, mutate):
            v = torch.gather(flat, 1, idx) * ok
            acc += v * wgt
            aacc += v.abs() * wgt
        if mutate == "swap_xy":
            acc, aacc = (t.view(q, 9, 9).transpose(1, 2).reshape(q, 81) for t in (acc, aacc))
        outs.append(acc)
        absouts.append(aacc)
    return torch.cat(outs, 1), torch.cat(absouts, 1)


def scatter_ref(coords_list, dout_list, h0, w0, extent=None):
    """The adjoint of lookup_ref, summed over the lookups: per level (Q, h_l, w_l) fp64 planes of
    sum_t sum_k dout_t[q, k] * weight - and the same scatter of |dout| (the scale of the error bound) and of ones WITHOUT
    the weights (the number of addends an element receives).  dout_t: (Q, >= 324), None = an absent lookup.
    -> (planes, abs_planes, count_planes), three lists of four.
    extent: [(hp_l, wp_l)] - the mutation "pad mask ignored": scatter into planes of the tile grid's extent instead."""
    q = coords_list[0].shape[0]
    sizes = level_sizes(h0, w0)
    ext = extent or sizes
    res = [[torch.zeros(q, he * we, dtype=torch.float64) for he, we in ext] for _ in range(3)]
    for coords, dout in zip(coords_list, dout_list):
        if dout is None:
            continue
        d = dout[:, :324].double()
        for l, (x0, y0, wx, wy) in enumerate(taps(coords, h0, w0)):
            he, we = ext[l]
            g = d[:, l * 81:(l + 1) * 81]
            for idx, ok, wgt in _corners(x0, y0, wx, wy, he, we):
                res[0][l].scatter_add_(1, idx, g * wgt * ok)
                res[1][l].scatter_add_(1, idx, g.abs() * wgt * ok)
                res[2][l].scatter_add_(1, idx, ok.double())
    return tuple([p.view(q, he, we) for p, (he, we) in zip(r, ext)] for r in res)


def pool_bwd_ref(d0, d1, d2, d3, scale=0.25, guard=True):
    """avg_pool2d(2, 2) backward down the chain: d_l += scale * upsample(d_{l+1}), level 2 first.  A child (y, x) has a
    parent only where (y >> 1) < h_{l+1} and (x >> 1) < w_{l+1} (odd planes: the last row / column has none).
    scale: 0.25 for gradient and abs planes; 1 for count planes (the addends of the parent arrive, all of them).
    guard=False is the mutation: the parent index is clamped instead of checked.  Returns new planes [d0, d1, d2, d3]."""
    out = [d0, d1, d2, d3]
    for l in (2, 1, 0):
        child, parent = out[l], out[l + 1]
        hc, wc = child.shape[-2:]
        hp, wp = parent.shape[-2:]
        ys, xs = torch.arange(hc) >> 1, torch.arange(wc) >> 1
        up = parent[:, ys.clamp(max=hp - 1)][:, :, xs.clamp(max=wp - 1)]
        if guard:
            up = up * ((ys < hp)[:, None] & (xs < wp)[None, :])
        out[l] = child + scale * up
    return out


def volume_bwd_ref(dvol, f1, f2):
    """BmmBackward of corr.py:58.  dvol (B, Q, Q), f1 / f2 (B, Q, C), any dtype -> fp64
    (df1, df2, abs1, abs2): df1 = dvol @ f2 / sqrt(C), df2 = dvol^T @ f1 / sqrt(C), abs1 = |dvol| @ |f2|,
    abs2 = |dvol|^T @ |f1| (the abs-products are NOT scaled: the tests scale the bound)."""
    dvol, f1, f2 = dvol.double(), f1.double(), f2.double()
    s = f1.shape[-1] ** -0.5
    return (dvol @ f2 * s, dvol.transpose(1, 2) @ f1 * s, dvol.abs() @ f2.abs(), dvol.abs().transpose(1, 2) @ f1.abs())


def tiled_layout(h0, w0, level, half):
    """csrc/corr_layout.h: (ntx, nty, th) of a level's tile grid."""
    th = 8 if half else 4
    ntx = ((((w0 + 15) // 16 * 16) >> level) + 7) // 8
    nty = ((((h0 + 7) // 8 * 8) >> level) + th - 1) // th
    return ntx, nty, th


def tiled_index(h0, w0, level, half):
    """-> (off, pad): off (h_l, w_l) int64, the element offset of (y, x) inside a tiled plane (csrc/corr_layout.h; the
    formula of test_retile_round_trip_and_layout); pad (plane elements,) bool, True where no (y, x) lands."""
    ntx, nty, th = tiled_layout(h0, w0, level, half)
    h, w = h0 >> level, w0 >> level
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    off = ((ys // th) * ntx + xs // 8) * (8 * th) + (ys % th) * 8 + xs % 8
    pad = torch.ones(ntx * nty * 8 * th, dtype=torch.bool)
    pad[off.reshape(-1)] = False
    return off, pad


def tile_extent(h0, w0, level, half=False):
    """Rows and columns the tile grid of a level covers (>= h_l, w_l)."""
    ntx, nty, th = tiled_layout(h0, w0, level, half)
    return nty * th, ntx * 8
