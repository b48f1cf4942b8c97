"""Torch restatements of csrc/frame_io.hip (ff_frame_ingest, ff_pad_replicate, ff_keypoint_matches) and of the route a
video application takes without frames.FrameSequence: the yardsticks of tests/test_frame_sequence.py.  Everything here is
plain torch indexing on whatever device its inputs live on; nothing calls the library."""
import torch
import torch.nn.functional as F


def pad_offsets(h, w, mode="sintel"):
    """(left, top, Hp, Wp) of replicate padding to multiples of 8: centred for 'sintel', rows at the bottom otherwise."""
    pad_h, pad_w = (8 - h % 8) % 8, (8 - w % 8) % 8
    left = pad_w // 2
    top = pad_h // 2 if mode == "sintel" else 0
    return left, top, h + pad_h, w + pad_w


def as_float_rgb_nchw(frame, layout="hwc", order="rgb"):
    """A uint8 frame -> contiguous fp32 (B,3,H,W) R,G,B: what a caller does with permute / flip / float."""
    if frame.dim() == 3:
        frame = frame[None]
    x = frame.permute(0, 3, 1, 2) if layout == "hwc" else frame
    if order == "bgr":
        x = x.flip(1)
    return x.float().contiguous()


def ingest(frame, layout="hwc", order="rgb", mode="sintel"):
    """The torch route: convert, then F.pad(mode='replicate') by the offsets above."""
    x = as_float_rgb_nchw(frame, layout, order)
    h, w = x.shape[-2:]
    left, top, hp, wp = pad_offsets(h, w, mode)
    return F.pad(x, [left, wp - w - left, top, hp - h - top], mode="replicate")


def pad_mask(mask, mode="sintel"):
    """(B,1,H,W) or (B,H,W), uint8 or fp32 -> fp32 (B,1,Hp,Wp), replicate-padded."""
    if mask.dim() == 3:
        mask = mask[:, None]
    h, w = mask.shape[-2:]
    left, top, hp, wp = pad_offsets(h, w, mode)
    return F.pad(mask.float(), [left, wp - w - left, top, hp - h - top], mode="replicate")


def matches(points, count, flow_up, left, top, h, w):
    """points (B,N,2) int32 [x, y], count (B) int32, flow_up (B,2,Hp,Wp) fp32 -> (matches (B,N,4) fp32, valid (B,N) uint8).
    A row is live if it lies below the count and its point inside the h x w frame; every other row is -1 / 0."""
    b, n, _ = points.shape
    x, y = points[..., 0].long(), points[..., 1].long()
    live = (torch.arange(n, device=points.device)[None] < count[:, None].long()) & (x >= 0) & (x < w) & (y >= 0) & (y < h)
    xs, ys = x.clamp(0, w - 1) + left, y.clamp(0, h - 1) + top      # (clamped only so that dead rows index something)
    bi = torch.arange(b, device=points.device)[:, None].expand(b, n)
    u, v = flow_up[bi, 0, ys, xs], flow_up[bi, 1, ys, xs]
    xf, yf = x.to(torch.float32), y.to(torch.float32)
    tx, ty = xf + u, yf + v      # one fp32 add each
    m = torch.stack([xf, yf, tx, ty], dim=-1)
    m = torch.where(live[..., None], m, torch.full_like(m, -1.0))
    valid = live & (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)
    return m, valid.to(torch.uint8)
