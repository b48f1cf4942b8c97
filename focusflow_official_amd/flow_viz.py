"""Flow images: the reference's core/utils/flow_viz.py (the Middlebury colour wheel of Baker et al., ICCV 2007) with its API, the
pixels coloured on the device (csrc/flow_viz.hip through ops.flow_to_image).

    flow_to_image(flow_uv)                   # numpy [H,W,2] in -> numpy [H,W,3] uint8 out, as a caller of the reference expects:
                                             # the field goes to the current HIP device and the image comes back
    flow_to_image(flow)                      # a device tensor (2,H,W) / (B,2,H,W) stays there: uint8 (H,W,3) / (B,H,W,3)

`max_flow` is the extension of the FF-FlowFormer copy of that file: a fixed scale instead of the frame's maximum, beyond which
vectors are darkened - what a video wants, so that the colours do not pump from frame to frame.  Inside a video session
frames.FrameSequence(render=...) writes the same images within its graph.  There is no CPU fallback."""
import numpy as np
import torch

from . import ops


def make_colorwheel():
    """The colour wheel: float64 (55,3), values 0 .. 255, the transitions RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 (on the host:
    the kernel builds its own copy)."""
    wheel = np.zeros((55, 3))
    col = 0
    # (the channel that stays at 255, the channel that moves, whether it rises) of the six transitions
    for n, full, moving, rises in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False)):
        ramp = np.floor(255 * np.arange(n) / n)
        wheel[col:col + n, full] = 255
        wheel[col:col + n, moving] = ramp if rises else 255 - ramp
        col += n
    return wheel


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False, max_flow=None):
    """flow_uv: a numpy [H,W,2] array -> numpy [H,W,3] uint8 (through the current HIP device); or a device tensor (2,H,W) /
    (B,2,H,W) -> a device tensor (H,W,3) / (B,H,W,3) uint8.  clip_flow: np.clip(flow, 0, clip_flow) first; convert_to_bgr: B,G,R
    out; max_flow: a fixed scale instead of the maximum magnitude (of every sample)."""
    order = "bgr" if convert_to_bgr else "rgb"
    if isinstance(flow_uv, torch.Tensor):
        if not flow_uv.is_cuda:
            raise ops._hip.FocusFlowHipError("flow_viz.flow_to_image: a torch tensor must be on a HIP device (got a CPU tensor); there is no CPU "
                                             "fallback (a numpy [H,W,2] array is uploaded and its image downloaded)")
        if flow_uv.dim() not in (3, 4) or flow_uv.shape[-3] != 2:
            raise ValueError(f"flow_uv: a device tensor (2,H,W) or (B,2,H,W) expected, got {tuple(flow_uv.shape)}")
        image = ops.flow_to_image(flow_uv.float() if flow_uv.dim() == 4 else flow_uv.float()[None], max_flow=max_flow, clip_flow=clip_flow, order=order)
        return image if flow_uv.dim() == 4 else image[0]
    flow_uv = np.asarray(flow_uv)
    if flow_uv.ndim != 3 or flow_uv.shape[2] != 2:
        raise ValueError(f"flow_uv: a numpy array of shape [H,W,2] expected, got {flow_uv.shape}")
    if not torch.cuda.is_available():
        raise ops._hip.FocusFlowHipError("flow_viz.flow_to_image: no HIP device; there is no CPU fallback")
    field = torch.from_numpy(np.ascontiguousarray(flow_uv, dtype=np.float32)).cuda()      # (H,W,2): passed as the (1,2,H,W) view it is
    return ops.flow_to_image(field.permute(2, 0, 1)[None], max_flow=max_flow, clip_flow=clip_flow, order=order)[0].cpu().numpy()
