"""Key-point masks on the device: the reference's `goodfeature` mask type.

The reference makes its masks offline (scripts/maskGenerate.py:11-30: cv.goodFeaturesToTrack(img, 500, 0.01, 10), then
mask[y, x] = 255).  `GoodFeatures` is that detector as HIP kernels (csrc/keypoints.hip, ops.good_features): alone, in
front of the model inside a captured graph (graph.GraphedForward(keypoints=det), warm_start.FlowSequence(keypoints=det))
and as the offline generator (tools/generate_masks.py).

    det = GoodFeatures()                   # the reference's parameters
    mask1 = det(image1)                    # (B,1,H,W): 255 at key points, 0 elsewhere
    points, count = det.points(image1)     # (B,500,2) int32 [x, y] in acceptance order (-1 beyond count), (B) int32
"""
import torch

from . import ops


class GoodFeatures:
    """Shi-Tomasi corners: block size 3, Sobel aperture 3, minimum eigenvalue, as cv.goodFeaturesToTrack defaults to."""

    def __init__(self, max_corners=500, quality_level=0.01, min_distance=10):
        if int(max_corners) < 1:
            raise ValueError(f"max_corners={max_corners}: at least 1")
        if not 0.0 < float(quality_level) <= 1.0:
            raise ValueError(f"quality_level={quality_level}: 0 < quality_level <= 1")
        if int(min_distance) != min_distance or int(min_distance) < 0:
            raise ValueError(f"min_distance={min_distance}: a whole number of pixels, 0 or more")
        self.max_corners, self.quality_level, self.min_distance = int(max_corners), float(quality_level), int(min_distance)
        self._ws = {}

    def _workspace(self, image):
        """One workspace per (device, stream, B, H, W), kept between eager calls: calls on one stream are ordered, so they
        may share it.  During a capture the allocation is left to the graph's own pool (None)."""
        if not image.is_cuda or image.dim() != 4 or torch.cuda.is_current_stream_capturing():
            return None
        b, _, h, w = image.shape
        key = (image.device, torch.cuda.current_stream(image.device).cuda_stream, b, h, w)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = ops.good_features_ws(b, h, w)
            if nbytes <= 0:
                return None      # (the call refuses the shape with its reason)
            if len(self._ws) >= 8:
                self._ws.clear()
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
        return ws

    def __call__(self, image, out=None):
        return ops.good_features(image, self.max_corners, self.quality_level, self.min_distance, out=out, ws=self._workspace(image))

    def points(self, image):
        _, points, count = ops.good_features(image, self.max_corners, self.quality_level, self.min_distance, return_points=True,
                                             ws=self._workspace(image))
        return points, count

    def __repr__(self):
        return f"GoodFeatures(max_corners={self.max_corners}, quality_level={self.quality_level}, min_distance={self.min_distance})"
