"""A diagnostic, not a test: how many key points of tests/keypoints_ref.py (= csrc/keypoints.hip, bit for bit) coincide
with cv.goodFeaturesToTrack(img, 500, 0.01, 10) on the test suite's generated images.  It asserts nothing.

    python tests/diagnostics/keypoints_vs_opencv.py

OpenCV evaluates the same quantities in float32 with a scale factor, so near-ties in the eigenvalue may order differently,
and the order of exact ties is its sort's own: full agreement is expected on images without near-ties, not guaranteed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import keypoints_ref as R  # noqa: E402


def main():
    try:
        import cv2 as cv
    except ImportError:
        print("cv2 is not importable here: nothing to compare")
        return
    for kind in ("noise", "blur1", "blur3", "flat", "tiled"):
        for h, w in ((48, 64), (128, 160), (384, 512)):
            img = R.make_image(kind, h, w)
            _, points, count = R.good_features_ref(img)
            kp = cv.goodFeaturesToTrack(img[0].astype(np.uint8), 500, 0.01, 10)
            theirs = set() if kp is None else {(int(p[0][0]), int(p[0][1])) for p in kp}
            ours = {tuple(p) for p in points[:count].tolist()}
            print(f"{kind:6s} {h}x{w}: restatement {len(ours):4d}  OpenCV {len(theirs):4d}  common {len(ours & theirs):4d}")


if __name__ == "__main__":
    main()
