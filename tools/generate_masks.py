"""Key-point masks for a tree of images, detected on the GPU: what the reference's scripts/maskGenerate.py does offline
with OpenCV (cv.goodFeaturesToTrack(img, 500, 0.01, 10), mask[y, x] = 255, one 8-bit PNG per image).

    python tools/generate_masks.py <image_root> <mask_root> [--type goodfeature] [--batch 16]

Every image below <image_root> (.png .ppm .jpg .jpeg) is read with PIL, images of equal size are detected in batches
(keypoints.GoodFeatures, csrc/keypoints.hip) and the mask goes to <mask_root>/<same relative path, extension replaced>.png
as 8-bit gray 0 / 255, which frame_utils.read_gen reads back unchanged.  Only `goodfeature` is built: the reference's sift
and orb masks are OpenCV's own pipelines and its silk creator is an empty stub.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IMAGE_EXT = (".png", ".ppm", ".jpg", ".jpeg")
REFERENCE_TYPES = ("goodfeature", "sift", "orb", "silk")


def find_images(image_root):
    """-> sorted paths relative to image_root."""
    out = []
    for d, _, files in os.walk(image_root):
        out += [os.path.relpath(os.path.join(d, f), image_root) for f in files if os.path.splitext(f)[1].lower() in IMAGE_EXT]
    return sorted(out)


def mask_path(mask_root, rel):
    return os.path.join(mask_root, os.path.splitext(rel)[0] + ".png")


def write_mask(path, mask):
    """(H,W) array of 0 / 255 -> 8-bit gray PNG."""
    from PIL import Image
    mask = np.asarray(mask)
    assert mask.ndim == 2 and np.isin(mask, (0, 255)).all(), "a mask holds 0 and 255 only"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(mask.astype(np.uint8), mode="L").save(path)


def read_image(path):
    """-> (C,H,W) float32, C = 3 (R,G,B) or 1."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("L" if im.mode in ("L", "1", "I;16", "I", "F", "LA") else "RGB"), np.float32)
    return a[None] if a.ndim == 2 else a.transpose(2, 0, 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("image_root")
    ap.add_argument("mask_root")
    ap.add_argument("--type", default="goodfeature")
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args(argv)
    if args.type != "goodfeature":
        known = "one of the reference's other mask types" if args.type in REFERENCE_TYPES else "not a mask type"
        raise SystemExit(f"--type {args.type}: {known}; goodfeature is the one built here")
    import torch
    from focusflow_official_amd.keypoints import GoodFeatures
    if not torch.cuda.is_available():
        raise SystemExit("generate_masks.py needs a HIP device: the detector has no CPU fallback")
    det = GoodFeatures()
    pending = {}      # (C,H,W) -> [(rel, array)]

    def flush(items):
        masks = det(torch.from_numpy(np.stack([a for _, a in items])).to("cuda:0")).cpu().numpy()
        for (rel, _), m in zip(items, masks):
            write_mask(mask_path(args.mask_root, rel), m[0])

    rels = find_images(args.image_root)
    for rel in rels:
        a = read_image(os.path.join(args.image_root, rel))
        group = pending.setdefault(a.shape, [])
        group.append((rel, a))
        if len(group) >= args.batch:
            flush(pending.pop(a.shape))
    for items in pending.values():
        flush(items)
    print(f"{len(rels)} masks written below {args.mask_root}")


if __name__ == "__main__":
    main()
