"""Flow images for a tree of .flo files, coloured on the GPU: what a script around the reference's core/utils/flow_viz.py does
on the host (flow_to_image per file, one 8-bit RGB PNG each).

    python tools/render_flows.py <flo_root> <png_root> [--max-flow X] [--batch 16]

Every .flo below <flo_root> is read with frame_utils.readFlow, flows of equal size are rendered in batches (ops.flow_to_image,
csrc/flow_viz.hip) and the image goes to <png_root>/<same relative path, extension replaced>.png.  Without --max-flow every
flow is scaled by its own maximum magnitude, as the reference does it; with it all share one scale, which is what a sequence wants.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def find_flows(flo_root):
    """-> sorted paths relative to flo_root."""
    out = []
    for d, _, files in os.walk(flo_root):
        out += [os.path.relpath(os.path.join(d, f), flo_root) for f in files if os.path.splitext(f)[1].lower() == ".flo"]
    return sorted(out)


def png_path(png_root, rel):
    return os.path.join(png_root, os.path.splitext(rel)[0] + ".png")


def write_image(path, image):
    """(H,W,3) uint8 R,G,B -> 8-bit RGB PNG."""
    from PIL import Image
    image = np.asarray(image)
    assert image.ndim == 3 and image.shape[2] == 3 and image.dtype == np.uint8, "an image is (H,W,3) uint8"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(image, mode="RGB").save(path)


def render_tree(flo_root, png_root, max_flow=None, batch=16, device="cuda:0"):
    """Render every .flo below flo_root; -> the relative paths, in the order of find_flows."""
    import torch
    from focusflow_official_amd import frame_utils, ops
    pending = {}      # (H,W,2) -> [(rel, array)]

    def flush(items):
        field = torch.from_numpy(np.stack([a for _, a in items])).to(device)      # (B,H,W,2): passed as the (B,2,H,W) view it is
        images = ops.flow_to_image(field.permute(0, 3, 1, 2), max_flow=max_flow).cpu().numpy()
        for (rel, _), image in zip(items, images):
            write_image(png_path(png_root, rel), image)

    rels = find_flows(flo_root)
    for rel in rels:
        a = frame_utils.readFlow(os.path.join(flo_root, rel))
        if a is None:
            raise ValueError(f"{os.path.join(flo_root, rel)}: not a Middlebury .flo file")
        a = np.ascontiguousarray(a, dtype=np.float32)
        group = pending.setdefault(a.shape, [])
        group.append((rel, a))
        if len(group) >= batch:
            flush(pending.pop(a.shape))
    for items in pending.values():
        flush(items)
    return rels


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("flo_root")
    ap.add_argument("png_root")
    ap.add_argument("--max-flow", type=float, default=None)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_flows.py needs a HIP device: the colour wheel has no CPU fallback")
    rels = render_tree(args.flo_root, args.png_root, args.max_flow, args.batch)
    print(f"{len(rels)} images written below {args.png_root}")


if __name__ == "__main__":
    main()
