#!/usr/bin/env python3
"""Generate ``tests/golden/scene_ref.npz``, the pictures the scene-cut thresholds are placed on (atm-vfi_amd/scene.py, README "Scene
cuts"): the reference's two example frames at half size and three of its other asset pictures resized to that size, as uint8 RGB
arrays.  The pictures are data of the reference; they are read with PIL by this script only.

    python tools/gen_scene_golden.py --reference DIR

Keys: ``frame0``, ``frame1`` (consecutive frames of one shot) and ``other.<name>`` (unrelated pictures), all [300, 207, 3] uint8."""
import argparse
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("davis-motor", "video_cover_resize", "extra-viz-data3-1")


def load(path, size=None):
    im = Image.open(path).convert("RGB")
    if size is None:
        size = (im.size[0] // 2, im.size[1] // 2)
    return np.asarray(im.resize(size, Image.BILINEAR), dtype=np.uint8), size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scene_ref.npz"))
    args = ap.parse_args()
    asset = os.path.join(os.path.abspath(args.reference), "asset")
    arrs = {}
    arrs["frame0"], size = load(os.path.join(asset, "example_frame0.png"))
    arrs["frame1"], _ = load(os.path.join(asset, "example_frame1.png"), size)
    for name in OTHERS:
        arrs[f"other.{name}"], _ = load(os.path.join(asset, name + ".png"), size)
    np.savez_compressed(args.out, **arrs)
    print(f"wrote {args.out}: {len(arrs)} pictures of {size[1]}x{size[0]}, {os.path.getsize(args.out)} bytes")
    assert os.path.getsize(args.out) < (1 << 20)


if __name__ == "__main__":
    main()
