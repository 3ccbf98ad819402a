#!/usr/bin/env python3
"""Write a synthetic Xiph-layout tree for timing ``benchmark/evaluate.py --dataset xiph``: ROOT/<clip>/001.png ... of a smooth seeded
scene drifting from frame to frame plus a little per-pixel noise (so that the PNGs do not compress to nothing), and a synthetic
checkpoint.  No real Xiph frame is involved; the scores of such a run mean nothing, its times do.

    python tools/gen_xiph_tree.py ROOT [--clips Synthetic] [--frames 7] [--height 2160] [--width 4096] [--ckpt ROOT/ck.pt --model base]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("--clips", default="Synthetic")
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--model", choices=("base", "lite"), default="base")
    a = ap.parse_args()
    h, w = a.height, a.width
    yy, xx = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    for ci, clip in enumerate(a.clips.split(",")):
        os.makedirs(os.path.join(a.root, clip), exist_ok=True)
        rng = np.random.default_rng(ci)
        ph = rng.uniform(0, 6.28, size=(3, 3))
        for k in range(1, a.frames + 1):
            s = 0.004 * k
            fr = np.stack([0.5 + 0.25 * np.sin(9 * (xx + s) + ph[c, 0]) * np.cos(7 * (yy - s) + ph[c, 1]) + 0.2 * np.sin(31 * (xx + yy + s) + ph[c, 2])
                           for c in range(3)], axis=2) * 255 + rng.integers(-2, 3, size=(h, w, 3))
            Image.fromarray(np.clip(np.round(fr), 0, 255).astype(np.uint8)).save(os.path.join(a.root, clip, f"{k:03d}.png"), compress_level=1)
    if a.ckpt:
        pkg = importlib.import_module("atm-vfi_amd")
        host_io = importlib.import_module("atm-vfi_amd.host_io")
        net = pkg.NetworkBase() if a.model == "base" else pkg.NetworkLite()
        net.load_state_dict(pkg.synthetic_state_dict(a.model, seed=1), strict=True)
        host_io.save_checkpoint(net, a.ckpt)
    print(f"wrote {a.root}")


if __name__ == "__main__":
    main()
