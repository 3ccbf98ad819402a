#!/usr/bin/env python3
"""Write a synthetic Xiph-layout tree for timing ``benchmark/evaluate.py --dataset xiph``: ROOT/<clip>/001.png ... of a smooth seeded
scene drifting from frame to frame plus a little per-pixel noise (so that the PNGs do not compress to nothing), and a synthetic
checkpoint.  No real Xiph frame is involved; the scores of such a run mean nothing, its times do.  ``--y4m`` writes the same generated
frames as Y4M clips instead, ROOT/<clip>.y4m, through ``yuv.Y4MWriter`` (``--depth 8``: C420jpeg, ``--depth 10``: C420p10, the form the
Xiph clips are distributed in).

    python tools/gen_xiph_tree.py ROOT [--clips Synthetic] [--frames 7] [--height 2160] [--width 4096] [--ckpt ROOT/ck.pt --model base]
                                  [--y4m [--depth 8|10]]"""
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
    ap.add_argument("--y4m", action="store_true", help="write ROOT/<clip>.y4m instead of ROOT/<clip>/NNN.png")
    ap.add_argument("--depth", type=int, choices=(8, 10), default=10, help="--y4m: bits per sample")
    a = ap.parse_args()
    yuv = importlib.import_module("atm-vfi_amd.yuv") if a.y4m else None
    h, w = a.height, a.width
    yy, xx = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    for ci, clip in enumerate(a.clips.split(",")):
        os.makedirs(a.root if a.y4m else os.path.join(a.root, clip), exist_ok=True)
        fmt = yuv.Format(h, w, depth=a.depth) if a.y4m else None
        wr = yuv.Y4MWriter(os.path.join(a.root, clip + ".y4m"), fmt, 60) if a.y4m else None
        rng = np.random.default_rng(ci)
        ph = rng.uniform(0, 6.28, size=(3, 3))
        for k in range(1, a.frames + 1):
            s = 0.004 * k
            fr = np.stack([0.5 + 0.25 * np.sin(9 * (xx + s) + ph[c, 0]) * np.cos(7 * (yy - s) + ph[c, 1]) + 0.2 * np.sin(31 * (xx + yy + s) + ph[c, 2])
                           for c in range(3)], axis=2) * 255 + rng.integers(-2, 3, size=(h, w, 3))
            u8 = np.clip(np.round(fr), 0, 255).astype(np.uint8)
            if wr is not None:          # (a 10-bit format encodes from fp32 in units of 1)
                wr.write(yuv.encode_numpy(u8.astype(np.float32) / np.float32(255) if a.depth == 10 else u8, fmt))
                continue
            Image.fromarray(u8).save(os.path.join(a.root, clip, f"{k:03d}.png"), compress_level=1)
        if wr is not None:
            wr.close()
    if a.ckpt:
        pkg = importlib.import_module("atm-vfi_amd")
        host_io = importlib.import_module("atm-vfi_amd.host_io")
        net = pkg.NetworkBase() if a.model == "base" else pkg.NetworkLite()
        net.load_state_dict(pkg.synthetic_state_dict(a.model, seed=1), strict=True)
        host_io.save_checkpoint(net, a.ckpt)
    print(f"wrote {a.root}")


if __name__ == "__main__":
    main()
