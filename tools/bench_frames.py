#!/usr/bin/env python3
"""Time the frame-preparation kernel (atm-vfi_amd/csrc/frames.hip, atmvfi_frame_u8_window) on 2160 x 4096 frames as the Xiph
evaluation uses it: mode 0 (the 1080 x 2048 centre window) and mode 1 (the whole frame reduced 2x), each into the padded fp32 input
[3,1088,2048] alone and together with the uint8 ground truth.  Device events around back-to-back calls after a warm-up; the calls
rotate over ``--buffers`` distinct source frames (12 x 26.5 MB exceeds the 256 MB Infinity Cache, so the source comes from HBM) and as
many destinations.  Prints microseconds per frame and the achieved bytes/s -- the algorithm's bytes: the source window read once, the
outputs written once -- as a share of 6.3 TB/s.

The yardstick, timed in the same run and alternating with the others: ``frame_u8_to_f32`` on a 1080 x 2048 frame into 1088 x 2048, the
kernel that wrote the same output bytes before this one existed.  Every configuration is timed ``--repeats`` times in rotation; the
spread of those repeats is the noise a difference has to exceed.

    python tools/bench_frames.py [--iters 240] [--repeats 5] [--buffers 12] [--json OUT]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
HBM = 6.3e12
H, W, h, w, HP, WP, TOP = 2160, 4096, 1080, 2048, 1088, 2048, 4


def timed(fn, iters):
    """us per call of fn(i), i = 0 .. iters-1 back to back."""
    for i in range(24):
        fn(i)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_frames: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops = hip_ops.HipOps(dev)
    n = max(1, a.buffers)
    gen = torch.Generator(device=dev).manual_seed(0)
    src4k = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    src2k = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    dst = [torch.empty(3, HP, WP, dtype=torch.float32, device=dev) for _ in range(n)]
    gt = [torch.empty(h, w, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    out_f32, out_u8 = 12.0 * HP * WP, 3.0 * h * w
    # name -> (call, bytes of the algorithm)
    cfg = {
        "frame_u8_to_f32 1080x2048 (yardstick)": (lambda i: ops.frame_u8_to_f32(src2k[i % n], dst[i % n], TOP, 0, False), 3.0 * h * w + out_f32),
        "window mode 0, 2k source, fp32": (lambda i: ops.frame_u8_window(src2k[i % n], 0, 0, 0, h, w, dst=dst[i % n], pad_top=TOP), 3.0 * h * w + out_f32),
        "window mode 0, 4k centre, fp32": (lambda i: ops.frame_u8_window(src4k[i % n], 0, H // 4, W // 4, h, w, dst=dst[i % n], pad_top=TOP),
                                           3.0 * h * w + out_f32),
        "window mode 0, 4k centre, fp32 + u8": (lambda i: ops.frame_u8_window(src4k[i % n], 0, H // 4, W // 4, h, w, dst=dst[i % n], dst_u8=gt[i % n],
                                                                                pad_top=TOP), 3.0 * h * w + out_f32 + out_u8),
        "window mode 1, 4k -> 2k, fp32": (lambda i: ops.frame_u8_window(src4k[i % n], 1, 0, 0, h, w, dst=dst[i % n], pad_top=TOP), 3.0 * H * W + out_f32),
        "window mode 1, 4k -> 2k, fp32 + u8": (lambda i: ops.frame_u8_window(src4k[i % n], 1, 0, 0, h, w, dst=dst[i % n], dst_u8=gt[i % n], pad_top=TOP),
                                               3.0 * H * W + out_f32 + out_u8),
        "window mode 1, 4k -> 2k, u8 only": (lambda i: ops.frame_u8_window(src4k[i % n], 1, 0, 0, h, w, dst_u8=gt[i % n]), 3.0 * H * W + out_u8),
    }
    times = {k: [] for k in cfg}
    for _ in range(a.repeats):           # in rotation: every repeat visits every configuration once
        for k, (fn, _) in cfg.items():
            times[k].append(timed(fn, a.iters))
    rows = []
    for k, (_, nbytes) in cfg.items():
        t = times[k]
        med = statistics.median(t)
        row = {"name": k, "us_per_frame_median": med, "us_min": min(t), "us_max": max(t), "bytes": nbytes,
               "GBps": nbytes / (med * 1e-6) / 1e9, "share_of_hbm": nbytes / (med * 1e-6) / HBM, "repeats_us": t}
        rows.append(row)
        print(f"{k:>40}: {med:8.2f} us/frame (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
              f"{row['GBps']:7.1f} GB/s  {100 * row['share_of_hbm']:5.1f}% of 6.3 TB/s", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": n, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
