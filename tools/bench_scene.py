#!/usr/bin/env python3
"""Time the frame-signature kernel of scene-cut detection (atm-vfi_amd/csrc/scene.hip, atmvfi_frame_signature: two launches per call)
on whole frames of 480 x 832, 1080 x 1920 and 2160 x 4096.  Device events around back-to-back calls after a warm-up; the calls rotate
over ``--buffers`` distinct source frames so that the source comes from HBM, not from the 256 MB Infinity Cache (at 480 x 832, 1.2 MB a
frame, the number of buffers is raised until they exceed it).  Prints microseconds per call and the achieved bytes/s -- the algorithm's
bytes: the window read once, 1 152 bytes written -- as a share of 6.3 TB/s.

Beside it, timed in the same run and in rotation with it: ``frame_u8_window`` mode 0 on the same frames (the whole frame into an
un-padded fp32 canvas: the kernel that reads the same bytes and writes 4x as many), and the cost of an (almost) empty call -- the
signature of a 16 x 16 window, two one-block-sized launches -- next to which a small frame's time has to be read.  Every configuration
is timed ``--repeats`` times in rotation; the spread of the repeats is the noise a difference has to exceed.

    python tools/bench_scene.py [--iters 200] [--repeats 5] [--buffers 12] [--json OUT]"""
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
SIZES = ((480, 832), (1080, 1920), (2160, 4096))
CACHE = 256 << 20


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scene: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops = hip_ops.HipOps(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    cfg = {}          # name -> (call, bytes of the algorithm)
    tiny = torch.randint(0, 256, (16, 16, 3), dtype=torch.uint8, device=dev, generator=gen)
    sig = torch.empty(288, dtype=torch.int32, device=dev)
    cfg["frame_signature 16x16 (launch cost, 2 launches)"] = (lambda i: ops.frame_signature(tiny, out=sig), 768.0 + 1152.0)
    for h, w in SIZES:
        n = max(a.buffers, -(-2 * CACHE // (3 * h * w)))
        src = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        dst = [torch.empty(3, h, w, dtype=torch.float32, device=dev) for _ in range(min(n, max(2, a.buffers)))]
        ws = ops.frame_signature_workspace(h, w)
        cfg[f"frame_signature {h}x{w}"] = (lambda i, s=src, n=n, ws=ws: ops.frame_signature(s[i % n], out=sig, workspace=ws), 3.0 * h * w + 1152.0)
        cfg[f"frame_signature {h}x{w} bgr"] = (lambda i, s=src, n=n, ws=ws: ops.frame_signature(s[i % n], bgr=True, out=sig, workspace=ws),
                                               3.0 * h * w + 1152.0)
        cfg[f"frame_u8_window mode 0 {h}x{w} -> fp32"] = (lambda i, s=src, n=n, d=dst, h=h, w=w: ops.frame_u8_window(s[i % n], 0, 0, 0, h, w, dst=d[i % len(d)]),
                                                          15.0 * h * w)
    times = {k: [] for k in cfg}
    for _ in range(a.repeats):           # in rotation: every repeat visits every configuration once
        for k, (fn, _) in cfg.items():
            times[k].append(timed(fn, a.iters))
    rows = []
    for k, (_, nbytes) in cfg.items():
        t = times[k]
        med = statistics.median(t)
        row = {"name": k, "us_median": med, "us_min": min(t), "us_max": max(t), "bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9,
               "share_of_hbm": nbytes / (med * 1e-6) / HBM, "repeats_us": t}
        rows.append(row)
        print(f"{k:>52}: {med:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.2f} MB  "
              f"{row['GBps']:7.1f} GB/s  {100 * row['share_of_hbm']:5.1f}% of 6.3 TB/s", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": a.buffers, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
