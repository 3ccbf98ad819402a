#!/usr/bin/env python3
"""Time the frame-difference kernel of duplicate detection (atm-vfi_amd/csrc/framediff.hip, atmvfi_frame_difference: two launches per
call) on whole frames of 480 x 832, 1080 x 1920 and 2160 x 4096, by the protocol of tools/bench_scene.py: device events around
back-to-back calls after a warm-up; the calls rotate over ``--buffers`` distinct frames (consecutive ones form the pair) so that the
sources come from HBM, not from the 256 MB Infinity Cache; every configuration is timed ``--repeats`` times in rotation and the
spread of the repeats is the noise a difference has to exceed.  Prints microseconds per call and the achieved bytes/s -- the
algorithm's bytes: both windows read once, 1 032 bytes written -- as a share of 6.3 TB/s.

``frame_signature`` runs in the same rotation and process on the same frames.  The expectation the kernel is held to: at 2160 x 4096,
where a call is not issue-bound, it reads twice the signature's bytes and should take no more than 2 x the signature's time + 15 %
(run-to-run spread); the last line prints the ratio and the verdict.

    python tools/bench_framediff.py [--iters 200] [--repeats 5] [--buffers 12] [--json OUT]"""
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
BOUND = 2.0 * 1.15


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
        sys.exit("bench_framediff: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops = hip_ops.HipOps(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    cfg = {}          # name -> (call, bytes of the algorithm)
    tiny = [torch.randint(0, 256, (16, 16, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(2)]
    sig = torch.empty(288, dtype=torch.int32, device=dev)
    dif = torch.empty(258, dtype=torch.int32, device=dev)
    cfg["frame_difference 16x16 (launch cost, 2 launches)"] = (lambda i: ops.frame_difference(tiny[0], tiny[1], out=dif), 2 * 768.0 + 1032.0)
    cfg["frame_signature 16x16 (launch cost, 2 launches)"] = (lambda i: ops.frame_signature(tiny[0], out=sig), 768.0 + 1152.0)
    for h, w in SIZES:
        n = max(a.buffers, -(-2 * CACHE // (3 * h * w)))
        src = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        ws_d, ws_s = ops.frame_difference_workspace(h, w), ops.frame_signature_workspace(h, w)
        cfg[f"frame_difference {h}x{w}"] = (lambda i, s=src, n=n, ws=ws_d: ops.frame_difference(s[i % n], s[(i + 1) % n], bgr=True, out=dif, workspace=ws),
                                            6.0 * h * w + 1032.0)
        cfg[f"frame_signature {h}x{w}"] = (lambda i, s=src, n=n, ws=ws_s: ops.frame_signature(s[i % n], bgr=True, out=sig, workspace=ws),
                                           3.0 * h * w + 1152.0)
    times = {k: [] for k in cfg}
    for _ in range(a.repeats):           # in rotation: every repeat visits every configuration once
        for k, (fn, _) in cfg.items():
            times[k].append(timed(fn, a.iters))
    rows, med = [], {}
    for k, (_, nbytes) in cfg.items():
        t = times[k]
        med[k] = statistics.median(t)
        row = {"name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes, "GBps": nbytes / (med[k] * 1e-6) / 1e9,
               "share_of_hbm": nbytes / (med[k] * 1e-6) / HBM, "repeats_us": t}
        rows.append(row)
        print(f"{k:>52}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.2f} MB  "
              f"{row['GBps']:7.1f} GB/s  {100 * row['share_of_hbm']:5.1f}% of 6.3 TB/s", flush=True)
    ratios = {}
    for h, w in SIZES:
        ratios[f"{h}x{w}"] = med[f"frame_difference {h}x{w}"] / med[f"frame_signature {h}x{w}"]
        print(f"difference / signature at {h}x{w}: {ratios[f'{h}x{w}']:.2f}")
    big = ratios["2160x4096"]
    print(f"expectation at 2160x4096: difference <= {BOUND:.2f} x signature -- {'met' if big <= BOUND else 'MISSED'} ({big:.2f})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": a.buffers, "rows": rows,
                       "ratios": ratios, "bound": BOUND}, f, indent=1)


if __name__ == "__main__":
    main()
