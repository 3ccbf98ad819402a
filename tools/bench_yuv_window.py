#!/usr/bin/env python3
"""Time the fused decode-window kernel (atm-vfi_amd/csrc/yuv.hip: atmvfi_yuv_decode with mode) on the protocol of tools/bench_yuv.py:
device events around ``--iters`` back-to-back calls after 24 warm-up calls, the calls rotating over ``--buffers`` distinct sources and
destinations, every configuration timed ``--repeats`` times in rotation (median, min - max).  Sizes 2160 x 4096 (10 bit, bt709: a
Xiph clip) and 1080 x 1920 (8 bit), each with the two windows of the Xiph evaluation (``evaluate.xiph_geometry``): mode 1 on the whole
frame ("resized-2k") and mode 0 on the centre window ("cropped-4k"), to the fp32 canvas padded to a multiple of 32 and to the uint8
ground truth.

The yardstick of every fused call is the two-call composition that gives the same output -- ``yuv420_to_rgb`` -> uint8 (the whole
frame), then ``frame_u8_window`` -- timed in the same rotation and process, call by call and back to back.  The expectation: the fused
call takes no longer than the sum of its two composition calls (it performs the same arithmetic per source pixel, drops one write and
one read of the RGB frame, and in mode 0 decodes a quarter of the pixels).  Bytes are the algorithm's -- inputs read once, outputs
written once -- as a share of 6.3 TB/s.

    python tools/bench_yuv_window.py [--iters 120] [--repeats 5] [--buffers 8] [--json OUT] [--lib PATH] [--baseline-lib PATH]

``--baseline-lib``: tools/yuv_timing.py."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
host_io = importlib.import_module("atm-vfi_amd.host_io")
evaluate = importlib.import_module("atm-vfi_amd.evaluate")
yuv = importlib.import_module("atm-vfi_amd.yuv")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation, --baseline-lib)
HBM = 6.3e12
SIZES = [(2160, 4096, 10), (1080, 1920, 8)]


def configs(ops, dev, H, W, depth, n):
    """name -> (call, bytes of the algorithm, names of the composition calls whose sum is the yardstick, or None)."""
    fmt = yuv.Format(H, W, depth=depth)
    gen = torch.Generator(device=dev).manual_seed(H)
    if depth == 10:
        src = [torch.randint(0, 1024, (fmt.frame_samples,), dtype=torch.int16, device=dev, generator=gen).view(torch.uint8) for _ in range(n)]
    else:
        src = [torch.randint(0, 256, (fmt.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    rgb = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    for i in range(n):
        ops.yuv420_to_rgb(src[i], fmt, dst_u8=rgb[i])
    cfg = {"yuv420_to_rgb -> uint8 (composition, 1st call)": (lambda i: ops.yuv420_to_rgb(src[i % n], fmt, dst_u8=rgb[i % n]),
                                                            fmt.frame_bytes + 3.0 * H * W, None)}
    decode = "yuv420_to_rgb -> uint8 (composition, 1st call)"
    for cat in evaluate.XIPH_CATEGORIES:
        mode, y0, x0, h, w = evaluate.xiph_geometry(H, W, cat)
        left, right, top, bottom = host_io.InputPadder((h, w), divisor=32)._pad
        hp, wp = h + top + bottom, w + left + right
        f32 = [torch.empty(3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]
        u8 = [torch.empty(h, w, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
        s = 2 if mode == 1 else 1
        read = 1.5 * (2 if depth == 10 else 1) * s * s * h * w          # the I420 samples under the window
        win = 3.0 * s * s * h * w                                       # the RGB pixels under the window

        def add(kind, out_bytes, kw, mode=mode, y0=y0, x0=x0, h=h, w=w, read=read, win=win):
            second = f"frame_u8_window mode {mode} -> {kind} (composition, 2nd call)"
            cfg[second] = (lambda i: ops.frame_u8_window(rgb[i % n], mode, y0, x0, h, w, **kw(i)), win + out_bytes, None)
            cfg[f"yuv420_window mode {mode} -> {kind} (fused)"] = (lambda i: ops.yuv420_window(src[i % n], fmt, mode, y0, x0, h, w, **kw(i)),
                                                                   read + out_bytes, (decode, second))
        add("fp32", 12.0 * hp * wp, lambda i, f32=f32, top=top, left=left: {"dst": f32[i % n], "pad_top": top, "pad_left": left})
        add("uint8", 3.0 * h * w, lambda i, u8=u8: {"dst_u8": u8[i % n]})
    return cfg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=8)
    ap.add_argument("--json", default=None)
    yuv_timing.add_library_arguments(ap)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_window: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops, base_ops = yuv_timing.libraries(a, dev)
    n = max(1, a.buffers)
    rows = []
    for H, W, depth in SIZES:
        cfg = configs(ops, dev, H, W, depth, n)
        base_cfg = configs(base_ops, dev, H, W, depth, n) if base_ops else None
        times, base = yuv_timing.rotation(cfg, base_cfg, a.repeats, a.iters)          # every repeat visits every configuration once
        med = {k: statistics.median(t) for k, t in times.items()}
        print(f"--- {H} x {W}, {depth} bit, {yuv.Format(H, W, depth=depth).matrix}", flush=True)
        for k, (_, nbytes, parts) in cfg.items():
            t = times[k]
            row = {"size": [H, W], "depth": depth, "name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                   "GBps": nbytes / (med[k] * 1e-6) / 1e9, "share_of_hbm": nbytes / (med[k] * 1e-6) / HBM, "repeats_us": t}
            rel = ""
            if parts:
                total = sum(med[q] for q in parts)
                lo, hi = sum(min(times[q]) for q in parts), sum(max(times[q]) for q in parts)
                row.update({"composition_us_median": total, "composition_us_min": lo, "composition_us_max": hi, "over_composition": med[k] / total,
                            "within_expectation": bool(min(t) <= hi)})
                rel = f"  composition {total:8.2f} us (min {lo:.2f}, max {hi:.2f}): fused = {med[k] / total:5.2f} x"
            rel += yuv_timing.against_baseline(row, times, base, k)
            rows.append(row)
            print(f"{k:>58}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
                  f"{row['GBps']:7.1f} GB/s  {100 * row['share_of_hbm']:5.1f}% of 6.3 TB/s{rel}", flush=True)
        del cfg, base_cfg
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": n, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
