#!/usr/bin/env python3
"""Time the YUV 4:2:0 kernels (atm-vfi_amd/csrc/yuv.hip: atmvfi_yuv_decode; yuv_encode.hip: atmvfi_yuv_encode) on the method of
tools/bench_frames.py: device events around ``--iters`` back-to-back calls after 24 warm-up calls, the calls rotating over
``--buffers`` distinct sources and destinations, every configuration timed ``--repeats`` times in rotation (median, min - max).  Bytes
are the algorithm's -- inputs read once, outputs written once -- as a share of 6.3 TB/s.  Sizes 480 x 832, 1080 x 1920, 2160 x 4096,
each into / out of the canvas padded to a multiple of 64 as the loops use it.

The yardsticks run in the same rotation on the same geometry: ``frame_u8_window`` mode 0 -> fp32 (15 B/px against the decode's 13.5)
and ``frame_f32_to_u8`` (15 B/px against the encode's 13.5).  The last column is the call's median over its yardstick's.

``--pipeline N``: ``FramePipeline`` on N 1080p pairs (network_base, synthetic weights) with and without ``pixfmt``, interleaved.

    python tools/bench_yuv.py [--iters 240] [--repeats 5] [--buffers 12] [--pipeline 0] [--json OUT] [--lib PATH] [--baseline-lib PATH]

``--baseline-lib``: tools/yuv_timing.py."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
host_io = importlib.import_module("atm-vfi_amd.host_io")
yuv = importlib.import_module("atm-vfi_amd.yuv")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation, --baseline-lib)
HBM = 6.3e12
SIZES = [(480, 832), (1080, 1920), (2160, 4096)]


def configs(ops, dev, H, W, n):
    pad = host_io.InputPadder((1, 3, H, W), divisor=64)
    pl, pr, pt, pb = pad._pad
    Hp, Wp = H + pt + pb, W + pl + pr
    gen = torch.Generator(device=dev).manual_seed(H)
    f8, f10 = yuv.Format(H, W), yuv.Format(H, W, depth=10)
    y8 = [torch.randint(0, 256, (f8.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    y10 = [torch.randint(0, 1024, (f10.frame_samples,), dtype=torch.int16, device=dev, generator=gen).view(torch.uint8) for _ in range(n)]
    rgb = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    f32 = [torch.rand(3, Hp, Wp, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
    o8 = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    oy = [torch.empty(f8.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(n)]
    px, can = float(H * W), 12.0 * Hp * Wp
    # name -> (call, bytes of the algorithm, yardstick's name or None)
    return {
        "frame_u8_window mode 0 -> fp32 (yardstick)": (lambda i: ops.frame_u8_window(rgb[i % n], 0, 0, 0, H, W, dst=f32[i % n], pad_top=pt, pad_left=pl),
                                                       3 * px + can, None),
        "yuv420_to_rgb -> fp32": (lambda i: ops.yuv420_to_rgb(y8[i % n], f8, dst=f32[i % n], pad_top=pt, pad_left=pl), 1.5 * px + can,
                                  "frame_u8_window mode 0 -> fp32 (yardstick)"),
        "yuv420_to_rgb -> fp32 + u8": (lambda i: ops.yuv420_to_rgb(y8[i % n], f8, dst_u8=o8[i % n], dst=f32[i % n], pad_top=pt, pad_left=pl),
                                       4.5 * px + can, "frame_u8_window mode 0 -> fp32 (yardstick)"),
        "yuv420_to_rgb 10 bit -> fp32": (lambda i: ops.yuv420_to_rgb(y10[i % n], f10, dst=f32[i % n], pad_top=pt, pad_left=pl), 3 * px + can,
                                         "frame_u8_window mode 0 -> fp32 (yardstick)"),
        "yuv420_to_rgb -> u8": (lambda i: ops.yuv420_to_rgb(y8[i % n], f8, dst_u8=o8[i % n]), 4.5 * px, None),
        "frame_f32_to_u8 (yardstick)": (lambda i: ops.frame_f32_to_u8(f32[i % n], o8[i % n], pt, pl, False), 15 * px, None),
        "rgb_to_yuv420 from fp32": (lambda i: ops.rgb_to_yuv420(oy[i % n], f8, src=f32[i % n], pad_top=pt, pad_left=pl), 13.5 * px,
                                    "frame_f32_to_u8 (yardstick)"),
        "rgb_to_yuv420 from fp32, left-sited": (lambda i: ops.rgb_to_yuv420(oy[i % n], yuv.Format(H, W, siting="left"), src=f32[i % n], pad_top=pt,
                                                                           pad_left=pl), 13.5 * px, "frame_f32_to_u8 (yardstick)"),
        "rgb_to_yuv420 from u8": (lambda i: ops.rgb_to_yuv420(oy[i % n], f8, src_u8=rgb[i % n]), 4.5 * px, None),
    }


def pipeline(dev, pairs_n, repeats):
    pkg = importlib.import_module("atm-vfi_amd")
    H, W = 1080, 1920
    net = pkg.NetworkBase()
    net.load_state_dict(pkg.synthetic_state_dict("base", seed=1), strict=True)
    net = net.to(dev).eval()
    fmt = yuv.Format(H, W)
    rng = np.random.default_rng(0)
    rgb = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
    i420 = [yuv.encode_numpy(f, fmt) for f in rgb]
    runs = {"RGB (9 B/px per pair)": (rgb, None), "I420 (4.5 B/px per pair)": (i420, fmt)}
    pipes = {k: host_io.FramePipeline(net, H, W, isBGR=False, pixfmt=f) for k, (_, f) in runs.items()}
    times = {k: [] for k in runs}
    for r in range(repeats + 1):             # interleaved; the first round warms up (workspace, launch plan)
        for k, (frames, _) in runs.items():
            pairs = [(frames[i % 4], frames[(i + 1) % 4]) for i in range(pairs_n)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in pipes[k].run(pairs):
                pass
            dt = time.perf_counter() - t0
            if r:
                times[k].append(1e3 * dt / pairs_n)
    rows = []
    for k, t in times.items():
        med = statistics.median(t)
        rows.append({"name": "FramePipeline 1080p " + k, "ms_per_pair_median": med, "ms_min": min(t), "ms_max": max(t), "pairs": pairs_n})
        print(f"FramePipeline 1080p network_base, {k:>26}: {med:7.2f} ms/pair (min {min(t):.2f}, max {max(t):.2f} over {len(t)} runs of "
              f"{pairs_n} pairs)  {1e3 / med:6.2f} frames/s", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--pipeline", type=int, default=0, help="pairs per FramePipeline run (0: skip)")
    ap.add_argument("--json", default=None)
    yuv_timing.add_library_arguments(ap)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops, base_ops = yuv_timing.libraries(a, dev)
    n = max(1, a.buffers)
    rows = []
    for H, W in SIZES:
        cfg = configs(ops, dev, H, W, n)
        base_cfg = configs(base_ops, dev, H, W, n) if base_ops else None
        times, base = yuv_timing.rotation(cfg, base_cfg, a.repeats, a.iters)          # every repeat visits every configuration once
        med = {k: statistics.median(t) for k, t in times.items()}
        print(f"--- {H} x {W}", flush=True)
        for k, (_, nbytes, ref) in cfg.items():
            t = times[k]
            row = {"size": [H, W], "name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                   "GBps": nbytes / (med[k] * 1e-6) / 1e9, "share_of_hbm": nbytes / (med[k] * 1e-6) / HBM,
                   "over_yardstick": med[k] / med[ref] if ref else None, "repeats_us": t}
            rows.append(row)
            rel = (f"  {row['over_yardstick']:5.2f} x its yardstick" if ref else "") + yuv_timing.against_baseline(row, times, base, k)
            print(f"{k:>44}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
                  f"{row['GBps']:7.1f} GB/s  {100 * row['share_of_hbm']:5.1f}% of 6.3 TB/s{rel}", flush=True)
        del cfg, base_cfg
        torch.cuda.empty_cache()
    if a.pipeline > 0:
        rows += pipeline(dev, a.pipeline, 3)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": n, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
