#!/usr/bin/env python3
"""Time the fused metric kernel (atm-vfi_amd/csrc/metrics.hip: ssim_matlab + squared-error mean in one call) at 256x448 (B = 1 and 8)
and 1080p, beside a torch conv3d restatement of the reference's ssim_matlab (benchmark/pytorch_msssim.py:82-135, what the reference's
scripts run) on the same GPU.  Device events around N back-to-back calls after a warm-up; prints microseconds per frame and the
fused kernel's achieved bytes/s (an fp32 prediction + a uint8 or fp32 ground truth, read once) against 6.3 TB/s.

    python tools/bench_metrics.py [--iters 50] [--json OUT]"""
import argparse
import importlib
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
metrics = importlib.import_module("atm-vfi_amd.metrics")
HBM = 6.3e12


def conv3d_ssim(img1, img2, window):
    """ssim_matlab as the reference computes it (L = 1): five conv3d on replicate-padded volumes."""
    a, b = img1.unsqueeze(1), img2.unsqueeze(1)
    cv = lambda v: F.conv3d(F.pad(v, (5, 5, 5, 5, 5, 5), mode="replicate"), window)
    mu1, mu2 = cv(a), cv(b)
    s1, s2, s12 = cv(a * a) - mu1 * mu1, cv(b * b) - mu2 * mu2, cv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    v1, v2 = 2.0 * s12 + C2, s1 + s2 + C2
    return (((2 * mu1 * mu2 + C1) * v1) / ((mu1 * mu1 + mu2 * mu2 + C1) * v2)).mean()


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters     # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_metrics: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    g = torch.tensor([math.exp(-(k - 5) ** 2 / 4.5) for k in range(11)])
    g = g / g.sum()
    window = (g[:, None, None] * g[None, :, None] * g[None, None, :])[None, None].to(dev)
    rows = []
    for b, h, w in ((1, 256, 448), (8, 256, 448), (1, 1080, 1920)):
        gen = torch.Generator(device=dev).manual_seed(0)
        y = torch.rand(b, 3, h, w, device=dev, generator=gen)
        x_f = (y + 0.05 * torch.randn(b, 3, h, w, device=dev, generator=gen)).clamp(0, 1)
        x_u8 = (x_f * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        out = torch.empty(b, 3, dtype=torch.float64, device=dev)
        t_u8 = timed(lambda: metrics.ssim_psnr_raw(y, x_u8, out=out), a.iters)
        t_f32 = timed(lambda: metrics.ssim_psnr_raw(y, x_f, out=out, val_range=1.0), a.iters)
        t_auto = timed(lambda: metrics.ssim_psnr_raw(y, x_f, out=out), a.iters)
        t_ref = timed(lambda: conv3d_ssim(x_f, y, window), max(3, a.iters // 10))
        px = b * h * w
        row = {"shape": f"{b}x3x{h}x{w}",
               "fused_u8_us_per_frame": t_u8 / b, "fused_u8_GBps": px * (12 + 3) / (t_u8 * 1e-6) / 1e9,
               "fused_f32_us_per_frame": t_f32 / b, "fused_f32_GBps": px * (12 + 12) / (t_f32 * 1e-6) / 1e9,
               "fused_f32_autorange_us_per_frame": t_auto / b,
               "torch_conv3d_us_per_frame": t_ref / b}
        row["fused_u8_share_of_hbm"] = row["fused_u8_GBps"] * 1e9 / HBM
        rows.append(row)
        print(f"{row['shape']:>16}: fused (u8 gt) {row['fused_u8_us_per_frame']:9.1f} us/frame  {row['fused_u8_GBps']:7.1f} GB/s "
              f"({100 * row['fused_u8_share_of_hbm']:.1f}% of 6.3 TB/s) | fused (f32 gt) {row['fused_f32_us_per_frame']:9.1f} us/frame, "
              f"autodetected L {row['fused_f32_autorange_us_per_frame']:9.1f} | torch conv3d {row['torch_conv3d_us_per_frame']:10.1f} us/frame",
              flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
