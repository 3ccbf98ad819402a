#!/usr/bin/env python3
"""Time the surface calls (atm-vfi_amd/csrc/yuv.hip: atmvfi_yuv_decode; yuv_encode.hip: atmvfi_yuv_encode) beside their
planar neighbours, on the protocol of tools/bench_yuv.py: device events around ``--iters`` back-to-back calls after 24 warm-up calls,
the calls rotating over ``--buffers`` distinct sources and destinations (beyond the Infinity Cache), every configuration timed
``--repeats`` times in rotation in one process (median, min - max).  Decode -> fp32 canvas and encode from the fp32 canvas, the canvas
padded to a multiple of 64 as the loops use it, for NV12, NV12 at pitch 2048 (1080p only: what a decoder hands over), P010 decoded to
8 bit, and P010 with the depth kept; sizes 1080 x 1920 and 2160 x 4096.

A semi-planar call moves the bytes its planar neighbour moves, so it is held to the project's standing bound for a neighbour: no more
than the planar call's median plus 15 % at 2160 x 4096 (``verdict``).  At 1080p both sit at the call-issue floor: reported, no verdict.

    python tools/bench_yuv_surface.py [--iters 240] [--repeats 5] [--buffers 12] [--json OUT] [--lib PATH]"""
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
yuv = importlib.import_module("atm-vfi_amd.yuv")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation)
HBM = 6.3e12
SIZES = [(1080, 1920), (2160, 4096)]
BOUND = 1.15


def configs(ops, dev, H, W, n):
    pad = host_io.InputPadder((1, 3, H, W), divisor=64)
    pl, pr, pt, pb = pad._pad
    Hp, Wp = H + pt + pb, W + pl + pr
    gen = torch.Generator(device=dev).manual_seed(H)
    f8, f10 = yuv.Format(H, W), yuv.Format(H, W, depth=10)
    nv12, p010 = yuv.Surface.nv12(H, W), yuv.Surface.p010(H, W)
    rand = lambda nbytes: [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    y8, y10 = rand(f8.frame_bytes), [torch.randint(0, 1024, (f10.frame_samples,), dtype=torch.int16, device=dev, generator=gen).view(torch.uint8)
                                     for _ in range(n)]
    s8, s10 = rand(nv12.nbytes), rand(p010.nbytes)          # (msb: every bit pattern is a sample)
    f32 = [torch.rand(3, Hp, Wp, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
    o8, o10 = [torch.empty(f8.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(n)], [torch.empty(f10.frame_bytes, dtype=torch.uint8,
                                                                                                         device=dev) for _ in range(n)]
    px, can = float(H * W), 12.0 * Hp * Wp
    geo = dict(pad_top=pt, pad_left=pl)
    # name -> (call, bytes of the algorithm, the planar neighbour's name or None)
    cfg = {
        "yuv420_to_rgb -> fp32 (planar)": (lambda i: ops.yuv420_to_rgb(y8[i % n], f8, dst=f32[i % n], **geo), 1.5 * px + can, None),
        "surface_decode NV12 -> fp32": (lambda i: ops.yuv_surface_decode(s8[i % n], nv12, dst=f32[i % n], **geo), 1.5 * px + can,
                                        "yuv420_to_rgb -> fp32 (planar)"),
        "yuv420_to_rgb 10 bit -> fp32 (planar)": (lambda i: ops.yuv420_to_rgb(y10[i % n], f10, dst=f32[i % n], **geo), 3 * px + can, None),
        "surface_decode P010 -> fp32": (lambda i: ops.yuv_surface_decode(s10[i % n], p010, dst=f32[i % n], **geo), 3 * px + can,
                                        "yuv420_to_rgb 10 bit -> fp32 (planar)"),
        "yuv420p10_to_f32 (planar, depth kept)": (lambda i: ops.yuv420p10_to_f32(y10[i % n], f10, f32[i % n], **geo), 3 * px + can, None),
        "surface_decode P010 -> fp32, depth kept": (lambda i: ops.yuv_surface_decode(s10[i % n], p010, dst=f32[i % n], keep_depth=True, **geo),
                                                    3 * px + can, "yuv420p10_to_f32 (planar, depth kept)"),
        "rgb_to_yuv420 from fp32 (planar)": (lambda i: ops.rgb_to_yuv420(o8[i % n], f8, src=f32[i % n], **geo), 13.5 * px, None),
        "surface_encode NV12 from fp32": (lambda i: ops.yuv_surface_encode(o8[i % n], nv12, src=f32[i % n], **geo), 13.5 * px,
                                          "rgb_to_yuv420 from fp32 (planar)"),
        "f32_to_yuv420p10 (planar, depth kept)": (lambda i: ops.f32_to_yuv420p10(o10[i % n], f10, f32[i % n], **geo), 15 * px, None),
        "surface_encode P010 from fp32, depth kept": (lambda i: ops.yuv_surface_encode(o10[i % n], p010, src=f32[i % n], **geo), 15 * px,
                                                      "f32_to_yuv420p10 (planar, depth kept)"),
    }
    if W == 1920:           # the surface a decoder hands over for 1080p
        pitched = yuv.Surface.nv12(H, W, pitch=2048)
        sp = rand(pitched.nbytes)
        cfg["surface_decode NV12 pitch 2048 -> fp32"] = (lambda i: ops.yuv_surface_decode(sp[i % n], pitched, dst=f32[i % n], **geo),
                                                         1.5 * px + can, "yuv420_to_rgb -> fp32 (planar)")
    return cfg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="the library under test (default: the package's)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_surface: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops = yuv_timing.hip_ops.HipOps(dev, lib_path=a.lib)
    n = max(1, a.buffers)
    rows, missed = [], []
    for H, W in SIZES:
        cfg = configs(ops, dev, H, W, n)
        times, _ = yuv_timing.rotation(cfg, None, a.repeats, a.iters)          # every repeat visits every configuration once
        med = {k: statistics.median(t) for k, t in times.items()}
        judged = (H, W) == SIZES[-1]
        print(f"--- {H} x {W}" + ("" if judged else "  (call-issue floor: no verdict)"), flush=True)
        for k, (_, nbytes, ref) in cfg.items():
            t = times[k]
            over = med[k] / med[ref] if ref else None
            verdict = None if (ref is None or not judged) else ("within" if over <= BOUND else "MISSED")
            if verdict == "MISSED":
                missed.append(k)
            rows.append({"size": [H, W], "name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                         "GBps": nbytes / (med[k] * 1e-6) / 1e9, "share_of_hbm": nbytes / (med[k] * 1e-6) / HBM, "over_planar": over,
                         "verdict": verdict, "repeats_us": t})
            rel = f"  {over:5.3f} x its planar neighbour" if ref else ""
            rel += f"  [{verdict}: bound {BOUND:.2f}]" if verdict else ""
            print(f"{k:>44}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
                  f"{nbytes / (med[k] * 1e-6) / 1e9:7.1f} GB/s  {100 * nbytes / (med[k] * 1e-6) / HBM:5.1f}% of 6.3 TB/s{rel}", flush=True)
        del cfg
        torch.cuda.empty_cache()
    print("verdict at %d x %d: %s" % (SIZES[-1] + ("every surface call within its planar neighbour + 15 %" if not missed else
                                                   "MISSED by " + "; ".join(missed),)), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": n, "bound": BOUND, "rows": rows}, f,
                      indent=1)


if __name__ == "__main__":
    main()
