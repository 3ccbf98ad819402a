#!/usr/bin/env python3
"""Time the 4:2:2 / 4:4:4 calls (atm-vfi_amd/csrc/yuv.hip: atmvfi_yuv_decode; yuv_encode.hip: atmvfi_yuv_encode) beside the planar
4:2:0 call of the same direction and depth, on the protocol of tools/bench_yuv.py: device events around ``--iters`` back-to-back calls
after 24 warm-up calls, the calls rotating over ``--buffers`` distinct sources and destinations (beyond the Infinity Cache), every
configuration timed ``--repeats`` times in rotation in one process (median, min - max).  Decode -> fp32 canvas and encode from the
fp32 canvas, the canvas padded to a multiple of 64 as the loops use it: 8 bit -> fp32, 10 bit kept -> fp32, fp32 -> 8 bit, fp32 ->
10 bit, for 4:2:2 (left-sited, as Y4M and decoders deliver it) and 4:4:4; sizes 1080 x 1920 and 2160 x 4096.

A 4:2:2 / 4:4:4 call moves more bytes than its 4:2:0 neighbour, so it is held to the project's bound for a byte-bound neighbour with
the bytes scaled: at 2160 x 4096 no more than ``(its bytes / the neighbour's bytes) x the neighbour's median + 15 %`` (``verdict``).
The neighbour is the 4:2:0 entry point that existed before these calls did (same siting, same depth); ``--neighbour-lib`` times it on
another build of the library (the parent commit's), in the same rotation.  At 1080p the calls sit at the call-issue floor: reported,
no verdict.

    python tools/bench_yuv_sub.py [--iters 240] [--repeats 5] [--buffers 12] [--json OUT] [--lib PATH] [--neighbour-lib PATH]"""
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
SITING = {"422": "left", "444": "centre"}


def configs(ops, near, dev, H, W, n):
    """name -> (call, bytes of the algorithm, the 4:2:0 neighbour's name or None); ``near`` runs the neighbours"""
    pad = host_io.InputPadder((1, 3, H, W), divisor=64)
    pl, pr, pt, pb = pad._pad
    Hp, Wp = H + pt + pb, W + pl + pr
    gen = torch.Generator(device=dev).manual_seed(H)
    f32 = [torch.rand(3, Hp, Wp, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
    geo = dict(pad_top=pt, pad_left=pl)
    can, src = 12.0 * Hp * Wp, 12.0 * H * W

    def frames(fmt):
        if fmt.depth == 8:
            return [torch.randint(0, 256, (fmt.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        return [torch.randint(0, 1024, (fmt.frame_samples,), dtype=torch.int16, device=dev, generator=gen).view(torch.uint8) for _ in range(n)]

    def outputs(fmt):
        return [torch.empty(fmt.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(n)]
    cfg = {}
    for siting in ("centre", "left"):           # the neighbours: the planar 4:2:0 entry points
        f8, f10 = yuv.Format(H, W, siting=siting), yuv.Format(H, W, siting=siting, depth=10)
        y8, y10, o8, o10 = frames(f8), frames(f10), outputs(f8), outputs(f10)
        cfg[f"4:2:0 {siting}  8 bit -> fp32"] = (lambda i, y=y8, f=f8: near.yuv420_to_rgb(y[i % n], f, dst=f32[i % n], **geo), f8.frame_bytes + can, None)
        cfg[f"4:2:0 {siting} 10 bit kept -> fp32"] = (lambda i, y=y10, f=f10: near.yuv420p10_to_f32(y[i % n], f, f32[i % n], **geo),
                                                      f10.frame_bytes + can, None)
        cfg[f"4:2:0 {siting} fp32 ->  8 bit"] = (lambda i, o=o8, f=f8: near.rgb_to_yuv420(o[i % n], f, src=f32[i % n], **geo), f8.frame_bytes + src, None)
        cfg[f"4:2:0 {siting} fp32 -> 10 bit"] = (lambda i, o=o10, f=f10: near.f32_to_yuv420p10(o[i % n], f, f32[i % n], **geo), f10.frame_bytes + src, None)
    for sub in ("422", "444"):
        s = SITING[sub]
        f8, f10 = yuv.Format(H, W, siting=s, subsampling=sub), yuv.Format(H, W, siting=s, depth=10, subsampling=sub)
        y8, y10, o8, o10 = frames(f8), frames(f10), outputs(f8), outputs(f10)
        name = f"4:{sub[1]}:{sub[2]} {s}"
        cfg[f"{name}  8 bit -> fp32"] = (lambda i, y=y8, f=f8: ops.yuv_sub_decode(y[i % n], f, dst=f32[i % n], **geo), f8.frame_bytes + can,
                                         f"4:2:0 {s}  8 bit -> fp32")
        cfg[f"{name} 10 bit kept -> fp32"] = (lambda i, y=y10, f=f10: ops.yuv_sub_decode(y[i % n], f, dst=f32[i % n], keep_depth=True, **geo),
                                              f10.frame_bytes + can, f"4:2:0 {s} 10 bit kept -> fp32")
        cfg[f"{name} fp32 ->  8 bit"] = (lambda i, o=o8, f=f8: ops.yuv_sub_encode(o[i % n], f, src=f32[i % n], **geo), f8.frame_bytes + src,
                                         f"4:2:0 {s} fp32 ->  8 bit")
        cfg[f"{name} fp32 -> 10 bit"] = (lambda i, o=o10, f=f10: ops.yuv_sub_encode(o[i % n], f, src=f32[i % n], **geo), f10.frame_bytes + src,
                                         f"4:2:0 {s} fp32 -> 10 bit")
    return cfg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="the library under test (default: the package's)")
    ap.add_argument("--neighbour-lib", default=None, help="the build that runs the 4:2:0 neighbours (default: the library under test)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_sub: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops = yuv_timing.hip_ops.HipOps(dev, lib_path=a.lib)
    near = yuv_timing.hip_ops.HipOps(dev, lib_path=a.neighbour_lib) if a.neighbour_lib else ops
    n = max(1, a.buffers)
    rows, missed = [], []
    print(f"device {torch.cuda.get_device_name(0)}; {a.iters} calls after 24 warm-ups, {n} rotating buffers, median of {a.repeats} repeats; "
          f"neighbours run on {'the library under test' if near is ops else a.neighbour_lib}", flush=True)
    for H, W in SIZES:
        cfg = configs(ops, near, dev, H, W, n)
        times, _ = yuv_timing.rotation(cfg, None, a.repeats, a.iters)          # every repeat visits every configuration once
        med = {k: statistics.median(t) for k, t in times.items()}
        judged = (H, W) == SIZES[-1]
        print(f"--- {H} x {W}" + ("" if judged else "  (call-issue floor: no verdict)"), flush=True)
        for k, (_, nbytes, ref) in cfg.items():
            t = times[k]
            limit = nbytes / cfg[ref][1] * med[ref] * BOUND if ref else None
            verdict = None if (ref is None or not judged) else ("within" if med[k] <= limit else "MISSED")
            if verdict == "MISSED":
                missed.append(k)
            rows.append({"size": [H, W], "name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                         "GBps": nbytes / (med[k] * 1e-6) / 1e9, "share_of_hbm": nbytes / (med[k] * 1e-6) / HBM, "neighbour": ref,
                         "limit_us": limit, "verdict": verdict, "repeats_us": t})
            rel = f"  limit {limit:7.2f} us = {nbytes / cfg[ref][1]:5.3f} x {med[ref]:6.2f} us + 15 %" if ref else ""
            rel += f"  [{verdict}]" if verdict else ""
            print(f"{k:>32}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
                  f"{nbytes / (med[k] * 1e-6) / 1e9:7.1f} GB/s  {100 * nbytes / (med[k] * 1e-6) / HBM:5.1f}% of 6.3 TB/s{rel}", flush=True)
        del cfg
        torch.cuda.empty_cache()
    print("verdict at %d x %d: %s" % (SIZES[-1] + ("every 4:2:2 / 4:4:4 call within its byte-scaled 4:2:0 neighbour + 15 %" if not missed else
                                                   "MISSED by " + "; ".join(missed),)), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": n, "bound": BOUND, "rows": rows}, f,
                      indent=1)


if __name__ == "__main__":
    main()
