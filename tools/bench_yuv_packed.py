#!/usr/bin/env python3
"""Time the packed 4:2:2 moves (atm-vfi_amd/csrc/yuv_packed.hip: atmvfi_yuv_unpack / atmvfi_yuv_pack) for uyvy and v210 beside a yardstick,
``atmvfi_frame_f32_to_u8`` of the same geometry, on the protocol of tools/bench_yuv_sub.py: device events around ``--iters``
back-to-back calls after 24 warm-up calls, the calls rotating over ``--buffers`` distinct sources and destinations (beyond the Infinity
Cache), every configuration timed ``--repeats`` times in rotation in one process (median, min - max); sizes 1080 x 1920 and 2160 x
4096.

The yardstick never runs from the code under test: ``--yardstick-lib`` names another build of the library, the parent commit's (built
from a worktree of the parent), loaded beside the library under test and timed in the same rotation.  At 2160 x 4096 a call is held to
the project's rule for byte-bound kernels: no more than ``(its bytes / the yardstick's bytes) x the yardstick's median + 15 %``; its
bytes are the packed rows' own bytes plus the planar frame.  At 1080p the calls sit at the rate calls can be issued: reported, no
verdict.

``--loop``: the N-x loop instead -- network_base, 1080 x 1920, 4x, 12 frames, ``keep_depth`` -- on uyvy against planar yuv422p and on
v210 against yuv422p10le, interleaved in one process, ``--loop-repeats`` times: output frames per second, median and min - max.

    python tools/bench_yuv_packed.py --yardstick-lib PATH [--iters 240] [--repeats 5] [--buffers 12] [--json OUT] [--lib PATH]
    python tools/bench_yuv_packed.py --loop [--loop-repeats 3] [--json OUT]"""
import argparse
import ctypes
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
pkg = importlib.import_module("atm-vfi_amd")
host_io = importlib.import_module("atm-vfi_amd.host_io")
yuv = importlib.import_module("atm-vfi_amd.yuv")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation)
HBM = 6.3e12
SIZES = [(1080, 1920), (2160, 4096)]
BOUND = 1.15
YARDSTICK = "frame_f32_to_u8 (yardstick)"


def yardstick_call(path):
    """``atmvfi_frame_f32_to_u8`` of the library at ``path`` alone (an older build lacks the newer symbols: it is not bound whole)"""
    lib = ctypes.CDLL(path)
    fn = lib.atmvfi_frame_f32_to_u8
    fn.restype, fn.argtypes = yuv_timing.hip_ops.SIGNATURES["atmvfi_frame_f32_to_u8"]
    lib.atmvfi_version.restype = ctypes.c_int
    return fn, lib.atmvfi_version()


def configs(ops, yard, dev, H, W, n):
    """name -> (call, bytes of the algorithm, judged against the yardstick?)"""
    pad = host_io.InputPadder((1, 3, H, W), divisor=64)
    pl, pr, pt, pb = pad._pad
    Hp, Wp = H + pt + pb, W + pl + pr
    gen = torch.Generator(device=dev).manual_seed(H)
    f32 = [torch.rand(3, Hp, Wp, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
    u8 = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run_yardstick(i):
        rc = yard(f32[i % n].data_ptr(), Hp, Wp, pt, pl, u8[i % n].data_ptr(), H, W, 0, stream())
        if rc:
            raise RuntimeError(f"the yardstick failed ({rc})")
    cfg = {YARDSTICK: (run_yardstick, 12.0 * H * W + 3.0 * H * W, False)}
    for layout, depth in (("uyvy", 8), ("v210", 10)):
        k = yuv.Packed(yuv.Format(H, W, depth=depth, subsampling="422", siting="left"), layout)
        frames = [torch.randint(0, 256, (k.nbytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        planes = [torch.randint(0, 4, (k.planar.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        nbytes = float(k.row_bytes * H + k.planar.frame_bytes)
        cfg[f"unpack {layout}"] = (lambda i, f=frames, p=planes, k=k: ops.yuv_unpack(f[i % n], k, dst=p[i % n]), nbytes, True)
        cfg[f"pack   {layout}"] = (lambda i, f=frames, p=planes, k=k: ops.yuv_pack(p[i % n], k, dst=f[i % n]), nbytes, True)
    return cfg


def kernels(a, dev):
    if not a.yardstick_lib:
        sys.exit("bench_yuv_packed: --yardstick-lib PATH is required (the parent commit's build: the yardstick never runs from the code under test)")
    ops = yuv_timing.hip_ops.HipOps(dev, lib_path=a.lib)
    yard, version = yardstick_call(a.yardstick_lib)
    n = max(1, a.buffers)
    rows, missed = [], []
    print(f"device {torch.cuda.get_device_name(0)}; {a.iters} calls after 24 warm-ups, {n} rotating buffers, median of {a.repeats} repeats; "
          f"yardstick from {a.yardstick_lib} (ABI 0.{(version >> 8) & 255}), the calls from ABI 0.{(ops.lib.atmvfi_version() >> 8) & 255}", flush=True)
    for H, W in SIZES:
        cfg = configs(ops, yard, dev, H, W, n)
        times, _ = yuv_timing.rotation(cfg, None, a.repeats, a.iters)
        med = {k: statistics.median(t) for k, t in times.items()}
        judged = (H, W) == SIZES[-1]
        print(f"--- {H} x {W}" + ("" if judged else "  (call-issue floor: no verdict)"), flush=True)
        for k, (_, nbytes, held) in cfg.items():
            t = times[k]
            limit = nbytes / cfg[YARDSTICK][1] * med[YARDSTICK] * BOUND if held else None
            verdict = None
            if held and judged:
                verdict = "met" if med[k] <= limit else f"missed by {100 * (med[k] / limit - 1):.1f} %"
                if med[k] > limit:
                    missed.append(k)
            rows.append({"size": [H, W], "name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                         "GBps": nbytes / (med[k] * 1e-6) / 1e9, "share_of_hbm": nbytes / (med[k] * 1e-6) / HBM, "limit_us": limit,
                         "verdict": verdict, "repeats_us": t})
            rel = f"  limit {limit:7.2f} us = {nbytes / cfg[YARDSTICK][1]:5.3f} x {med[YARDSTICK]:6.2f} us + 15 %" if held else ""
            rel += f"  [{verdict}]" if verdict else ""
            print(f"{k:>28}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
                  f"{nbytes / (med[k] * 1e-6) / 1e9:7.1f} GB/s  {100 * nbytes / (med[k] * 1e-6) / HBM:5.1f}% of 6.3 TB/s{rel}", flush=True)
        del cfg
        torch.cuda.empty_cache()
    print("verdict at %d x %d: %s" % (SIZES[-1] + ("every call within its byte-scaled yardstick + 15 %" if not missed else
                                                   "MISSED by " + "; ".join(missed),)), flush=True)
    return {"iters": a.iters, "repeats": a.repeats, "buffers": n, "bound": BOUND, "rows": rows}


def loop(a, dev):
    H, W, frames, factor = 1080, 1920, 12, 4
    net = pkg.Network()
    net.load_state_dict(pkg.synthetic_state_dict("base", seed=1), strict=True)
    net = net.to(dev).eval()
    rng = np.random.default_rng(1)
    streams = {}
    for layout, depth, planar_name in (("uyvy", 8, "yuv422p"), ("v210", 10, "yuv422p10le")):
        k = yuv.Packed(yuv.Format(H, W, depth=depth, subsampling="422", siting="left"), layout)
        lo, hi = (16, 236) if depth == 8 else (64, 941)
        Q = [rng.integers(lo, hi, k.planar.frame_samples).astype(k.planar.dtype) for _ in range(frames)]
        streams[planar_name] = (k.planar, Q)
        streams[layout] = (k, [yuv.pack_numpy(q, k) for q in Q])
    print(f"device {torch.cuda.get_device_name(0)}; network_base {H} x {W}, {factor}x, {frames} frames, keep_depth, {a.loop_repeats} repeats "
          "interleaved in one process; output frames per second", flush=True)
    fps = {name: [] for name in streams}
    for rep in range(a.loop_repeats + 1):            # (the first pass warms every stream up: not counted)
        for name, (fmt, video) in streams.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count = sum(1 for _ in host_io.interpolate_video_nx(iter(video), net, factor=factor, pixfmt=fmt, keep_depth=True))
            torch.cuda.synchronize()
            if rep:
                fps[name].append(count / (time.perf_counter() - t0))
    rows = []
    for name, v in fps.items():
        rows.append({"stream": name, "fps_median": statistics.median(v), "fps_min": min(v), "fps_max": max(v), "repeats_fps": v})
        print(f"{name:>12}: {statistics.median(v):7.2f} frames/s (min {min(v):.2f}, max {max(v):.2f} over {len(v)} repeats)", flush=True)
    for packed, planar in (("uyvy", "yuv422p"), ("v210", "yuv422p10le")):
        p, q = fps[packed], fps[planar]
        inside = min(q) <= statistics.median(p) <= max(q) or statistics.median(p) >= statistics.median(q)
        print(f"{packed} / {planar}: {statistics.median(p) / statistics.median(q):.4f} x "
              f"({'within' if inside else 'outside'} the planar repeats' spread {min(q):.2f} - {max(q):.2f})", flush=True)
    return {"loop": {"size": [H, W], "factor": factor, "frames": frames, "repeats": a.loop_repeats, "rows": rows}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="the library under test (default: the package's)")
    ap.add_argument("--yardstick-lib", default=None, help="the parent commit's build of the library: runs the yardstick")
    ap.add_argument("--loop", action="store_true", help="time the N-x loop on packed against planar streams instead of the kernels")
    ap.add_argument("--loop-repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_packed: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    out = loop(a, dev) if a.loop else kernels(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **out}, f, indent=1)


if __name__ == "__main__":
    main()
