#!/usr/bin/env python3
"""Time the two kernels of interlaced input (atm-vfi_amd/csrc/fields.hip: atmvfi_field_bob with both outputs, atmvfi_field_rows on a uint8
RGB frame and on a 4:2:2 10-bit frame) beside two yardsticks, ``atmvfi_frame_rot180`` and ``atmvfi_frame_f32_to_u8``, on the protocol
of tools/bench_active.py: device events around ``--iters`` back-to-back calls after 24 warm-up calls, the calls rotating over
``--buffers`` distinct sources and destinations (beyond the Infinity Cache), every configuration timed ``--repeats`` times in rotation in
one process (median, min - max); sizes 1080 x 1920 (canvas 1088 x 1920) and 2160 x 4096 (canvas 2176 x 4096).

The yardsticks never run from the code under test: ``--yardstick-lib`` names another build of the library, the parent commit's (built
from a worktree of the parent), loaded beside the library under test and timed in the same rotation, as tools/bench_yuv_packed.py
does.  At 2176 x 4096 a call is held to the project's rule for byte-bound kernels: no more than ``(its bytes / the yardstick's bytes) x
the yardstick's median + 15 %`` -- ``field_bob`` against ``frame_rot180`` (fp32 canvases on both sides), ``field_rows`` against
``frame_f32_to_u8`` (a byte frame on one side).  A call's bytes are what the algorithm needs: ``field_bob`` reads the picture once and
writes two canvases; ``field_rows`` reads and writes half the rows.  At 1080p the calls sit at the rate calls can be issued: reported,
no verdict.  A missed bound is reported as missed.

``--loop``: ``deinterlace_video`` instead -- network_base, 1080 x 1920 interlaced uint8, ``mode="mc"`` and ``"bob"`` -- beside
``interpolate_video_nx(factor=2, pool=True)`` on the same frames, interleaved in one process ``--loop-repeats`` times: output frames per
second (of the yardstick: interpolated frames per second too) and the time to the first output.

    python tools/bench_fields.py --yardstick-lib PATH [--iters 240] [--repeats 5] [--buffers 12] [--json OUT] [--lib PATH]
    python tools/bench_fields.py --loop [--loop-repeats 3] [--frames 12] [--json OUT]"""
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
fields = importlib.import_module("atm-vfi_amd.fields")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation)
HBM = 6.3e12
SIZES = [(1080, 1920), (2160, 4096)]
BOUND = 1.15
ROT, U8 = "frame_rot180 (yardstick)", "frame_f32_to_u8 (yardstick)"


def yardstick_calls(path):
    """The two yardstick entry points of the library at ``path`` alone (an older build lacks the newer symbols: it is not bound whole)"""
    lib = ctypes.CDLL(path)
    fns = []
    for name in ("atmvfi_frame_rot180", "atmvfi_frame_f32_to_u8"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = yuv_timing.hip_ops.SIGNATURES[name]
        fns.append(fn)
    lib.atmvfi_version.restype = ctypes.c_int
    return fns[0], fns[1], lib.atmvfi_version()


def configs(ops, rot, to_u8, dev, H, W, n):
    """name -> (call, bytes of the algorithm, the yardstick it is judged against or None)"""
    pl, pr, pt, pb = host_io.InputPadder((1, 3, H, W), divisor=64)._pad
    Hp, Wp = H + pt + pb, W + pl + pr
    gen = torch.Generator(device=dev).manual_seed(H)
    f32 = [torch.rand(3, Hp, Wp, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
    even = [torch.empty(3, Hp, Wp, dtype=torch.float32, device=dev) for _ in range(n)]
    odd = [torch.empty(3, Hp, Wp, dtype=torch.float32, device=dev) for _ in range(n)]
    u8 = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(2 * n)]
    fmt = yuv.Format(H, W, depth=10, subsampling="422", siting="left")
    deep = [torch.randint(0, 256, (fmt.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(2 * n)]
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def check(rc):
        if rc:
            raise RuntimeError(f"a yardstick failed ({rc})")
    g_rgb, g_deep = fields.plane_geometry(None, None, H, W), fields.plane_geometry(fmt, fmt)
    canvas = 12.0 * Hp * Wp
    return {
        ROT: (lambda i: check(rot(f32[i % n].data_ptr(), even[i % n].data_ptr(), 3, Hp, Wp, stream())), 2 * canvas, None),
        U8: (lambda i: check(to_u8(f32[i % n].data_ptr(), Hp, Wp, pt, pl, u8[i % n].data_ptr(), H, W, 0, stream())), 12.0 * H * W + 3.0 * H * W, None),
        "field_bob (both outputs)": (lambda i: ops.field_bob(f32[i % n], even[i % n], odd[i % n], pt, pl, H, W), 12.0 * H * W + 2 * canvas, ROT),
        "field_rows rgb uint8": (lambda i: ops.field_rows(u8[i % n].view(-1), u8[n + i % n].view(-1), g_rgb, i & 1), 3.0 * H * W, U8),
        "field_rows 4:2:2 10 bit": (lambda i: ops.field_rows(deep[i % n], deep[n + i % n], g_deep, i & 1), float(fmt.frame_bytes), U8),
    }


def kernels(a, dev):
    if not a.yardstick_lib:
        sys.exit("bench_fields: --yardstick-lib PATH is required (the parent commit's build: the yardsticks never run from the code under test)")
    ops = yuv_timing.hip_ops.HipOps(dev, lib_path=a.lib)
    rot, to_u8, version = yardstick_calls(a.yardstick_lib)
    n = max(1, a.buffers)
    rows, missed = [], []
    print(f"device {torch.cuda.get_device_name(0)}; {a.iters} calls after 24 warm-ups, {n} rotating buffers, median of {a.repeats} repeats; "
          f"yardsticks from {a.yardstick_lib} (ABI 0.{(version >> 8) & 255}), the calls from ABI 0.{(ops.lib.atmvfi_version() >> 8) & 255}", flush=True)
    for H, W in SIZES:
        cfg = configs(ops, rot, to_u8, dev, H, W, n)
        times, _ = yuv_timing.rotation(cfg, None, a.repeats, a.iters)
        med = {k: statistics.median(t) for k, t in times.items()}
        judged = (H, W) == SIZES[-1]
        print(f"--- {H} x {W}" + ("" if judged else "  (call-issue floor: no verdict)"), flush=True)
        for k, (_, nbytes, yard) in cfg.items():
            t = times[k]
            limit = nbytes / cfg[yard][1] * med[yard] * BOUND if yard else None
            verdict = None
            if yard and judged:
                verdict = "met" if med[k] <= limit else f"missed by {100 * (med[k] / limit - 1):.1f} %"
                if med[k] > limit:
                    missed.append(k)
            rows.append({"size": [H, W], "name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                         "GBps": nbytes / (med[k] * 1e-6) / 1e9, "share_of_hbm": nbytes / (med[k] * 1e-6) / HBM, "limit_us": limit,
                         "yardstick": yard, "verdict": verdict, "repeats_us": t})
            rel = f"  limit {limit:7.2f} us = {nbytes / cfg[yard][1]:5.3f} x {med[yard]:6.2f} us ({yard.split()[0]}) + 15 %" if yard else ""
            rel += f"  [{verdict}]" if verdict else ""
            print(f"{k:>28}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
                  f"{nbytes / (med[k] * 1e-6) / 1e9:7.1f} GB/s  {100 * nbytes / (med[k] * 1e-6) / HBM:5.1f}% of 6.3 TB/s{rel}", flush=True)
        del cfg
        torch.cuda.empty_cache()
    print("verdict at %d x %d: %s" % (SIZES[-1] + ("every call within its byte-scaled yardstick + 15 %" if not missed else
                                                   "MISSED by " + "; ".join(missed),)), flush=True)
    return {"iters": a.iters, "repeats": a.repeats, "buffers": n, "bound": BOUND, "rows": rows}


def loop(a, dev):
    H, W, frames = 1080, 1920, a.frames
    net = pkg.Network()
    net.load_state_dict(pkg.synthetic_state_dict("base", seed=1), strict=True)
    net = net.to(dev).eval()
    rng = np.random.default_rng(1)
    video = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(frames)]
    runs = {
        "deinterlace mc": (lambda: host_io.deinterlace_video(iter(video), net, mode="mc"), 2 * frames),
        "deinterlace bob": (lambda: host_io.deinterlace_video(iter(video), net, mode="bob"), 2 * frames),
        "interpolate_video_nx 2x (yardstick)": (lambda: host_io.interpolate_video_nx(iter(video), net, factor=2, pool=True), 2 * frames - 1),
    }
    print(f"device {torch.cuda.get_device_name(0)}; network_base {H} x {W} interlaced uint8, {frames} woven frames, {a.loop_repeats} repeats "
          "interleaved in one process; output frames per second and seconds to the first output", flush=True)
    fps, first = {k: [] for k in runs}, {k: [] for k in runs}
    for rep in range(a.loop_repeats + 1):            # (the first pass warms every loop up: not counted)
        for name, (run, expect) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count, t_first = 0, None
            for _ in run():
                if t_first is None:
                    t_first = time.perf_counter() - t0
                count += 1
            torch.cuda.synchronize()
            if count != expect:
                raise RuntimeError(f"{name}: {count} frames, {expect} expected")
            if rep:
                fps[name].append(count / (time.perf_counter() - t0))
                first[name].append(t_first)
    rows = []
    for name, v in fps.items():
        row = {"loop": name, "fps_median": statistics.median(v), "fps_min": min(v), "fps_max": max(v), "repeats_fps": v,
               "first_output_s_median": statistics.median(first[name]), "repeats_first_output_s": first[name]}
        extra = ""
        if "yardstick" in name:                       # of its 2n - 1 outputs n - 1 are interpolated: one forward and one encode each
            row["interpolated_fps_median"] = row["fps_median"] * (frames - 1) / (2 * frames - 1)
            extra = f"  = {row['interpolated_fps_median']:.2f} interpolated frames/s"
        rows.append(row)
        print(f"{name:>38}: {row['fps_median']:7.2f} frames/s (min {min(v):.2f}, max {max(v):.2f} over {len(v)} repeats){extra}  first output after "
              f"{row['first_output_s_median'] * 1e3:.1f} ms", flush=True)
    return {"loop": {"size": [H, W], "frames": frames, "repeats": a.loop_repeats, "rows": rows}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="the library under test (default: the package's)")
    ap.add_argument("--yardstick-lib", default=None, help="the parent commit's build of the library: runs the yardsticks")
    ap.add_argument("--loop", action="store_true", help="time deinterlace_video beside interpolate_video_nx(factor=2) instead of the kernels")
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=12, help="with --loop: woven frames per run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fields: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    out = loop(a, dev) if a.loop else kernels(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **out}, f, indent=1)


if __name__ == "__main__":
    main()
