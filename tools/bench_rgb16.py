#!/usr/bin/env python3
"""Time the deep RGB calls (atm-vfi_amd/csrc/rgb16.hip: atmvfi_rgb16_decode -- fp32 only, and fp32 + probe -- and atmvfi_rgb16_encode) for
rgb48 and gbrp beside their yardsticks, the existing uint8 kernels ``atmvfi_frame_u8_to_f32`` and ``atmvfi_frame_f32_to_u8`` on frames
of the same size, on the protocol of tools/bench_yuv_packed.py: device events around ``--iters`` back-to-back calls after 24 warm-up
calls, the calls rotating over ``--buffers`` distinct sources and destinations (beyond the Infinity Cache), every configuration
timed ``--repeats`` times in rotation in one process (median, min - max); sizes 1080 x 1920 and 2160 x 4096, the canvas that of
``InputPadder(divisor=64)``.

At 2160 x 4096 a call is held to the project's rule for byte-bound kernels: no more than ``(its bytes / the yardstick's bytes) x the
yardstick's median + 15 %`` -- a decode against ``frame_u8_to_f32``, an encode against ``frame_f32_to_u8``.  At 1080p the calls sit at
the rate calls can be issued: reported, no verdict.  The yardsticks are pointwise.hip's kernels, by default from the library under
test (this change does not touch them); ``--yardstick-lib`` names another build to take them from.

``--loop``: the N-x loop instead -- network_base, 1080 x 1920, 4x, 12 frames -- on gbrp10le frames (``keep_depth``) beside the same
loop on uint8 frames of the same picture, interleaved in one process, ``--loop-repeats`` times: output frames per second, median and
min - max.

``--host-copies``: what one 1080p frame costs on its way through the host, 6.2 MB (uint8) against 12.4 MB (deep): the single-threaded
copy into a pinned slot, the host -> device copy, the device -> host copy and the copy out of the pinned ring, each alone and
synchronised, median of 40 after 5 warm-ups, in ms.

    python tools/bench_rgb16.py [--iters 240] [--repeats 5] [--buffers 12] [--json OUT] [--lib PATH] [--yardstick-lib PATH]
    python tools/bench_rgb16.py --loop [--loop-repeats 3] [--json OUT]
    python tools/bench_rgb16.py --host-copies"""
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
rgb16 = importlib.import_module("atm-vfi_amd.rgb16")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation)
HBM = 6.3e12
SIZES = [(1080, 1920), (2160, 4096)]
BOUND = 1.15
Y_DEC, Y_ENC = "frame_u8_to_f32 (yardstick)", "frame_f32_to_u8 (yardstick)"


def yardstick_calls(path):
    """the two uint8 kernels of the library at ``path`` alone (an older build lacks the newer symbols: it is not bound whole)"""
    lib = ctypes.CDLL(path)
    fns = []
    for name in ("atmvfi_frame_u8_to_f32", "atmvfi_frame_f32_to_u8"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = yuv_timing.hip_ops.SIGNATURES[name]
        fns.append(fn)
    lib.atmvfi_version.restype = ctypes.c_int
    return fns[0], fns[1], lib.atmvfi_version()


def configs(ops, yard_dec, yard_enc, dev, H, W, n):
    """name -> (call, bytes of the algorithm, the yardstick it is held to or None)"""
    pl, pr, pt, pb = host_io.InputPadder((1, 3, H, W), divisor=64)._pad
    Hp, Wp = H + pt + pb, W + pl + pr
    gen = torch.Generator(device=dev).manual_seed(H)
    f32 = [torch.rand(3, Hp, Wp, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
    u8 = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run_y_dec(i):
        if yard_dec(u8[i % n].data_ptr(), H, W, 0, f32[i % n].data_ptr(), Hp, Wp, pt, pl, stream()):
            raise RuntimeError("the decode yardstick failed")

    def run_y_enc(i):
        if yard_enc(f32[i % n].data_ptr(), Hp, Wp, pt, pl, u8[i % n].data_ptr(), H, W, 0, stream()):
            raise RuntimeError("the encode yardstick failed")
    cfg = {Y_DEC: (run_y_dec, 3.0 * H * W + 12.0 * Hp * Wp, None), Y_ENC: (run_y_enc, 12.0 * H * W + 3.0 * H * W, None)}
    for layout in ("rgb48", "gbrp"):
        fmt = yuv.DeepRGB(H, W, 16, layout)
        frames = [torch.randint(0, 256, (fmt.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        cfg[f"decode {layout}"] = (lambda i, f=frames, k=fmt: ops.rgb16_decode(f[i % n], k, dst=f32[i % n], pad_top=pt, pad_left=pl),
                                   6.0 * H * W + 12.0 * Hp * Wp, Y_DEC)
        cfg[f"decode {layout} + probe"] = (lambda i, f=frames, k=fmt: ops.rgb16_decode(f[i % n], k, dst=f32[i % n], dst_u8=u8[i % n], pad_top=pt,
                                                                                       pad_left=pl), 9.0 * H * W + 12.0 * Hp * Wp, Y_DEC)
        cfg[f"encode {layout}"] = (lambda i, f=frames, k=fmt: ops.rgb16_encode(f[i % n], k, f32[i % n], pad_top=pt, pad_left=pl),
                                   18.0 * H * W, Y_ENC)
    return cfg


def kernels(a, dev):
    ops = yuv_timing.hip_ops.HipOps(dev, lib_path=a.lib)
    ypath = a.yardstick_lib or a.lib or yuv_timing.hip_ops.LIB_PATH
    yard_dec, yard_enc, version = yardstick_calls(ypath)
    n = max(1, a.buffers)
    rows, missed = [], []
    print(f"device {torch.cuda.get_device_name(0)}; {a.iters} calls after 24 warm-ups, {n} rotating buffers, median of {a.repeats} repeats; "
          f"yardsticks from {'the library under test' if not a.yardstick_lib else a.yardstick_lib} (ABI 0.{(version >> 8) & 255}), the calls from "
          f"ABI 0.{(ops.lib.atmvfi_version() >> 8) & 255}; depth 16, canvas of InputPadder(divisor=64)", flush=True)
    for H, W in SIZES:
        cfg = configs(ops, yard_dec, yard_enc, dev, H, W, n)
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
                         "verdict": verdict, "repeats_us": t})
            rel = f"  limit {limit:7.2f} us = {nbytes / cfg[yard][1]:5.3f} x {med[yard]:6.2f} us + 15 %" if yard else ""
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
    fmt = yuv.DeepRGB(H, W, 10, "gbrp")
    rgb8 = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(frames)]
    deep = [rgb16._layout_of(f.astype(np.uint16) * 4 + rng.integers(0, 4, f.shape).astype(np.uint16), fmt) for f in rgb8]
    streams = {"uint8 rgb": (dict(isBGR=False), rgb8), "gbrp10le": (dict(pixfmt=fmt, keep_depth=True), deep)}
    print(f"device {torch.cuda.get_device_name(0)}; network_base {H} x {W}, {factor}x, {frames} frames, {a.loop_repeats} repeats "
          "interleaved in one process; output frames per second", flush=True)
    fps = {name: [] for name in streams}
    for rep in range(a.loop_repeats + 1):            # (the first pass warms every stream up: not counted)
        for name, (kw, video) in streams.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count = sum(1 for _ in host_io.interpolate_video_nx(iter(video), net, factor=factor, **kw))
            torch.cuda.synchronize()
            if rep:
                fps[name].append(count / (time.perf_counter() - t0))
    rows = []
    for name, v in fps.items():
        rows.append({"stream": name, "fps_median": statistics.median(v), "fps_min": min(v), "fps_max": max(v), "repeats_fps": v})
        print(f"{name:>12}: {statistics.median(v):7.2f} frames/s (min {min(v):.2f}, max {max(v):.2f} over {len(v)} repeats)", flush=True)
    p, q = fps["gbrp10le"], fps["uint8 rgb"]
    inside = min(q) <= statistics.median(p) <= max(q) or statistics.median(p) >= statistics.median(q)
    print(f"gbrp10le / uint8 rgb: {statistics.median(p) / statistics.median(q):.4f} x "
          f"({'within' if inside else 'outside'} the uint8 repeats' spread {min(q):.2f} - {max(q):.2f})", flush=True)
    return {"loop": {"size": [H, W], "factor": factor, "frames": frames, "repeats": a.loop_repeats, "rows": rows}}


def host_copies(a, dev):
    print(f"device {torch.cuda.get_device_name(0)}; one 1080 x 1920 frame, each step alone and synchronised, median of 40 after 5 warm-ups; ms", flush=True)
    rows = []
    for name, n in (("uint8 rgb, 6.2 MB", 1080 * 1920 * 3), ("deep rgb, 12.4 MB", 1080 * 1920 * 6)):
        src = np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8)
        pin, out_pin = torch.empty(n, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.uint8).pin_memory()
        pin_np, d = pin.numpy(), torch.empty(n, dtype=torch.uint8, device=dev)
        steps = {"copy into pinned": lambda: np.copyto(pin_np, src), "host -> device": lambda: d.copy_(pin, non_blocking=True),
                 "device -> host": lambda: out_pin.copy_(d, non_blocking=True), "copy out of pinned": lambda: out_pin.numpy().copy()}
        res = {}
        for label, fn in steps.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            v = []
            for _ in range(40):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                v.append((time.perf_counter() - t0) * 1e3)
            res[label] = statistics.median(v)
        rows.append({"frame": name, **res})
        print(f"{name:>18}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()), flush=True)
    return {"host_copies": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="the library under test (default: the package's)")
    ap.add_argument("--yardstick-lib", default=None, help="another build of the library to take the two uint8 yardsticks from")
    ap.add_argument("--loop", action="store_true", help="time the N-x loop on gbrp10le against uint8 frames instead of the kernels")
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--host-copies", action="store_true", help="time the host-side copies of one 1080p frame, uint8 against deep")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rgb16: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    out = host_copies(a, dev) if a.host_copies else loop(a, dev) if a.loop else kernels(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), **out}, f, indent=1)


if __name__ == "__main__":
    main()
