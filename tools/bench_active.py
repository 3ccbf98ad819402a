#!/usr/bin/env python3
"""Time the active-picture kernels (atm-vfi_amd/csrc/active.hip) with the protocol of tools/bench_shutter.py: device events around
back-to-back calls after a warm-up, buffers in rotation so that every source comes from HBM (each rotation exceeds the 256 MB Infinity
Cache), every configuration timed ``--repeats`` times in rotation, median with min - max.  Sizes 1080 x 1920 and 2160 x 4096.

``frame_borders`` against ``frame_signature`` on the same frames: both read the frame once (3 bytes per pixel; the partials of either
are small against it).  ``frame_compose`` -- a letterbox window of 804 / 1080 of the rows, from an fp32 canvas padded to a multiple of
64 and from a uint8 window -- against ``frame_f32_to_u8`` of a whole frame of the same size (15 bytes per pixel).  Bytes of compose:
3 H W written, 3 (H W - h w) of bars and 12 h w (fp32) or 3 h w (uint8) of window read.  What the kernels are held to, at 2160 x 4096
(at 1080p the calls sit at the rate they can be issued): a call takes no longer than (its bytes / the yardstick's bytes) x the
yardstick's time + 15 %.  The verdict is printed per call; it is a report, not an exit code.

``--loop``: instead, ``interpolate_video_nx`` 4x on a letterboxed video (bars of 138 / 1080 of the rows) with ``active=None`` and with
``active=ActiveArea()`` in one process, interleaved: output frames per second of the steady state (from the first output to the
last), and the time to the first output, which holds the probing.

``--yuv``: the same protocol for the YUV calls.  ``yuv_borders`` on an NV12 and on a P010 surface beside ``frame_borders`` on an RGB
frame of the same size, in the same rotation: it reads a third (two thirds) of the bytes, but ``frame_borders`` already sits near the
rate at which two launches can be issued, so it is held to ``frame_borders``' time + 15 %, not to a byte ratio.  ``yuv_compose`` --
the same letterbox window from the fp32 canvas, into an NV12 and into a planar 10-bit frame -- beside ``yuv_encode`` of a whole frame of
that format from fp32 (12 bytes per pixel read, the frame written), held to (its bytes / the yardstick's bytes) x the yardstick's time
+ 15 %; bytes of compose: the frame written, the bars' samples and 12 h w of window read.  ``--loop --pix-fmt nv12``: the loop on NV12
frames of the same video.

    python tools/bench_active.py [--yuv] [--iters 240] [--repeats 5] [--json OUT]
    python tools/bench_active.py --loop [--pix-fmt nv12] [--model base|lite] [--size 1080x1920] [--frames 12] [--repeats 3]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):          # (tests/: cpu_active.letterboxed, cpu_yuv_active.letterboxed_yuv for --loop)
    if _p not in sys.path:
        sys.path.insert(0, _p)
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
HBM = 6.3e12
SIZES = ((1080, 1920), (2160, 4096))
MARGIN = 1.15


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


def letterbox(h, w):
    """(y0, x0, hw, ww), (Hp, pad_top): a 2.39:1 picture in the frame (bars of 138 / 1080 of the rows, even) padded to 64"""
    bar = (138 * h // 1080) & ~1
    hw = h - 2 * bar
    hp = -(-hw // 64) * 64
    return (bar, 0, hw, w), (hp, (hp - hw) // 2)


def kernels(a):
    dev = torch.device("cuda:0")
    ops = hip_ops.HipOps(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for h, w in SIZES:
        px = h * w
        win, (hp, pad_top) = letterbox(h, w)
        wpx = win[2] * win[3]
        n = max(3, -(-320_000_000 // (12 * px)) + 1)         # fp32 rotations beyond the Infinity Cache
        nb = max(3, -(-320_000_000 // (3 * px)) + 1)         # the same for the uint8 frames
        f32 = [torch.rand(3, h, w, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
        canvas = [t.view(-1)[:3 * hp * w].view(3, hp, w) for t in f32]          # the window's padded canvas, in the same rotation
        u8 = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nb)]
        wu8 = [t.view(-1)[:3 * wpx].view(win[2], win[3], 3) for t in u8]
        out = [torch.empty(h, w, 3, dtype=torch.uint8, device=dev) for _ in range(nb)]
        sig, bor = torch.empty(288, dtype=torch.int32, device=dev), torch.empty(h + w, dtype=torch.int32, device=dev)
        sig_ws, bor_ws = ops.frame_signature_workspace(h, w), ops.frame_borders_workspace(h, w)
        cfg = {      # name -> (call, bytes of the algorithm, the yardstick it is held to)
            "frame_signature (yardstick)": (lambda i: ops.frame_signature(u8[i % nb], out=sig, workspace=sig_ws), 3.0 * px, None),
            "frame_borders": (lambda i: ops.frame_borders(u8[i % nb], out=bor, workspace=bor_ws), 3.0 * px, "frame_signature (yardstick)"),
            "frame_f32_to_u8 (yardstick)": (lambda i: ops.frame_f32_to_u8(f32[i % n], out[i % nb], 0, 0, False), 15.0 * px, None),
            "frame_compose fp32 window": (lambda i: ops.frame_compose(out[i % nb], u8[(i + 1) % nb], win, src=canvas[i % n], pad_top=pad_top),
                                          3.0 * px + 3.0 * (px - wpx) + 12.0 * wpx, "frame_f32_to_u8 (yardstick)"),
            "frame_compose uint8 window": (lambda i: ops.frame_compose(out[i % nb], u8[(i + 1) % nb], win, win_u8=wu8[(i + 2) % nb]),
                                           3.0 * px + 3.0 * (px - wpx) + 3.0 * wpx, "frame_f32_to_u8 (yardstick)"),
        }
        print(f"--- {h} x {w}, window {win[2]} x {win[3]} at row {win[0]} (canvas {hp} x {w}): rotations of {n} fp32 and {nb} uint8 buffers, "
              f"{a.iters} calls x {a.repeats} repeats", flush=True)
        rows += measure(a, cfg, h, w)
        del f32, canvas, u8, wu8, out
        torch.cuda.empty_cache()
    dump(a, rows)


def measure(a, cfg, h, w):
    """Time every configuration of ``cfg`` -- name -> (call, bytes of the algorithm, the yardstick it is held to or None, time-only: the
    bound is the yardstick's time + 15 % whatever the bytes) -- ``a.repeats`` times in rotation and print median, min - max and verdict."""
    times = {k: [] for k in cfg}
    for _ in range(a.repeats):               # in rotation: every repeat visits every configuration once
        for k, c in cfg.items():
            times[k].append(timed(c[0], a.iters))
    rows = []
    for k, c in cfg.items():
        nbytes, yard, by_time = c[1], c[2], len(c) > 3 and c[3]
        t = times[k]
        med = statistics.median(t)
        bound = None if yard is None else (1.0 if by_time else nbytes / cfg[yard][1]) * statistics.median(times[yard]) * MARGIN
        held = (h, w) == SIZES[-1]
        verdict = "" if bound is None else f"  bound {bound:7.2f} us: {('met' if med <= bound else 'MISSED') if held else 'not held at this size'}"
        rows.append({"size": [h, w], "name": k, "us_median": med, "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                     "GBps": nbytes / (med * 1e-6) / 1e9, "bound_us": bound, "repeats_us": t})
        print(f"{k:>30}: {med:8.2f} us (min {min(t):.2f}, max {max(t):.2f})  {nbytes / 1e6:6.1f} MB  {nbytes / (med * 1e-6) / 1e9:7.1f} GB/s  "
              f"{100 * nbytes / (med * 1e-6) / HBM:5.1f}% of 6.3 TB/s{verdict}", flush=True)
    return rows


def dump(a, rows):
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "rows": rows}, f, indent=1)


def kernels_yuv(a):
    yuv = importlib.import_module("atm-vfi_amd.yuv")
    dev = torch.device("cuda:0")
    ops = hip_ops.HipOps(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for h, w in SIZES:
        px = h * w
        win, (hp, pad_top) = letterbox(h, w)
        wpx = win[2] * win[3]
        nv12, p010, p10 = yuv.Surface.nv12(h, w), yuv.Surface.p010(h, w), yuv.Format(h, w, depth=10)
        rot = lambda nbytes: max(3, -(-320_000_000 // nbytes) + 1)           # rotations whose READ bytes exceed the Infinity Cache
        n, nb, n8, n16 = rot(12 * px), rot(3 * px), rot(px), rot(2 * px)         # (of a surface only the luma plane / the bars are read)
        f32 = [torch.rand(3, h, w, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
        canvas = [t.view(-1)[:3 * hp * w].view(3, hp, w) for t in f32]
        u8 = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nb)]
        s8 = [torch.randint(0, 256, (nv12.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n8)]
        s16 = [torch.randint(0, 256, (p010.frame_bytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n16)]
        o8 = [torch.empty(nv12.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(n8)]
        o16 = [torch.empty(p10.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(n16)]
        bor = torch.empty(h + w, dtype=torch.int32, device=dev)
        bor_ws, ybor_ws = ops.frame_borders_workspace(h, w), ops.yuv_borders_workspace(h, w)
        bars = 1.5 * (px - wpx)
        cfg = {
            "frame_borders (yardstick)": (lambda i: ops.frame_borders(u8[i % nb], out=bor, workspace=bor_ws), 3.0 * px, None),
            "yuv_borders nv12": (lambda i: ops.yuv_borders(s8[i % n8], nv12, out=bor, workspace=ybor_ws), 1.0 * px, "frame_borders (yardstick)", True),
            "yuv_borders p010": (lambda i: ops.yuv_borders(s16[i % n16], p010, out=bor, workspace=ybor_ws), 2.0 * px, "frame_borders (yardstick)", True),
            "yuv_encode nv12 (yardstick)": (lambda i: ops.yuv_encode(o8[i % n8], nv12, src=f32[i % n]), 13.5 * px, None),
            "yuv_compose nv12": (lambda i: ops.yuv_compose(o8[i % n8], nv12, s8[(i + 1) % n8], nv12, win, src=canvas[i % n], pad_top=pad_top),
                                 1.5 * px + bars + 12.0 * wpx, "yuv_encode nv12 (yardstick)"),
            "yuv_encode p10 (yardstick)": (lambda i: ops.yuv_encode(o16[i % n16], p10, src=f32[i % n]), 15.0 * px, None),
            "yuv_compose planar 10 bit": (lambda i: ops.yuv_compose(o16[i % n16], p10, s16[(i + 1) % n16], p10, win, src=canvas[i % n], pad_top=pad_top),
                                          3.0 * px + 2 * bars + 12.0 * wpx, "yuv_encode p10 (yardstick)"),
        }
        print(f"--- {h} x {w}, window {win[2]} x {win[3]} at row {win[0]} (canvas {hp} x {w}): rotations of {n} fp32, {nb} RGB, {n8} 8-bit and "
              f"{n16} 10-bit buffers, {a.iters} calls x {a.repeats} repeats", flush=True)
        rows += measure(a, cfg, h, w)
        del f32, canvas, u8, s8, s16, o8, o16
        torch.cuda.empty_cache()
    dump(a, rows)


def loop(a):
    import cpu_active
    pkg = importlib.import_module("atm-vfi_amd")
    active = importlib.import_module("atm-vfi_amd.active")
    host_io = importlib.import_module("atm-vfi_amd.host_io")
    dev = torch.device("cuda:0")
    net = (pkg.NetworkBase if a.model == "base" else pkg.NetworkLite)()
    net.load_state_dict(pkg.synthetic_state_dict(a.model, seed=1), strict=True)
    net = net.to(dev).eval()
    h, w = (int(v) for v in a.size.split("x"))
    win, _ = letterbox(h, w)
    frames, _ = cpu_active.letterboxed(a.frames, h, w, (win[0], win[0] + win[2]), seed=3)
    kw = {}
    if a.pix_fmt:                                        # the same video as frames of that format
        import cpu_yuv_active
        yuv = importlib.import_module("atm-vfi_amd.yuv")
        kw["pixfmt"] = yuv.surface_of(a.pix_fmt, h, w)
        frames = cpu_yuv_active.letterboxed_yuv(yuv, kw["pixfmt"], frames)

    def run(make_area):
        area = make_area()
        t0 = time.perf_counter()
        first = last = None
        n = 0
        for _ in host_io.interpolate_video_nx(iter(frames), net, factor=4, active=area, **kw):
            last = time.perf_counter()
            first = last if first is None else first
            n += 1
        assert n == 4 * (len(frames) - 1) + 1 and (area is None or (area.window == win and area.fallback_at is None))
        return (n - 1) / (last - first), (first - t0) * 1e3
    cfg = {"active=None": lambda: None, "active=ActiveArea()": active.ActiveArea}
    for mk in cfg.values():                              # warm-up: workspaces, launch plans
        run(mk)
    res = {k: [] for k in cfg}
    for _ in range(a.repeats):
        for k, mk in cfg.items():
            res[k].append(run(mk))
    print(f"--- loop: network_{a.model} {h} x {w}{' ' + a.pix_fmt if a.pix_fmt else ''}, picture {win[2]} x {win[3]} at row {win[0]}, {a.frames} frames, 4x, {a.repeats} repeats interleaved")
    for k, r in res.items():
        fps, ttf = [x[0] for x in r], [x[1] for x in r]
        print(f"{k:>22}: {statistics.median(fps):8.2f} output frames/s (min {min(fps):.2f}, max {max(fps):.2f});  first output after "
              f"{statistics.median(ttf):8.1f} ms (min {min(ttf):.1f}, max {max(ttf):.1f})", flush=True)
    base, act = (statistics.median([x[0] for x in res[k]]) for k in cfg)
    print(f"{'ratio':>22}: {act / base:8.3f} x (padded rows {-(-h // 64) * 64} / {-(-win[2] // 64) * 64} = {(-(-h // 64) * 64) / (-(-win[2] // 64) * 64):.3f})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--yuv", action="store_true", help="the YUV calls: yuv_borders and yuv_compose")
    ap.add_argument("--pix-fmt", default=None, choices=("nv12", "yuv420p"), help="with --loop: frames of that 8-bit format instead of RGB")
    ap.add_argument("--model", choices=("base", "lite"), default="base")
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--frames", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_active: no GPU")
    torch.set_grad_enabled(False)
    if a.repeats is None:
        a.repeats = 3 if a.loop else 5
    loop(a) if a.loop else kernels_yuv(a) if a.yuv else kernels(a)


if __name__ == "__main__":
    main()
