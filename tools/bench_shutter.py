#!/usr/bin/env python3
"""Time the synthetic shutter's kernels (atm-vfi_amd/csrc/shutter.hip) with the protocol of tools/bench_frames.py: device events around
back-to-back calls after a warm-up, buffers in rotation so that every source comes from HBM (each rotation exceeds the 256 MB Infinity
Cache), every configuration timed ``--repeats`` times in rotation, median with min - max.  Sizes 1080 x 1920 and 2160 x 4096 (no padding).

Calls: ``shutter_accumulate`` with an fp32 and with a uint8 source, ``first`` and read-modify-write, and ``shutter_resolve``; the yardstick,
in the same rotation on the same geometry, is ``frame_f32_to_u8`` (12 bytes read and 3 written per pixel).  Bytes per pixel of the
algorithm: accumulate fp32 first 24, fp32 read-modify-write 36, uint8 first 15, uint8 read-modify-write 27, resolve 15, yardstick 15.
What the kernels are held to, at 2160 x 4096 (at 1080p the neighbours sit at the rate calls can be issued): a call takes no longer than
(its bytes / the yardstick's bytes) x the yardstick's time + 15 %.  The verdict is printed per call; it is a report, not an exit code.

``--loop``: instead, ``interpolate_video_retimed`` 60 -> 60 fps with 3 levels at 180 degrees (positions 1, 6, 7 of every segment: 5
forwards) against the unblurred loop's backend running the same sparse schedule and taking those three positions to the host, in one
process, interleaved, as ms per forward (wall / forwards).

    python tools/bench_shutter.py [--iters 240] [--repeats 5] [--json OUT]
    python tools/bench_shutter.py --loop [--model base|lite] [--size 1080x1920] [--frames 7] [--repeats 3]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):          # (tests/: pairs.uint8_video for --loop)
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


def kernels(a):
    dev = torch.device("cuda:0")
    ops = hip_ops.HipOps(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for h, w in SIZES:
        px = h * w
        n = max(3, -(-320_000_000 // (12 * px)) + 1)         # fp32 and accumulator rotations beyond the Infinity Cache
        nb = max(3, -(-320_000_000 // (3 * px)) + 1)         # the same for the uint8 frames
        f32 = [torch.rand(3, h, w, dtype=torch.float32, device=dev, generator=gen) for _ in range(n)]
        u8 = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nb)]
        acc = [torch.randint(0, 65535 * 4, (3, h, w), dtype=torch.int32, device=dev, generator=gen) for _ in range(n)]
        out = [torch.empty(h, w, 3, dtype=torch.uint8, device=dev) for _ in range(nb)]
        cfg = {      # name -> (call, bytes per pixel of the algorithm)
            "frame_f32_to_u8 (yardstick)": (lambda i: ops.frame_f32_to_u8(f32[i % n], out[i % nb], 0, 0, False), 15),
            "shutter_accumulate fp32 first": (lambda i: ops.shutter_accumulate(acc[i % n], src=f32[(i + 1) % n], first=True), 24),
            "shutter_accumulate fp32 rmw": (lambda i: ops.shutter_accumulate(acc[i % n], src=f32[(i + 1) % n], weight=1), 36),
            "shutter_accumulate uint8 first": (lambda i: ops.shutter_accumulate(acc[i % n], src_u8=u8[i % nb], first=True), 15),
            "shutter_accumulate uint8 rmw": (lambda i: ops.shutter_accumulate(acc[i % n], src_u8=u8[i % nb], weight=1), 27),
            "shutter_resolve": (lambda i: ops.shutter_resolve(acc[i % n], 4, out[i % nb]), 15),
        }

        def refill():
            """(the read-modify-write calls grow the accumulators: keep them inside what a total weight of 4 allows)"""
            for t in acc:
                t.random_(0, 65535 * 4, generator=gen)
        times = {k: [] for k in cfg}
        for _ in range(a.repeats):           # in rotation: every repeat visits every configuration once
            for k, (fn, _) in cfg.items():
                times[k].append(timed(fn, a.iters))
                if k.endswith("rmw"):
                    refill()
        yard = statistics.median(times["frame_f32_to_u8 (yardstick)"])
        print(f"--- {h} x {w}: rotations of {n} fp32 / int32 and {nb} uint8 buffers, {a.iters} calls x {a.repeats} repeats", flush=True)
        for k, (_, bpp) in cfg.items():
            t = times[k]
            med, nbytes = statistics.median(t), float(bpp) * px
            bound = bpp / 15.0 * yard * MARGIN
            verdict = "" if "yardstick" in k else f"  bound {bound:7.2f} us: {'met' if med <= bound else 'MISSED'}"
            rows.append({"size": [h, w], "name": k, "us_median": med, "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                         "GBps": nbytes / (med * 1e-6) / 1e9, "bound_us": None if "yardstick" in k else bound, "repeats_us": t})
            print(f"{k:>34}: {med:8.2f} us (min {min(t):.2f}, max {max(t):.2f})  {nbytes / 1e6:6.1f} MB  {nbytes / (med * 1e-6) / 1e9:7.1f} GB/s  "
                  f"{100 * nbytes / (med * 1e-6) / HBM:5.1f}% of 6.3 TB/s{verdict}", flush=True)
        del f32, u8, acc, out
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "rows": rows}, f, indent=1)


def loop(a):
    import pairs
    pkg = importlib.import_module("atm-vfi_amd")
    rt = importlib.import_module("atm-vfi_amd.retime")
    sg = importlib.import_module("atm-vfi_amd.segments")
    sh = importlib.import_module("atm-vfi_amd.shutter")
    host_io = importlib.import_module("atm-vfi_amd.host_io")
    dev = torch.device("cuda:0")
    net = (pkg.NetworkBase if a.model == "base" else pkg.NetworkLite)()
    net.load_state_dict(pkg.synthetic_state_dict(a.model, seed=1), strict=True)
    net = net.to(dev).eval()
    h, w = (int(v) for v in a.size.split("x"))
    frames = pairs.uint8_video(a.frames, h, w, seed=3)
    levels, positions = 3, [1, 6, 7]
    nodes = sum(len(lv) for lv in rt.sparse_levels(positions, levels))
    assert {p for _, _, s in sh.shutter_slots(range(3), 60, 60, levels, 180) for j, p, _ in s if j == 1 and 0 < p < 8} == set(positions)

    def blurred():
        report = {}
        t0 = time.perf_counter()
        n = sum(1 for _ in rt.interpolate_video_retimed(iter(frames), net, 60, 60, levels=levels, shutter=sh.Shutter(180), report=report))
        torch.cuda.synchronize()
        assert n == len(frames) and report["forwards"] == nodes * (len(frames) - 1)
        return (time.perf_counter() - t0) * 1e3 / report["forwards"]

    def plain():
        """shutter=None's backend on the same sparse schedule: the three positions of every segment leave for the host"""
        ops, _ = host_io._hip_ops_of(net)
        t0 = time.perf_counter()
        st = sg.open_stream(frames[0], None, None, False, True, "bench_shutter")
        be = sg.DeviceBackend(net, ops, dev, st, n=1 << levels, crop=None, divisor=64, tta=False, max_batch=4, pool=True, sparse=True,
                              out_slots=len(positions))
        try:
            entries = []
            for i, f in enumerate(frames):          # uploads one frame ahead of the segments, as the loop has them
                e = {"i": i, "f": f}
                be.admit(e)
                if i == 0:
                    be.first(e)
                entries.append(e)
                if i >= 2:
                    be.segment(entries[i - 2], entries[i - 1], positions, False)
            be.segment(entries[-2], entries[-1], positions, False)
            torch.cuda.synchronize()
        finally:
            be.close()
        return (time.perf_counter() - t0) * 1e3 / (nodes * (len(frames) - 1))
    blurred(), plain()                               # warm-up: workspaces, launch plans
    times = {"shutter=Shutter(180)": [], "shutter=None, same schedule": []}
    for _ in range(a.repeats):
        times["shutter=Shutter(180)"].append(blurred())
        times["shutter=None, same schedule"].append(plain())
    print(f"--- loop: network_{a.model} {h} x {w}, {a.frames} frames, 60 -> 60 fps, levels 3, {nodes} forwards per segment, {a.repeats} repeats interleaved")
    for k, t in times.items():
        print(f"{k:>30}: {statistics.median(t):8.3f} ms per forward (min {min(t):.3f}, max {max(t):.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--model", choices=("base", "lite"), default="base")
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--frames", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_shutter: no GPU")
    torch.set_grad_enabled(False)
    if a.repeats is None:
        a.repeats = 3 if a.loop else 5
    loop(a) if a.loop else kernels(a)


if __name__ == "__main__":
    main()
