#!/usr/bin/env python3
"""Time half-resolution motion (atm-vfi_amd/scaled.py; csrc/warp.hip atmvfi_frame_half, atmvfi_synth_up2) on the project's protocol
(tools/yuv_timing.py): device events around ``--iters`` back-to-back calls after 24 warm-up calls, the calls rotating over ``--buffers``
distinct sources and destinations (beyond the Infinity Cache), every configuration timed ``--repeats`` times in rotation in one process
(median, min - max).

Kernels (default): ``frame_half`` of one [3,H,W] frame and ``synth_up2`` (B = 1; the direct form -- ``path="auto"`` -- with fp32,
fp32 + uint8 and uint8 output, the staged form with fp32; bytes: the six full-size source planes, the outputs, 14 floats per half-size
pixel) at
1088 x 1920 -> 2176 x 3840 and 1088 x 2048 -> 2176 x 4096, beside ``warp_blend`` (the LDS-staged kernel, as the forward's finest level
calls it: flows and masks written) and ``frame_f32_to_u8`` on full-size frames from the same library in the same rotation.  At 4K a
call is held to ``(its bytes / the yardstick's bytes) x the yardstick's median + 15 %``: ``synth_up2`` against ``warp_blend``,
``frame_half`` against ``frame_f32_to_u8``.  Flows: ``--flow`` half-size pixels of Gaussian sigma (small: 0.5; large: 6); the share of
output tiles whose taps leave the staged box is computed on the host from the same flows with the kernel's rule
(tests/warp_ref.py staged_boxes, on a 256 x 512 corner of the frame).

``--forward``: network_base ``forward_scaled`` at 2176 x 4096 beside ``forward`` at 2176 x 4096 and ``forward`` at 1088 x 2048 in one
process (``--fwd-iters`` calls, ``--fwd-repeats`` repeats in rotation), the ratios, and ``forward_scaled`` minus the half-size forward
against the sum of the two kernels' own times.
``--loop``: the 4x N-x loop on 2160 x 4096 uint8 frames with ``motion_scale`` 1 and 2, interleaved: output frames per second.

The kernel run exits with status 1 when a 4K limit is missed.

    python tools/bench_scaled.py [--iters 240] [--repeats 5] [--buffers 4] [--forward] [--loop] [--json OUT]"""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation)
HBM = 6.3e12
SIZES = [(1088, 1920), (1088, 2048)]
BOUND = 1.15
Y_WARP, Y_U8 = "warp_blend tiled (yardstick)", "frame_f32_to_u8 (yardstick)"


def fallback_share(f0, f1):
    """share of (tile, source) pairs of a 256 x 512 corner whose taps leave the staged box"""
    import warp_ref as WR
    st = [v["state"] for f in (f0, f1) for v in WR.staged_boxes(f[:, :, :256, :512].cpu().numpy()).values()]
    return sum(s == "falls back" for s in st) / len(st)


def configs(ops, dev, h, w, n, sigma):
    H, W = 2 * h, 2 * w
    gen = torch.Generator(device=dev).manual_seed(h + w)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float32, device=dev, generator=gen)
    nrm = lambda *s: torch.randn(*s, dtype=torch.float32, device=dev, generator=gen)
    stores = [rnd(2, 3, H, W) for _ in range(n)]
    halves = [{"im_t_list": [rnd(1, 3, h, w)], "I_t_0": rnd(1, 3, h, w), "I_t_1": rnd(1, 3, h, w), "opt_flow_0": nrm(1, 2, h, w) * sigma,
               "opt_flow_1": nrm(1, 2, h, w) * sigma, "occ_mask1": rnd(1, 1, h, w)} for _ in range(n)]
    dst = [torch.empty(1, 3, H, W, dtype=torch.float32, device=dev) for _ in range(n)]
    u8 = [torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    hdst = [torch.empty(3, h, w, dtype=torch.float32, device=dev) for _ in range(n)]
    # the yardstick's operands: a full-size motion map [1,H,W,5] with flows of the same size as the synthesis sees (2 x sigma)
    motion = [torch.cat([nrm(1, H, W, 4) * (2 * sigma), nrm(1, H, W, 1)], -1).contiguous() for _ in range(n)]
    outs = [[torch.empty(1, c, H, W, dtype=torch.float32, device=dev) for c in (3, 3, 3, 2, 2, 1, 1)] for _ in range(n)]
    full = 4.0 * H * W
    half_in = 14.0 * 4 * h * w
    cfg = {
        Y_WARP: (lambda i: ops.warp_blend(stores[i % n][0:1], stores[i % n][1:2], motion[i % n], *outs[i % n][:3], flow0=outs[i % n][3],
                                          flow1=outs[i % n][4], mask1=outs[i % n][5], mask2=outs[i % n][6]), full * (6 + 5 + 9 + 6), None),
        Y_U8: (lambda i: ops.frame_f32_to_u8(dst[i % n][0], u8[i % n][0], 0, 0, False), 15.0 * H * W, None),
        "frame_half": (lambda i: ops.frame_half(stores[i % n][0], hdst[i % n]), 3 * full * 1.25, Y_U8),
        "synth_up2 direct, fp32": (lambda i: ops.synth_up2(halves[i % n], stores[i % n], stores[i % n], [0], [1], dst=dst[i % n], path="direct"),
                                   half_in + 9 * full, Y_WARP),
        "synth_up2 direct, fp32 + uint8": (lambda i: ops.synth_up2(halves[i % n], stores[i % n], stores[i % n], [0], [1], dst=dst[i % n],
                                                                   dst_u8=u8[i % n], path="direct"), half_in + 9 * full + 3.0 * H * W, Y_WARP),
        "synth_up2 direct, uint8": (lambda i: ops.synth_up2(halves[i % n], stores[i % n], stores[i % n], [0], [1], dst_u8=u8[i % n], path="direct"),
                                    half_in + 6 * full + 3.0 * H * W, Y_WARP),
        "synth_up2 staged, fp32": (lambda i: ops.synth_up2(halves[i % n], stores[i % n], stores[i % n], [0], [1], dst=dst[i % n], path="staged"),
                                   half_in + 9 * full, Y_WARP),
    }
    got = ops.synth_up2(halves[0], stores[0], stores[0], [0], [1], want=("opt_flow_0", "opt_flow_1"))
    return cfg, fallback_share(got["opt_flow_0"], got["opt_flow_1"])


def kernels(a, dev, rows):
    ops = yuv_timing.hip_ops.HipOps(dev)
    n = max(1, a.buffers)
    missed = []
    print(f"device {torch.cuda.get_device_name(0)}; {a.iters} calls after 24 warm-ups, {n} rotating buffers, median of {a.repeats} repeats; "
          f"ABI 0.{(ops.lib.atmvfi_version() >> 8) & 255}", flush=True)
    for sigma in a.flow:
        for h, w in SIZES:
            cfg, share = configs(ops, dev, h, w, n, sigma)
            times, _ = yuv_timing.rotation(cfg, None, a.repeats, a.iters)
            med = {k: statistics.median(t) for k, t in times.items()}
            judged = (h, w) == SIZES[-1]
            print(f"--- {h} x {w} -> {2 * h} x {2 * w}, half-size flows sigma {sigma}: {100 * share:.1f} % of the (tile, source) pairs fall back to gathers"
                  + ("" if judged else "  (no verdict at this size)"), flush=True)
            for k, (_, nbytes, yard) in cfg.items():
                t = times[k]
                limit = nbytes / cfg[yard][1] * med[yard] * BOUND if yard else None
                verdict = None
                if yard and judged:
                    verdict = "met" if med[k] <= limit else f"missed by {100 * (med[k] / limit - 1):.1f} %"
                    if med[k] > limit:
                        missed.append((sigma, k))
                rows.append({"size": [h, w], "sigma": sigma, "name": k, "us_median": med[k], "us_min": min(t), "us_max": max(t), "bytes": nbytes,
                             "limit_us": limit, "verdict": verdict, "fallback_share": share})
                rel = f"  limit {limit:7.2f} us = {nbytes / cfg[yard][1]:5.3f} x {med[yard]:6.2f} us + 15 %" if yard else ""
                rel += f"  [{verdict}]" if verdict else ""
                print(f"{k:>32}: {med[k]:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
                      f"{nbytes / (med[k] * 1e-6) / 1e9:7.1f} GB/s  {100 * nbytes / (med[k] * 1e-6) / HBM:5.1f}% of 6.3 TB/s{rel}", flush=True)
            del cfg
            torch.cuda.empty_cache()
    print("4K limits: " + ("all met" if not missed else f"MISSED: {missed}"), flush=True)
    return not missed


def _net(dev):
    torch.set_grad_enabled(False)
    net = pkg.NetworkBase()
    net.load_state_dict(pkg.synthetic_state_dict("base", seed=1), strict=True)
    return net.to(dev).eval()


def forward(a, dev, rows):
    net, ops = _net(dev), None
    H, W = 2176, 4096
    gen = torch.Generator(device=dev).manual_seed(1)
    big = [torch.rand(1, 3, H, W, device=dev, generator=gen) for _ in range(2)]
    small = [torch.rand(1, 3, H // 2, W // 2, device=dev, generator=gen) for _ in range(2)]
    ops = net._ops(dev)
    o = net.forward(*small)
    hdst = torch.empty(1, 3, H // 2, W // 2, device=dev)
    cfg = {"forward 2176 x 4096": (lambda i: net.forward(*big),), "forward 1088 x 2048": (lambda i: net.forward(*small),),
           "forward_scaled 2176 x 4096": (lambda i: net.forward_scaled(*big),),
           "frame_half x 2 (alone)": (lambda i: (ops.frame_half(big[0], hdst), ops.frame_half(big[1], hdst)),),
           "synth_up2 (alone)": (lambda i: ops.synth_up2(o, big[0], big[1]),)}
    times, _ = yuv_timing.rotation(cfg, None, a.fwd_repeats, a.fwd_iters)
    med = {k: statistics.median(t) / 1e3 for k, t in times.items()}
    print(f"--- network_base, {a.fwd_iters} calls after 24 warm-ups, median of {a.fwd_repeats} repeats in rotation (ms)", flush=True)
    for k, t in times.items():
        print(f"{k:>30}: {med[k]:9.3f} ms (min {min(t) / 1e3:.3f}, max {max(t) / 1e3:.3f})", flush=True)
        rows.append({"name": k, "ms_median": med[k], "ms_min": min(t) / 1e3, "ms_max": max(t) / 1e3})
    full, half, sc = med["forward 2176 x 4096"], med["forward 1088 x 2048"], med["forward_scaled 2176 x 4096"]
    extra, own = sc - half, med["frame_half x 2 (alone)"] + med["synth_up2 (alone)"]
    spread = max(max(t) - min(t) for k, t in times.items() if k.startswith("forward")) / 1e3
    print(f"forward / forward_scaled = {full / sc:.2f} x; forward_scaled / half-size forward = {sc / half:.3f} x; forward_scaled - half-size forward = "
          f"{extra:.3f} ms against {own:.3f} ms of the two kernels alone (largest spread of the forwards' repeats: {spread:.3f} ms): "
          f"{'within' if extra <= own + spread else 'BEYOND'} the spread", flush=True)
    rows.append({"name": "ratios", "full_over_scaled": full / sc, "scaled_over_half": sc / half, "extra_ms": extra, "kernels_ms": own, "spread_ms": spread})


def loop(a, dev, rows):
    net = _net(dev)
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, (2160, 4096 + 8, 3)).astype(np.uint8)
    video = [np.ascontiguousarray(base[:, k:k + 4096]) for k in range(a.loop_frames)]
    fps = {1: [], 2: []}
    for rep in range(a.loop_repeats + 1):
        for sc in (1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(1 for _ in mf.interpolate_video_nx(iter(video), net, factor=4, motion_scale=sc))
            torch.cuda.synchronize()
            if rep:                                 # (the first round warms both up: workspaces, plans)
                fps[sc].append(n / (time.perf_counter() - t0))
    print(f"--- 4x loop, network_base, {a.loop_frames} frames of 2160 x 4096, interleaved, {a.loop_repeats} repeats after one warm-up round: output frames / s", flush=True)
    for sc in (1, 2):
        print(f"motion_scale={sc}: {statistics.median(fps[sc]):7.2f} (min {min(fps[sc]):.2f}, max {max(fps[sc]):.2f})", flush=True)
        rows.append({"name": f"loop motion_scale={sc}", "fps_median": statistics.median(fps[sc]), "fps": fps[sc]})
    print(f"motion_scale 2 / 1 = {statistics.median(fps[2]) / statistics.median(fps[1]):.2f} x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--flow", type=float, nargs="+", default=[0.5, 6.0])
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--fwd-iters", type=int, default=12)
    ap.add_argument("--fwd-repeats", type=int, default=3)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--loop-frames", type=int, default=4)
    ap.add_argument("--loop-repeats", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scaled: no GPU")
    dev, rows = torch.device("cuda:0"), []
    ok = (forward if a.forward else loop if a.loop else kernels)(a, dev, rows)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    if ok is False:
        sys.exit(1)                                 # a byte-scaled limit was missed


if __name__ == "__main__":
    main()
