#!/usr/bin/env python3
"""Time the image-geometry kernels (atm-vfi_amd/csrc/warp.hip) in the shapes of the 1080p forward's calls (network.py, the global-motion
walk and the synthesis levels), on the method of tools/bench_yuv.py: device events around ``--iters`` back-to-back calls after 24
warm-up calls, the calls rotating over ``--buffers`` distinct inputs and outputs, every row timed ``--repeats`` times in rotation
(median, min - max).  Bytes are the algorithm's -- inputs read once, outputs written once -- as a share of 6.3 TB/s.

Rows.  Every warp goes with smooth flows of about 4 px and about 24 px (low-pass noise; 24 px overflows many of the staged boxes) and
with ``warp_tiles`` on and off (LDS-staged tiles / direct gathers); ``flow_warp_nhwc`` and ``flow_warp_ex`` have no tiled form and go
once per flow.
    warp_blend      1088 x 1920 with every output and the refiner's plane sink; 544 x 960, 272 x 480, 136 x 240 with the three frames only
    flow_warp_up2   C = 3, B = 2 at 136 x 240, 272 x 480, 544 x 960
    flow_warp       C = 3 at 1088 x 1920
    flow_warp_nhwc  C = 64 at 136 x 240
    flow_warp_ex    reflection padding with a mask at 272 x 480
    resize          68 x 120 -> 136 x 240 with values x 2; 1088 x 1920 -> 544 x 960
    image_pyramid   1088 x 1920, with and without the NHWC4 pack

    python tools/bench_warp.py [--iters 100] [--repeats 5] [--buffers 3] [--json OUT] [--lib PATH] [--baseline-lib PATH]

``--baseline-lib`` (tools/yuv_timing.py): the same rows on another build of the library in the same rotation, AND the bits of every
output of every row compared between the two libraries (torch.equal after nan_to_num); a differing output ends the run with exit
status 1 after the table.  The comparison is ONE call per row and library, on buffer set 0 at the row's ``warp_tiles`` setting: it does
not cover the other buffer sets of the rotation, and "all bit-identical" says no more than that."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
import yuv_timing  # noqa: E402  (tools/yuv_timing.py: timed(), the rotation, --baseline-lib)
HBM = 6.3e12
AMPS = (4.0, 24.0)


def smooth(gen, b, c, h, w, amp, dev):
    """[b, c, h, w] low-pass noise of standard deviation about ``amp``"""
    low = torch.randn(b, c, max(2, h // 32), max(2, w // 32), generator=gen)
    return (torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=True) * amp).contiguous().to(dev)


def configs(ops, dev, n):
    """name -> (call(i), bytes of the algorithm, the output tensors of call(0)).  Deterministic: two libraries get equal inputs."""
    gen = torch.Generator().manual_seed(0)
    cfg = {}

    def rand(*shape):
        return [torch.rand(*shape, generator=gen).to(dev) for _ in range(n)]

    def empty(*shape, dtype=torch.float32):
        return [torch.empty(*shape, dtype=dtype, device=dev) for _ in range(n)]

    def add(name, tiles, fn, nbytes, outs):
        def call(i, fn=fn, tiles=tiles):
            ops.warp_tiles = tiles
            fn(i % n)
        cfg[name] = (call, nbytes, outs)

    def both(name, fn, nbytes, outs):
        add(name + ", tiles", True, fn, nbytes, outs)
        add(name + ", direct", False, fn, nbytes, outs)

    for amp in AMPS:
        tag = f"~{amp:.0f} px"
        # ---- warp_blend: the full-resolution call with every output and the plane sink, then the coarser levels
        for H, W, full in ((1088, 1920, True), (544, 960, False), (272, 480, False), (136, 240, False)):
            im0, im1 = rand(1, 3, H, W), rand(1, 3, H, W)
            motion = [smooth(gen, 1, 5, H, W, amp, dev).permute(0, 2, 3, 1).contiguous() for _ in range(n)]
            a, c, t = empty(1, 3, H, W), empty(1, 3, H, W), empty(1, 3, H, W)
            if full:
                f0, f1, m1, m2 = empty(1, 2, H, W), empty(1, 2, H, W), empty(1, 1, H, W), empty(1, 1, H, W)
                pl = [hip_ops.Planes.alloc(H * W, 32, dev) for _ in range(n)]
                both(f"warp_blend {H}x{W} all outputs + plane sink, {tag}",
                     lambda i, v=(im0, im1, motion, a, c, t, f0, f1, m1, m2, pl): ops.warp_blend(
                         v[0][i], v[1][i], v[2][i], v[3][i], v[4][i], v[5][i], v[6][i], v[7][i], v[8][i], v[9][i], v[0][i], v[1][i], None,
                         pack_planes=v[10][i], pack_c0=8),
                     4.0 * H * W * (6 + 5 + 9 + 6 + 6 + 16), [a[0], c[0], t[0], f0[0], f1[0], m1[0], m2[0], pl[0].t])
            else:
                both(f"warp_blend {H}x{W}, {tag}",
                     lambda i, v=(im0, im1, motion, a, c, t): ops.warp_blend(v[0][i], v[1][i], v[2][i], v[3][i], v[4][i], v[5][i]),
                     4.0 * H * W * (6 + 5 + 9), [a[0], c[0], t[0]])
        # ---- the global flow's walk down the pyramid: warp + x2 up-sampling of the flow, both frames stacked
        for H, W in ((136, 240), (272, 480), (544, 960)):
            src, dst, up = rand(2, 3, H, W), empty(2, 3, H, W), empty(2, 2, 2 * H, 2 * W)
            flow = [smooth(gen, 2, 2, H, W, amp, dev) for _ in range(n)]
            both(f"flow_warp_up2 C=3 B=2 {H}x{W}, {tag}", lambda i, v=(src, flow, dst, up): ops.flow_warp_up2(v[0][i], v[1][i], v[2][i], v[3][i]),
                 4.0 * 2 * H * W * (2 * 3 + 2 + 8), [dst[0], up[0]])
        H, W = 1088, 1920
        src, dst = rand(1, 3, H, W), empty(1, 3, H, W)
        flow = [smooth(gen, 1, 2, H, W, amp, dev) for _ in range(n)]
        both(f"flow_warp C=3 {H}x{W}, {tag}", lambda i, v=(src, flow, dst): ops.flow_warp(v[0][i], v[1][i], v[2][i]), 4.0 * H * W * 8, [dst[0]])
        H, W = 136, 240
        src, dst = rand(1, H, W, 64), empty(1, H, W, 64)
        flow = [smooth(gen, 1, 2, H, W, amp, dev) for _ in range(n)]
        add(f"flow_warp_nhwc C=64 {H}x{W}, {tag}", True, lambda i, v=(src, flow, dst): ops.flow_warp_nhwc(v[0][i], v[1][i], v[2][i]),
            4.0 * H * W * 130, [dst[0]])
        H, W = 272, 480
        src, dst, mask = rand(1, 3, H, W), empty(1, 3, H, W), empty(1, H, W, dtype=torch.uint8)
        flow = [smooth(gen, 1, 2, H, W, amp, dev) for _ in range(n)]
        add(f"flow_warp_ex reflection + mask C=3 {H}x{W}, {tag}", True,
            lambda i, v=(src, flow, dst, mask): ops.flow_warp_ex(v[0][i], v[1][i], v[2][i], mask=v[3][i], padding_mode="reflection"),
            4.0 * H * W * 8 + H * W, [dst[0], mask[0]])
    # ---- no flows
    src, dst = rand(2, 2, 68, 120), empty(2, 2, 136, 240)
    add("resize 68x120 -> 136x240, values x 2", True, lambda i, v=(src, dst): ops.resize(v[0][i], v[1][i], 2.0), 4.0 * 4 * (68 * 120 + 136 * 240),
        [dst[0]])
    src, dst = rand(2, 3, 1088, 1920), empty(2, 3, 544, 960)
    add("resize 1088x1920 -> 544x960", True, lambda i, v=(src, dst): ops.resize(v[0][i], v[1][i]), 4.0 * 6 * (1088 * 1920 + 544 * 960), [dst[0]])
    H, W = 1088, 1920
    im0, im1 = rand(1, 3, H, W), rand(1, 3, H, W)
    lv = [empty(2, 3, H >> l, W >> l) for l in (1, 2, 3)]
    pack = empty(2, H, W, 4)
    pyr_bytes = 4.0 * 6 * H * W * (1 + 0.25 + 0.0625 + 0.015625)
    add(f"image_pyramid {H}x{W}", True, lambda i, v=(im0, im1, lv): ops.image_pyramid(v[0][i], v[1][i], v[2][0][i], v[2][1][i], v[2][2][i]),
        pyr_bytes, [lv[0][0], lv[1][0], lv[2][0]])
    add(f"image_pyramid {H}x{W} + pack", True,
        lambda i, v=(im0, im1, lv, pack): ops.image_pyramid(v[0][i], v[1][i], v[2][0][i], v[2][1][i], v[2][2][i], pack=v[3][i]),
        pyr_bytes + 4.0 * 2 * H * W * 7, [lv[0][0], lv[1][0], lv[2][0], pack[0]])
    return cfg


def differing_outputs(cfg, base_cfg):
    """Every row once on each library, outputs filled with NaN first -> the names of the rows with an output that differs in a bit."""
    bad = []
    for k in cfg:
        got = []
        for c in (cfg, base_cfg):
            for t in c[k][2]:
                t.fill_(float("nan")) if t.is_floating_point() else t.fill_(255)
            c[k][0](0)
            torch.cuda.synchronize()
            got.append([torch.nan_to_num(t.float(), nan=12345.0).clone() for t in c[k][2]])
        if not all(torch.equal(a, b) for a, b in zip(*got)):
            bad.append(k)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=3)
    ap.add_argument("--json", default=None)
    yuv_timing.add_library_arguments(ap)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_warp: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops, base_ops = yuv_timing.libraries(a, dev)
    n = max(1, a.buffers)
    cfg = configs(ops, dev, n)
    base_cfg = configs(base_ops, dev, n) if base_ops else None
    bad = differing_outputs(cfg, base_cfg) if base_cfg else []
    times, base = yuv_timing.rotation(cfg, base_cfg, a.repeats, a.iters)
    rows = []
    for k, (_, nbytes, _) in cfg.items():
        t = times[k]
        med = statistics.median(t)
        row = {"name": k, "us_median": med, "us_min": min(t), "us_max": max(t), "bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9,
               "share_of_hbm": nbytes / (med * 1e-6) / HBM, "repeats_us": t}
        if base_cfg:
            row["bits_equal_baseline"] = k not in bad
        rel = yuv_timing.against_baseline(row, times, base, k) + ("" if not base_cfg else ("  bits DIFFER" if k in bad else "  bits equal"))
        rows.append(row)
        print(f"{k:>62}: {med:8.2f} us (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats)  {nbytes / 1e6:6.1f} MB  "
              f"{100 * row['share_of_hbm']:5.1f}% of 6.3 TB/s{rel}", flush=True)
    if base_cfg:
        print(f"outputs compared with the baseline library on {len(cfg)} rows: " + (f"{len(bad)} DIFFER: {bad}" if bad else "all bit-identical"), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "buffers": n, "lib": a.lib,
                       "baseline_lib": a.baseline_lib, "rows": rows}, f, indent=1)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
