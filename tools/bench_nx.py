#!/usr/bin/env python3
"""Time N-x recursive interpolation (atm-vfi_amd/multiframe.py) and its two data-movement kernels (csrc/multiframe.hip).

End to end: ``interpolate_video_nx`` on uint8 frames in host memory, network_base, global branch on, ``factor`` 4 and 8, at 480x832
(``divisor=None``, the DAVIS size of benchmark/davis-vid.py) and 1080x1920 (padded to 1088x1920), for ``pool=False`` (plain forwards on
launch plans: what a caller composing ``Network.forward`` gets), ``pool=True, max_batch=1`` and ``pool=True, max_batch=4``, the last two
also with the pooled launch plans off (``forward_pooled`` on direct launches, the behaviour before it was planned; a tool-only switch
on the model, not a selection).  Device events around the steady state of one video: the first ``--warm`` segments (workspaces, pool)
are not timed, the next ``--segments`` are; output frames/s = N x segments / time.  Before anything is timed every mode runs the video
once untimed (``--prime``): a launch plan is recorded by the third call of its key and a key of the steady state first occurs in the
second segment, so the recordings would otherwise fall into the first repeat's timed segments.  Every configuration is timed
``--repeats`` times in rotation (median, min-max: the spread is the noise a difference has to exceed).  Also printed: frames through
``stem_fused`` per steady-state segment, and ``Network.plan_stats()`` of the mode's timed runs (a steady state that still records or
runs eagerly shows there).

Kernels alone: ``pool_blocks`` (gather of 8 frame / local-token / global-token blocks of a 1088x1920 base pool, and a scatter) and
``tta_merge`` / ``frame_rot180`` on 1088x1920 frames, in GB/s of bytes read + written beside the 6.3 TB/s streaming ceiling; the calls
rotate over ``--buffers`` distinct buffers so that a block does not come from the 256 MB Infinity Cache.

``--scene``: every mode is also timed with scene-cut detection on (``scene=SceneCuts()``: a frame signature per uploaded frame and a
host read of it per segment), interleaved with the same mode without it; the input is cut-free (asserted), so the difference is
the detection's cost.  ``--modes``: only the modes whose name contains one of the given comma-separated strings.

    python tools/bench_nx.py [--sizes 480x832,1080x1920] [--factors 4,8] [--segments 4] [--repeats 3] [--kernels-only] [--scene]
                             [--modes "mb=4"] [--json OUT]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
mf = importlib.import_module("atm-vfi_amd.multiframe")
scene = importlib.import_module("atm-vfi_amd.scene")
HBM = 6.3e12
MODES = (("pool=False", dict(pool=False, max_batch=4)),
         ("pool=True mb=1 plans off", dict(pool=True, max_batch=1, pooled_plans=False)), ("pool=True mb=1", dict(pool=True, max_batch=1)),
         ("pool=True mb=4 plans off", dict(pool=True, max_batch=4, pooled_plans=False)), ("pool=True mb=4", dict(pool=True, max_batch=4)))


def timed(fn, iters, warm=8):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def video(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h + 2 * n, w + 2 * n, 3), dtype=np.uint8)
    return [np.ascontiguousarray(base[k:k + h, 2 * k:2 * k + w]) for k in range(n)]


def run_video(net, frames, factor, warm, segments, divisor, **kw):
    """-> (ms of the timed segments, frames produced in them).  ``pooled_plans=False`` among ``kw``: forward_pooled on direct launches."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    got = 0
    kw = dict(kw)
    net._pooled_plans_on = kw.pop("pooled_plans", True)
    try:
        for k, _ in enumerate(mf.interpolate_video_nx(iter(frames), net, factor=factor, divisor=divisor, **kw)):
            if k == warm * factor:
                torch.cuda.synchronize()
                s.record()
            got = k
        e.record()
        e.synchronize()
    finally:
        net._pooled_plans_on = True
    assert got == (warm + segments) * factor
    assert kw.get("scene") is None or kw["scene"].cuts == [], "the benchmark video must be cut-free"
    return s.elapsed_time(e), segments * factor


def add_stats(total, before, after):
    """``total`` + (``after`` - ``before``) of two ``Network.plan_stats()`` readings."""
    return {kind: {k: (total[kind][k] if total else 0) + v - before[kind][k] for k, v in c.items()} for kind, c in after.items()}


def show_stats(stats):
    """eager/recorded/replayed/refused per kind, kinds without a call left out."""
    return "; ".join(f"{kind} {c['eager']}e/{c['recorded']}rec/{c['replayed']}rep/{c['refused']}ref" for kind, c in stats.items()
                     if any(c.values())) or "-"


def stem_per_segment(net, ops, frames, factor, divisor, **kw):
    counts = []
    kw = {k: v for k, v in kw.items() if k != "pooled_plans"}       # (profiling takes the direct launches anyway)
    ops.profile = []
    try:
        for k, _ in enumerate(mf.interpolate_video_nx(iter(frames[:4]), net, factor=factor, divisor=divisor, **kw)):
            if k % factor == 0:
                counts.append(sum(int(m["shape"].split("x")[0]) for nm, m, _, _ in ops.profile if nm == "stem_fused"))
    finally:
        ops.profile = None
    return counts[2] - counts[1]


def kernels(ops, dev, iters, nbuf, rows):
    v = pkg.VARIANTS["base"]
    hp, wp = 1088, 1920
    blocks = {"frames": 3 * hp * wp, "local tokens": (hp // 8) * (wp // 8) * v.local_dim, "global tokens": (hp // 16) * (wp // 16) * v.global_dim}
    slots = [8, 0, 4, 2, 6, 1, 3, 5]
    cfg = {}
    for name, elems in blocks.items():
        pools = [torch.rand(9, elems, device=dev) for _ in range(2)]
        bufs = [torch.empty(8, elems, device=dev) for _ in range(2)]
        cfg[f"pool_blocks gather 8 x {name}"] = (lambda i, p=pools, b=bufs: ops.pool_blocks(p[i % 2], slots, b[i % 2]), 2.0 * 8 * elems * 4)
        cfg[f"pool_blocks scatter 8 x {name}"] = (lambda i, p=pools, b=bufs: ops.pool_blocks(p[i % 2], slots, b[i % 2], to_pool=True), 2.0 * 8 * elems * 4)
    cfg["pool_blocks gather 1 x 16 B"] = (lambda i, p=torch.rand(9, 4, device=dev), b=torch.empty(1, 4, device=dev): ops.pool_blocks(p, [3], b), 32.0)
    fr = [torch.rand(3, hp, wp, device=dev) for _ in range(nbuf)]
    outs = [torch.empty(3, hp, wp, device=dev) for _ in range(nbuf)]
    u8 = [torch.empty(1080, 1920, 3, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    pl = 12.0 * hp * wp
    cfg["tta_merge fp32 + u8"] = (lambda i: ops.tta_merge(fr[i % nbuf], fr[(i + 1) % nbuf], out=outs[i % nbuf], out_u8=u8[i % nbuf], pad_top=4), 3 * pl + 3.0 * 1080 * 1920)
    cfg["tta_merge u8 only"] = (lambda i: ops.tta_merge(fr[i % nbuf], fr[(i + 1) % nbuf], out_u8=u8[i % nbuf], pad_top=4), 2 * pl + 3.0 * 1080 * 1920)
    cfg["frame_rot180"] = (lambda i: ops.frame_rot180(fr[i % nbuf], outs[i % nbuf]), 2 * pl)
    cfg["torch flip/flip/add/div (yardstick)"] = (lambda i: (fr[i % nbuf] + fr[(i + 1) % nbuf].flip(1).flip(2)) / 2, 3 * pl)
    times = {k: [] for k in cfg}
    for _ in range(3):
        for k, (fn, _) in cfg.items():
            times[k].append(timed(fn, iters))
    for k, (_, nbytes) in cfg.items():
        t = times[k]
        med = statistics.median(t)
        rows.append({"name": k, "us_median": med, "us_min": min(t), "us_max": max(t), "bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9})
        print(f"{k:>42}: {med:9.2f} us (min {min(t):.2f}, max {max(t):.2f})  {nbytes / 1e6:8.1f} MB  {rows[-1]['GBps']:7.1f} GB/s  "
              f"{100 * rows[-1]['GBps'] * 1e9 / HBM:5.1f}% of 6.3 TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="480x832,1080x1920")
    ap.add_argument("--factors", default="4,8")
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prime", type=int, default=1, help="untimed runs of the video per mode before the timed rotation")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--scene", action="store_true", help="also time every mode with scene-cut detection on")
    ap.add_argument("--modes", default=None, help="comma-separated substrings of the mode names to run")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nx: no GPU")
    modes = [(n, kw) for n, kw in MODES if a.modes is None or any(m in n for m in a.modes.split(","))]
    if a.scene:           # off and on next to each other: the rotation below interleaves them
        modes = [m for n, kw in modes for m in ((n, kw), (n + " +scene", dict(kw, scene=scene.SceneCuts())))]
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    result = {"device": torch.cuda.get_device_name(0), "kernels": [], "videos": []}
    if not a.no_kernels:
        kernels(hip_ops.HipOps(dev), dev, a.iters, max(2, a.buffers), result["kernels"])
    if not a.kernels_only:
        net = pkg.NetworkBase()
        net.load_state_dict(pkg.synthetic_state_dict("base", seed=1), strict=True)
        net.to(dev).eval()
        net.global_motion, net.ensemble_global_motion = True, False
        ops = net._ops(dev)
        for size in a.sizes.split(","):
            h, w = (int(x) for x in size.split("x"))
            divisor = None if (h % 16 == 0 and w % 16 == 0) else 64
            frames = video(a.warm + a.segments + 1, h, w)
            for factor in (int(x) for x in a.factors.split(",")):
                times = {name: [] for name, _ in modes}
                stats = {name: None for name, _ in modes}
                for _ in range(a.prime):              # every key of the steady state recorded before anything is timed
                    for name, kw in modes:
                        run_video(net, frames, factor, a.warm, a.segments, divisor, **kw)
                for _ in range(a.repeats):            # in rotation: pool=False is the baseline of the same process and run
                    for name, kw in modes:
                        before = net.plan_stats()
                        ms, n = run_video(net, frames, factor, a.warm, a.segments, divisor, **kw)
                        times[name].append(n / (ms * 1e-3))
                        stats[name] = add_stats(stats[name], before, net.plan_stats())
                for name, kw in modes:
                    t = times[name]
                    row = {"size": size, "factor": factor, "mode": name, "fps_median": statistics.median(t), "fps_min": min(t), "fps_max": max(t),
                           "stem_frames_per_segment": stem_per_segment(net, ops, frames, factor, divisor, **kw), "repeats_fps": t,
                           "plan_stats": stats[name]}
                    result["videos"].append(row)
                    print(f"{size:>10} {factor}x {name:>24}: {row['fps_median']:8.2f} output frames/s (min {min(t):.2f}, max {max(t):.2f} over "
                          f"{len(t)} repeats)  stem_fused frames / segment {row['stem_frames_per_segment']}  plans {show_stats(stats[name])}",
                          flush=True)
                net.release_workspace()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
