#!/usr/bin/env python3
"""Time frame-rate conversion (atm-vfi_amd/retime.py ``interpolate_video_retimed``) end to end beside the 8x recursion of
``interpolate_video_nx``, by the protocol of tools/bench_nx.py: uint8 frames in host memory, network_base, global branch on, 1080x1920
(padded to 1088x1920), ``pool=True, max_batch=4``; device events around the steady state of one video -- the outputs of the first
``--warm`` source segments are not timed, those of the next ``--segments`` are -- output frames/s = outputs / time.  The modes -- 8x,
``--retime IN:OUT`` (default 24:60) with ``dedup`` off and with ``dedup=Duplicates()`` on, and the retimed loop with ``pool=False``
(plain planned forwards) and with the pooled launch plans off (``forward_pooled`` on direct launches: a tool-only switch on the
model) -- run in the same process, ``--repeats`` times in rotation (median, min-max: the spread is the noise a difference has to
exceed), after ``--prime`` untimed runs of every mode (launch plans are recorded by the third call of a key: the sparse levels of a
retimed segment bring their keys late).  ``Network.plan_stats()`` of each mode's timed runs is printed.  The input has no duplicates
(asserted), so on minus off is the detection's cost: a difference kernel per uploaded frame and a host read of 1 032 bytes.

    python tools/bench_retime.py [--retime 24:60] [--levels 3] [--size 1080x1920] [--segments 8] [--warm 4] [--repeats 3] [--json OUT]"""
import argparse
import importlib
import json
import os
import statistics
import sys
from fractions import Fraction

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")


def video(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h + 2 * n, w + 2 * n, 3), dtype=np.uint8)
    return [np.ascontiguousarray(base[k:k + h, 2 * k:2 * k + w]) for k in range(n)]


def run(gen, first):
    """-> (ms from output ``first`` to the end, outputs in them)."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    got = 0
    for k, _ in enumerate(gen):
        if k == first:
            torch.cuda.synchronize()
            s.record()
        got = k
    e.record()
    e.synchronize()
    return s.elapsed_time(e), got - first


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--retime", default="24:60")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prime", type=int, default=1, help="untimed runs of every mode before the timed rotation")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_retime: no GPU")
    fi, fo = (Fraction(x) for x in a.retime.split(":"))
    h, w = (int(x) for x in a.size.split("x"))
    n = 1 << a.levels
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    net = pkg.NetworkBase()
    net.load_state_dict(pkg.synthetic_state_dict("base", seed=1), strict=True)
    net.to(dev).eval()
    net.global_motion, net.ensemble_global_motion = True, False
    divisor = None if (h % 16 == 0 and w % 16 == 0) else 64
    frames = video(a.warm + a.segments + 1, h, w)
    slots = list(rt.retime_slots(range(len(frames)), fi, fo, a.levels))
    first = next(k for k, (j, _) in enumerate(slots) if j >= a.warm)          # the first output of the first timed segment
    kw = dict(divisor=divisor, pool=True, max_batch=4)
    dd = rt.Duplicates()
    retimed = lambda **over: run(rt.interpolate_video_retimed(iter(frames), net, fi, fo, levels=a.levels, **dict(kw, **over)), first)

    def plans_off():
        net._pooled_plans_on = False           # tool-only: forward_pooled on direct launches, as before it was planned
        try:
            return retimed()
        finally:
            net._pooled_plans_on = True
    modes = {
        f"{n}x": lambda: run(mf.interpolate_video_nx(iter(frames), net, factor=n, **kw), a.warm * n),
        f"{a.retime} levels={a.levels} pool=False": lambda: retimed(pool=False),
        f"{a.retime} levels={a.levels} plans off": plans_off,
        f"{a.retime} levels={a.levels}": retimed,
        f"{a.retime} levels={a.levels} +dedup": lambda: retimed(dedup=dd),
    }
    fps, ms_out, stats = {k: [] for k in modes}, {}, {k: None for k in modes}
    for _ in range(a.prime):                 # every key of the steady state recorded before anything is timed
        for fn in modes.values():
            fn()
    for _ in range(a.repeats):               # in rotation
        for name, fn in modes.items():
            before = net.plan_stats()
            ms, outs = fn()
            after = net.plan_stats()
            fps[name].append(outs / (ms * 1e-3))
            ms_out[name] = (ms, outs)
            stats[name] = {kind: {k: (stats[name][kind][k] if stats[name] else 0) + v - before[kind][k] for k, v in c.items()}
                           for kind, c in after.items()}
        assert dd.dropped == [], "the benchmark video must be free of duplicates"
    report = {}
    list(rt.interpolate_video_retimed(iter(frames), net, fi, fo, levels=a.levels, report=report, **kw))
    rows = []
    for name, t in fps.items():
        rows.append({"size": a.size, "mode": name, "fps_median": statistics.median(t), "fps_min": min(t), "fps_max": max(t), "repeats_fps": t,
                     "timed_outputs": ms_out[name][1], "plan_stats": stats[name]})
        shown = "; ".join(f"{kind} {c['eager']}e/{c['recorded']}rec/{c['replayed']}rep/{c['refused']}ref" for kind, c in stats[name].items()
                          if any(c.values()))
        print(f"{a.size:>10} {name:>34}: {rows[-1]['fps_median']:8.2f} output frames/s (min {min(t):.2f}, max {max(t):.2f} over {len(t)} repeats; "
              f"{ms_out[name][1]} outputs timed)  plans {shown or '-'}", flush=True)
    print(f"{a.retime}: {report['forwards']} forwards for {report['interpolated']} interpolated of {report['outputs']} outputs "
          f"({report['forwards'] / max(1, report['interpolated']):.2f} per interpolated frame; {n}x: {(n - 1) / (n - 1):.2f})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows, "report": report}, f, indent=1)


if __name__ == "__main__":
    main()
