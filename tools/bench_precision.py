#!/usr/bin/env python3
"""Time the precision modes of the plane kernels (Network.set_precision: "f16x3" = three 16-bit MFMAs per product, the default; "f16" =
one) on the protocol of tools/bench_yuv_packed.py: device events, warm-ups, every column timed ``--repeats`` times IN ROTATION in one
process, median with min - max.  Three columns:

  parent f16x3   the default mode from the PARENT commit's library (``--yardstick-lib PATH``: built from a worktree of the parent and
                 loaded beside the library under test) -- the yardstick never runs from the code under test;
  f16x3          the default mode from the library under test: has to sit within the repeats' spread of the parent's on every row;
  f16            the new mode from the library under test: a strict subset of the same instruction stream, so a row on which it is
                 slower than the parent's f16x3 beyond the spread is a defect; the speed-up is reported as measured, no threshold.

Two levels.  Per launch: every distinct 3x3-plane and plane-input GEMM shape of a network_base 1088 x 1920 forward, timed INSIDE the
forward (HipOps.profile: a pair of device events around every launch, real operands, the caches as the neighbouring layers leave
them), launches of one (kernel, shape) summed; a fourth column is the A/A control -- a second model on the library under test, default mode
again: what two models of one library differ by on a row (their buffers sit elsewhere) is not a difference of code.  Whole forward: network_base at 1088 x 1920 and 544 x 960 and network_lite at 256 x 448,
single stream, launch plans on (``--iters`` replayed forwards between two events).

    python tools/bench_precision.py --yardstick-lib PATH [--repeats 5] [--iters 20] [--out profiles/precision_f16_bench.txt] [--json OUT]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pairs  # noqa: E402  (tests/pairs.py: the seeded frame pairs of the suite)
pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
COLUMNS = ("parent f16x3", "f16x3", "f16")
CONTROL = "f16x3 (2nd model)"       # per launch only: a second model on the library under test, default mode -- the A/A control
PLANE_KERNELS = ("conv3x3_planes", "linear_split", "deconv2x2_split", "conv2d_split")
NEWER = ("atmvfi_conv3p",)       # what an older build lacks; every mode calls it, so main() refuses a yardstick without it
FORWARDS = [("base", 1088, 1920), ("base", 544, 960), ("lite", 256, 448)]
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_nets(variant, dev, parent_lib, control=False):
    """One model per column, each with a backend of its own: the parent's library, and twice the library under test (``control``: a
    third time, default mode again -- what two models of ONE library differ by: buffer placement, not code)."""
    nets = {}
    for col in COLUMNS + ((CONTROL,) if control else ()):
        net = (pkg.NetworkBase if variant == "base" else pkg.NetworkLite)()
        net.load_state_dict(pkg.synthetic_state_dict(variant, seed=1), strict=True)
        net = net.to(dev).eval()
        ops = hip_ops.HipOps(dev, lib_path=parent_lib, lib_optional=NEWER) if col == "parent f16x3" else hip_ops.HipOps(dev)
        ops.gemm_workspace = net._gemm_scratch
        net.set_ops(ops)
        net.set_precision("f16" if col == "f16" else "f16x3")
        nets[col] = net
    return nets


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ({min(ts):.3f}-{max(ts):.3f})"


def verdicts(t):
    """(default within the parent's spread?, f16 not slower than the parent beyond the spread?) -- ranges of the repeats overlap /
    the f16 median is no higher than the parent's slowest repeat."""
    p, n, f = (t[c] for c in COLUMNS)
    within = min(n) <= max(p) and min(p) <= max(n)
    not_slower = statistics.median(f) <= max(p)
    return within, not_slower


def per_launch(a, dev):
    variant, H, W = FORWARDS[0]
    nets = make_nets(variant, dev, a.yardstick_lib, control=True)
    x, y = (t.to(dev) for t in pairs.random_pair(1, H, W, seed=3))
    for net in nets.values():
        net.enable_plans(False)
        for _ in range(2):
            net(x, y)
    torch.cuda.synchronize()
    times = {c: {} for c in nets}             # column -> (kernel, shape) -> [ms per repeat]
    counts, totals = {}, {c: [] for c in nets}
    for rep in range(a.repeats):
        for col, net in nets.items():
            ops = net._ops_obj
            ops.profile = []
            net(x, y)
            torch.cuda.synchronize()
            prof = [(n, m.get("shape", ""), s.elapsed_time(e)) for n, m, s, e in ops.profile]
            ops.profile = None
            acc = {}
            for n, shape, t in prof:
                if n in PLANE_KERNELS:
                    acc[(n, shape)] = acc.get((n, shape), 0.0) + t
                    if rep == 0 and col == COLUMNS[0]:
                        counts[(n, shape)] = counts.get((n, shape), 0) + 1
            for k, t in acc.items():
                times[col].setdefault(k, []).append(t)
            totals[col].append((sum(acc.values()), sum(t for _, _, t in prof)))
    say(f"--- per launch, inside a network_{variant} {H} x {W} forward (direct launches, a pair of events per launch); ms, median (min-max) of "
        f"{a.repeats} repeats in rotation; launches of one (kernel, shape) summed")
    say(f"{'kernel':16s} {'shape':26s} {'x':>2s} {'parent f16x3':>24s} {'f16x3':>24s} {'f16':>24s} {'f16x3/f16':>9s}  default within spread | f16 not slower | "
        f"{CONTROL}: within the spread of f16x3")
    rows, bad_default, bad_f16, bad_ctl = [], [], [], []
    fam = {}
    for k in times[COLUMNS[0]]:
        t = {c: times[c][k] for c in nets}
        within, not_slower = verdicts(t)
        ctl = min(t[CONTROL]) <= max(t["f16x3"]) and min(t["f16x3"]) <= max(t[CONTROL])
        sp = statistics.median(t["parent f16x3"]) / statistics.median(t["f16"])
        say(f"{k[0]:16s} {k[1]:26s} {counts[k]:2d} {fmt(t['parent f16x3']):>24s} {fmt(t['f16x3']):>24s} {fmt(t['f16']):>24s} {sp:9.2f}  "
            f"{'yes' if within else 'NO':>3s} | {'yes' if not_slower else 'NO':>3s} | {fmt(t[CONTROL])} {'yes' if ctl else 'NO'}")
        rows.append({"kernel": k[0], "shape": k[1], "launches": counts[k], "ms": t, "speedup": sp, "default_within_spread": within,
                     "f16_not_slower": not_slower, "control_within_spread": ctl})
        if not ctl:
            bad_ctl.append(k)
        if not within:
            bad_default.append(k)
        if not not_slower:
            bad_f16.append(k)
        f = fam.setdefault(k[0], {c: [0.0] * a.repeats for c in COLUMNS})
        for c in COLUMNS:
            f[c] = [u + v for u, v in zip(f[c], t[c])]
    say("--- by kernel family (sums of the rows above)")
    for n, t in fam.items():
        say(f"{n:16s} {'':26s}    {fmt(t['parent f16x3']):>24s} {fmt(t['f16x3']):>24s} {fmt(t['f16']):>24s} "
            f"{statistics.median(t['parent f16x3']) / statistics.median(t['f16']):9.2f}")
    for c in nets:
        say(f"{c:>18s}: plane kernels {statistics.median([p for p, _ in totals[c]]):7.3f} ms of {statistics.median([s for _, s in totals[c]]):7.3f} ms "
            "(sum of all launches of the forward)")
    say(f"default path: {'every row within the spread of the parent' if not bad_default else 'OUTSIDE the spread on ' + '; '.join(map(str, bad_default))}")
    say(f"f16: {'no row slower than the parent f16x3 beyond the spread' if not bad_f16 else 'SLOWER than the parent f16x3 on ' + '; '.join(map(str, bad_f16))}")
    say(f"A/A control (two models of the library under test, both f16x3): {len(bad_ctl)} of {len(rows)} rows outside each other's spread"
        + (": " + "; ".join(map(str, bad_ctl)) if bad_ctl else ""))
    for net in nets.values():
        net.release_workspace()
    del nets
    torch.cuda.empty_cache()
    return rows


def forwards(a, dev):
    say(f"--- whole forward, single stream, launch plans on: ms per forward, {a.iters} replayed forwards between two events after 6 warm-up "
        f"forwards, median (min-max) of {a.repeats} repeats in rotation")
    say(f"{'model':24s} {'parent f16x3':>24s} {'f16x3':>24s} {'f16':>24s} {'f16x3/f16':>9s}  default within spread | f16 not slower")
    rows = []
    for variant, H, W in FORWARDS:
        nets = make_nets(variant, dev, a.yardstick_lib)
        x, y = (t.to(dev) for t in pairs.random_pair(1, H, W, seed=3))
        for col, net in nets.items():
            net.enable_plans(True)
            for _ in range(6):
                net(x, y)
            st = net.plan_stats()["forward"]
            if not st["replayed"]:
                say(f"  ({col}: the forward is not replayed from a plan: {st})")
        torch.cuda.synchronize()
        t = {c: [] for c in COLUMNS}
        for rep in range(a.repeats):
            for col, net in nets.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    net(x, y)
                e.record()
                torch.cuda.synchronize()
                t[col].append(s.elapsed_time(e) / a.iters)
        within, not_slower = verdicts(t)
        sp = statistics.median(t["parent f16x3"]) / statistics.median(t["f16"])
        say(f"network_{variant:5s} {H:4d} x {W:4d}  {fmt(t['parent f16x3']):>24s} {fmt(t['f16x3']):>24s} {fmt(t['f16']):>24s} {sp:9.2f}  "
            f"{'yes' if within else 'NO':>3s} | {'yes' if not_slower else 'NO'}")
        rows.append({"model": variant, "size": [H, W], "ms": t, "speedup": sp, "default_within_spread": within, "f16_not_slower": not_slower})
        for net in nets.values():
            net.release_workspace()
        del nets
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--yardstick-lib", default=None, help="the parent commit's build of the library: runs the 'parent f16x3' column")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/precision_f16_bench.txt)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not a.yardstick_lib:
        sys.exit("bench_precision: --yardstick-lib PATH is required (the parent commit's build: the yardstick never runs from the code under test)")
    if a.repeats < 3:
        sys.exit("bench_precision: at least 3 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_precision: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    parent = hip_ops.load_library(a.yardstick_lib, NEWER)
    missing = [name for name in NEWER if not hasattr(parent, name)]
    if missing:
        sys.exit(f"bench_precision: {a.yardstick_lib} does not export {', '.join(missing)}: the 3x3 plane kernel is reached through it in every mode, "
                 "so the yardstick has to be a build of the commit that introduced it (ABI 0.28) or a later one")
    pv = parent.atmvfi_version()
    nv = hip_ops.load_library().atmvfi_version()
    say(f"device {torch.cuda.get_device_name(0)}; parent library ABI 0.{(pv >> 8) & 255} ({os.path.basename(a.yardstick_lib)}), library under test "
        f"ABI 0.{(nv >> 8) & 255}; stress weights (seed 1), random frame pair (seed 3)")
    out = {"per_launch": per_launch(a, dev), "forward": forwards(a, dev)}
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters, **out}, f, indent=1)


if __name__ == "__main__":
    main()
