"""What tools/bench_yuv.py, bench_yuv10.py and bench_yuv_window.py share: the timing of one configuration, the rotation over all of
them, and ``--baseline-lib``: the same configurations on another build of the library (the parent commit's, say), timed in the same
rotation right after the library under test -- A, B, A, B ... per repeat -- so that a ratio of medians compares two builds under
one state of the machine.  Pointing ``--lib`` and ``--baseline-lib`` at two copies of one file gives the noise floor of that ratio."""
import importlib
import statistics

import torch

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")


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


def add_library_arguments(ap):
    ap.add_argument("--lib", default=None, help="the library under test (default: the package's)")
    ap.add_argument("--baseline-lib", default=None, help="another build of the library, timed in the same rotation: rows gain over_baseline")


def libraries(a, dev):
    """-> (ops of the library under test, ops of the baseline library or None)"""
    return hip_ops.HipOps(dev, lib_path=a.lib), (hip_ops.HipOps(dev, lib_path=a.baseline_lib) if a.baseline_lib else None)


def rotation(cfg, base_cfg, repeats, iters):
    """-> (times, baseline times or None), name -> us per call of every repeat.  Every repeat visits every configuration once, the
    baseline library's twin (``base_cfg``: the same names) right after it."""
    times = {k: [] for k in cfg}
    base = {k: [] for k in cfg} if base_cfg else None
    for _ in range(repeats):
        for k in cfg:
            times[k].append(timed(cfg[k][0], iters))
            if base_cfg:
                base[k].append(timed(base_cfg[k][0], iters))
    return times, base


def against_baseline(row, times, base, k):
    """Adds the baseline's median and ``over_baseline = median(new) / median(baseline)`` to ``row``; -> the text for the table."""
    if base is None:
        return ""
    b = statistics.median(base[k])
    row.update({"baseline_us_median": b, "baseline_repeats_us": base[k], "over_baseline": statistics.median(times[k]) / b})
    return f"  baseline {b:8.2f} us: {row['over_baseline']:6.3f} x"
