"""A recorder of what the video loops launch, and the cases ``tests/test_gpu_loop_trace.py`` pins with it (``tools/record_loop_trace.py``
writes ``tests/golden/loop_trace.json`` from the same list).

A trace is a list of entries in launch order:

* ``["forward" | "forward_pooled", batch, Hp, Wp]`` for a call of the model; the ``HipOps._run`` calls inside it are not recorded (a
  launch plan, recorded on the third call of a key, replays them without ``_run``: the trace must not see the switch);
* ``[name, meta.get("bytes"), default]`` for every other ``HipOps._run``: the launch's name, its byte count where it states one, and
  whether the current stream is the device's default compute stream (False: the copy stream of the uploader);
* ``[name, None, default]`` for a launch that does not go through ``_run`` (signature, difference, borders, compose, the shutter's two
  kernels): their wrappers hand the library's return code to ``HipOps._check`` with the launch's name, and that call is recorded.
"""
import contextlib
import importlib

import numpy as np
import torch

import cpu_active
import cpu_scene
import pairs

pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
host_io = importlib.import_module("atm-vfi_amd.host_io")
scene = importlib.import_module("atm-vfi_amd.scene")
active = importlib.import_module("atm-vfi_amd.active")
rt = importlib.import_module("atm-vfi_amd.retime")
shutter = importlib.import_module("atm-vfi_amd.shutter")
yuv = importlib.import_module("atm-vfi_amd.yuv")


@contextlib.contextmanager
def recording(net):
    """The trace of everything run inside the ``with`` on ``net`` and its ``HipOps``."""
    trace, depth, saved = [], [0], []
    dev = next(net.parameters()).device

    def patch(klass, name, make):
        saved.append((klass, name, klass.__dict__[name]))
        setattr(klass, name, make(klass.__dict__[name]))

    def forward_of(name):
        def make(orig):
            def wrapper(self, *a, **kw):
                if depth[0] == 0:
                    trace.append([name, len(a[1]), a[0].hp, a[0].wp] if name == "forward_pooled" else [name, int(a[0].shape[0]), *a[0].shape[-2:]])
                depth[0] += 1
                try:
                    return orig(self, *a, **kw)
                finally:
                    depth[0] -= 1
            return wrapper
        return make

    def on_default():
        return torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)

    def make_run(orig):
        def _run(self, name, meta, fn, *args):
            if depth[0] == 0:
                trace.append([name, meta.get("bytes"), on_default()])
            depth[0] += 1                            # (its own ``_check`` is not a second entry)
            try:
                return orig(self, name, meta, fn, *args)
            finally:
                depth[0] -= 1
        return _run

    def make_check(orig):
        def _check(self, rc, name):
            if depth[0] == 0:
                trace.append([name, None, on_default()])
            return orig(self, rc, name)
        return _check
    for name in ("forward", "forward_pooled"):
        patch(next(k for k in type(net).__mro__ if name in k.__dict__), name, forward_of(name))
    patch(hip_ops.HipOps, "_run", make_run)
    patch(hip_ops.HipOps, "_check", make_check)
    try:
        yield trace
    finally:
        for klass, name, orig in reversed(saved):
            setattr(klass, name, orig)


def lite_network(dev):
    torch.set_grad_enabled(False)
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    net = net.to(dev).eval()
    net.global_motion, net.ensemble_global_motion = True, False
    return net


# ------------------------------------------------------------------------------------------------ the cases
H, W = 64, 96
HL, WL, ROWS, WIN = 128, 96, (32, 96), (32, 0, 64, 96)


def _video(n):
    return pairs.uint8_video(n, H, W, seed=5)


def _two_shots():
    return cpu_scene.shot(3, H, W, seed=11, tone=60) + cpu_scene.shot(2, H, W, seed=12, tone=190)


def _repeats():
    v = _video(4)
    return [v[0], v[0].copy(), v[1], v[2], v[2].copy(), v[2].copy(), v[3]]


def _i420(frames, fmt):
    if fmt.depth == 8:
        return [yuv.encode_numpy(f, fmt) for f in frames]
    return [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt) for f in frames]


def _letterboxed(bar_content=False):
    video = [f.copy() for f in cpu_active.letterboxed(5, HL, WL, ROWS, seed=21, tone=150)[0]]
    if bar_content:
        video[3][5, 7] = 255
    return video


def _nx(frames, **kw):
    return lambda net: list(host_io.interpolate_video_nx(iter(frames()), net, **dict(dict(isBGR=True, divisor=32), **kw)))


def _retimed(frames, fi, fo, **kw):
    return lambda net: list(host_io.interpolate_video_retimed(iter(frames()), net, fi, fo, **dict(dict(isBGR=True, divisor=32, levels=3), **kw)))


F8, F10 = yuv.Format(H, W), yuv.Format(H, W, depth=10)

CASES = {
    "nx_4x_pool": _nx(lambda: _video(4), factor=4, pool=True, max_batch=4),
    "nx_8x_plain_tta": _nx(lambda: _video(4), factor=8, pool=False, tta=True, max_batch=2),
    "nx_crop_scene": _nx(_two_shots, factor=4, crop=(48, 64), scene=scene.SceneCuts()),
    "nx_time_interval_2": _nx(lambda: _video(7), factor=4, time_interval=2),
    "nx_i420": _nx(lambda: _i420(_video(4), F8), factor=4, pixfmt=F8),
    "nx_i420p10_keep_tta": _nx(lambda: _i420(_video(4), F10), factor=4, pixfmt=F10, keep_depth=True, tta=True),
    "nx_active": _nx(_letterboxed, factor=4, active=active.ActiveArea()),
    "nx_active_fallback": _nx(lambda: _letterboxed(True), factor=4, active=active.ActiveArea(probe=2)),
    "nx_active_fixed": _nx(lambda: _letterboxed()[:4], factor=4, active=WIN),
    "rt_24_60_pool": _retimed(lambda: _video(4), 24, 60, pool=True),
    # (ten segments, of which two run a forward: a segment without an interpolated output only uploads)
    "rt_60_24": _retimed(lambda: _video(11), 60, 24),
    "rt_dedup": _retimed(_repeats, 24, 60, dedup=rt.Duplicates(max_run=2)),
    "rt_scene": _retimed(_two_shots, 24, 60, scene=scene.SceneCuts()),
    "rt_shutter_180_linear": _retimed(lambda: _video(4), 24, 60, shutter=shutter.Shutter(180, "linear")),
    "rt_shutter_360_i420": _retimed(lambda: _i420(_video(4), F8), 24, 60, shutter=360, pixfmt=F8),
    "rt_shutter_tta": _retimed(lambda: _video(4), 24, 60, shutter=180, tta=True),
    "rt_shutter_dedup": _retimed(_repeats, 24, 60, shutter=180, dedup=rt.Duplicates(max_run=2)),
}


def trace_of(net, case):
    """The trace of one case as JSON gives it back (lists, None, numbers)."""
    with recording(net) as trace:
        CASES[case](net)
    plain = lambda v: float(v) if isinstance(v, (float, np.floating)) else int(v) if isinstance(v, np.integer) else v
    return [[plain(v) for v in e] for e in trace]
