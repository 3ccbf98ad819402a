"""A recorder of what ONE eager forward launches, and the cases ``tests/test_gpu_forward_trace.py`` pins with it
(``tools/record_forward_trace.py`` writes ``tests/golden/forward_trace.json`` from the same list).  The other half of
``tests/loop_trace.py``, which deliberately does not look inside ``forward``.

A trace is the list of ``[name, meta.get("bytes"), meta.get("shape")]`` of every ``HipOps._run`` call, in launch order.  Every case runs
with launch plans off (a replay does not go through ``_run``), on the synthetic weights of the tests' ``weights`` fixture and seeded
inputs of ``tests/pairs.py``.  The shapes are the smallest that still reach every branch of the forward's orchestration: the three
regimes (planes, rows under "f32", rows with plane-fed deconvs beyond 2^26 plane rows), global motion on / off / ensemble, one pair and
two, and both stages of ``forward_pooled``.
"""
import contextlib
import importlib

import torch

import pairs

pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
multiframe = importlib.import_module("atm-vfi_amd.multiframe")


@contextlib.contextmanager
def recording():
    """The trace of every ``HipOps._run`` inside the ``with``."""
    trace = []
    orig = hip_ops.HipOps._run

    def _run(self, name, meta, fn, *args):
        trace.append([name, meta.get("bytes"), meta.get("shape")])
        return orig(self, name, meta, fn, *args)
    hip_ops.HipOps._run = _run
    try:
        yield trace
    finally:
        hip_ops.HipOps._run = orig


@contextlib.contextmanager
def rows_beyond_planes(net):
    """The regime of a batch beyond 2^26 plane rows, pinned the way tests/test_gpu_e2e.py pins it: through the switch the forward reads."""
    cls = type(net)
    orig = cls._plane_convs
    cls._plane_convs = lambda self, ops: False
    try:
        yield
    finally:
        cls._plane_convs = orig


# name -> (variant, H, W, batch, global_motion, ensemble, what is special)
CASES = {
    "base_64x64_g_b1": ("base", 64, 64, 1, True, False, None),              # the single-resize branch of the global flows
    "base_160x96_nog_b2": ("base", 160, 96, 2, False, False, None),
    "lite_128x192_g_b2": ("lite", 128, 192, 2, True, False, None),
    "lite_384x576_ens_b1": ("lite", 384, 576, 1, True, True, None),
    "lite_128x192_g_b2_rows_beyond_planes": ("lite", 128, 192, 2, True, False, "mixed"),
    "base_64x64_g_b1_f32": ("base", 64, 64, 1, True, False, "f32"),
    "base_64x96_g_pooled": ("base", 64, 96, 2, True, False, "pooled"),      # 4 slots, pairs ([0, 1], [2, 3]), every slot stale
}


def network(name, dev, state_dict=None, plans=False):
    variant, _, _, _, glob, ens, special = CASES[name]
    torch.set_grad_enabled(False)
    net = (pkg.NetworkBase if variant == "base" else pkg.NetworkLite)()
    net.load_state_dict(state_dict if state_dict is not None else pkg.synthetic_state_dict(variant, seed=1), strict=True)
    net = net.to(dev).eval()
    net.global_motion, net.ensemble_global_motion = glob, ens
    net.enable_plans(plans)
    if special == "f32":
        net.set_precision("f32")
    return net


def caller(name, net, dev):
    """-> (prepare, run): ``run()`` is the case's forward on ``net`` and returns (its dict, the pool or None); ``prepare()`` goes before
    every ``run()`` and is not part of the trace (the pooled case: put the four frames again, which makes every slot stale)."""
    _, h, w, b, _, _, special = CASES[name]
    seed = 100 + list(CASES).index(name)
    if special == "pooled":
        stacked = torch.cat(pairs.smooth_pair(2, h, w, seed=seed), 0).to(dev)
        pool = multiframe.FramePool(net, h, w, 4)

        def prepare():
            for s in range(4):
                pool.put(s, stacked[s])
        return prepare, lambda: (net.forward_pooled(pool, [0, 1], [2, 3]), pool)
    im0, im1 = (t.to(dev) for t in pairs.smooth_pair(b, h, w, seed=seed))

    def run():
        if special == "mixed":
            with rows_beyond_planes(net):
                return net(im0, im1), None
        return net(im0, im1), None
    return (lambda: None), run


def trace_of(name, dev, state_dict=None):
    """The trace of one case as JSON gives it back (lists, None, numbers, strings)."""
    net = network(name, dev, state_dict)
    prepare, run = caller(name, net, dev)
    prepare()
    with recording() as trace:
        run()
    torch.cuda.synchronize()
    return [[launch, None if nbytes is None else float(nbytes), shape] for launch, nbytes, shape in trace]
