"""GPU: scene-cut detection on the device (csrc/scene.hip atmvfi_frame_signature, the ``scene=`` argument of the video loops): the
signature kernel against the loop model of tests/cpu_scene.py bit for bit, and two-shot videos through the HIP loops -- the frames of
A ++ B with the cut detected are the frames of A alone, copies of the two originals at the cut, and the frames of B alone."""
import importlib

import numpy as np
import pytest
import torch

import cpu_scene as C
import pairs

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    torch.set_grad_enabled(False)
    out = {}
    for v, cls in (("lite", pkg.NetworkLite), ("base", pkg.NetworkBase)):
        net = cls()
        net.load_state_dict(pkg.synthetic_state_dict(v, seed=1), strict=True)
        out[v] = net.to(dev).eval()
    return out


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


# ------------------------------------------------------------------------------------------------ the kernel
def picture(h, w, seed):
    """uint8 [h,w,3]: smooth structure (flat regions put whole waves into one bin) plus noise (every bin and byte value occurs)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    f = np.stack([127 + 120 * np.sin(yy / (7.0 + 3 * c) + xx / (11.0 - 2 * c) + c) for c in range(3)], -1)
    f += rng.normal(0, 12, f.shape).astype(np.float32)
    f[: h // 5] = rng.integers(0, 256, 3)                        # a flat band
    return np.clip(np.round(f), 0, 255).astype(np.uint8)


CASES = [            # H, W, window (y0, x0, h, w) or None
    (16, 16, None),
    (64, 96, (3, 5, 33, 47)),              # an odd window at an odd x0: general path
    (64, 96, (4, 8, 32, 44)),              # aligned path, 11 lanes wide, 2 rows per cell
    (480, 832, None),
    (1080, 1920, None),
    (1080, 1920, (180, 320, 720, 1280)),   # a centre crop, aligned
    (1080, 1920, (181, 321, 719, 1278)),   # ... and not
    (2160, 4096, None),
]


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,win", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_frame_signature_is_the_model(ops, dev, H, W, win, bgr):
    frame = picture(H, W, seed=H + W)
    y0, x0, h, w = win or (0, 0, H, W)
    want = C.signature_model(frame, y0, x0, h, w, bgr)
    src = torch.from_numpy(frame).to(dev)
    out = torch.full((288,), -0x12345678, dtype=torch.int32, device=dev)         # poisoned: the call writes every word
    ret = ops.frame_signature(src, y0, x0, h, w, bgr=bgr, out=out)
    assert ret is out
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    again = ops.frame_signature(src, y0, x0, h, w, bgr=bgr).cpu().numpy()           # a second call, a fresh output: identical bits
    assert np.array_equal(again, got)
    assert np.array_equal(scene.signature_numpy(frame, (y0, x0, h, w), bgr=bgr), got)
    # the same pixels behind a pointer offset by one byte: the general path gives the same bits
    buf = torch.empty(H * W * 3 + 1, dtype=torch.uint8, device=dev)
    shifted = buf[1:].view(H, W, 3)
    shifted.copy_(src)
    assert shifted.data_ptr() % 4 != src.data_ptr() % 4
    out.fill_(-1)
    ops.frame_signature(shifted, y0, x0, h, w, bgr=bgr, out=out, workspace=ops.frame_signature_workspace(h, w))
    assert np.array_equal(out.cpu().numpy(), want)


def test_frame_signature_defaults_and_refusals(ops, dev):
    frame = picture(40, 52, seed=3)
    src = torch.from_numpy(frame).to(dev)
    assert np.array_equal(ops.frame_signature(src).cpu().numpy(), C.signature_model(frame))
    assert np.array_equal(ops.frame_signature(src, 2, 6, bgr=True).cpu().numpy(), C.signature_model(frame, 2, 6, 38, 46, True))
    with pytest.raises(ValueError):
        ops.frame_signature(src.float())
    with pytest.raises(ValueError):
        ops.frame_signature(src, out=torch.zeros(287, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.frame_signature(src, h=15)
    with pytest.raises(RuntimeError, match="window outside the frame"):
        ops.frame_signature(src, 1, 0, 40, 52)
    with pytest.raises(RuntimeError, match="workspace of"):
        ops.frame_signature(src, workspace=torch.zeros(8, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------ the loops
def count_forwards(monkeypatch, net):
    """Counting wrappers around ``forward`` / ``forward_pooled`` of the model's class (replicas included)."""
    calls = {"forward": 0, "forward_pooled": 0}
    for name in calls:
        klass = next(k for k in type(net).__mro__ if name in k.__dict__)

        def wrapper(self, *a, _orig=klass.__dict__[name], _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(klass, name, wrapper)
    return calls


def same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), k


NX_CASES = [          # variant, H, W, factor, pool, tta, time_interval, crop, divisor
    ("lite", 64, 96, 4, True, False, 1, None, 32),
    ("lite", 64, 96, 4, False, False, 1, None, 32),
    ("lite", 64, 96, 4, True, True, 1, None, 32),
    ("lite", 64, 96, 4, False, True, 1, None, 32),
    ("lite", 64, 96, 8, True, False, 1, None, 32),
    ("lite", 64, 96, 8, False, False, 1, None, 32),
    ("lite", 64, 96, 8, True, True, 1, None, 32),
    ("lite", 64, 96, 8, False, True, 1, None, 32),
    ("lite", 80, 112, 4, True, False, 2, (64, 96), 32),
    ("base", 192, 320, 4, True, False, 1, None, 64),
]


@pytest.mark.parametrize("variant,H,W,factor,pool,tta,s,crop,divisor", NX_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_two_shot_video_through_interpolate_video_nx(nets, dev, monkeypatch, variant, H, W, factor, pool, tta, s, crop, divisor):
    net = nets[variant]
    net.global_motion, net.ensemble_global_motion = True, False
    A = C.shot(2 * s + 1, H, W, seed=11, tone=60)
    B = C.shot(2 * s + 1, H, W, seed=12, tone=190)
    kw = dict(factor=factor, time_interval=s, crop=crop, isBGR=True, divisor=divisor, tta=tta, max_batch=4, pool=pool)
    nx = lambda shot, **more: list(host_io.interpolate_video_nx(iter(shot), net, **kw, **more))
    y0, x0, h, w = mf.centre_window(H, W, crop)
    crop_of = lambda f: f[y0:y0 + h, x0:x0 + w]
    calls = count_forwards(monkeypatch, net)
    a_alone, n_a = nx(A), dict(calls)
    b_alone = nx(B)
    n_ab = {k: calls[k] for k in calls}
    sc = scene.SceneCuts()
    # frames between segment ends are consumed and dropped: s - 1 fillers behind A put B's frames on segment ends again, so the video's
    # segments are A's, the segment (A_last, B_0), and B's
    got = nx(A + [A[-1]] * (s - 1) + B, scene=sc)
    n_cut = {k: calls[k] - n_ab[k] for k in calls}
    want = a_alone + [crop_of(A[-1])] * (factor // 2) + [crop_of(B[0])] * (factor // 2 - 1) + b_alone
    same(got, want)
    assert sc.cuts == [2] and len(sc.stats) == 5
    # no forward ran for the cut segment: the video cost what the two shots cost
    assert n_cut == n_ab and sum(n_cut.values()) > 0 and n_a["forward_pooled" if pool else "forward"] > 0
    # the segment after the cut is B's first segment (position N's frame and tokens became position 0 across the cut)
    same(got[3 * factor:4 * factor + 1], b_alone[:factor + 1])
    # the host model of the signatures saw what the device computed
    sigs = [scene.signature_numpy(f, (y0, x0, h, w), bgr=True) for f in (A[-1], B[0])]
    assert scene.cut_statistics(sigs[0], sigs[1], h, w) == sc.stats[2]


def test_one_frame_shot_and_edge_cuts_on_the_device(nets, dev, monkeypatch):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    A, B = C.shot(3, 64, 96, seed=11, tone=60), C.shot(3, 64, 96, seed=12, tone=190)
    X = C.shot(1, 64, 96, seed=13, tone=120, span=20)
    for pool in (True, False):
        kw = dict(factor=4, divisor=32, pool=pool)
        nx = lambda shot, **more: list(host_io.interpolate_video_nx(iter(shot), net, **kw, **more))
        fill = lambda p, q: [p, p, q]
        a_alone, b_alone = nx(A), nx(B)
        sc = scene.SceneCuts()
        same(nx(A + X + B, scene=sc), a_alone + fill(A[-1], X[0]) + X + fill(X[0], B[0]) + b_alone)          # two cuts in a row
        assert sc.cuts == [2, 3]
        same(nx(X + A + X, scene=sc), X + fill(X[0], A[0]) + a_alone + fill(A[-1], X[0]) + X)                # first and last segment
        assert sc.cuts == [0, 3]
        calls = count_forwards(monkeypatch, net)
        same(nx([A[0], B[0]], scene=sc), [A[0]] + fill(A[0], B[0]) + [B[0]])                                 # nothing but a cut
        assert sc.cuts == [0] and sum(calls.values()) == 0
        monkeypatch.undo()


@pytest.mark.parametrize("streams", [1, 2])
def test_two_shot_video_through_interpolate_video_2x(nets, dev, monkeypatch, streams):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    A, B = C.shot(4, 64, 96, seed=11, tone=60), C.shot(3, 64, 96, seed=12, tone=190)
    X = C.shot(1, 64, 96, seed=13, tone=120, span=20)
    two = lambda shot, **more: list(host_io.interpolate_video_2x(iter(shot), net, isBGR=True, divisor=32, streams=streams, **more))
    calls = count_forwards(monkeypatch, net)
    a_alone, b_alone = two(A), two(B)
    n_ab = calls["forward"]
    assert n_ab >= 5                                             # 3 + 2 pairs
    sc = scene.SceneCuts()
    got = two(A + B, scene=sc)
    same(got, a_alone + [A[-1]] + b_alone)
    assert sc.cuts == [3] and len(sc.stats) == 6 and calls["forward"] == 2 * n_ab
    assert got[7] is not A[-1]
    same(two(A + X + B, scene=sc), a_alone + [A[-1]] + X + [X[0]] + b_alone)             # a one-frame shot
    assert sc.cuts == [3, 4]
    same(two(X + A + X, scene=sc), X + [X[0]] + a_alone + [A[-1]] + X)                   # the first and the last pair
    assert sc.cuts == [0, 4]
    # pairs that do not chain (the first frame is not the previous pair's second): both signatures are computed
    pipe = host_io.FramePipeline(net, 64, 96, isBGR=True, divisor=32, depth=2, streams=streams, scene=sc)
    out = list(pipe.run([(A[0], B[0]), (A[1], A[2]), (A[2], X[0])]))
    assert sc.cuts == [0, 2] and np.array_equal(out[0], A[0]) and np.array_equal(out[2], A[2])
    same(out[1:2], a_alone[3:4])


def test_cut_free_video_is_unchanged(nets, dev):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    frames = pairs.uint8_video(5, 80, 112, seed=4)
    for kw in (dict(factor=4, pool=True), dict(factor=4, pool=False, tta=True), dict(factor=8, pool=True, time_interval=2, crop=(64, 96))):
        sc = scene.SceneCuts()
        want = list(host_io.interpolate_video_nx(iter(frames), net, divisor=32, scene=None, **kw))
        same(list(host_io.interpolate_video_nx(iter(frames), net, divisor=32, scene=sc, **kw)), want)
        assert sc.cuts == [] and len(sc.stats) == (len(frames) - 1) // kw.get("time_interval", 1)
        y0, x0, h, w = mf.centre_window(80, 112, kw.get("crop"))
        s = kw.get("time_interval", 1)
        sig = [scene.signature_numpy(f, (y0, x0, h, w), bgr=True) for f in frames]
        assert sc.stats == [scene.cut_statistics(sig[i], sig[i + s], h, w) for i in range(0, len(frames) - s, s)]
    for streams in (1, 2):
        sc = scene.SceneCuts()
        want = list(host_io.interpolate_video_2x(iter(frames), net, divisor=32, streams=streams))
        same(list(host_io.interpolate_video_2x(iter(frames), net, divisor=32, streams=streams, scene=sc)), want)
        assert sc.cuts == [] and len(sc.stats) == 4
