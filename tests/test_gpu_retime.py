"""GPU: frame-rate conversion on the device (csrc/framediff.hip atmvfi_frame_difference; atm-vfi_amd/retime.py): the difference kernel
against the pixel-loop model of tests/cpu_framediff.py bit for bit, and the retimed loop against the frames of the same (segment,
position) of the full 8x recursion -- sparse schedule, pool, scene cuts, dropped duplicates, I420 frames, TTA."""
import importlib

import numpy as np
import pytest
import torch

import cpu_framediff as D
import cpu_scene as C
import pairs

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")
rt = importlib.import_module("atm-vfi_amd.retime")
yuv = importlib.import_module("atm-vfi_amd.yuv")


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
def picture_pair(h, w, seed):
    """Two uint8 [h,w,3] frames: noise over smooth structure; the second equals the first in a third of the pixels, differs by a little
    in another third and by anything in the rest (zero, small and large differences in every cell)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    f = np.stack([127 + 100 * np.sin(yy / (7.0 + 3 * c) + xx / (11.0 - 2 * c) + c) for c in range(3)], -1)
    a = np.clip(np.round(f + rng.normal(0, 12, f.shape)), 0, 255).astype(np.uint8)
    kind = rng.integers(0, 3, (h, w, 1))
    near = np.clip(a.astype(np.int64) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    b = np.where(kind == 0, a, np.where(kind == 1, near, rng.integers(0, 256, a.shape).astype(np.uint8)))
    return a, np.ascontiguousarray(b.astype(np.uint8))


def shifted_copy(t, dev):
    """the same pixels behind a pointer offset by one byte"""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=dev)
    s = buf[1:].view(t.shape)
    s.copy_(t)
    assert s.data_ptr() % 4 != t.data_ptr() % 4
    return s


CASES = [            # H, W, window (y0, x0, h, w) or None
    (16, 16, None),
    (64, 96, (3, 5, 33, 47)),              # an odd window at an odd x0: general path
    (64, 96, (4, 8, 32, 44)),              # aligned path, 11 lanes wide, 2 rows per cell
    (40, 1100, None),                      # crosses a 1024-pixel column tile
]


@pytest.fixture(scope="module")
def models():
    """the loop model of every case and channel order, computed once"""
    out = {}
    for H, W, win in CASES:
        a, b = picture_pair(H, W, seed=H + W)
        y0, x0, h, w = win or (0, 0, H, W)
        for bgr in (False, True):
            out[(H, W, win, bgr)] = (a, b, D.difference_model(a, b, y0, x0, h, w, bgr))
    return out


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,win", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_frame_difference_is_the_model(ops, dev, models, H, W, win, bgr):
    a, b, want = models[(H, W, win, bgr)]
    y0, x0, h, w = win or (0, 0, H, W)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.full((258,), -0x12345678, dtype=torch.int32, device=dev)           # poisoned: the call writes every word
    ret = ops.frame_difference(ta, tb, y0, x0, h, w, bgr=bgr, out=out)
    assert ret is out
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(ops.frame_difference(tb, ta, y0, x0, h, w, bgr=bgr).cpu().numpy(), want)      # a fresh output; symmetric
    assert np.array_equal(rt.difference_numpy(a, b, (y0, x0, h, w), bgr=bgr), got)
    # either source behind a pointer offset by one byte: the byte path gives the same bits
    ws = ops.frame_difference_workspace(h, w)
    for sa, sb in ((shifted_copy(ta, dev), tb), (ta, shifted_copy(tb, dev))):
        out.fill_(-1)
        ops.frame_difference(sa, sb, y0, x0, h, w, bgr=bgr, out=out, workspace=ws)
        assert np.array_equal(out.cpu().numpy(), want)
    # identical frames: all zeros, whatever the words held before
    out.fill_(0x7fffffff)
    ops.frame_difference(ta, ta.clone(), y0, x0, h, w, bgr=bgr, out=out)
    assert not out.cpu().numpy().any()


@pytest.mark.parametrize("H,W,win", CASES[:3], ids=lambda v: str(v).replace(" ", ""))
def test_one_differing_pixel_in_each_corner(ops, dev, H, W, win):
    a, _ = picture_pair(H, W, seed=1)
    a[..., 1] = np.minimum(a[..., 1], 150)                            # room for + 100 in green
    y0, x0, h, w = win or (0, 0, H, W)
    ta = torch.from_numpy(a).to(dev)
    for (r, c), cell in (((0, 0), 0), ((0, w - 1), 15), ((h - 1, 0), 240), ((h - 1, w - 1), 255)):
        b = a.copy()
        b[y0 + r, x0 + c, 1] += 100
        for rr, cc in ((y0 - 1, x0 + c), (y0 + h, x0 + c), (y0 + r, x0 - 1), (y0 + r, x0 + w)):      # just outside: must not count
            if 0 <= rr < H and 0 <= cc < W:
                b[rr, cc] = 255 - b[rr, cc]
        got = ops.frame_difference(ta, torch.from_numpy(b).to(dev), y0, x0, h, w, bgr=True).cpu().numpy()
        d = abs(D.luma_of(a[y0 + r, x0 + c], True) - D.luma_of(b[y0 + r, x0 + c], True))
        assert d in (58, 59)                                          # 150 * 100 / 256, rounding either way
        want = np.zeros(258, np.int32)
        want[cell], want[256], want[257] = d, d, 1
        assert np.array_equal(got, want), ((r, c), np.flatnonzero(got != want)[:8])


def test_frame_difference_defaults_and_refusals(ops, dev):
    a, b = picture_pair(40, 52, seed=3)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert np.array_equal(ops.frame_difference(ta, tb).cpu().numpy(), D.difference_model(a, b, bgr=True))           # whole frame, BGR
    assert np.array_equal(ops.frame_difference(ta, tb, 2, 6, bgr=False).cpu().numpy(), D.difference_model(a, b, 2, 6, 38, 46, False))
    with pytest.raises(ValueError):
        ops.frame_difference(ta.float(), tb)
    with pytest.raises(ValueError):
        ops.frame_difference(ta, tb[:, :40].contiguous())
    with pytest.raises(ValueError):
        ops.frame_difference(ta, tb, out=torch.zeros(257, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.frame_difference(ta, tb, h=15)
    with pytest.raises(RuntimeError, match="window outside the frame"):
        ops.frame_difference(ta, tb, 1, 0, 40, 52)
    with pytest.raises(RuntimeError, match="workspace of"):
        ops.frame_difference(ta, tb, workspace=torch.zeros(8, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------ the loop
H, W = 64, 96
KW = dict(isBGR=True, divisor=32)


def count_forwards(monkeypatch, net):
    """Counting wrappers around ``forward`` / ``forward_pooled`` of the model's class."""
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
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError(f"frame {k}: first difference at {tuple(at)}: {g[tuple(at)]} != {w[tuple(at)]} ({np.count_nonzero(g != w)} elements)")


def lite(nets):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    return net


@pytest.fixture(scope="module")
def video():
    return pairs.uint8_video(7, H, W, seed=5)


@pytest.fixture(scope="module")
def full8(nets, video):
    """the 8x recursion of the video, one pair per forward, no pool: frame 8 j + p is position p of segment j.  Computed once."""
    return list(host_io.interpolate_video_nx(iter(video), lite(nets), factor=8, pool=False, max_batch=1, **KW))


def retimed(net, frames, fi, fo, **kw):
    return list(host_io.interpolate_video_retimed(iter(frames), net, fi, fo, **dict(KW, **kw)))


def test_eight_times_the_rate_is_the_8x_loop(nets, video, full8):
    net = lite(nets)
    keep = net.max_workspaces
    got = retimed(net, video, 1, 8, levels=3, pool=False, max_batch=1)
    assert net.max_workspaces == keep
    same(got, full8)
    assert all(got[8 * i] is video[i] for i in range(7))              # originals: the caller's arrays


@pytest.mark.parametrize("pool", [False, True])
def test_24_to_60_shows_the_frames_of_the_8x_loop(nets, video, full8, monkeypatch, pool):
    net = lite(nets)
    calls = count_forwards(monkeypatch, net)
    report = {}
    got = retimed(net, video, 24, 60, levels=3, pool=pool, max_batch=1, report=report)
    slots = list(rt.retime_slots(range(7), 24, 60, 3))
    assert len(got) == len(slots) == 16
    # pool=True: forward_pooled's bit-identity with forward, on the batches of one pair that both runs use
    same(got, [full8[8 * j + p] for j, p in slots])
    n_int = sum(0 < p < 8 for _, p in slots)
    assert n_int == 12 and report == {"outputs": 16, "interpolated": 12, "forwards": 24}
    assert calls["forward_pooled" if pool else "forward"] == 24 == 2 * n_int                      # 2 per interpolated frame
    assert pool or calls["forward_pooled"] == 0


def test_pooled_equals_plain_with_the_default_batches(nets, video):
    net = lite(nets)
    keep = net.max_workspaces
    for fi, fo, levels in ((24, 60, 3), (25, 60, 4)):
        same(retimed(net, video, fi, fo, levels=levels, pool=True), retimed(net, video, fi, fo, levels=levels, pool=False))
    assert net.max_workspaces == keep


def test_60_to_24_runs_five_forwards_for_25_frames(nets, monkeypatch):
    net = lite(nets)
    frames = pairs.uint8_video(25, H, W, seed=6)
    calls = count_forwards(monkeypatch, net)
    got = retimed(net, frames, 60, 24, levels=3, pool=True)
    slots = list(rt.retime_slots(range(25), 60, 24, 3))
    assert len(got) == len(slots) == 10 and sum(calls.values()) == 5
    for k, (j, p) in enumerate(slots):
        if p == 0:
            assert got[k] is frames[j], k
    monkeypatch.undo()
    mids = [k for k, (_, p) in enumerate(slots) if p == 4]
    j = slots[mids[0]][0]
    same([got[mids[0]]], list(host_io.interpolate_video_nx(iter(frames[j:j + 2]), net, factor=2, pool=True, **KW))[1:2])


def test_a_cut_segment_is_copies_and_runs_no_forward(nets, monkeypatch):
    net = lite(nets)
    A, B = C.shot(3, H, W, seed=11, tone=60), C.shot(3, H, W, seed=12, tone=190)
    shots = A + B
    free = retimed(net, shots, 24, 60, levels=3, pool=True, max_batch=1)
    calls = count_forwards(monkeypatch, net)
    sc = scene.SceneCuts()
    got = retimed(net, shots, 24, 60, levels=3, pool=True, max_batch=1, scene=sc)
    slots = list(rt.retime_slots(range(6), 24, 60, 3))
    assert sc.cuts == [2] and len(sc.stats) == 5 and len(got) == len(slots) == 13
    in_cut = [(k, p) for k, (j, p) in enumerate(slots) if j == 2]
    assert [p for _, p in in_cut] == [0, 3, 6]
    for k, (j, p) in enumerate(slots):
        if j != 2:
            assert np.array_equal(got[k], free[k]), k                # the segment behind the cut starts from position N's frame
    assert got[in_cut[0][0]] is shots[2]
    for k, p in in_cut[1:]:
        src = shots[2] if p <= 4 else shots[3]
        assert np.array_equal(got[k], src) and got[k] is not src, (k, p)
    assert sum(calls.values()) == 20 - 4                              # the cut segment's four nodes never ran
    sig = [scene.signature_numpy(f, (0, 0, H, W), bgr=True) for f in shots[2:4]]
    assert scene.cut_statistics(sig[0], sig[1], H, W) == sc.stats[2]


def test_duplicates_are_dropped_on_the_device(nets, monkeypatch):
    net = lite(nets)
    A, B, Cc = (C.shot(1, H, W, seed=30 + k, tone=tone)[0] for k, tone in enumerate((60, 120, 180)))
    video = [A, D.primed(A, 1), B, D.primed(B, 2), Cc]
    for pool in (True, False):
        dd = rt.Duplicates()
        calls = count_forwards(monkeypatch, net)
        got = retimed(net, video, 24, 24, levels=3, pool=pool, dedup=dd)
        assert dd.dropped == [1, 3] and sum(calls.values()) == 2
        monkeypatch.undo()
        same(got, retimed(net, [A, B, Cc], 12, 24, levels=3, pool=pool))
        assert got[0] is A and got[2] is B and got[4] is Cc
        # the host model of the differences saw what the device computed
        assert dd.stats == [rt.duplicate_statistics(D.difference_fast(video[i - 1], video[i], bgr=True), H, W) for i in range(1, 5)]
    # more frames than upload slots, duplicates in runs, a crop window, a duplicate as the last frame, 24 -> 60
    rng_video = pairs.uint8_video(4, 80, 112, seed=8)                 # fresh grain of +-10 on every frame: no duplicates of each other
    long = []
    for k, f in enumerate(rng_video):
        long += [f] + [D.primed(f, 10 * k + r) for r in range(k % 3 + 1)]
    dd = rt.Duplicates(max_run=2)
    got = retimed(net, long, 24, 60, levels=3, dedup=dd, crop=(64, 96), pool=False, max_batch=1)
    y0, x0, h, w = mf.centre_window(80, 112, (64, 96))
    model = rt.Duplicates(max_run=2)
    for i in range(1, len(long)):
        model.judge(D.difference_fast(long[i - 1], long[i], y0, x0, h, w, True), h, w)
    model.finish()
    assert dd.stats == model.stats and dd.dropped == model.dropped and len(dd.dropped) >= 5
    kept = [i for i in range(len(long)) if i not in dd.dropped]
    assert kept[-1] == len(long) - 1
    same(got, reference_on_kept(net, long, kept, 24, 60, 3, crop=(64, 96)))


def reference_on_kept(net, frames, kept, fi, fo, levels, crop):
    """The retimed frames from the full recursion of every kept pair: (j, p) -> frame p of interpolate_video_nx on (kept_j, kept_j+1)."""
    n = 1 << levels
    y0, x0, h, w = mf.centre_window(*frames[0].shape[:2], crop)
    seg = {}
    out = []
    for j, p in rt.retime_slots(kept, fi, fo, levels):
        if p in (0, n):
            out.append(np.ascontiguousarray(frames[kept[j] if p == 0 else kept[j + 1]][y0:y0 + h, x0:x0 + w]))
            continue
        if j not in seg:
            seg = {j: list(host_io.interpolate_video_nx(iter([frames[kept[j]], frames[kept[j + 1]]]), net, factor=n, crop=crop, pool=False,
                                                        max_batch=1, **KW))}
        out.append(seg[j][p])
    return out


def test_network_base_once(nets):
    net = nets["base"]
    net.global_motion, net.ensemble_global_motion = True, False
    frames = pairs.uint8_video(3, 128, 192, seed=9)
    kw = dict(isBGR=True, divisor=64)
    full = list(host_io.interpolate_video_nx(iter(frames), net, factor=8, pool=True, max_batch=1, **kw))
    got = list(host_io.interpolate_video_retimed(iter(frames), net, 24, 60, levels=3, pool=True, max_batch=1, **kw))
    same(got, [full[8 * j + p] for j, p in rt.retime_slots(range(3), 24, 60, 3)])


@pytest.mark.parametrize("depth", [8, 10])
def test_i420_frames(nets, video, depth):
    net = lite(nets)
    fmt = yuv.Format(H, W, depth=depth)
    if depth == 8:
        frames = [yuv.encode_numpy(f, fmt) for f in video[:4]]
    else:
        frames = [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt) for f in video[:4]]
    kw = dict(divisor=32, pool=False, max_batch=1, pixfmt=fmt, keep_depth=depth == 10)
    slots = list(rt.retime_slots(range(4), 24, 60, 3))
    dd = rt.Duplicates(cell=0.5, peak=2)                              # compares every frame (the resident RGB frame exists) and drops none
    got = list(host_io.interpolate_video_retimed(iter(frames), net, 24, 60, levels=3, dedup=dd, scene=scene.SceneCuts(), **kw))
    assert len(got) == len(slots) == 8 and dd.dropped == []
    out_dtype, out_size = (np.uint8, fmt.frame_bytes) if depth == 8 else (np.uint16, fmt.frame_samples)
    assert all(g.dtype == out_dtype and g.shape == (out_size,) for g in got)
    full = list(host_io.interpolate_video_nx(iter(frames), net, factor=8, **kw))
    same(got, [full[8 * j + p] for j, p in slots])
    for k, (j, p) in enumerate(slots):
        if p == 0:
            assert got[k] is frames[j], k                             # originals: the caller's own bytes
    if depth == 8:                                                    # produced frames: the encode of the RGB loop's frames
        rgb = [yuv.decode_numpy(v, fmt) for v in frames]
        want = list(host_io.interpolate_video_retimed(iter(rgb), net, 24, 60, levels=3, isBGR=False, divisor=32, pool=False, max_batch=1))
        for k, (j, p) in enumerate(slots):
            if 0 < p < 8:
                assert np.array_equal(got[k], yuv.encode_numpy(want[k], fmt)), k
        assert dd.stats == [rt.duplicate_statistics(rt.difference_numpy(rgb[i - 1], rgb[i], bgr=False), H, W) for i in range(1, 4)]


def test_tta_once(nets, video):
    net = lite(nets)
    full = list(host_io.interpolate_video_nx(iter(video[:3]), net, factor=8, pool=True, max_batch=1, tta=True, **KW))
    report = {}
    got = retimed(net, video[:3], 24, 60, levels=3, pool=True, max_batch=1, tta=True, report=report)
    same(got, [full[8 * j + p] for j, p in rt.retime_slots(range(3), 24, 60, 3)])
    assert report["forwards"] == 2 * report["interpolated"]
