"""GPU: the active picture of letterboxed video on the device (csrc/active.hip atmvfi_frame_borders / atmvfi_frame_compose, the
``active=`` argument of ``interpolate_video_nx``): both kernels against the loop models of tests/cpu_active.py bit for bit, and
letterboxed videos through the HIP loop -- inside the window the frames of the picture alone, outside it the bars of the nearer
original, and the plain loop's frames from the segment on at which content enters the bars."""
import importlib

import numpy as np
import pytest
import torch

import cpu_active as C

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")
active = importlib.import_module("atm-vfi_amd.active")


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


def shifted_copy(t, by):
    """the same bytes behind a pointer offset by ``by`` bytes"""
    buf = torch.empty(t.numel() * t.element_size() + 16, dtype=torch.uint8, device=t.device)
    out = buf[by:by + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    out.copy_(t)
    assert (out.data_ptr() - buf.data_ptr()) == by
    return out


# ------------------------------------------------------------------------------------------------ frame_borders
def picture(h, w, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "corners":                                         # one lit pixel in each corner, each of another colour
        f = np.zeros((h, w, 3), np.uint8)
        f[0, 0], f[0, w - 1], f[h - 1, 0], f[h - 1, w - 1] = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
        return f
    if kind == "hot":                                             # dim noise, one hot row and one hot column
        f = rng.integers(0, 40, (h, w, 3), dtype=np.uint8)
        f[h // 3] = rng.integers(200, 256, (w, 3), dtype=np.uint8)
        f[:, (2 * w) // 3] = rng.integers(120, 200, (h, 3), dtype=np.uint8)
        return f
    f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)           # noise whose level differs from line to line
    f = (f * rng.uniform(0.05, 1, (h, 1, 1)) * rng.uniform(0.3, 1, (1, w, 1))).astype(np.uint8)
    return f


BORDER_CASES = [          # H, W, picture
    (16, 16, "black"),
    (18, 22, "noise"),                 # W % 4 != 0: byte loads, a partial row step
    (18, 22, "corners"),
    (40, 1100, "noise"),               # across a column tile, dword loads
    (40, 1100, "corners"),
    (24, 1030, "hot"),                 # across a column tile, byte loads
    (64, 96, "hot"),
    (33000, 16, "noise"),              # more row chunks than the launch keeps at 8 rows each: 16 rows per chunk
]


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,kind", BORDER_CASES, ids=lambda v: str(v))
def test_frame_borders_is_the_model(ops, dev, H, W, kind, bgr):
    frame = picture(H, W, H + W, kind)
    want = C.borders_model(frame, bgr)
    src = torch.from_numpy(frame).to(dev)
    out = torch.full((H + W,), -0x12345678, dtype=torch.int32, device=dev)       # poisoned: the call writes every word
    ret = ops.frame_borders(src, bgr=bgr, out=out)
    assert ret is out
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(ops.frame_borders(src, bgr=bgr).cpu().numpy(), got)      # a second call, a fresh output: identical bits
    assert np.array_equal(active.borders_numpy(frame, bgr=bgr), got)
    # the same pixels behind a pointer offset by one byte: the general path gives the same bits
    moved = shifted_copy(src, 1)
    assert moved.data_ptr() % 4 != src.data_ptr() % 4
    out.fill_(-1)
    ws = ops.frame_borders_workspace(H, W)
    ws.fill_(0x7f7f7f7f)                                                           # a poisoned workspace too: nothing is pre-zeroed
    ops.frame_borders(moved, bgr=bgr, out=out, workspace=ws)
    assert np.array_equal(out.cpu().numpy(), want)


def test_frame_borders_at_4k_and_refusals(ops, dev):
    frame = picture(2160, 4096, 7, "noise")
    frame[:270] //= 32
    frame[-270:] //= 32
    src = torch.from_numpy(frame).to(dev)
    got = ops.frame_borders(src, bgr=True).cpu().numpy()
    assert np.array_equal(got, C.borders_model(frame, True))
    small = torch.zeros(40, 52, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ops.frame_borders(small.float())
    with pytest.raises(ValueError):
        ops.frame_borders(small, out=torch.zeros(91, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="at least 16 x 16"):
        ops.frame_borders(small[:15].contiguous())
    with pytest.raises(RuntimeError, match="workspace of"):
        ops.frame_borders(small, workspace=torch.zeros(8, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------ frame_compose
def canvas_values(rng, shape):
    """fp32 values: exact .5 ties of x * 255, values outside [0, 1], ordinary ones"""
    ties = np.array([C_TIES[k] for k in rng.integers(0, 255, int(np.prod(shape)))], np.float32).reshape(shape)
    wide = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
    pick = rng.integers(0, 3, shape)
    return np.where(pick == 0, ties, np.where(pick == 1, wide, rng.uniform(0, 1, shape).astype(np.float32))).astype(np.float32)


def _tie(k):
    x = np.float32((k + 0.5) / 255.0)
    for cand in (x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-1))):
        if np.float32(cand) * np.float32(255.0) == np.float32(k + 0.5):
            return np.float32(cand)
    raise AssertionError(k)


C_TIES = [_tie(k) for k in range(255)]

COMPOSE_CASES = [         # H, W, window (y0, x0, h, w), (pad_top, pad_left), (Hp, Wp)
    (3, 5, (1, 2, 1, 1), (0, 0), (1, 1)),                  # a 1 x 1 window
    (8, 12, (0, 0, 8, 12), (4, 4), (16, 20)),              # window == frame: the aligned path, no byte of the border read
    (9, 14, (0, 3, 4, 11), (1, 2), (7, 16)),               # touching the top and the right edge
    (9, 14, (5, 0, 4, 7), (0, 5), (4, 13)),                # touching the bottom and the left edge, an odd origin
    (10, 16, (3, 5, 5, 7), (3, 4), (11, 12)),              # odd everything
    (12, 16, (2, 4, 8, 8), (4, 4), (16, 16)),              # aligned: groups wholly inside or outside
    (16, 32, (4, 8, 8, 16), (0, 0), (8, 16)),              # aligned, no padding
    (16, 32, (4, 8, 8, 16), (2, 3), (12, 20)),             # aligned frame, a pad_left that is no multiple of 4: the general path
]


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,win,pad,canvas", COMPOSE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_frame_compose_is_the_model(ops, dev, H, W, win, pad, canvas, bgr):
    rng = np.random.default_rng(H * 100 + W + win[1])
    border = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    h, w = win[2:]
    src = canvas_values(rng, (3,) + canvas)
    u8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = C.compose_model(border, win, src=src, pad_top=pad[0], pad_left=pad[1], bgr=bgr)
    want_u8 = C.compose_model(border, win, win_u8=u8)
    d_border, d_src, d_u8 = (torch.from_numpy(a).to(dev) for a in (border, src, u8))
    dst = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev)               # poisoned: the call writes every byte
    ops.frame_compose(dst, d_border, win, src=d_src, pad_top=pad[0], pad_left=pad[1], bgr=bgr)
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(active.compose_numpy(border, win, src=src, pad_top=pad[0], pad_left=pad[1], bgr=bgr), got)
    dst.fill_(0x5A)
    ops.frame_compose(dst, d_border, win, win_u8=d_u8, bgr=bgr)
    assert np.array_equal(dst.cpu().numpy(), want_u8)
    # the same sources behind other alignments: an fp32 canvas offset by 4 bytes, uint8 frames offset by 1 -- the same bits
    dst2 = shifted_copy(torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev), 1)
    ops.frame_compose(dst2, shifted_copy(d_border, 1), win, src=shifted_copy(d_src, 4), pad_top=pad[0], pad_left=pad[1], bgr=bgr)
    assert np.array_equal(dst2.cpu().numpy(), want)
    dst.fill_(0x5A)
    ops.frame_compose(dst, shifted_copy(d_border, 3), win, win_u8=shifted_copy(d_u8, 1))
    assert np.array_equal(dst.cpu().numpy(), want_u8)
    dst.fill_(0x5A)
    ops.frame_compose(dst, d_border, win, src=shifted_copy(d_src, 4), pad_top=pad[0], pad_left=pad[1], bgr=bgr)
    assert np.array_equal(dst.cpu().numpy(), want)


def test_frame_compose_many_blocks_and_refusals(ops, dev):
    # 1080p, both paths, against the host twin (tests/test_active_cpu.py holds the twin to the loop model)
    rng = np.random.default_rng(5)
    H, W, win = 1080, 1920, (138, 0, 804, 1920)
    border = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    src = rng.uniform(-0.1, 1.1, (3, 832, 1920)).astype(np.float32)
    d_border, d_src = torch.from_numpy(border).to(dev), torch.from_numpy(src).to(dev)
    dst = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev)
    for bgr in (False, True):
        want = active.compose_numpy(border, win, src=src, pad_top=14, pad_left=0, bgr=bgr)
        ops.frame_compose(dst, d_border, win, src=d_src, pad_top=14, pad_left=0, bgr=bgr)
        assert np.array_equal(dst.cpu().numpy(), want)
        dst.fill_(0)
        ops.frame_compose(dst, shifted_copy(d_border, 1), win, src=d_src, pad_top=14, pad_left=0, bgr=bgr)
        assert np.array_equal(dst.cpu().numpy(), want)
    u8 = torch.zeros(804, 1920, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="must not alias"):
        ops.frame_compose(dst, dst, win, win_u8=u8)
    both = torch.zeros(2 * H, W, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="must not alias"):
        ops.frame_compose(both[:H], both[1:H + 1], win, win_u8=u8)
    with pytest.raises(ValueError, match="exactly one"):
        ops.frame_compose(dst, d_border, win)
    with pytest.raises(ValueError, match="exactly one"):
        ops.frame_compose(dst, d_border, win, src=d_src, win_u8=u8)
    with pytest.raises(ValueError):
        ops.frame_compose(dst, d_border[:H - 2].contiguous(), win, win_u8=u8)
    with pytest.raises(ValueError):
        ops.frame_compose(dst, d_border, win, win_u8=u8[:800].contiguous())
    with pytest.raises(RuntimeError, match="window outside the frame"):
        ops.frame_compose(dst, d_border, (300, 0, 804, 1920), win_u8=u8)
    with pytest.raises(RuntimeError, match="bad geometry"):
        ops.frame_compose(dst, d_border, win, src=d_src, pad_top=30)


# ------------------------------------------------------------------------------------------------ the loops
def record_forwards(monkeypatch, net):
    """Recording wrappers around ``forward`` / ``forward_pooled`` of the model's class: the frame size each call ran at."""
    sizes = []
    for name in ("forward", "forward_pooled"):
        klass = next(k for k in type(net).__mro__ if name in k.__dict__)

        def wrapper(self, *a, _orig=klass.__dict__[name], _name=name, **kw):
            sizes.append((a[0].hp, a[0].wp) if _name == "forward_pooled" else tuple(a[0].shape[-2:]))
            return _orig(self, *a, **kw)
        monkeypatch.setattr(klass, name, wrapper)
    return sizes


def check_windowed(got, video, alone, factor, win, first_segment=0, segments=None):
    """``got``: the frames of segments ``first_segment ...`` of the letterboxed ``video``; ``alone``: the loop's frames on the pictures"""
    y0, x0, h, w = win
    n_seg = len(video) - 1 if segments is None else segments
    mask = np.ones(video[0].shape[:2], bool)
    mask[y0:y0 + h, x0:x0 + w] = False
    for s in range(first_segment, first_segment + n_seg):
        for k in range(factor):
            g = got[(s - first_segment) * factor + k]
            if k == 0:
                assert g is video[s], (s, k)                       # originals are the caller's objects
                continue
            assert g.dtype == np.uint8 and g.shape == video[s].shape
            assert np.array_equal(g[y0:y0 + h, x0:x0 + w], alone[s * factor + k]), (s, k)
            bars = video[s] if k <= factor // 2 else video[s + 1]  # the nearer original, ties to the earlier one
            assert np.array_equal(g[mask], bars[mask]), (s, k)


HL, WL, ROWS, WIN = 128, 96, (32, 96), (32, 0, 64, 96)            # the window 64 x 96 pads to 64 x 128, the frame to 128 x 128
L, PIC = C.letterboxed(5, HL, WL, ROWS, seed=21, tone=150)        # bars hold noise <= 3, the picture is >= 116 everywhere

NX_CASES = [          # factor, pool, tta, isBGR
    (4, True, False, True),
    (4, False, False, True),
    (8, True, False, False),
    (8, False, False, True),
    (4, True, True, True),
    (8, False, True, False),
]


@pytest.mark.parametrize("factor,pool,tta,bgr", NX_CASES, ids=lambda v: str(v))
def test_letterboxed_video_through_interpolate_video_nx(nets, dev, monkeypatch, factor, pool, tta, bgr):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    kw = dict(factor=factor, isBGR=bgr, tta=tta, max_batch=4, pool=pool)
    video, pics = L[:3], PIC[:3]
    alone = list(host_io.interpolate_video_nx(iter(pics), net, **kw))
    sizes = record_forwards(monkeypatch, net)
    area = active.ActiveArea()
    got = list(host_io.interpolate_video_nx(iter(video), net, active=area, **kw))
    assert len(got) == len(alone) == 2 * factor + 1 and got[-1] is video[-1]
    check_windowed(got, video, alone, factor, WIN)
    assert area.window == WIN and area.probed == 3 and area.fallback_at is None
    assert sizes and set(sizes) == {(64, 128)}                     # the forwards ran at the window's padded size
    # the line maxima the device computed are the host's
    assert area.stats[3:] == [active.rect_of(active.borders_numpy(f, bgr=bgr), HL, WL, area.peak) for f in video]


def test_scene_cut_in_a_letterboxed_video(nets, dev):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    other, other_pic = C.letterboxed(3, HL, WL, ROWS, seed=22, tone=60, span=20)
    video, pics = L[:3] + other, PIC[:3] + other_pic
    area, sc = active.ActiveArea(), scene.SceneCuts()
    got = list(host_io.interpolate_video_nx(iter(video), net, factor=4, active=area, scene=sc))
    alone = list(host_io.interpolate_video_nx(iter(pics), net, factor=4, scene=scene.SceneCuts()))
    assert sc.cuts == [2] and area.window == WIN and area.fallback_at is None
    check_windowed(got[:8], video, alone, 4, WIN, segments=2)
    assert got[8] is video[2] and all(np.array_equal(got[8 + k], video[2 if k <= 2 else 3]) and got[8 + k] is not video[2] for k in (1, 2, 3))
    check_windowed(got[12:], video, alone, 4, WIN, first_segment=3, segments=2)


@pytest.mark.parametrize("pool", [True, False])
def test_content_in_the_bars_sends_the_loop_back_to_the_whole_frame(nets, dev, monkeypatch, pool):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    k = 3
    video = [f.copy() for f in L]
    video[k][5, 7] = 255                                           # frame 3, inside the top bar
    kw = dict(factor=4, pool=pool)
    alone = list(host_io.interpolate_video_nx(iter(PIC), net, **kw))
    plain = list(host_io.interpolate_video_nx(iter(video), net, active=None, **kw))
    sizes = record_forwards(monkeypatch, net)
    area = active.ActiveArea(probe=2)
    got = list(host_io.interpolate_video_nx(iter(video), net, active=area, **kw))
    assert area.window == WIN and area.probed == 2 and area.fallback_at == k - 1 and len(got) == len(plain)
    at = (k - 1) * 4
    check_windowed(got[:at], video, alone, 4, WIN, segments=k - 1)
    for i in range(at, len(got)):
        assert np.array_equal(got[i], plain[i]), i
    assert all(got[4 * i] is video[i] for i in range(len(video)))
    assert not np.array_equal(got[at - 1], plain[at - 1])          # (the bars of a windowed frame are an original's)
    assert set(sizes[:len(sizes) // 2]) == {(64, 128)} and set(sizes[len(sizes) // 2:]) == {(128, 128)}      # two segments each


def test_black_frames_first_no_bars_no_gain_and_a_fixed_window(nets, dev, monkeypatch):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    # three black frames first: undecided, and no violation -- the window locks on the later frames
    black = [np.zeros((HL, WL, 3), np.uint8) for _ in range(3)]
    video = black + L[:2]
    area = active.ActiveArea()
    got = list(host_io.interpolate_video_nx(iter(video), net, factor=2, active=area))
    alone = list(host_io.interpolate_video_nx(iter([np.ascontiguousarray(b[32:96]) for b in black] + PIC[:2]), net, factor=2))
    assert area.window == WIN and area.probed == 5 and area.fallback_at is None
    check_windowed(got, video, alone, 2, WIN)
    # a video without bars, and one whose bars gain nothing (96 rows pad to 128 as 128 do): the plain loop's frames and sizes
    full = C.cpu_scene.shot(3, HL, WL, seed=4, tone=150)
    thin, _ = C.letterboxed(3, HL, WL, (16, 112), seed=5)
    for vid in (full, thin):
        plain = list(host_io.interpolate_video_nx(iter(vid), net, factor=4))
        sizes = record_forwards(monkeypatch, net)
        area = active.ActiveArea()
        got = list(host_io.interpolate_video_nx(iter(vid), net, factor=4, active=area))
        monkeypatch.undo()
        assert area.window == (0, 0, HL, WL) and area.fallback_at is None and len(got) == len(plain)
        assert all(np.array_equal(g, p) for g, p in zip(got, plain)) and all(got[4 * i] is vid[i] for i in range(3))
        assert set(sizes) == {(128, 128)}
    # a fixed window: never probed, never checked -- a lit bar pixel changes nothing
    video = [f.copy() for f in L[:3]]
    video[1][1, 1] = 255
    got = list(host_io.interpolate_video_nx(iter(video), net, factor=4, active=WIN))
    check_windowed(got, video, list(host_io.interpolate_video_nx(iter(PIC[:3]), net, factor=4)), 4, WIN)
    # refusals
    with pytest.raises(ValueError, match="crop"):
        list(host_io.interpolate_video_nx(iter(L), net, active=active.ActiveArea(), crop=(64, 64)))
    yuv = importlib.import_module("atm-vfi_amd.yuv")
    with pytest.raises(ValueError, match="pixfmt"):
        list(host_io.interpolate_video_nx(iter(L), net, active=WIN, pixfmt=yuv.Format(HL, WL)))
    with pytest.raises(ValueError, match="even"):
        list(host_io.interpolate_video_nx(iter(L), net, active=(31, 0, 64, 96)))


def test_letterboxed_video_network_base(nets, dev, monkeypatch):
    net = nets["base"]
    net.global_motion, net.ensemble_global_motion = True, False
    video, pics = C.letterboxed(3, 192, 320, (32, 160), seed=23, tone=150)
    alone = list(host_io.interpolate_video_nx(iter(pics), net, factor=4))
    sizes = record_forwards(monkeypatch, net)
    area = active.ActiveArea()
    got = list(host_io.interpolate_video_nx(iter(video), net, factor=4, active=area))
    assert area.window == (32, 0, 128, 320) and area.fallback_at is None and set(sizes) == {(128, 320)}
    check_windowed(got, video, alone, 4, (32, 0, 128, 320))
