"""GPU: planar YUV 4:2:0 on the device (csrc/yuv.hip atmvfi_yuv_decode, csrc/yuv_encode.hip atmvfi_yuv_encode, the ``pixfmt=`` argument of the video
loops, ``yuv.interpolate_y4m``): both kernels against the per-pixel model of tests/cpu_yuv.py bit for bit -- every matrix, range and
siting, 10-bit, BGR, odd sizes, both the vector and the general path -- and the loops against the RGB loops on the decoded frames."""
import importlib
import itertools
import os

import numpy as np
import pytest
import torch

import cpu_scene as CS
import cpu_yuv as C
import pairs

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")
yuv = importlib.import_module("atm-vfi_amd.yuv")

COMBOS = list(itertools.product(("bt601", "bt709"), (False, True), ("centre", "left")))
SIZES = [(1, 1), (2, 2), (3, 5), (16, 16), (17, 31), (64, 96)]


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


def to_dev(arr, dev, offset=0):
    """The bytes of ``arr`` on the device as a 1-D uint8 tensor whose pointer is ``offset`` bytes past an allocation's start."""
    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy())
    buf = torch.empty(raw.numel() + offset, dtype=torch.uint8, device=dev)
    view = buf[offset:]
    view.copy_(raw)
    return view


def canvas_of(H, W):
    """(Hp, Wp, pad_top, pad_left): an odd top padding everywhere; multiples of 4 across when W is one (the vector path's geometry)."""
    if W % 4 == 0:
        return H + 5, W + 12, 3, 4
    return H + 4, W + 7, 1, 3


def decode_on_device(ops, dev, buf, fmt, bgr, geometry, offset=0):
    """-> (dst_u8, dst) as numpy / torch, both outputs poisoned before the call"""
    Hp, Wp, pt, pl = geometry
    src = to_dev(buf, dev, offset)
    d8 = torch.full((fmt.height, fmt.width, 3), 0xA5, dtype=torch.uint8, device=dev)
    df = torch.full((3, Hp, Wp), float("nan"), dtype=torch.float32, device=dev)
    ops.yuv420_to_rgb(src, fmt, dst_u8=d8, dst=df, pad_top=pt, pad_left=pl, bgr=bgr)
    return d8, df


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_decode_is_the_model(ops, dev, H, W):
    geo = canvas_of(H, W)
    for k, (matrix, full, siting) in enumerate(COMBOS):
        for depth in ((8,) if full else (8, 10)):
            bgr = bool((k + depth) & 1)
            fmt = yuv.Format(H, W, matrix, full, siting, depth)
            buf = C.random_frame(H, W, depth, seed=100 * H + W + k)
            want = C.decode(buf, H, W, matrix, int(full), siting, depth, bgr=bgr)
            d8, df = decode_on_device(ops, dev, buf, fmt, bgr, geo)
            got = d8.cpu().numpy()
            assert np.array_equal(got, want), (matrix, full, siting, depth, np.argwhere(got != want)[:4])
            # the fp32 canvas: the bits of frame_u8_to_f32 on dst_u8, padding included; every word written
            ref = torch.empty_like(df)
            ops.frame_u8_to_f32(d8, ref, geo[2], geo[3], bgr)
            assert torch.equal(df, ref), (matrix, full, siting, depth)
            # one output at a time gives the same bits
            only8 = torch.full_like(d8, 0x5A)
            ops.yuv420_to_rgb(to_dev(buf, dev), fmt, dst_u8=only8, bgr=bgr)
            assert torch.equal(only8, d8)
            onlyf = torch.full_like(df, float("nan"))
            ops.yuv420_to_rgb(to_dev(buf, dev), fmt, dst=onlyf, pad_top=geo[2], pad_left=geo[3])
            assert torch.equal(onlyf, df)
            # the same frame behind a pointer offset by one byte (8 bit) or one sample (10 bit): the general path, the same bits
            o8, of = decode_on_device(ops, dev, buf, fmt, bgr, geo, offset=1 if depth == 8 else 2)
            assert torch.equal(o8, d8) and torch.equal(of, df)
            if depth == 10:
                o8, of = decode_on_device(ops, dev, buf, fmt, bgr, geo, offset=1)          # an odd byte address under uint16 samples
                assert torch.equal(o8, d8) and torch.equal(of, df)


@pytest.mark.parametrize("H,W,divisor", [(64, 96, 128), (66, 98, 64)])
def test_decode_into_the_padded_network_input(ops, dev, H, W, divisor):
    """64 x 96 -> 64 x 128 (aligned, left padding 16) and 66 x 98 -> 128 x 128 (general, odd paddings): InputPadder's geometry."""
    pad = host_io.InputPadder((1, 3, H, W), divisor=divisor)
    pl, pr, pt, pb = pad._pad
    if (H, W) == (64, 96):
        pt = pb = 0
    Hp, Wp = H + pt + pb, W + pl + pr
    assert (Hp, Wp) == ((64, 128) if (H, W) == (64, 96) else (128, 128))
    for matrix, full, siting in COMBOS:
        fmt = yuv.Format(H, W, matrix, full, siting)
        buf = C.random_frame(H, W, 8, seed=H + W)
        d8, df = decode_on_device(ops, dev, buf, fmt, False, (Hp, Wp, pt, pl))
        assert np.array_equal(d8.cpu().numpy(), yuv.decode_numpy(buf, fmt))
        ref = torch.empty_like(df)
        ops.frame_u8_to_f32(d8, ref, pt, pl, False)
        assert torch.equal(df, ref)
        rgb = torch.from_numpy(yuv.decode_numpy(buf, fmt)).permute(2, 0, 1)[None].float() / 255.0
        assert torch.equal(df.cpu(), torch.nn.functional.pad(rgb, [pl, pr, pt, pb], mode="replicate")[0])


def test_decode_1080p_once(ops, dev):
    H, W = 1080, 1920
    for depth, siting in ((8, "centre"), (10, "left")):
        fmt = yuv.Format(H, W, "auto", False, siting, depth)
        assert fmt.matrix == "bt709"
        buf = C.random_frame(H, W, depth, seed=depth)
        want = yuv.decode_numpy(buf, fmt)                  # the vectorised twin (held to the loop model in tests/test_yuv_cpu.py)
        d8, df = decode_on_device(ops, dev, buf, fmt, False, (1088, 1920, 4, 0))
        assert np.array_equal(d8.cpu().numpy(), want)
        ref = torch.empty_like(df)
        ops.frame_u8_to_f32(d8, ref, 4, 0, False)
        assert torch.equal(df, ref)
        o8, of = decode_on_device(ops, dev, buf, fmt, False, (1088, 1920, 4, 0), offset=2)
        assert torch.equal(o8, d8) and torch.equal(of, df)


def test_the_three_decode_entry_points_are_one_kernel(ops, dev):
    """``yuv420_to_rgb`` is ``yuv420_window`` mode 0 with the window set to the whole frame -- the same bits in the canvas (padding
    included) and in the uint8 frame -- and ``yuv420p10_to_f32`` walks a window the same way: the numpy twin's window, replicate padded.
    On the aligned path, and behind a source pointer offset by 2 bytes on the general path."""
    H, W = 20, 36
    Hp, Wp, pt, pl = geo = (H + 5, W + 12, 3, 4)
    y0, x0, h, w = window = (4, 8, 12, 24)
    for k, (depth, siting) in enumerate(itertools.product((8, 10), ("centre", "left"))):
        fmt = yuv.Format(H, W, ("bt601", "bt709")[k & 1], False, siting, depth)
        buf = C.random_frame(H, W, depth, seed=40 + k)
        for offset in (0, 2):
            d8, df = decode_on_device(ops, dev, buf, fmt, False, geo, offset)
            w8 = torch.full_like(d8, 0xA5)
            wf = torch.full_like(df, float("nan"))
            ops.yuv420_window(to_dev(buf, dev, offset), fmt, 0, 0, 0, H, W, dst=wf, dst_u8=w8, pad_top=pt, pad_left=pl)
            assert torch.equal(w8, d8) and torch.equal(wf.view(torch.int32), df.view(torch.int32)), (depth, siting, offset)
            assert not torch.isnan(df).any()
            if depth == 10:
                kf = torch.full((3, Hp, Wp), float("nan"), dtype=torch.float32, device=dev)
                ops.yuv420p10_to_f32(to_dev(buf, dev, offset), fmt, kf, window=window, pad_top=pt, pad_left=pl)
                inner = torch.from_numpy(yuv.decode_numpy_f32(buf, fmt, window)).permute(2, 0, 1)[None]
                want = torch.nn.functional.pad(inner, [pl, Wp - pl - w, pt, Hp - pt - h], mode="replicate")[0]
                assert torch.equal(kf.cpu().view(torch.int32), want.contiguous().view(torch.int32)), (siting, offset)


# ------------------------------------------------------------------------------------------------ encode
def tie_values():
    """fp32 values x with x * 255 (in fp32) exactly k + 0.5"""
    k = np.arange(255, dtype=np.float64)
    x = ((k + 0.5) / 255.0).astype(np.float32)
    keep = (x * np.float32(255.0)).astype(np.float64) == k + 0.5
    assert keep.sum() > 20
    return x[keep]


def fp32_frame(H, W, Hp, Wp, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.3, 1.3, (3, Hp, Wp)).astype(np.float32)
    ties = tie_values()
    m = rng.random((3, Hp, Wp)) < 0.3
    x[m] = ties[rng.integers(0, len(ties), int(m.sum()))]
    return x


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_encode_is_the_model(ops, dev, H, W):
    Hp, Wp, pt, pl = canvas_of(H, W)
    for k, (matrix, full, siting) in enumerate(COMBOS):
        bgr = bool(k & 1)
        fmt = yuv.Format(H, W, matrix, full, siting)
        rgb = np.random.default_rng(7 * H + W + k).integers(0, 256, (H, W, 3)).astype(np.uint8)
        want = C.encode(rgb, matrix, int(full), siting, bgr=bgr)
        outs = []
        for src_off, dst_off in ((0, 0), (0, 1), (1, 0)):           # aligned where the size allows; an offset destination; an offset source
            dst = torch.full((fmt.frame_bytes + dst_off,), 0xA5, dtype=torch.uint8, device=dev)[dst_off:]
            ops.rgb_to_yuv420(dst, fmt, src_u8=to_dev(rgb, dev, src_off).view(H, W, 3), bgr=bgr)
            outs.append(dst.cpu().numpy())
        for got in outs:
            assert np.array_equal(got, want), (matrix, full, siting, np.flatnonzero(got != want)[:4])
        # from fp32: encode of frame_f32_to_u8's pixels (values outside [0, 1], exact .5 ties), the frame inside a padded canvas
        x = fp32_frame(H, W, Hp, Wp, seed=H * W + k)
        xd = torch.from_numpy(x).to(dev)
        q = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        ops.frame_f32_to_u8(xd, q, pt, pl, False)
        qn = q.cpu().numpy()
        assert np.array_equal(qn, C.f32_to_u8(x[:, pt:pt + H, pl:pl + W]).transpose(1, 2, 0))
        want_f = C.encode(qn, matrix, int(full), siting)
        for dst_off in (0, 1):
            dst = torch.full((fmt.frame_bytes + dst_off,), 0xA5, dtype=torch.uint8, device=dev)[dst_off:]
            ops.rgb_to_yuv420(dst, fmt, src=xd, pad_top=pt, pad_left=pl)
            got = dst.cpu().numpy()
            assert np.array_equal(got, want_f), (matrix, full, siting, dst_off, np.flatnonzero(got != want_f)[:4])


def test_encode_1080p_once(ops, dev):
    H, W = 1080, 1920
    fmt = yuv.Format(H, W, siting="left")
    x = fp32_frame(H, W, 1088, 1920, seed=5)
    xd = torch.from_numpy(x).to(dev)
    q = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    ops.frame_f32_to_u8(xd, q, 4, 0, False)
    want = yuv.encode_numpy(q.cpu().numpy(), fmt)
    for dst_off in (0, 1):
        dst = torch.full((fmt.frame_bytes + dst_off,), 0xA5, dtype=torch.uint8, device=dev)[dst_off:]
        ops.rgb_to_yuv420(dst, fmt, src=xd, pad_top=4, pad_left=0)
        assert np.array_equal(dst.cpu().numpy(), want)
    dst = torch.full((fmt.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    ops.rgb_to_yuv420(dst, fmt, src_u8=q)
    assert np.array_equal(dst.cpu().numpy(), want)


def test_wrapper_refusals(ops, dev):
    fmt = yuv.Format(16, 16)
    buf = to_dev(C.random_frame(16, 16), dev)
    d8 = torch.empty(16, 16, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb(buf, fmt)
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb(buf[:-1], fmt, dst_u8=d8)
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb(buf, fmt, dst_u8=d8[:8])
    with pytest.raises(RuntimeError, match="smaller than the window"):
        ops.yuv420_to_rgb(buf, fmt, dst=torch.empty(3, 16, 16, device=dev), pad_left=4)
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(buf, fmt)
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(buf, fmt, src_u8=d8, src=torch.empty(3, 16, 16, device=dev))
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(buf, yuv.Format(16, 16, depth=10), src_u8=d8)


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


def two_shot(n, H, W, fmt):
    """(I420 frames of two shots back to back, their decoded RGB frames)"""
    rgb = CS.shot(n, H, W, seed=11, tone=60) + CS.shot(n, H, W, seed=12, tone=190)
    video = [yuv.encode_numpy(f, fmt) for f in rgb]
    return video, [yuv.decode_numpy(v, fmt) for v in video]


def check_loop(got, want_rgb, video, factor, s, cuts, fmt, window):
    """Originals are the caller's bytes, cut copies are copies of them, every other frame is the RGB loop's frame encoded."""
    y0, x0, h, w = window
    out_fmt = fmt.as_8bit().cropped(h, w)
    whole = (h, w) == (fmt.height, fmt.width)
    assert len(got) == len(want_rgb)
    for k, (g, wnt) in enumerate(zip(got, want_rgb)):
        seg, pos = divmod(k, factor)
        if pos == 0:
            src = video[seg * s]
            assert (g is src) if whole else np.array_equal(g, yuv.crop(src, fmt, y0, x0, h, w)), k
        elif seg in cuts:
            src = video[seg * s] if pos <= factor // 2 else video[(seg + 1) * s]
            assert g is not src and np.array_equal(g, yuv.crop(src, fmt, y0, x0, h, w)), k
        else:
            assert g.dtype == np.uint8 and g.shape == (out_fmt.frame_bytes,) and np.array_equal(g, yuv.encode_numpy(wnt, out_fmt)), k


@pytest.mark.parametrize("streams", [1, 2])
def test_interpolate_video_2x_with_pixfmt(nets, dev, monkeypatch, streams):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    H, W = 64, 96
    fmt = yuv.Format(H, W, "bt709", False, "left")
    video, rgb = two_shot(4, H, W, fmt)
    calls = count_forwards(monkeypatch, net)
    for with_scene in (False, True):
        sc_y, sc_r = (scene.SceneCuts(), scene.SceneCuts()) if with_scene else (None, None)
        n0 = calls["forward"]
        want = list(host_io.interpolate_video_2x(iter(rgb), net, isBGR=False, divisor=32, streams=streams, scene=sc_r))
        n_rgb = calls["forward"] - n0
        got = list(host_io.interpolate_video_2x(iter(video), net, isBGR=True, divisor=32, streams=streams, scene=sc_y, pixfmt=fmt))
        assert calls["forward"] - n0 - n_rgb == n_rgb > 0                     # the forward count is the RGB loop's
        cuts = set()
        if with_scene:
            assert sc_y.cuts == sc_r.cuts == [3] and sc_y.stats == sc_r.stats
            cuts = {3}
        check_loop(got, want, video, 2, 1, cuts, fmt, (0, 0, H, W))


NX_CASES = [          # variant, H, W, factor, pool, tta, time_interval, crop, divisor, depth
    ("lite", 64, 96, 4, True, False, 1, None, 32, 8),
    ("lite", 64, 96, 4, False, False, 1, None, 32, 8),
    ("lite", 64, 96, 8, True, False, 1, None, 32, 8),
    ("lite", 64, 96, 4, True, True, 1, None, 32, 8),
    ("lite", 80, 112, 4, True, False, 2, (64, 96), 32, 8),
    ("lite", 64, 96, 4, True, False, 1, None, 32, 10),
    ("base", 192, 320, 4, True, False, 1, None, 64, 8),
]


@pytest.mark.parametrize("variant,H,W,factor,pool,tta,s,crop,divisor,depth", NX_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_interpolate_video_nx_with_pixfmt(nets, dev, monkeypatch, variant, H, W, factor, pool, tta, s, crop, divisor, depth):
    net = nets[variant]
    net.global_motion, net.ensemble_global_motion = True, False
    fmt8 = yuv.Format(H, W, "bt601", True, "centre")
    fmt = fmt8 if depth == 8 else yuv.Format(H, W, "bt601", False, "centre", 10)
    video, rgb = two_shot(2 * s + 1, H, W, fmt8)
    if depth == 10:
        video = [v.astype(np.uint16) << 2 for v in video]
        rgb = [yuv.decode_numpy(v, fmt) for v in video]
    window = mf.centre_window(H, W, crop)
    kw = dict(factor=factor, time_interval=s, crop=crop, divisor=divisor, tta=tta, max_batch=4, pool=pool)
    calls = count_forwards(monkeypatch, net)
    sc_y, sc_r = scene.SceneCuts(), scene.SceneCuts()
    want = list(host_io.interpolate_video_nx(iter(rgb), net, isBGR=False, scene=sc_r, **kw))
    n_rgb = dict(calls)
    got = list(host_io.interpolate_video_nx(iter(video), net, isBGR=True, scene=sc_y, pixfmt=fmt, **kw))
    assert {k: calls[k] - n_rgb[k] for k in calls} == n_rgb and sum(n_rgb.values()) > 0
    n_seg = (len(video) - 1) // s
    assert sc_y.cuts == sc_r.cuts == [n_seg // 2] and sc_y.stats == sc_r.stats and len(sc_y.stats) == n_seg
    check_loop(got, want, video, factor, s, set(sc_y.cuts), fmt, window)


def test_odd_crop_origin_is_refused_on_the_device_path(nets, dev):
    net = nets["lite"]
    fmt = yuv.Format(80, 112)
    video, _ = two_shot(2, 80, 112, fmt)
    with pytest.raises(ValueError, match="even"):
        list(host_io.interpolate_video_nx(iter(video), net, factor=2, crop=(66, 96), divisor=32, pixfmt=fmt))       # rows 7 .. 73
    with pytest.raises(ValueError):
        host_io.FramePipeline(net, 64, 96, pixfmt=fmt)


def test_interpolate_y4m_on_the_device(nets, dev, tmp_path):
    from fractions import Fraction
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    H, W, n = 66, 98, 5
    fmt = yuv.Format(H, W, siting="left")
    video = [yuv.encode_numpy(f, fmt) for f in pairs.uint8_video(n, H, W, seed=4)]
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with yuv.Y4MWriter(src, fmt, Fraction(30000, 1001)) as wr:
        for f in video:
            wr.write(f)
    info = yuv.interpolate_y4m(str(src), str(dst), net, divisor=32)
    assert info == {"fps_in": Fraction(30000, 1001), "fps_out": Fraction(60000, 1001), "size": (W, H), "frames_in": n, "frames_out": 2 * n - 1}
    with yuv.Y4MReader(dst) as rd:
        assert rd.fmt == fmt and rd.fps == Fraction(60000, 1001) and rd.ctag == "420mpeg2" and len(rd) == 2 * n - 1
        got = list(rd)
    want = list(host_io.interpolate_video_2x(iter([yuv.decode_numpy(v, fmt) for v in video]), net, isBGR=False, divisor=32))
    for k, g in enumerate(got):
        assert np.array_equal(g, video[k // 2] if k % 2 == 0 else yuv.encode_numpy(want[k], fmt)), k
    assert os.path.getsize(dst) == len(open(dst, "rb").readline()) + (2 * n - 1) * (6 + fmt.frame_bytes)
    # 4x with flip-TTA goes through the N-x loop
    info = yuv.interpolate_y4m(str(src), str(dst), net, factor=4, tta=True, divisor=32)
    assert info["frames_out"] == 4 * (n - 1) + 1 and info["fps_out"] == Fraction(120000, 1001)
    with yuv.Y4MReader(dst) as rd:
        got = list(rd)
    want = list(host_io.interpolate_video_nx(iter([yuv.decode_numpy(v, fmt) for v in video]), net, factor=4, tta=True, isBGR=False, divisor=32))
    for k, g in enumerate(got):
        assert np.array_equal(g, video[k // 4] if k % 4 == 0 else yuv.encode_numpy(want[k], fmt)), k
