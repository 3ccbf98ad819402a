"""GPU: 10-bit depth kept end to end on the device (csrc/yuv.hip atmvfi_yuv_decode with keep_depth, csrc/yuv_encode.hip atmvfi_yuv_encode at depth 10, ``keep_depth=`` of
the video loops and ``yuv.interpolate_y4m``): both kernels against the per-pixel model of tests/cpu_yuv10.py bit for bit -- both
matrices and sitings, odd sizes, windows, the vector and the general path -- and the loops against ``encode_numpy`` of the fp32
prediction that plain ``net.forward`` gives on inputs decoded by ``HipOps.yuv420p10_to_f32``."""
import importlib
import io
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import cpu_scene as CS
import cpu_yuv10 as C10

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")
yuv = importlib.import_module("atm-vfi_amd.yuv")

COMBOS = list(itertools.product(("bt601", "bt709"), ("centre", "left")))
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


def f32_to_dev(x, dev, offset_floats=0):
    """``x`` on the device behind a pointer ``4 * offset_floats`` bytes past an allocation's start"""
    buf = torch.empty(x.size + offset_floats, dtype=torch.float32, device=dev)
    view = buf[offset_floats:].view(*x.shape)
    view.copy_(torch.from_numpy(x))
    return view


def canvas_of(h, w):
    """(Hp, Wp, pad_top, pad_left): an odd top padding everywhere; multiples of 4 across when w is one (the vector path's geometry)."""
    if w % 4 == 0:
        return h + 5, w + 12, 3, 4
    return h + 4, w + 7, 1, 3


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def decode_on_device(ops, dev, buf, fmt, geometry, offset=0, window=None):
    """-> dst [3,Hp,Wp], poisoned with NaN before the call"""
    Hp, Wp, pt, pl = geometry
    df = torch.full((3, Hp, Wp), float("nan"), dtype=torch.float32, device=dev)
    ops.yuv420p10_to_f32(to_dev(buf, dev, offset), fmt, df, window=window, pad_top=pt, pad_left=pl)
    return df


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_decode_is_the_model(ops, dev, H, W):
    geo = canvas_of(H, W)
    for k, (matrix, siting) in enumerate(COMBOS):
        fmt = yuv.Format(H, W, matrix, False, siting, 10)
        buf = C10.random_frame(H, W, 10, seed=100 * H + W + k)
        want = C10.replicate_pad(C10.decode(buf, H, W, matrix, siting), *geo)
        df = decode_on_device(ops, dev, buf, fmt, geo)
        got = bits(df)
        assert np.array_equal(got, want.view(np.uint32)), (matrix, siting, np.argwhere(got != want.view(np.uint32))[:4])       # every word written
        # the same frame behind a pointer offset by one byte and by one sample: the general path, the same bits
        for off in (1, 2):
            assert torch.equal(decode_on_device(ops, dev, buf, fmt, geo, offset=off), df), (matrix, siting, off)
        # a canvas that is only 4-byte aligned
        whole = torch.full((3 * geo[0] * geo[1] + 1,), float("nan"), dtype=torch.float32, device=dev)
        odd = whole[1:].view(3, geo[0], geo[1])
        ops.yuv420p10_to_f32(to_dev(buf, dev), fmt, odd, pad_top=geo[2], pad_left=geo[3])
        assert torch.equal(odd, df) and bool(torch.isnan(whole[0]))
        # no padding at all
        plain = decode_on_device(ops, dev, buf, fmt, (H, W, 0, 0))
        assert np.array_equal(bits(plain), yuv.decode_numpy_f32(buf, fmt).transpose(2, 0, 1).view(np.uint32))


@pytest.mark.parametrize("H,W,wins", [(20, 36, [(2, 4, 12, 24), (0, 0, 20, 36), (2, 4, 18, 32), (4, 6, 15, 29)]),
                                      (21, 37, [(2, 4, 19, 33), (0, 0, 21, 37), (20, 36, 1, 1), (8, 12, 13, 24)])], ids=lambda v: str(v)[:8])
def test_windows_are_windows_of_the_whole_decode(ops, dev, H, W, wins):
    """(2, 4, 12, 24) and the whole frame of 20 x 36 (the vector path), windows that end at the frame's last row and column (an odd
    one for 20 x 36, the unpaired one for 21 x 37), general-path windows: chroma neighbours are the frame's."""
    for k, (matrix, siting) in enumerate(COMBOS):
        fmt = yuv.Format(H, W, matrix, False, siting, 10)
        buf = C10.random_frame(H, W, 10, seed=H + k)
        full = C10.decode(buf, H, W, matrix, siting)
        for win in wins:
            y0, x0, h, w = win
            geo = canvas_of(h, w)
            want = C10.replicate_pad(full[y0:y0 + h, x0:x0 + w], *geo)
            for off in (0, 2):
                df = decode_on_device(ops, dev, buf, fmt, geo, offset=off, window=win)
                assert np.array_equal(bits(df), want.view(np.uint32)), (matrix, siting, win, off)
            assert np.array_equal(full[y0:y0 + h, x0:x0 + w].view(np.uint32), yuv.decode_numpy_f32(buf, fmt, window=win).view(np.uint32))


@pytest.mark.parametrize("H,W,divisor", [(64, 96, 128), (66, 98, 64)])
def test_decode_into_the_padded_network_input(ops, dev, H, W, divisor):
    """64 x 96 -> 128 x 128 (vector path, paddings that are multiples of 4) and 66 x 98 -> 128 x 128 (general, odd paddings):
    InputPadder's geometry; equal to replicate-padding the unpadded decode."""
    pad = host_io.InputPadder((1, 3, H, W), divisor=divisor)
    pl, pr, pt, pb = pad._pad
    Hp, Wp = H + pt + pb, W + pl + pr
    assert (Hp, Wp) == (128, 128)
    for matrix, siting in COMBOS:
        fmt = yuv.Format(H, W, matrix, False, siting, 10)
        buf = C10.random_frame(H, W, 10, seed=H + W)
        df = decode_on_device(ops, dev, buf, fmt, (Hp, Wp, pt, pl))
        rgb = torch.from_numpy(yuv.decode_numpy_f32(buf, fmt)).permute(2, 0, 1)[None]
        assert torch.equal(df.cpu(), torch.nn.functional.pad(rgb, [pl, pr, pt, pb], mode="replicate")[0])
        assert torch.equal(df.cpu(), pad.pad(rgb)[0])


# ------------------------------------------------------------------------------------------------ encode
def fp32_canvas(H, W, Hp, Wp, pt, pl, seed):
    """An fp32 [3,Hp,Wp] canvas: values on both sides of [0, 1], exact levels, exact ties; outside the frame NaN (never read)."""
    x = np.full((3, Hp, Wp), np.nan, np.float32)
    pic = C10.random_rgb(H, W, seed)
    k = np.arange(1023, dtype=np.float64)
    ties = ((k + 0.5) / 1023.0).astype(np.float32)
    ties = ties[(ties * np.float32(1023.0)).astype(np.float64) == k + 0.5]
    rng = np.random.default_rng(seed + 1)
    m = rng.random(pic.shape) < 0.2
    pic[m] = ties[rng.integers(0, len(ties), int(m.sum()))]
    x[:, pt:pt + H, pl:pl + W] = pic.transpose(2, 0, 1)
    return x, pic


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_encode_is_the_model(ops, dev, H, W):
    Hp, Wp, pt, pl = canvas_of(H, W)
    for k, (matrix, siting) in enumerate(COMBOS):
        fmt = yuv.Format(H, W, matrix, False, siting, 10)
        x, pic = fp32_canvas(H, W, Hp, Wp, pt, pl, seed=H * W + k)
        want = C10.encode(pic, matrix, siting)
        assert np.array_equal(want, yuv.encode_numpy(pic, fmt))
        for src_off, dst_off in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1)):      # vector path where the size allows; offset frame; fp32 source + 4 bytes
            dst = torch.full((fmt.frame_bytes + dst_off + 2,), 0xA5, dtype=torch.uint8, device=dev)
            view = dst[dst_off:dst_off + fmt.frame_bytes]
            ops.f32_to_yuv420p10(view, fmt, f32_to_dev(x, dev, src_off), pad_top=pt, pad_left=pl)
            got = view.cpu().numpy().view("<u2")
            assert np.array_equal(got, want), (matrix, siting, src_off, dst_off, np.flatnonzero(got != want)[:4])     # every word written
            rest = dst.cpu().numpy()
            assert (rest[:dst_off] == 0xA5).all() and (rest[dst_off + fmt.frame_bytes:] == 0xA5).all()                # and nothing else


def test_encode_and_decode_1080p_once(ops, dev):
    """More than one grid-stride round is not reached at this size (16384 blocks cover it); it is the size the loops run at: the
    vectorised twins (held to the loop model on the CPU) on the vector and the general path."""
    H, W = 1080, 1920
    fmt = yuv.Format(H, W, "auto", False, "left", 10)
    buf = C10.random_frame(H, W, 10, seed=10)
    want = C10.replicate_pad(yuv.decode_numpy_f32(buf, fmt), 1088, 1920, 4, 0)
    df = decode_on_device(ops, dev, buf, fmt, (1088, 1920, 4, 0))
    assert np.array_equal(bits(df), want.view(np.uint32))
    assert torch.equal(decode_on_device(ops, dev, buf, fmt, (1088, 1920, 4, 0), offset=2), df)
    x = np.random.default_rng(5).uniform(-0.1, 1.1, (3, 1088, 1920)).astype(np.float32)
    want = yuv.encode_numpy(np.ascontiguousarray(x[:, 4:4 + H].transpose(1, 2, 0)), fmt)
    for dst_off in (0, 1):
        dst = torch.full((fmt.frame_bytes + dst_off,), 0xA5, dtype=torch.uint8, device=dev)[dst_off:]
        ops.f32_to_yuv420p10(dst, fmt, f32_to_dev(x, dev), pad_top=4, pad_left=0)
        assert np.array_equal(dst.cpu().numpy().view("<u2"), want)


def test_wrapper_refusals(ops, dev):
    fmt = yuv.Format(16, 16, depth=10)
    buf = to_dev(C10.random_frame(16, 16, 10), dev)
    dst = torch.empty(3, 16, 16, device=dev)
    with pytest.raises(ValueError, match="10-bit"):
        ops.yuv420p10_to_f32(buf[:fmt.frame_bytes // 2], fmt.as_8bit(), dst)
    with pytest.raises(ValueError):
        ops.yuv420p10_to_f32(buf[:-1], fmt, dst)
    with pytest.raises(ValueError):
        ops.yuv420p10_to_f32(buf.view(torch.int16), fmt, dst)
    with pytest.raises(ValueError):
        ops.yuv420p10_to_f32(buf, fmt, dst[:2])
    with pytest.raises(ValueError):
        ops.yuv420p10_to_f32(buf, fmt, dst.half())
    with pytest.raises(ValueError, match="even"):
        ops.yuv420p10_to_f32(buf, fmt, dst, window=(1, 0, 8, 8))
    with pytest.raises(ValueError, match="even"):
        ops.yuv420p10_to_f32(buf, fmt, dst, window=(0, 3, 8, 8))
    with pytest.raises(ValueError, match="outside"):
        ops.yuv420p10_to_f32(buf, fmt, dst, window=(8, 8, 10, 8))
    with pytest.raises(ValueError, match="smaller than the window"):
        ops.yuv420p10_to_f32(buf, fmt, dst, pad_left=4)
    with pytest.raises(ValueError, match="10-bit"):
        ops.f32_to_yuv420p10(buf[:fmt.frame_bytes // 2], fmt.as_8bit(), dst)
    with pytest.raises(ValueError):
        ops.f32_to_yuv420p10(buf[:-2], fmt, dst)
    with pytest.raises(ValueError):
        ops.f32_to_yuv420p10(buf, fmt, dst.permute(1, 2, 0))
    with pytest.raises(ValueError):
        ops.f32_to_yuv420p10(buf, fmt, torch.empty(16, 16, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="smaller than the frame"):
        ops.f32_to_yuv420p10(buf, fmt, dst, pad_top=1)
    # the 8-bit calls keep refusing 10-bit encodes
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(buf, fmt, src_u8=torch.empty(16, 16, 3, dtype=torch.uint8, device=dev))


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


def two_shot(n, fmt, seed=0):
    """10-bit I420 frames of two shots back to back: encoded at 10 bits from the uint8 shots, the two low bits of every sample random"""
    rng = np.random.default_rng(seed)
    out = []
    for f in CS.shot(n, fmt.height, fmt.width, seed=11, tone=60) + CS.shot(n, fmt.height, fmt.width, seed=12, tone=190):
        v = yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt)
        out.append(((v & ~np.uint16(3)) | rng.integers(0, 4, v.shape).astype(np.uint16)).astype(np.uint16))
    return out


class Reference:
    """The loops' frames from plain ``net.forward``: inputs decoded by ``ops.yuv420p10_to_f32`` into InputPadder's canvas, the recursion
    composed here in the loop's batch composition (``forward_pooled`` is documented bit-identical to ``forward``), the fp32 ``I_t``
    un-padded and encoded by ``yuv.encode_numpy``."""

    def __init__(self, net, ops, dev, fmt, window, divisor, max_batch=4):
        self.net, self.ops, self.dev, self.fmt, self.window, self.max_batch = net, ops, dev, fmt, window, max_batch
        _, _, h, w = window
        self.pl, pr, self.pt, pb = host_io.InputPadder((1, 3, h, w), divisor=divisor)._pad
        self.hp, self.wp = h + self.pt + pb, w + self.pl + pr
        self.out_fmt = fmt.cropped(h, w)

    def load(self, frame):
        t = torch.empty(1, 3, self.hp, self.wp, dtype=torch.float32, device=self.dev)
        self.ops.yuv420p10_to_f32(to_dev(frame, self.dev), self.fmt, t[0], window=self.window, pad_top=self.pt, pad_left=self.pl)
        return t

    def store(self, t):
        _, _, h, w = self.window
        img = t[0, :, self.pt:self.pt + h, self.pl:self.pl + w].permute(1, 2, 0).contiguous().cpu().numpy()
        return yuv.encode_numpy(img, self.out_fmt)

    def segment(self, a, b, factor, tta=False):
        fr = {0: self.load(a), factor: self.load(b)}
        shown = {}
        for level in mf.nx_levels(factor):
            for i in range(0, len(level), self.max_batch):
                chunk = level[i:i + self.max_batch]
                l = torch.cat([fr[x] for x, _, _ in chunk], 0).contiguous()
                r = torch.cat([fr[y] for _, y, _ in chunk], 0).contiguous()
                pred = self.net.forward(l, r)["I_t"].clone()
                out = pred
                if tta:
                    pf = self.net.forward(l.flip(2).flip(3).contiguous(), r.flip(2).flip(3).contiguous())["I_t"]
                    out = (pred + pf.flip(2).flip(3)) / 2
                for j, (_, _, pos) in enumerate(chunk):
                    fr[pos], shown[pos] = pred[j:j + 1], out[j:j + 1]
        return [self.store(shown[pos]) for pos in range(1, factor)]


def check_loop(got, ref, video, factor, s, cuts, tta=False):
    fmt, (y0, x0, h, w) = ref.fmt, ref.window
    whole = (h, w) == (fmt.height, fmt.width)
    n_seg = (len(video) - 1) // s
    assert len(got) == factor * n_seg + 1
    for seg in range(n_seg + 1):                       # originals: the caller's arrays
        g, src = got[seg * factor], video[seg * s]
        assert (g is src) if whole else (g.dtype == np.uint16 and np.array_equal(g, yuv.crop(src, fmt, y0, x0, h, w))), seg
    for seg in range(n_seg):
        a, b = video[seg * s], video[(seg + 1) * s]
        g = got[seg * factor + 1:(seg + 1) * factor]
        if seg in cuts:                                # copies of the 10-bit originals
            for pos in range(1, factor):
                src = a if pos <= factor // 2 else b
                assert g[pos - 1] is not src and g[pos - 1].dtype == np.uint16 and np.array_equal(g[pos - 1], yuv.crop(src, fmt, y0, x0, h, w))
        else:
            want = ref.segment(a, b, factor, tta)
            for pos in range(1, factor):
                assert g[pos - 1].dtype == np.uint16 and g[pos - 1].shape == (ref.out_fmt.frame_samples,)
                assert np.array_equal(g[pos - 1], want[pos - 1]), (seg, pos, int((g[pos - 1] != want[pos - 1]).sum()))


NX_CASES = [          # variant, H, W, factor, pool, tta, time_interval, crop, divisor
    ("lite", 64, 96, 4, True, False, 1, None, 32),
    ("lite", 64, 96, 4, False, False, 1, None, 32),
    ("lite", 64, 96, 8, True, False, 1, None, 32),
    ("lite", 64, 96, 8, False, False, 1, None, 32),
    ("lite", 64, 96, 4, True, True, 1, None, 32),
    ("lite", 64, 96, 4, False, True, 1, None, 32),
    ("lite", 80, 112, 4, True, False, 2, (64, 96), 32),
    ("base", 192, 320, 4, True, False, 1, None, 64),
]


@pytest.mark.parametrize("variant,H,W,factor,pool,tta,s,crop,divisor", NX_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_interpolate_video_nx_keeps_the_depth(nets, ops, dev, monkeypatch, variant, H, W, factor, pool, tta, s, crop, divisor):
    net = nets[variant]
    net.global_motion, net.ensemble_global_motion = True, False
    fmt = yuv.Format(H, W, "bt601", False, "centre", 10)
    video = two_shot(s + 1, fmt)
    window = mf.centre_window(H, W, crop)
    assert window[0] % 2 == 0 and window[1] % 2 == 0
    kw = dict(factor=factor, time_interval=s, crop=crop, divisor=divisor, tta=tta, max_batch=4, pool=pool)
    calls = count_forwards(monkeypatch, net)
    sc_8, sc_deep = scene.SceneCuts(), scene.SceneCuts()
    flat = list(host_io.interpolate_video_nx(iter(video), net, scene=sc_8, pixfmt=fmt, **kw))
    n_8 = dict(calls)
    got = list(host_io.interpolate_video_nx(iter(video), net, scene=sc_deep, pixfmt=fmt, keep_depth=True, **kw))
    n_deep = {k: calls[k] - n_8[k] for k in calls}
    n_seg = (len(video) - 1) // s
    # the cuts are the 8-bit path's, and a cut segment runs no forward: the forward counts are those of the run without keep_depth
    assert sc_deep.cuts == sc_8.cuts == [1] and sc_deep.stats == sc_8.stats and len(sc_deep.stats) == n_seg
    assert n_deep == n_8 and sum(n_8.values()) > 0
    per_seg = sum(-(-len(lv) // 4) for lv in mf.nx_levels(factor)) * (2 if tta else 1)
    assert sum(n_deep.values()) == per_seg * (n_seg - 1)
    assert all(f.dtype == np.uint8 for k, f in enumerate(flat) if k % factor and k // factor != 1)          # the default stays 8-bit
    check_loop(got, Reference(net, ops, dev, fmt, window, divisor), video, factor, s, {1}, tta)
    # without a scene detector nothing changes about the produced frames of the segments that are not cuts
    plain = list(host_io.interpolate_video_nx(iter(video[:s + 1]), net, pixfmt=fmt, keep_depth=True, **kw))
    assert len(plain) == factor + 1 and all(np.array_equal(x, y) for x, y in zip(plain, got[:factor + 1]))


@pytest.mark.parametrize("streams", [1, 2])
def test_interpolate_video_2x_keeps_the_depth(nets, ops, dev, monkeypatch, streams):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    H, W = 64, 96
    fmt = yuv.Format(H, W, "bt709", False, "left", 10)
    video = two_shot(3, fmt)
    calls = count_forwards(monkeypatch, net)
    for with_scene in (False, True):
        sc_8, sc_deep = (scene.SceneCuts(), scene.SceneCuts()) if with_scene else (None, None)
        n0 = calls["forward"]
        flat = list(host_io.interpolate_video_2x(iter(video), net, divisor=32, streams=streams, scene=sc_8, pixfmt=fmt))
        n_8 = calls["forward"] - n0
        got = list(host_io.interpolate_video_2x(iter(video), net, divisor=32, streams=streams, scene=sc_deep, pixfmt=fmt, keep_depth=True))
        assert calls["forward"] - n0 - n_8 == n_8 == (4 if with_scene else 5)
        cuts = set()
        if with_scene:
            assert sc_deep.cuts == sc_8.cuts == [2] and sc_deep.stats == sc_8.stats
            cuts = {2}
        assert [f.dtype for f in flat[1::2]] == [np.uint16 if k in cuts else np.uint8 for k in range(5)]
        check_loop(got, Reference(net, ops, dev, fmt, (0, 0, H, W), 32), video, 2, 1, cuts)


def test_keep_depth_changes_nothing_for_eight_bit_frames_on_the_device(nets, dev):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    fmt = yuv.Format(64, 96)
    video = [yuv.encode_numpy(f, fmt) for f in CS.shot(3, 64, 96, seed=11, tone=60)]
    for loop, kw in ((host_io.interpolate_video_2x, {}), (host_io.interpolate_video_nx, dict(factor=4))):
        a = list(loop(iter(video), net, divisor=32, pixfmt=fmt, **kw))
        b = list(loop(iter(video), net, divisor=32, pixfmt=fmt, keep_depth=True, **kw))
        assert len(a) == len(b) and all(x.dtype == y.dtype == np.uint8 and np.array_equal(x, y) for x, y in zip(a, b))


def test_interpolate_y4m_keeps_c420p10_on_the_device(nets, dev):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    H, W, n = 66, 98, 4
    fmt = yuv.Format(H, W, depth=10)
    video = two_shot(2, fmt)
    src, dst = io.BytesIO(), io.BytesIO()
    wr = yuv.Y4MWriter(src, fmt, Fraction(30000, 1001), aspect="1:1")
    for f in video:
        wr.write(f)
    src.seek(0)
    info = yuv.interpolate_y4m(src, dst, net, keep_depth=True, divisor=32)
    assert info == {"fps_in": Fraction(30000, 1001), "fps_out": Fraction(60000, 1001), "size": (W, H), "frames_in": n, "frames_out": 2 * n - 1}
    dst.seek(0)
    rd = yuv.Y4MReader(dst)
    assert rd.fmt == fmt and rd.fps == Fraction(60000, 1001) and rd.ctag == "420p10" and rd.aspect == "1:1"
    got = list(rd)
    want = list(host_io.interpolate_video_2x(iter(video), net, divisor=32, pixfmt=fmt, keep_depth=True))
    assert len(got) == len(want) == 2 * n - 1
    for k, g in enumerate(got):
        assert g.dtype == np.uint16 and np.array_equal(g, video[k // 2] if k % 2 == 0 else want[k]), k
    assert len(dst.getvalue()) == len(dst.getvalue().split(b"\n", 1)[0]) + 1 + (2 * n - 1) * (6 + fmt.frame_bytes)
    # 4x with flip-TTA goes through the N-x loop
    src.seek(0)
    dst = io.BytesIO()
    info = yuv.interpolate_y4m(src, dst, net, factor=4, tta=True, keep_depth=True, divisor=32)
    assert info["frames_out"] == 4 * (n - 1) + 1 and info["fps_out"] == Fraction(120000, 1001)
    dst.seek(0)
    got = list(yuv.Y4MReader(dst))
    want = list(host_io.interpolate_video_nx(iter(video), net, factor=4, tta=True, divisor=32, pixfmt=fmt, keep_depth=True))
    assert all(g.dtype == np.uint16 and np.array_equal(g, w_) for g, w_ in zip(got, want)) and len(got) == len(want)
    assert all(np.array_equal(got[4 * k], video[k]) for k in range(n))
