"""GPU: deep RGB frames on the device (csrc/rgb16.hip atmvfi_rgb16_decode / atmvfi_rgb16_encode; ``pixfmt=DeepRGB`` of the video loops).
Both kernels bit for bit against the per-sample loop models of tests/cpu_rgb16.py -- every layout, the aligned and the general path
(reached by size and by a pointer advanced by one sample), windows, unequal pads, either output alone, poisoned outputs between
guards, ties, clamps and a NaN pad region, the grid stride at 2160 x 4096 (there against the vectorised twins, which the CPU suite
holds to the loops: 26 million samples are no work for a Python loop) -- the host refusals, and the HIP loops: every produced frame is
``rgb16.encode_numpy`` of the fp32 ``I_t`` that ``model.forward`` returns on the ``rgb16_decode``d canvases."""
import importlib

import numpy as np
import pytest
import torch

import cpu_rgb16 as M
import cpu_scene as CS

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")
rgb16 = importlib.import_module("atm-vfi_amd.rgb16")
mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
scene = importlib.import_module("atm-vfi_amd.scene")

GUARD, POISON = 256, 0xA5         # bytes on each side of an output (a multiple of 16: the view keeps the allocation's alignment)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


@pytest.fixture(scope="module")
def net(dev):
    torch.set_grad_enabled(False)
    n = pkg.NetworkLite()
    n.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    n = n.to(dev).eval()
    n.global_motion, n.ensemble_global_motion = True, False
    return n


def on_dev(raw, dev, offset=0):
    """the bytes on the device, ``offset`` bytes past an allocation's start"""
    raw = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1))
    buf = torch.empty(raw.numel() + offset, dtype=torch.uint8, device=dev)
    buf[offset:].copy_(raw)
    return buf[offset:]


def poisoned(nbytes, dev, offset=0):
    """(the whole buffer, its nbytes view behind GUARD + offset bytes): POISON everywhere"""
    buf = torch.full((GUARD + offset + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD + offset:GUARD + offset + nbytes]


def guards_intact(buf, view):
    lo = view.data_ptr() - buf.data_ptr()
    return bool((buf[:lo] == POISON).all()) and bool((buf[lo + view.numel():] == POISON).all())


def decode_on(ops, dev, fmt, frame, window=None, canvas=None, pt=0, pl=0, f32=True, u8=True, offset=0):
    """-> (fp32 [3,Hp,Wp] or None, uint8 [h,w,3] or None) of the device call, both outputs poisoned beforehand between intact guards"""
    src = on_dev(frame, dev, offset)
    _, _, h, w = window or (0, 0, fmt.height, fmt.width)
    Hp, Wp = canvas or (h, w)
    fb = fv = ub = uv = None
    if f32:
        fb, fv = poisoned(12 * Hp * Wp, dev)
        fv = fv.view(torch.float32).view(3, Hp, Wp)
    if u8:
        ub, uv = poisoned(3 * h * w, dev)
        uv = uv.view(h, w, 3)
    ops.rgb16_decode(src, fmt, dst=fv, dst_u8=uv, window=window, pad_top=pt, pad_left=pl)
    torch.cuda.synchronize()
    assert (fb is None or guards_intact(fb, fv.view(-1).view(torch.uint8))) and (ub is None or guards_intact(ub, uv.view(-1)))
    return (None if fv is None else fv.cpu().numpy()), (None if uv is None else uv.cpu().numpy())


def encode_on(ops, dev, fmt, canvas, pt=0, pl=0, offset=0):
    src = torch.from_numpy(canvas).to(dev)
    buf, dst = poisoned(fmt.frame_bytes, dev, offset)
    ops.rgb16_encode(dst, fmt, src, pad_top=pt, pad_left=pl)
    torch.cuda.synchronize()
    assert guards_intact(buf, dst)
    return dst.cpu().numpy().view(np.uint16)


# (H, W, window or None, canvas or None, pad_top, pad_left)
GEOMETRIES = [
    (16, 16, None, None, 0, 0),                     # the aligned fast path
    (18, 22, None, None, 0, 0),                     # W % 4 != 0: the 2-byte path
    (16, 16, None, (32, 32), 8, 8),                 # the fast path with padding groups on all four sides
    (16, 32, (4, 8, 8, 16), (16, 32), 4, 12),       # an aligned window of the fast path, unequal pads
    (18, 22, (3, 5, 11, 13), (24, 32), 6, 9),       # odd origin and size, unequal pads on all four sides
    (18, 22, (0, 0, 18, 22), None, 0, 0),           # window == frame
    (18, 22, (17, 21, 1, 1), (3, 4), 1, 2),         # a 1 x 1 window
    (5, 260, None, (6, 264), 1, 4),                 # more than one block of lanes
]
DEPTH_CASES = [(layout, depth) for layout in M.LAYOUTS for depth in (10, 16)]


@pytest.mark.parametrize("layout,depth", DEPTH_CASES + [(layout, 12) for layout in M.LAYOUTS], ids=lambda v: str(v))
def test_both_kernels_are_the_sample_loops(ops, dev, layout, depth):
    geos = GEOMETRIES if depth != 12 else GEOMETRIES[:2] + GEOMETRIES[4:5]        # (depth 12 once per layout: one geometry per path)
    for H, W, window, canvas, pt, pl in geos:
        rng = np.random.default_rng(H * 1000 + W + depth)
        fmt = yuv.DeepRGB(H, W, depth, layout)
        frame = M.random_frame(rng, H, W, depth, over=True)
        want_f, want_u = M.decode_loop(frame, layout, depth, H, W, window, canvas, pt, pl)
        for offset in (0, 2):                       # the pointer advanced by one sample: the general path on the same shape
            for f32, u8 in ((True, True), (True, False), (False, True)):
                got_f, got_u = decode_on(ops, dev, fmt, frame, window, canvas, pt, pl, f32, u8, offset)
                assert (got_f is None) == (not f32) and (got_u is None) == (not u8)
                assert got_f is None or np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)), (H, W, window, offset, "fp32")
                assert got_u is None or np.array_equal(got_u, want_u), (H, W, window, offset, "probe")
        # the encode of the picture at the pads of a canvas whose pad region is NaN: never read
        _, _, h, w = window or (0, 0, H, W)
        Hp, Wp = canvas or (h, w)
        src = np.full((3, Hp, Wp), np.nan, np.float32)
        src[:, pt:pt + h, pl:pl + w] = rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)
        out = fmt.cropped(h, w)
        want = M.encode_loop(src, layout, depth, h, w, pt, pl)
        for offset in (0, 2):
            assert np.array_equal(encode_on(ops, dev, out, src, pt, pl, offset), want), (H, W, window, offset, "encode")


@pytest.mark.parametrize("depth", M.DEPTHS)
@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_encode_ties_clamps_and_every_code(ops, dev, layout, depth):
    top = M.top_of(depth)
    t = M.ties(depth)
    xs = np.array([x for x, _ in t] + [-0.0, 0.0, -1.0, -1e30, 1.0, 1.0 + 2.0 ** -20, 2.0, 1e30, 0.5 / top * 0.999, 1.0 - 0.25 / top], np.float32)
    want = np.array([k for _, k in t] + [0, 0, 0, 0, top, top, top, top, 0, top], np.uint16)
    xs, want = np.resize(xs, 64), np.resize(want, 64)
    for W in (64, 63):                              # both paths
        fmt = yuv.DeepRGB(1, W, depth, layout)
        src = np.full((3, 3, 72), np.nan, np.float32)
        src[:, 1, 4:4 + W] = np.stack([xs[:W], xs[:W][::-1], xs[:W]])
        got = encode_on(ops, dev, fmt, src, 1, 4)
        assert np.array_equal(got, M.encode_loop(src, layout, depth, 1, W, 1, 4))
        assert np.array_equal(got[[M.sample_index(layout, 1, W, 0, x, 0) for x in range(W)]], want[:W])
    # every code survives decode -> encode on the device, and decodes to the division's bits
    n = top + 1
    fmt = yuv.DeepRGB(1, n, depth, layout)
    rgb = np.stack([np.arange(n), np.arange(n)[::-1], (np.arange(n) * 7) % n], axis=1).astype(np.uint16).reshape(1, n, 3)
    frame = rgb16._layout_of(rgb, fmt)
    f, u = decode_on(ops, dev, fmt, frame)
    assert np.array_equal(f, (rgb.astype(np.float32) / np.float32(top)).transpose(2, 0, 1)) and np.array_equal(u, (rgb >> (depth - 8)).astype(np.uint8))
    assert np.array_equal(encode_on(ops, dev, fmt, f), frame)


_big = {}


@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_grid_stride_at_2160x4096(ops, dev, layout):
    """2160 x 1024 groups of four pixels exceed grid_for's 8192 x 256 lanes: the one size at which the walk takes a second step"""
    H, W = 2160, 4096
    assert H * (W // 4) > 8192 * 256
    if "frame" not in _big:
        rng = np.random.default_rng(99)
        _big["frame"] = rng.integers(0, 65536, 3 * H * W, dtype=np.uint16)
        _big["canvas"] = rng.uniform(-0.05, 1.05, (3, H, W)).astype(np.float32)
    fmt = yuv.DeepRGB(H, W, 16, layout)
    frame, canvas = _big["frame"], _big["canvas"]
    f, u = decode_on(ops, dev, fmt, frame)
    assert np.array_equal(f, rgb16.decode_numpy_f32(frame, fmt).transpose(2, 0, 1)) and np.array_equal(u, rgb16.probe_numpy(frame, fmt))
    got = encode_on(ops, dev, fmt, canvas)
    assert np.array_equal(got, rgb16.encode_numpy(np.ascontiguousarray(canvas.transpose(1, 2, 0)), fmt))


def test_refusals_return_without_launching(ops, dev):
    fmt = yuv.DeepRGB(16, 16, 16, "rgb48")
    src = on_dev(np.zeros(fmt.frame_samples, np.uint16), dev)
    canvas = torch.full((3, 16, 16), 7.0, device=dev)
    u8 = torch.full((16, 16, 3), 9, dtype=torch.uint8, device=dev)
    lib, st, err = ops.lib, ops._stream(), lambda: ops.lib.atmvfi_last_error().decode()
    S, C, U = src.data_ptr(), canvas.data_ptr(), u8.data_ptr()

    def dec(src=S, H=16, W=16, depth=16, layout=0, y0=0, x0=0, h=16, w=16, dst=C, Hp=16, Wp=16, pt=0, pl=0, u8=U):
        return lib.atmvfi_rgb16_decode(src, H, W, depth, layout, y0, x0, h, w, dst, Hp, Wp, pt, pl, u8, st)

    def enc(src=C, Hp=16, Wp=16, pt=0, pl=0, dst=S, H=16, W=16, depth=16, layout=0):
        return lib.atmvfi_rgb16_encode(src, Hp, Wp, pt, pl, dst, H, W, depth, layout, st)
    for kw, msg in ((dict(src=None), "null source"), (dict(dst=None, u8=None), "both outputs are null"), (dict(depth=8), "depth must be"),
                    (dict(layout=3), "unknown layout 3"), (dict(H=0), "zero size"), (dict(y0=1), "outside"), (dict(x0=8, w=9), "outside"),
                    (dict(Hp=15), "Hp 15 < h 16"), (dict(pl=1), "Wp 16 < w 16 + pad_left 1"), (dict(src=S + 1), "2-byte aligned")):
        assert dec(**kw) == -1 and "rgb16_decode" in err() and msg in err(), (kw, err())
    for kw, msg in ((dict(src=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(depth=11), "depth must be"),
                    (dict(layout=-1), "unknown layout"), (dict(Hp=15), "bad geometry"), (dict(pl=1), "bad geometry"), (dict(dst=S + 1), "2-byte aligned")):
        assert enc(**kw) == -1 and "rgb16_encode" in err() and msg in err(), (kw, err())
    torch.cuda.synchronize()
    assert bool((canvas == 7.0).all()) and bool((u8 == 9).all()) and bool((src == 0).all())        # nothing ran
    # the wrapper's own
    for call, msg in ((lambda: ops.rgb16_decode(src, fmt), "give dst, dst_u8 or both"),
                      (lambda: ops.rgb16_decode(src[:-2], fmt, dst=canvas), "source buf must be a contiguous CUDA uint8 tensor of 1536 bytes"),
                      (lambda: ops.rgb16_decode(src, yuv.Format(16, 16), dst=canvas), "a yuv.DeepRGB expected"),
                      (lambda: ops.rgb16_decode(src, fmt, dst=canvas, window=(8, 8, 9, 8)), "outside the 16 x 16 frame"),
                      (lambda: ops.rgb16_decode(src, fmt, dst=canvas, pad_top=1), "smaller than the window"),
                      (lambda: ops.rgb16_decode(src, fmt, dst_u8=u8[:8]), "dst_u8"),
                      (lambda: ops.rgb16_encode(src, fmt, None), "src must be"),
                      (lambda: ops.rgb16_encode(src, fmt, canvas, pad_left=4), "smaller than the frame"),
                      (lambda: ops.yuv_encode(src, fmt, src_u8=u8), "fp32 src")):
        with pytest.raises(ValueError, match=msg):
            call()


# ------------------------------------------------------------------------------------------------ the loops
H, W, DIV = 64, 96, 64


def deep_video(fmt, rgb8, seed=17):
    """uint8 RGB frames -> frames of ``fmt`` ([H,W,3] or [3,H,W]: the caller's shape) that use the depth's low bits"""
    rng = np.random.default_rng(seed)
    out = []
    for f in rgb8:
        q = (f.astype(np.int64) * M.top_of(fmt.depth)) // 255
        q = np.clip(q + rng.integers(-3, 4, q.shape), 0, M.top_of(fmt.depth)).astype(np.uint16)
        out.append(rgb16._layout_of(q, fmt).reshape((3, fmt.height, fmt.width) if fmt.layout == "gbrp" else (fmt.height, fmt.width, 3)))
    return out


def two_shot(fmt, n=2, h=H, w=W):
    return deep_video(fmt, CS.shot(n, h, w, seed=11, tone=60) + CS.shot(n, h, w, seed=12, tone=190))


def count_forwards(monkeypatch, net):
    calls = {"forward": 0, "forward_pooled": 0}
    for name in calls:
        klass = next(k for k in type(net).__mro__ if name in k.__dict__)

        def wrapper(self, *a, _orig=klass.__dict__[name], _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(klass, name, wrapper)
    return calls


class Reference:
    """The loops' frames from plain ``net.forward``: inputs decoded by ``ops.rgb16_decode`` into InputPadder's canvas, the recursion
    composed here in the loop's batch composition (``forward_pooled`` is documented bit-identical to ``forward``), the fp32 ``I_t``
    un-padded and encoded by ``rgb16.encode_numpy``."""

    def __init__(self, net, ops, dev, fmt, window, divisor=DIV, max_batch=4):
        self.net, self.ops, self.dev, self.fmt, self.window, self.max_batch = net, ops, dev, fmt, window, max_batch
        _, _, h, w = window
        self.pl, pr, self.pt, pb = host_io.InputPadder((1, 3, h, w), divisor=divisor)._pad
        self.hp, self.wp = h + self.pt + pb, w + self.pl + pr
        self.out_fmt = fmt.cropped(h, w)

    def load(self, frame):
        t = torch.empty(1, 3, self.hp, self.wp, dtype=torch.float32, device=self.dev)
        self.ops.rgb16_decode(on_dev(frame, self.dev), self.fmt, dst=t[0], window=self.window, pad_top=self.pt, pad_left=self.pl)
        return t

    def store(self, t):
        _, _, h, w = self.window
        img = t[0, :, self.pt:self.pt + h, self.pl:self.pl + w].permute(1, 2, 0).contiguous().cpu().numpy()
        return rgb16.encode_numpy(img, self.out_fmt)

    def segment(self, a, b, factor, tta=False, levels=None, emit=None):
        fr = {0: self.load(a), factor: self.load(b)}
        shown = {}
        for level in (mf.nx_levels(factor) if levels is None else levels):
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
        return [self.store(shown[pos]) for pos in (range(1, factor) if emit is None else emit)]


def check_loop(got, ref, video, factor, s=1, cuts=(), tta=False):
    fmt, (y0, x0, h, w) = ref.fmt, ref.window
    whole = (h, w) == (fmt.height, fmt.width)
    n_seg = (len(video) - 1) // s
    assert len(got) == factor * n_seg + 1
    for seg in range(n_seg + 1):                       # originals: the caller's arrays
        g, src = got[seg * factor], video[seg * s]
        assert (g is src) if whole else (g.dtype == np.uint16 and np.array_equal(g, rgb16.crop(src, fmt, y0, x0, h, w))), seg
    for seg in range(n_seg):
        a, b = video[seg * s], video[(seg + 1) * s]
        g = got[seg * factor + 1:(seg + 1) * factor]
        if seg in cuts:                                # copies of the caller's arrays
            for pos in range(1, factor):
                src = a if pos <= factor // 2 else b
                assert g[pos - 1] is not src and g[pos - 1].dtype == np.uint16
                assert np.array_equal(g[pos - 1], src if whole else rgb16.crop(src, fmt, y0, x0, h, w))
        else:
            want = ref.segment(a, b, factor, tta)
            for pos in range(1, factor):
                assert g[pos - 1].dtype == np.uint16 and g[pos - 1].shape == (ref.out_fmt.frame_samples,)
                assert np.array_equal(g[pos - 1], want[pos - 1]), (seg, pos, int((g[pos - 1] != want[pos - 1]).sum()))


NX_CASES = [          # layout, depth, H, W, factor, pool, tta, time_interval, crop
    ("rgb48", 16, 64, 96, 4, True, False, 1, None),
    ("rgb48", 16, 64, 96, 4, False, False, 1, None),
    ("gbrp", 10, 64, 96, 8, True, False, 1, None),
    ("gbrp", 12, 64, 96, 4, True, True, 1, None),
    ("bgr48", 16, 64, 96, 4, True, False, 1, (48, 80)),
    ("gbrp", 10, 64, 96, 4, True, False, 2, None),
]


@pytest.mark.parametrize("layout,depth,H_,W_,factor,pool,tta,s,crop", NX_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_interpolate_video_nx_on_deep_rgb(net, ops, dev, layout, depth, H_, W_, factor, pool, tta, s, crop):
    fmt = yuv.DeepRGB(H_, W_, depth, layout)
    video = deep_video(fmt, CS.shot(2 * s + 1, H_, W_, seed=11, tone=100))
    keep = [v.copy() for v in video]
    window = mf.centre_window(H_, W_, crop)
    kw = dict(factor=factor, time_interval=s, crop=crop, divisor=DIV, tta=tta, max_batch=4, pixfmt=fmt, keep_depth=True)
    got = list(host_io.interpolate_video_nx(iter(video), net, pool=pool, **kw))
    check_loop(got, Reference(net, ops, dev, fmt, window), video, factor, s, (), tta)
    assert all(np.array_equal(a, b) for a, b in zip(video, keep))      # the caller's buffers are untouched
    if pool:                                                            # pooled equals plain
        plain = list(host_io.interpolate_video_nx(iter(video), net, pool=False, **kw))
        assert len(plain) == len(got) and all(np.array_equal(x, y) for x, y in zip(plain, got))


def test_2x_loop_and_frame_pipeline_on_deep_rgb(net, ops, dev):
    fmt = yuv.DeepRGB(H, W, 12, "gbrp")
    video = deep_video(fmt, CS.shot(3, H, W, seed=11, tone=100))
    ref = Reference(net, ops, dev, fmt, (0, 0, H, W))
    got = list(host_io.interpolate_video_2x(iter(video), net, divisor=DIV, pixfmt=fmt, keep_depth=True))
    check_loop(got, ref, video, 2)
    pipe = host_io.FramePipeline(net, H, W, divisor=DIV, pixfmt=fmt, keep_depth=True)
    mids = list(pipe.run(zip(video, video[1:])))
    assert len(mids) == 2 and all(np.array_equal(m, g) for m, g in zip(mids, got[1::2]))
    with pytest.raises(ValueError, match="keep_depth"):
        host_io.FramePipeline(net, H, W, divisor=DIV, pixfmt=fmt)
    with pytest.raises(ValueError, match="keep_depth"):
        list(host_io.interpolate_video_2x(iter(video), net, divisor=DIV, pixfmt=fmt))


def test_retimed_24_to_60_with_dedup_on_deep_rgb(net, ops, dev):
    fmt = yuv.DeepRGB(H, W, 10, "gbrp")
    video = deep_video(fmt, CS.shot(5, H, W, seed=11, tone=100)[::2])   # (two pixels of drift per frame: no false duplicate)
    video = video[:2] + [video[1].copy()] + video[2:]                  # a repeated frame
    d, L = rt.Duplicates(), 2
    got = list(host_io.interpolate_video_retimed(iter(video), net, 24, 60, levels=L, divisor=DIV, dedup=d, pixfmt=fmt, keep_depth=True))
    assert d.dropped == [2]
    kept = [i for i in range(len(video)) if i not in d.dropped]
    slots = list(rt.retime_slots(kept, 24, 60, L))
    assert len(got) == len(slots)
    ref, n, made = Reference(net, ops, dev, fmt, (0, 0, H, W)), 1 << L, {}
    for j in sorted({j for j, _ in slots}):
        interior = sorted({p for jj, p in slots if jj == j and 0 < p < n})
        if interior:
            frames = ref.segment(video[kept[j]], video[kept[j + 1]], n, levels=rt.sparse_levels(interior, L), emit=interior)
            made.update({(j, p): f for p, f in zip(interior, frames)})
    assert made
    for g, (j, p) in zip(got, slots):
        if p in (0, n):
            assert g is video[kept[j + (p == n)]]
        else:
            assert g.dtype == np.uint16 and np.array_equal(g, made[j, p]), (j, p)


def test_depth_16_of_257_b_is_the_uint8_loop(net, ops, dev):
    rgb8 = CS.shot(3, H, W, seed=11, tone=100)
    fmt = yuv.DeepRGB(H, W, 16, "rgb48")
    video = [(f.astype(np.uint16) * 257) for f in rgb8]
    # the network's inputs are the uint8 path's, bit for bit, and so is what forward returns on them
    pl, pr, pt, pb = host_io.InputPadder((1, 3, H, W), divisor=DIV)._pad
    a16, a8, b16, b8 = (torch.empty(1, 3, H + pt + pb, W + pl + pr, device=dev) for _ in range(4))
    for f8, f16, t8, t16 in ((rgb8[0], video[0], a8, a16), (rgb8[1], video[1], b8, b16)):
        ops.rgb16_decode(on_dev(f16, dev), fmt, dst=t16[0], pad_top=pt, pad_left=pl)
        ops.frame_u8_to_f32(torch.from_numpy(f8).to(dev), t8[0], pt, pl, False)
    assert torch.equal(a16, a8) and torch.equal(b16, b8)
    assert torch.equal(net.forward(a16, b16)["I_t"].clone(), net.forward(a8, b8)["I_t"].clone())
    kw = dict(factor=4, divisor=DIV, max_batch=4)
    got16 = list(host_io.interpolate_video_nx(iter(video), net, pixfmt=fmt, keep_depth=True, **kw))
    got8 = list(host_io.interpolate_video_nx(iter(rgb8), net, isBGR=False, **kw))
    assert len(got16) == len(got8) == 9
    for k, (g16, g8) in enumerate(zip(got16, got8)):
        if k % 4:
            # p16 = rint(65535 x), p8 = rint(255 x) of the same x: |p16 / 257 - 255 x| <= 0.5 / 257 and |255 x - p8| <= 0.5
            gap = np.abs(g16.astype(np.float64) / 257 - g8.reshape(-1))
            print(f"frame {k}: max |p16 / 257 - p8| = {gap.max():.6f}")
            assert gap.max() <= 0.5 + 1 / 257


def test_scene_cuts_are_those_of_the_truncated_picture(net, ops, dev, monkeypatch):
    fmt = yuv.DeepRGB(H, W, 16, "rgb48")
    video = two_shot(fmt)
    video8 = [(v >> 8).astype(np.uint8) for v in video]
    calls = count_forwards(monkeypatch, net)
    kw = dict(factor=4, divisor=DIV, max_batch=4)
    s16, s8 = scene.SceneCuts(), scene.SceneCuts()
    list(host_io.interpolate_video_nx(iter(video8), net, isBGR=False, scene=s8, **kw))
    n8 = sum(calls.values())
    got = list(host_io.interpolate_video_nx(iter(video), net, pixfmt=fmt, keep_depth=True, scene=s16, **kw))
    assert s16.cuts == s8.cuts == [1] and s16.stats == s8.stats
    assert sum(calls.values()) - n8 == n8 > 0                           # no forward runs for the cut segment, as in the uint8 loop
    check_loop(got, Reference(net, ops, dev, fmt, (0, 0, H, W)), video, 4, 1, {1})
    # the 2x loop and the rate conversion decide alike
    s2 = scene.SceneCuts()
    two = list(host_io.interpolate_video_2x(iter(video), net, divisor=DIV, pixfmt=fmt, keep_depth=True, scene=s2))
    assert s2.cuts == [1] and np.array_equal(two[3], video[1]) and two[3] is not video[1]
    s3, s3_8 = scene.SceneCuts(), scene.SceneCuts()
    list(host_io.interpolate_video_retimed(iter(video), net, 24, 60, levels=2, divisor=DIV, pixfmt=fmt, keep_depth=True, scene=s3))
    list(host_io.interpolate_video_retimed(iter(video8), net, 24, 60, levels=2, divisor=DIV, isBGR=False, scene=s3_8))
    assert s3.cuts == s3_8.cuts and s3.cuts and s3.stats == s3_8.stats


def test_layouts_give_the_same_samples_permuted(net, dev):
    rgb8 = CS.shot(2, H, W, seed=11, tone=100)
    kw = dict(factor=4, divisor=DIV, max_batch=4, keep_depth=True)
    for depth, other in ((10, "gbrp"), (16, "bgr48")):
        base, fmt = yuv.DeepRGB(H, W, depth, "rgb48"), yuv.DeepRGB(H, W, depth, other)
        P = deep_video(base, rgb8)
        Q = [rgb16._layout_of(p, fmt) for p in P]
        want = list(host_io.interpolate_video_nx(iter(P), net, pixfmt=base, **kw))
        got = list(host_io.interpolate_video_nx(iter(Q), net, pixfmt=fmt, **kw))
        assert len(got) == len(want) == 5
        for k in (1, 2, 3):
            assert np.array_equal(got[k], rgb16._layout_of(want[k].reshape(H, W, 3), fmt)) and not np.array_equal(got[k], want[k])
