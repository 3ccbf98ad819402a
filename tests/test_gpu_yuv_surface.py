"""GPU: decoder surfaces on the device (csrc/yuv.hip atmvfi_yuv_decode, csrc/yuv_encode.hip atmvfi_yuv_encode,
``pixfmt=yuv.Surface(...)`` of the video loops): both entry points against the per-sample loop model of tests/cpu_yuv_surface.py
(small shapes) and the numpy twins (large ones; the CPU suite holds them to the model), bit for bit -- planar / uv / vu, 8 bit,
10 -> 8 bit, 10 bit kept, msb, both sitings, the vector and the general path reached every way, poisoned destinations and padding --
then equality with the planar entry points, and the loops against ``repack`` of their I420 runs."""
import importlib
import itertools

import numpy as np
import pytest
import torch

import cpu_scene as CS
import cpu_yuv_surface as M

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")

KINDS = {"8": (8, False), "10": (10, False), "10msb": (10, True)}
SITINGS = ("centre", "left")


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


def to_dev(arr, dev, offset=0):
    """The bytes of ``arr`` on the device as a 1-D uint8 tensor whose pointer is ``offset`` bytes past an allocation's start."""
    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy())
    buf = torch.empty(raw.numel() + offset, dtype=torch.uint8, device=dev)
    view = buf[offset:]
    view.copy_(raw)
    return view


def surfaces(H, W, chroma, depth, msb, **fkw):
    """tight; a pitch that is no multiple of 4 with a chroma offset beyond pitch * H; pitches and offset multiples of 4"""
    fmt = yuv.Format(H, W, depth=depth, **fkw)
    b, cw = (2 if depth == 10 else 1), (W + 1) // 2
    crow = (cw if chroma == "planar" else 2 * cw) * b
    odd = lambda n: next(p for p in range(n + b, n + 16, b) if p % 4)
    mul4 = lambda n: (n + 11) // 4 * 4
    return [yuv.Surface(fmt, chroma, msb),
            yuv.Surface(fmt, chroma, msb, pitch=odd(W * b), chroma_pitch=odd(crow), chroma_offset=odd(W * b) * H + 3 * b),
            yuv.Surface(fmt, chroma, msb, pitch=mul4(W * b), chroma_pitch=mul4(crow), chroma_offset=mul4(W * b) * H + 8)]


def layout_of(s):
    return M.layout(s.height, s.width, s.depth, s.chroma, s.msb, s.pitch, s.chroma_pitch, s.chroma_offset)


def fill(s, seed, poison):
    """A frame of ``s`` with seeded random samples over the whole range (msb: the low six bits random too) and every padding byte
    ``poison``: vectorised, for the sizes the loop model is too slow for."""
    rng = np.random.default_rng(seed)
    buf = np.full(s.nbytes, poison, np.uint8).view(s.dtype).copy()
    for p in s.planes(buf):
        p[...] = rng.integers(0, 65536 if s.msb else (1024 if s.depth == 10 else 256), p.shape).astype(s.dtype)
    return buf


def canvas_of(h, w):
    """(Hp, Wp, pad_top, pad_left): an odd top padding; multiples of 4 across when w is one (the vector path's geometry)."""
    return (h + 5, w + 12, 3, 4) if w % 4 == 0 else (h + 4, w + 7, 1, 3)


def padded(q, geo, top):
    """int [h,w,3] pixels -> the fp32 canvas [3,Hp,Wp] = q / top with replicate padding, as uint32 bits"""
    Hp, Wp, pt, pl = geo
    h, w = q.shape[:2]
    x = (q.astype(np.float32) / np.float32(top)).transpose(2, 0, 1)
    return np.ascontiguousarray(np.pad(x, ((0, 0), (pt, Hp - h - pt), (pl, Wp - w - pl)), mode="edge")).view(np.uint32)


def run_decode(ops, dev, buf, s, geo=None, window=None, keep=False, u8=False, bgr=False, offset=0):
    """-> (fp32 canvas bits or None, uint8 window or None); both destinations poisoned before the call"""
    h, w = (s.height, s.width) if window is None else window[2:]
    dst = dst_u8 = None
    if geo is not None:
        dst = torch.full((3, geo[0], geo[1]), float("nan"), dtype=torch.float32, device=dev)
    if u8:
        dst_u8 = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device=dev)
    pt, pl = (geo[2], geo[3]) if geo is not None else (0, 0)
    ops.yuv_surface_decode(to_dev(buf, dev, offset), s, dst_u8=dst_u8, dst=dst, window=window, pad_top=pt, pad_left=pl, bgr=bgr, keep_depth=keep)
    return (None if dst is None else dst.cpu().numpy().view(np.uint32)), (None if dst_u8 is None else dst_u8.cpu().numpy())


def check_decode(ops, dev, buf, s, want, want10, geos, window=None, offsets=(0,)):
    """``want`` int [h,w,3] 0..255, ``want10`` 0..1023 or None: every output of the call, on every geometry and pointer offset"""
    for geo, off in itertools.product(geos, offsets):
        f, u = run_decode(ops, dev, buf, s, geo, window, u8=True, offset=off)
        assert np.array_equal(u, want.astype(np.uint8)), (s, geo, off, "u8")
        assert np.array_equal(f, padded(want, geo, 255)), (s, geo, off, "f32", np.argwhere(f != padded(want, geo, 255))[:3])
        if want10 is not None:
            f, _ = run_decode(ops, dev, buf, s, geo, window, keep=True, offset=off)
            assert np.array_equal(f, padded(want10, geo, 1023)), (s, geo, off, "keep")
    _, u = run_decode(ops, dev, buf, s, None, window, u8=True, bgr=True)
    assert np.array_equal(u, want[:, :, ::-1].astype(np.uint8)), (s, "bgr")


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("chroma", yuv.CHROMAS)
@pytest.mark.parametrize("H,W,wins", [(1, 1, []), (3, 5, [(2, 2, 1, 3)]), (8, 16, [(2, 2, 5, 13), (0, 4, 8, 12), (4, 2, 4, 8)])],
                         ids=lambda v: str(v)[:8])
def test_decode_is_the_loop_model(ops, dev, H, W, wins, chroma, kind):
    """1 x 1, 3 x 5 (general) and 8 x 16 (the vector path on the tight and the multiple-of-4 layout, the general path through a pitch
    that is no multiple of 4, a pointer offset by one sample, pad_left 3 and windows at x0 = 2; (0, 4, 8, 12) is a vector window)."""
    depth, msb = KINDS[kind]
    for k, siting in enumerate(SITINGS):
        matrix = ("bt601", "bt709")[k]
        for n, s in enumerate(surfaces(H, W, chroma, depth, msb, matrix=matrix, siting=siting)):
            L = layout_of(s)
            buf = M.random_surface(L, seed=31 * H + 7 * k + n, poison=(0xFF, 0x00, 0x5A)[n])
            kw = dict(matrix=matrix, siting=siting)
            want = M.decode(buf, L, **kw)
            want10 = M.decode(buf, L, keep=True, **kw) if depth == 10 else None
            assert np.array_equal(want.astype(np.uint8), yuv.decode_numpy(buf, s))
            check_decode(ops, dev, buf, s, want, want10, [canvas_of(H, W), (H + 4, W + 7, 1, 3), (H, W, 0, 0)], offsets=(0, s.itemsize))
            for win in wins:
                w10 = M.decode(buf, L, window=win, keep=True, **kw) if depth == 10 else None
                check_decode(ops, dev, buf, s, M.decode(buf, L, window=win, **kw), w10, [canvas_of(*win[2:])], window=win)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("chroma", yuv.CHROMAS)
def test_decode_40x1100_is_the_twin(ops, dev, chroma, kind):
    """Several column groups and workgroups (40 x 1100: 20 row pairs x 278 groups = 22 blocks), the vector and the general path."""
    H, W = 40, 1100
    depth, msb = KINDS[kind]
    siting = SITINGS[(len(chroma) + depth) % 2]
    for n, s in enumerate(surfaces(H, W, chroma, depth, msb, siting=siting)):
        bufs = [fill(s, 5 + n, poison) for poison in (0xFF, 0x00)]           # padding that would change the result if it were read
        want = yuv.decode_numpy(bufs[0], s).astype(np.int32)
        want10 = np.rint(yuv.decode_numpy_f32(bufs[0], s).astype(np.float64) * 1023).astype(np.int32) if depth == 10 else None
        for buf in bufs:
            check_decode(ops, dev, buf, s, want, want10, [canvas_of(H, W)], offsets=(0, s.itemsize) if n == 0 else (0,))
        win = (2, 2, 37, 1001)
        w10 = np.rint(yuv.decode_numpy_f32(bufs[0], s, window=win).astype(np.float64) * 1023).astype(np.int32) if depth == 10 else None
        check_decode(ops, dev, bufs[0], s, yuv.window_numpy(bufs[0], s, 0, *win).astype(np.int32), w10, [canvas_of(37, 1001)], window=win)


@pytest.mark.parametrize("name", ["nv12", "p010", "nv21", "i420"])
def test_the_vector_path_at_pitch_2048(ops, dev, name):
    """8 x 1920 at pitch 2048 (what a decoder hands over for 1080p), everything aligned: the vector path; the 128 padding bytes of
    every row poisoned two ways."""
    H, W = 8, 1920
    s = {"nv12": yuv.Surface.nv12(H, W, pitch=2048), "p010": yuv.Surface.p010(H, W, pitch=4096, chroma_offset=4096 * 16, siting="left"),
         "nv21": yuv.Surface(yuv.Format(H, W, siting="left"), "vu", pitch=2048, chroma_pitch=2048), "i420": yuv.Surface.i420(H, W, pitch=2048)}[name]
    bufs = [fill(s, 9, poison) for poison in (0xFF, 0x00)]
    want = yuv.decode_numpy(bufs[0], s).astype(np.int32)
    want10 = np.rint(yuv.decode_numpy_f32(bufs[0], s).astype(np.float64) * 1023).astype(np.int32) if s.depth == 10 else None
    for buf in bufs:
        check_decode(ops, dev, buf, s, want, want10, [(H + 8, W, 4, 0)])
    win = (2, 4, 6, 1912)
    check_decode(ops, dev, bufs[1], s, yuv.window_numpy(bufs[1], s, 0, *win).astype(np.int32), None, [canvas_of(6, 1912)], window=win)


# ------------------------------------------------------------------------------------------------ encode
def sources(H, W, depth, seed):
    """(uint8 RGB or None, fp32 canvas [3,Hp,Wp] with NaN outside the frame, its frame [H,W,3], geometry)"""
    rng = np.random.default_rng(seed)
    Hp, Wp, pt, pl = canvas_of(H, W)
    pic = rng.uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32)
    top = 1023 if depth == 10 else 255
    ties = ((np.arange(top) + 0.5) / top).astype(np.float32)
    m = rng.random(pic.shape) < 0.2
    pic[m] = ties[rng.integers(0, top, int(m.sum()))]
    x = np.full((3, Hp, Wp), np.nan, np.float32)
    x[:, pt:pt + H, pl:pl + W] = pic.transpose(2, 0, 1)
    return (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) if depth == 8 else None), x, pic, (Hp, Wp, pt, pl)


def run_encode(ops, dev, s, offset=0, **kw):
    """-> the surface's bytes; the destination and guards around it poisoned"""
    dst = torch.full((s.nbytes + offset + 4,), 0xA5, dtype=torch.uint8, device=dev)
    ops.yuv_surface_encode(dst[offset:offset + s.nbytes], s, **kw)
    got = dst.cpu().numpy()
    assert (got[:offset] == 0xA5).all() and (got[offset + s.nbytes:] == 0xA5).all()
    return got[offset:offset + s.nbytes]


def check_encode(ops, dev, s, want_of, seed, offsets=(0, 1)):
    """``want_of(pixel source) -> bytes``: from uint8 RGB and BGR (8 bit) and from the fp32 canvas, on every destination offset"""
    rgb, x, pic, (Hp, Wp, pt, pl) = sources(s.height, s.width, s.depth, seed)
    for off in offsets:
        if rgb is not None:
            want = want_of(rgb)
            assert np.array_equal(run_encode(ops, dev, s, off, src_u8=torch.from_numpy(rgb).to(dev)), want), (s, off, "rgb")
            bgr = torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1])).to(dev)
            assert np.array_equal(run_encode(ops, dev, s, off, src_u8=bgr, bgr=True), want), (s, off, "bgr")
        got = run_encode(ops, dev, s, off, src=torch.from_numpy(x).to(dev), pad_top=pt, pad_left=pl)
        assert np.array_equal(got, want_of(pic)), (s, off, "f32", np.flatnonzero(got != want_of(pic))[:4])
    whole = torch.full((x.size + 1,), float("nan"), dtype=torch.float32, device=dev)          # a canvas that is only 4-byte aligned
    whole[1:].copy_(torch.from_numpy(x).reshape(-1))
    got = run_encode(ops, dev, s, 0, src=whole[1:].view(*x.shape), pad_top=pt, pad_left=pl)
    assert np.array_equal(got, want_of(pic))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("chroma", yuv.CHROMAS)
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 16)], ids=lambda v: str(v))
def test_encode_is_the_loop_model(ops, dev, H, W, chroma, kind):
    depth, msb = KINDS[kind]
    for k, siting in enumerate(SITINGS):
        matrix = ("bt709", "bt601")[k]
        s = yuv.Surface(yuv.Format(H, W, matrix, False, siting, depth), chroma, msb)
        L = layout_of(s)
        check_encode(ops, dev, s, lambda src: M.encode(M.pixels(src, depth), L, matrix=matrix, siting=siting), seed=H * W + k)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("chroma", yuv.CHROMAS)
def test_encode_40x1100_is_the_twin(ops, dev, chroma, kind):
    depth, msb = KINDS[kind]
    s = yuv.Surface(yuv.Format(40, 1100, siting=SITINGS[(len(chroma) + depth) % 2], depth=depth), chroma, msb)
    as_source = lambda src: src if (depth == 10 or src.dtype == np.uint8) else M.pixels(src, 8).astype(np.uint8)     # (the fp32 source's pixel)
    check_encode(ops, dev, s, lambda src: yuv.encode_numpy(as_source(src), s).astype("<u2" if depth == 10 else np.uint8).view(np.uint8), seed=3)


# ------------------------------------------------------------------------------------------------ 4K, once
@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_2160x4096_once(ops, dev, name):
    """The largest picture of the suite (1080 x 1024 lanes, 4320 blocks): decode on the vector path, then the encode of what was
    decoded; the twins give the expected bits."""
    H, W = 2160, 4096
    s = yuv.Surface.nv12(H, W, siting="left") if name == "nv12" else yuv.Surface.p010(H, W)
    buf = fill(s, 4, 0)
    dbuf = to_dev(buf, dev)
    dst = torch.full((3, H, W), float("nan"), dtype=torch.float32, device=dev)
    if name == "nv12":
        u8 = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev)
        ops.yuv_surface_decode(dbuf, s, dst_u8=u8, dst=dst)
        want = yuv.decode_numpy(buf, s)
        assert np.array_equal(u8.cpu().numpy(), want)
        assert np.array_equal(dst.cpu().numpy().view(np.uint32), (want.transpose(2, 0, 1).astype(np.float32) / np.float32(255)).view(np.uint32))
        out = torch.full((s.nbytes,), 0xA5, dtype=torch.uint8, device=dev)
        ops.yuv_surface_encode(out, s, src_u8=u8)
        assert np.array_equal(out.cpu().numpy(), yuv.encode_numpy(want, s))
    else:
        ops.yuv_surface_decode(dbuf, s, dst=dst, keep_depth=True)
        want = yuv.decode_numpy_f32(buf, s)
        got = dst.permute(1, 2, 0).contiguous().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        out = torch.full((s.nbytes,), 0xA5, dtype=torch.uint8, device=dev)
        ops.yuv_surface_encode(out, s, src=dst)
        assert np.array_equal(out.cpu().numpy().view("<u2"), yuv.encode_numpy(want, s))


# ------------------------------------------------------------------------------------------------ the planar entry points
@pytest.mark.parametrize("H,W", [(3, 5), (8, 16), (40, 1100)], ids=lambda v: str(v))
def test_the_new_calls_give_the_bytes_of_the_planar_calls(ops, dev, H, W):
    Hp, Wp, pt, pl = geo = canvas_of(H, W)
    for siting in SITINGS:
        f8, f10 = yuv.Format(H, W, siting=siting), yuv.Format(H, W, siting=siting, depth=10)
        rng = np.random.default_rng(H + W)
        b8 = rng.integers(0, 256, f8.frame_samples).astype(np.uint8)
        b10 = rng.integers(0, 1024, f10.frame_samples).astype(np.uint16)
        # decode: 8 bit and 10 -> 8 bit through yuv420_to_rgb, 10 bit kept through yuv420p10_to_f32
        old = {}
        for key, (buf, fmt) in {"8": (b8, f8), "10": (b10, f10)}.items():
            u = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev)
            f = torch.full((3, Hp, Wp), float("nan"), dtype=torch.float32, device=dev)
            ops.yuv420_to_rgb(to_dev(buf, dev), fmt, dst_u8=u, dst=f, pad_top=pt, pad_left=pl)
            old[key] = (u.cpu().numpy(), f.cpu().numpy().view(np.uint32))
        k = torch.full((3, Hp, Wp), float("nan"), dtype=torch.float32, device=dev)
        ops.yuv420p10_to_f32(to_dev(b10, dev), f10, k, pad_top=pt, pad_left=pl)
        old["keep"] = k.cpu().numpy().view(np.uint32)
        for chroma, msb in (("planar", False), ("uv", False), ("vu", False), ("uv", True), ("planar", True)):
            s8, s10 = yuv.Surface(f8, chroma), yuv.Surface(f10, chroma, msb)
            f, u = run_decode(ops, dev, yuv.repack(b8, f8, s8), s8, geo, u8=True)
            assert np.array_equal(u, old["8"][0]) and np.array_equal(f, old["8"][1]), (chroma, "8")
            f, u = run_decode(ops, dev, yuv.repack(b10, f10, s10), s10, geo, u8=True)
            assert np.array_equal(u, old["10"][0]) and np.array_equal(f, old["10"][1]), (chroma, msb, "10")
            f, _ = run_decode(ops, dev, yuv.repack(b10, f10, s10), s10, geo, keep=True)
            assert np.array_equal(f, old["keep"]), (chroma, msb, "keep")
        # encode
        rgb, x, pic, _ = sources(H, W, 8, seed=H)
        _, x10, _, _ = sources(H, W, 10, seed=H + 1)
        d_rgb, d_x, d_x10 = torch.from_numpy(rgb).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(x10).to(dev)
        o_u8, o_f = (torch.full((f8.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(2))
        o_10 = torch.full((f10.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev)
        ops.rgb_to_yuv420(o_u8, f8, src_u8=d_rgb)
        ops.rgb_to_yuv420(o_f, f8, src=d_x, pad_top=pt, pad_left=pl)
        ops.f32_to_yuv420p10(o_10, f10, d_x10, pad_top=pt, pad_left=pl)
        o_u8, o_f, o_10 = o_u8.cpu().numpy(), o_f.cpu().numpy(), o_10.cpu().numpy().view("<u2")
        for chroma, msb in (("planar", False), ("uv", False), ("vu", False), ("uv", True)):
            s8, s10 = yuv.Surface(f8, chroma), yuv.Surface(f10, chroma, msb)
            assert np.array_equal(run_encode(ops, dev, s8, src_u8=d_rgb), yuv.repack(o_u8, f8, s8)), (chroma, "u8")
            assert np.array_equal(run_encode(ops, dev, s8, src=d_x, pad_top=pt, pad_left=pl), yuv.repack(o_f, f8, s8)), (chroma, "f32")
            assert np.array_equal(run_encode(ops, dev, s10, src=d_x10, pad_top=pt, pad_left=pl).view("<u2"), yuv.repack(o_10, f10, s10)), (chroma, msb)


def test_wrapper_refusals(ops, dev):
    s = yuv.Surface.nv12(16, 16, pitch=24)
    buf = torch.zeros(s.nbytes, dtype=torch.uint8, device=dev)
    dst, u8 = torch.empty(3, 16, 16, device=dev), torch.empty(16, 16, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="surface must be a yuv.Surface"):
        ops.yuv_surface_decode(buf, s.fmt, dst=dst)
    with pytest.raises(ValueError, match="buf must be"):
        ops.yuv_surface_decode(buf[:-1], s, dst=dst)
    with pytest.raises(ValueError, match="give dst, dst_u8 or both"):
        ops.yuv_surface_decode(buf, s)
    with pytest.raises(ValueError, match="keep_depth needs"):
        ops.yuv_surface_decode(buf, s, dst=dst, keep_depth=True)
    with pytest.raises(ValueError, match="dst must be"):
        ops.yuv_surface_decode(buf, s, dst=dst.half())
    with pytest.raises(ValueError, match="dst_u8 must be"):
        ops.yuv_surface_decode(buf, s, dst_u8=u8[:8])
    with pytest.raises(ValueError, match="even"):
        ops.yuv_surface_decode(buf, s, dst=dst, window=(0, 3, 8, 8))
    with pytest.raises(ValueError, match="outside"):
        ops.yuv_surface_decode(buf, s, dst=dst, window=(8, 8, 10, 8))
    with pytest.raises(ValueError, match="smaller than the window"):
        ops.yuv_surface_decode(buf, s, dst=dst, pad_left=4)
    with pytest.raises(ValueError, match="must be tight"):
        ops.yuv_surface_encode(buf, s, src=dst)
    t = s.tight()
    with pytest.raises(ValueError, match="buf must be"):
        ops.yuv_surface_encode(buf, t, src=dst)
    with pytest.raises(ValueError, match="exactly one"):
        ops.yuv_surface_encode(buf[:t.nbytes], t, src=dst, src_u8=u8)
    with pytest.raises(ValueError, match="smaller than the frame"):
        ops.yuv_surface_encode(buf[:t.nbytes], t, src=dst, pad_top=1)
    p = yuv.Surface.p010(16, 16)
    with pytest.raises(ValueError, match="8-bit surfaces only"):
        ops.yuv_surface_encode(torch.zeros(p.nbytes, dtype=torch.uint8, device=dev), p, src_u8=u8)
    with pytest.raises(ValueError, match="not with keep_depth"):
        ops.yuv_surface_decode(torch.zeros(p.nbytes, dtype=torch.uint8, device=dev), p, dst=dst, dst_u8=u8, keep_depth=True)


# ------------------------------------------------------------------------------------------------ the loops
H, W = 64, 96


def shots(fmt):
    rgb = CS.shot(3, H, W, seed=11, tone=60) + CS.shot(2, H, W, seed=12, tone=190)
    if fmt.depth == 8:
        return [yuv.encode_numpy(f, fmt) for f in rgb]
    return [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt) | np.uint16(k % 4) for k, f in enumerate(rgb)]


LOOP_CASES = {"nv12": (8, yuv.Surface(yuv.Format(H, W), "uv"), {}),
              "nv12_pitch128": (8, yuv.Surface.nv12(H, W, pitch=128, chroma_offset=128 * 72), {}),
              "p010_keep": (10, yuv.Surface.p010(H, W), dict(keep_depth=True)),
              "p010_pitch_crop_keep": (10, yuv.Surface.p010(H, W, pitch=2 * W + 6), dict(keep_depth=True, crop=(48, 64)))}


@pytest.mark.parametrize("loop", ["nx_pooled", "nx_plain", "pipeline"])
@pytest.mark.parametrize("case", list(LOOP_CASES))
def test_loops_yield_the_repack_of_the_i420_run(net, dev, case, loop):
    depth, s, kw = LOOP_CASES[case]
    if loop == "pipeline" and "crop" in kw:
        kw = {k: v for k, v in kw.items() if k != "crop"}           # (the 2x pipeline has no crop)
    fmt = s.fmt
    video = shots(fmt)
    frames = [yuv.repack(f, fmt, s) for f in video]
    run = {"nx_pooled": lambda fr, p: host_io.interpolate_video_nx(fr, net, factor=4, divisor=32, pool=True, pixfmt=p, **kw),
           "nx_plain": lambda fr, p: host_io.interpolate_video_nx(fr, net, factor=2, divisor=32, pool=False, tta=True, pixfmt=p, **kw),
           "pipeline": lambda fr, p: host_io.interpolate_video_2x(fr, net, divisor=32, pixfmt=p, **kw)}[loop]
    ref, got = list(run(iter(video), fmt)), list(run(iter(frames), s))
    assert len(got) == len(ref) > len(video)
    h, w = kw.get("crop", (H, W))
    for k, (g, r) in enumerate(zip(got, ref)):
        rf = (fmt if r.dtype == np.uint16 else fmt.as_8bit()).cropped(h, w)
        rs = (s.tight() if r.dtype == np.uint16 else s.as_8bit()).cropped(h, w)
        assert g.dtype == r.dtype and np.array_equal(g, yuv.repack(r, rf, rs)), (k, int((g != yuv.repack(r, rf, rs)).sum()))
    if s.is_tight and "crop" not in kw:
        assert got[0] is frames[0] and got[-1] is frames[-1]
    else:
        assert got[0] is not frames[0] and got[0].shape == (s.tight().cropped(h, w).frame_samples,)
