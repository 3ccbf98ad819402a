"""GPU: planar 4:2:2 / 4:4:4 frames on the device (csrc/yuv.hip atmvfi_yuv_decode, csrc/yuv_encode.hip atmvfi_yuv_encode,
``pixfmt=`` of the video loops): both entry points against the per-sample loop model of tests/cpu_yuv_sub.py (small shapes) and the
numpy twins (large ones; the CPU suite holds them to the model), bit for bit -- 8 bit, 10 -> 8 bit, 10 bit kept, both sitings, the
vector and the general path reached every way, poisoned destinations, guards and padding -- then equality with the surface calls at
subsampling 4:2:0, the identities across the old and the new instances, a planned replay and the loops."""
import importlib
import itertools

import numpy as np
import pytest
import torch

import cpu_scene as CS
import cpu_yuv_sub as M

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")

SUBS = ("422", "444")
GUARD = 64


def sitings(sub):
    return ("centre", "left") if sub != "444" else ("centre",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


def make_net(dev, kind):
    torch.set_grad_enabled(False)
    n = pkg.NetworkLite() if kind == "lite" else pkg.Network()
    n.load_state_dict(pkg.synthetic_state_dict(kind, seed=1), strict=True)
    n = n.to(dev).eval()
    n.global_motion, n.ensemble_global_motion = True, False
    return n


@pytest.fixture(scope="module")
def net(dev):
    return make_net(dev, "lite")


def to_dev(arr, dev, offset=0):
    """The bytes of ``arr`` on the device as a 1-D uint8 tensor whose pointer is ``offset`` bytes past an allocation's start."""
    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy())
    buf = torch.empty(raw.numel() + offset, dtype=torch.uint8, device=dev)
    view = buf[offset:]
    view.copy_(raw)
    return view


def surfaces(fmt):
    """tight; a pitch that is no multiple of 4 with a chroma offset beyond pitch * H; pitches and offset multiples of 4"""
    b, (H, W), (_, cw) = (2 if fmt.depth == 10 else 1), (fmt.height, fmt.width), fmt.chroma_shape
    odd = lambda n: next(p for p in range(n + b, n + 16, b) if p % 4)
    mul4 = lambda n: (n + 11) // 4 * 4
    return [yuv.Surface(fmt),
            yuv.Surface(fmt, pitch=odd(W * b), chroma_pitch=odd(cw * b), chroma_offset=odd(W * b) * H + 3 * b),
            yuv.Surface(fmt, pitch=mul4(W * b), chroma_pitch=mul4(cw * b), chroma_offset=mul4(W * b) * H + 8)]


def layout_of(s):
    s = yuv.as_surface(s)
    return M.layout(s.height, s.width, s.depth, s.subsampling, s.pitch, s.chroma_pitch, s.chroma_offset)


def fill(s, seed, poison):
    """A frame of ``s`` with seeded random samples over the whole range and every padding byte ``poison`` (vectorised)."""
    s = yuv.as_surface(s)
    rng = np.random.default_rng(seed)
    buf = np.full(s.nbytes, poison, np.uint8).view(s.dtype).copy()
    for p in s.planes(buf):
        p[...] = rng.integers(0, 1024 if s.depth == 10 else 256, p.shape).astype(s.dtype)
    return buf


def canvas_of(h, w):
    """(Hp, Wp, pad_top, pad_left): an odd top padding; multiples of 4 across when w is one (the vector path's geometry)."""
    return (h + 5, w + 12, 3, 4) if w % 4 == 0 else (h + 4, w + 7, 1, 3)


def decode_vector_ok(s, offset, window, geo):
    """The library's condition for the vector path of a decode, written out from include/atmvfi.h: 4-byte frame pointer, W, x0, w, Wp,
    pad_left multiples of 4, pitch a multiple of 4 bytes, planar chroma rows and origins of 2 samples -- for 4:4:4 of 4 bytes, like
    luma rows.  (Device allocations are 256-byte aligned; the canvas and uint8 destinations of these tests are whole allocations.)"""
    s = yuv.as_surface(s)
    b = s.itemsize
    y0, x0, h, w = (0, 0, s.height, s.width) if window is None else window
    ch = s.chroma_shape[0]
    uoff, voff, cs = s.chroma_offset // b, (s.chroma_offset + s.chroma_pitch * ch) // b, s.chroma_pitch // b
    if s.subsampling == "444":
        chroma = (uoff * b) % 4 == 0 and (voff * b) % 4 == 0 and (cs * b) % 4 == 0
    else:
        chroma = uoff % 2 == 0 and voff % 2 == 0 and cs % 2 == 0
    canvas = geo is None or (geo[1] % 4 == 0 and geo[3] % 4 == 0)
    return offset % 4 == 0 and s.width % 4 == 0 and s.pitch % 4 == 0 and chroma and x0 % 4 == 0 and w % 4 == 0 and canvas


def encode_vector_ok(s, offset, geo, src_offset=0):
    """The same for an encode into a tight frame: 4-byte frame pointer, W % 4 == 0, a 16-byte aligned canvas with Wp and pad_left
    multiples of 4 (or a 4-byte aligned uint8 source)."""
    return offset % 4 == 0 and s.width % 4 == 0 and (geo is None or (geo[1] % 4 == 0 and geo[3] % 4 == 0 and src_offset % 16 == 0))


def padded(q, geo, top):
    """int [h,w,3] pixels -> the fp32 canvas [3,Hp,Wp] = q / top with replicate padding, as uint32 bits"""
    Hp, Wp, pt, pl = geo
    h, w = q.shape[:2]
    x = (q.astype(np.float32) / np.float32(top)).transpose(2, 0, 1)
    return np.ascontiguousarray(np.pad(x, ((0, 0), (pt, Hp - h - pt), (pl, Wp - w - pl)), mode="edge")).view(np.uint32)


def run_decode(ops, dev, buf, s, geo=None, window=None, keep=False, u8=False, bgr=False, offset=0):
    """-> (fp32 canvas bits or None, uint8 window or None); both destinations are pre-filled with a sentinel and followed by a guard
    region that must come back intact."""
    s = yuv.as_surface(s)
    h, w = (s.height, s.width) if window is None else window[2:]
    dst = dst_u8 = fbuf = ubuf = None
    if geo is not None:
        n = 3 * geo[0] * geo[1]
        fbuf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        dst = fbuf[:n].view(3, geo[0], geo[1])
    if u8:
        ubuf = torch.full((h * w * 3 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        dst_u8 = ubuf[:h * w * 3].view(h, w, 3)
    pt, pl = (geo[2], geo[3]) if geo is not None else (0, 0)
    ops.yuv_sub_decode(to_dev(buf, dev, offset), s, dst_u8=dst_u8, dst=dst, window=window, pad_top=pt, pad_left=pl, bgr=bgr, keep_depth=keep)
    if fbuf is not None:
        assert torch.isnan(fbuf[-GUARD:]).all() and not torch.isnan(dst).any()      # every element inside written, the guard intact
    if ubuf is not None:
        assert (ubuf[-GUARD:] == 0xA5).all()
    return (None if dst is None else dst.cpu().numpy().view(np.uint32)), (None if dst_u8 is None else dst_u8.cpu().numpy())


def check_decode(ops, dev, buf, s, want, want10, geos, window=None, offsets=(0,)):
    """``want`` int [h,w,3] 0..255, ``want10`` 0..1023 or None: every output of the call, on every geometry and pointer offset.
    Returns the set of paths the cases took (True: vector)."""
    paths = set()
    for geo, off in itertools.product(geos, offsets):
        paths.add(decode_vector_ok(s, off, window, geo))
        f, u = run_decode(ops, dev, buf, s, geo, window, u8=True, offset=off)
        assert np.array_equal(u, want.astype(np.uint8)), (s, geo, off, "u8")
        assert np.array_equal(f, padded(want, geo, 255)), (s, geo, off, "f32", np.argwhere(f != padded(want, geo, 255))[:3])
        if want10 is not None:
            f, _ = run_decode(ops, dev, buf, s, geo, window, keep=True, offset=off)
            assert np.array_equal(f, padded(want10, geo, 1023)), (s, geo, off, "keep")
    _, u = run_decode(ops, dev, buf, s, None, window, u8=True, bgr=True)
    assert np.array_equal(u, want[:, :, ::-1].astype(np.uint8)), (s, "bgr")
    return paths


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W,wins", [(1, 1, []), (2, 2, [(1, 0, 1, 2)]), (3, 5, [(1, 2, 2, 3)]), (5, 3, [(3, 2, 2, 1)]),
                                      (8, 16, [(3, 2, 5, 13), (1, 4, 7, 12), (5, 8, 3, 8)]), (31, 41, [(7, 10, 20, 31)])], ids=lambda v: str(v)[:8])
def test_decode_is_the_loop_model(ops, dev, H, W, wins, sub, depth):
    """8 x 16 reaches the vector path (the tight and the multiple-of-4 layout, canvas (.., 4), windows at x0 = 4 / 8 with an odd y0) and
    the general path (a pitch that is no multiple of 4, a pointer offset by one sample, pad_left 3, windows at x0 = 2); every other
    size is general.  4:4:4 windows also start at odd x0."""
    paths = set()
    if sub == "444":
        wins = wins + [(y0, x0 + 1, h, w - 1) for y0, x0, h, w in wins if w > 1][:1]
    for k, siting in enumerate(sitings(sub)):
        matrix = ("bt601", "bt709")[k]
        for n, s in enumerate(surfaces(yuv.Format(H, W, matrix, False, siting, depth, sub))):
            if (H, W) == (31, 41) and n != k:
                continue
            L = layout_of(s)
            buf = M.random_frame(L, seed=31 * H + 7 * k + n, poison=(0xFF, 0x00, 0x5A)[n])
            kw = dict(matrix=matrix, siting=siting)
            want = M.decode(buf, L, **kw)
            want10 = M.decode(buf, L, keep=True, **kw) if depth == 10 else None
            paths |= check_decode(ops, dev, buf, s, want, want10, [canvas_of(H, W), (H + 4, W + 7, 1, 3), (H, W, 0, 0)], offsets=(0, s.itemsize))
            for win in wins:
                w10 = M.decode(buf, L, window=win, keep=True, **kw) if depth == 10 else None
                paths |= check_decode(ops, dev, buf, s, M.decode(buf, L, window=win, **kw), w10, [canvas_of(*win[2:])], window=win)
    assert paths == ({True, False} if (H, W) == (8, 16) else {False})


@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("sub", SUBS)
def test_decode_40x1100_is_the_twin(ops, dev, sub, depth):
    """Several column groups and workgroups (40 x 1100: 20 row pairs x 278 groups = 22 blocks), the vector and the general path;
    padding poisoned two ways: the same output, so it is not read."""
    H, W = 40, 1100
    siting = sitings(sub)[(depth // 2) % len(sitings(sub))]
    paths = set()
    for n, s in enumerate(surfaces(yuv.Format(H, W, "bt709", False, siting, depth, sub))):
        bufs = [fill(s, 5 + n, poison) for poison in (0xFF, 0x00)]
        want = yuv.decode_numpy(bufs[0], s).astype(np.int32)
        want10 = np.rint(yuv.decode_numpy_f32(bufs[0], s).astype(np.float64) * 1023).astype(np.int32) if depth == 10 else None
        for buf in bufs:
            paths |= check_decode(ops, dev, buf, s, want, want10, [canvas_of(H, W)], offsets=(0, s.itemsize) if n == 0 else (0,))
        win = (3, 2, 37, 1001)
        w10 = np.rint(yuv.decode_numpy_f32(bufs[0], s, window=win).astype(np.float64) * 1023).astype(np.int32) if depth == 10 else None
        paths |= check_decode(ops, dev, bufs[0], s, want[3:40, 2:1003], w10, [canvas_of(37, 1001)], window=win)
    assert paths == {True, False}


# ------------------------------------------------------------------------------------------------ encode
def sources(H, W, depth, seed):
    """(uint8 RGB or None, fp32 canvas [3,Hp,Wp] with NaN outside the frame, its frame [H,W,3], geometry): the fp32 picture has values
    outside [0, 1], exact .5 ties of the pixel grid, and exact 0 and 1"""
    rng = np.random.default_rng(seed)
    Hp, Wp, pt, pl = canvas_of(H, W)
    pic = rng.uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32)
    top = 1023 if depth == 10 else 255
    ties = ((np.arange(top) + 0.5) / top).astype(np.float32)
    m = rng.random(pic.shape) < 0.2
    pic[m] = ties[rng.integers(0, top, int(m.sum()))]
    ends = rng.random(pic.shape) < 0.1
    pic[ends] = rng.integers(0, 2, int(ends.sum())).astype(np.float32)
    x = np.full((3, Hp, Wp), np.nan, np.float32)
    x[:, pt:pt + H, pl:pl + W] = pic.transpose(2, 0, 1)
    return (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) if depth == 8 else None), x, pic, (Hp, Wp, pt, pl)


def run_encode(ops, dev, s, offset=0, **kw):
    """-> the frame's bytes; the destination pre-filled with a sentinel, guards before and behind it intact afterwards"""
    s = yuv.as_surface(s)
    dst = torch.full((offset + s.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ops.yuv_sub_encode(dst[offset:offset + s.nbytes], s, **kw)
    got = dst.cpu().numpy()
    assert (got[:offset] == 0xA5).all() and (got[offset + s.nbytes:] == 0xA5).all()
    return got[offset:offset + s.nbytes]


def check_encode(ops, dev, s, want_of, seed, offsets=(0, 1)):
    """``want_of(pixel source) -> bytes``: from uint8 RGB and BGR (8 bit) and from the fp32 canvas, on every destination offset.  A
    sentinel that survives shows as a wrong byte: the expected bytes are compared whole.  Returns the paths taken."""
    s = yuv.as_surface(s)
    rgb, x, pic, geo = sources(s.height, s.width, s.depth, seed)
    Hp, Wp, pt, pl = geo
    paths = set()
    for off in offsets:
        if rgb is not None:
            want = want_of(rgb)
            paths.add(encode_vector_ok(s, off, None))
            assert np.array_equal(run_encode(ops, dev, s, off, src_u8=torch.from_numpy(rgb).to(dev)), want), (s, off, "rgb")
            bgr = torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1])).to(dev)
            assert np.array_equal(run_encode(ops, dev, s, off, src_u8=bgr, bgr=True), want), (s, off, "bgr")
        paths.add(encode_vector_ok(s, off, geo))
        got = run_encode(ops, dev, s, off, src=torch.from_numpy(x).to(dev), pad_top=pt, pad_left=pl)
        assert np.array_equal(got, want_of(pic)), (s, off, "f32", np.flatnonzero(got != want_of(pic))[:4])
    whole = torch.full((x.size + 1,), float("nan"), dtype=torch.float32, device=dev)          # a source pointer offset by one sample
    whole[1:].copy_(torch.from_numpy(x).reshape(-1))
    paths.add(encode_vector_ok(s, 0, geo, src_offset=4))
    got = run_encode(ops, dev, s, 0, src=whole[1:].view(*x.shape), pad_top=pt, pad_left=pl)
    assert np.array_equal(got, want_of(pic))
    return paths


@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (5, 3), (8, 16), (31, 41)], ids=lambda v: str(v))
def test_encode_is_the_loop_model(ops, dev, H, W, sub, depth):
    paths = set()
    for k, siting in enumerate(sitings(sub)):
        matrix = ("bt709", "bt601")[k]
        fmt = yuv.Format(H, W, matrix, False, siting, depth, sub)
        L = layout_of(fmt)
        paths |= check_encode(ops, dev, fmt, lambda src: M.encode(M.pixels(src, depth), L, matrix=matrix, siting=siting), seed=H * W + k)
    assert paths == ({True, False} if (H, W) == (8, 16) else {False})


@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("sub", SUBS)
def test_encode_40x1100_is_the_twin(ops, dev, sub, depth):
    siting = sitings(sub)[(depth // 2) % len(sitings(sub))]
    fmt = yuv.Format(40, 1100, "bt601", False, siting, depth, sub)
    as_source = lambda src: src if (depth == 10 or src.dtype == np.uint8) else M.pixels(src, 8).astype(np.uint8)     # (the fp32 source's pixel)
    paths = check_encode(ops, dev, fmt, lambda src: yuv.encode_numpy(as_source(src), fmt).astype("<u2" if depth == 10 else np.uint8).view(np.uint8), seed=3)
    assert paths == {True, False}


# ------------------------------------------------------------------------------------------------ 1080p, once per subsampling
@pytest.mark.parametrize("sub", SUBS)
def test_1080x1920_once(ops, dev, sub):
    """8 bit: decode to both outputs on the vector path, then the encode of what was decoded.  10 bit kept: decode at pitch 4096 with
    poisoned padding into the padded 1088-row canvas, then the encode of that canvas.  The twins give the expected bits."""
    H, W = 1080, 1920
    siting = sitings(sub)[-1]
    f8 = yuv.Format(H, W, "bt709", False, siting, 8, sub)
    buf = fill(f8, 4, 0)
    assert decode_vector_ok(f8, 0, None, (H, W, 0, 0)) and encode_vector_ok(f8, 0, None)
    dst = torch.full((3, H, W), float("nan"), dtype=torch.float32, device=dev)
    u8 = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev)
    ops.yuv_sub_decode(to_dev(buf, dev), f8, dst_u8=u8, dst=dst)
    want = yuv.decode_numpy(buf, f8)
    assert np.array_equal(u8.cpu().numpy(), want)
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), (want.transpose(2, 0, 1).astype(np.float32) / np.float32(255)).view(np.uint32))
    out = torch.full((f8.frame_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ops.yuv_sub_encode(out[:f8.frame_bytes], f8, src_u8=u8)
    assert np.array_equal(out[:f8.frame_bytes].cpu().numpy(), yuv.encode_numpy(want, f8)) and (out[f8.frame_bytes:] == 0xA5).all()
    s10 = yuv.surface_of("yuv" + sub + "p10le", H, W, pitch=4096, matrix="bt709", siting=siting)
    assert decode_vector_ok(s10, 0, None, (1088, W, 4, 0))
    b10 = fill(s10, 5, 0xFF)
    canvas = torch.full((3, 1088, W), float("nan"), dtype=torch.float32, device=dev)
    ops.yuv_sub_decode(to_dev(b10, dev), s10, dst=canvas, pad_top=4, keep_depth=True)
    want = yuv.decode_numpy_f32(b10, s10)
    got = canvas[:, 4:4 + H].permute(1, 2, 0).contiguous().cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert torch.equal(canvas[:, :4], canvas[:, 4:5].expand(3, 4, W)) and torch.equal(canvas[:, 4 + H:], canvas[:, 3 + H:4 + H].expand(3, 4, W))
    t10 = s10.tight()
    out = torch.full((t10.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ops.yuv_sub_encode(out[:t10.nbytes], t10, src=canvas, pad_top=4)
    assert np.array_equal(out[:t10.nbytes].cpu().numpy().view("<u2"), yuv.encode_numpy(want, t10)) and (out[t10.nbytes:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 4:2:0 through the new calls
@pytest.mark.parametrize("H,W", [(3, 5), (8, 16), (40, 1100)], ids=lambda v: str(v))
def test_subsampling_420_is_the_surface_call(ops, dev, H, W):
    geo = canvas_of(H, W)
    for siting, (chroma, depth, msb) in itertools.product(("centre", "left"), (("planar", 8, False), ("uv", 8, False), ("vu", 8, False),
                                                                               ("planar", 10, False), ("uv", 10, True))):
        s = yuv.Surface(yuv.Format(H, W, siting=siting, depth=depth), chroma, msb)
        buf = np.random.default_rng(H + W).integers(0, 65536 if msb else (1 << depth), s.frame_samples).astype(s.dtype)
        d = to_dev(buf, dev)
        for keep in ((False, True) if depth == 10 else (False,)):
            outs = []
            for call in (ops.yuv_surface_decode, ops.yuv_sub_decode):
                f = torch.full((3, geo[0], geo[1]), float("nan"), dtype=torch.float32, device=dev)
                u = None if keep else torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev)
                call(d, s, dst_u8=u, dst=f, pad_top=geo[2], pad_left=geo[3], keep_depth=keep)
                outs.append((f.cpu().numpy().view(np.uint32), None if u is None else u.cpu().numpy()))
            assert np.array_equal(outs[0][0], outs[1][0]) and (keep or np.array_equal(outs[0][1], outs[1][1])), (s, keep)
        rgb, x, _, _ = sources(H, W, depth, seed=H)
        kw = dict(src=torch.from_numpy(x).to(dev), pad_top=geo[2], pad_left=geo[3])
        pair = []
        for call in (ops.yuv_surface_encode, ops.yuv_sub_encode):
            o = torch.full((s.nbytes,), 0xA5, dtype=torch.uint8, device=dev)
            call(o, s, **kw)
            pair.append(o.cpu().numpy())
        assert np.array_equal(pair[0], pair[1]), (s, "encode")
    # a Format goes the same way, and the dispatchers send 4:2:0 where it went before
    fmt = yuv.Format(H, W)
    buf = np.random.default_rng(1).integers(0, 256, fmt.frame_samples).astype(np.uint8)
    a, b = (torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev) for _ in range(2))
    ops.yuv420_to_rgb(to_dev(buf, dev), fmt, dst_u8=a)
    ops.yuv_sub_decode(to_dev(buf, dev), fmt, dst_u8=b)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ identities on the device
@pytest.mark.parametrize("H,W", [(5, 3), (8, 16), (40, 1100)], ids=lambda v: str(v))
def test_identities_across_the_old_and_the_new_instances(ops, dev, H, W):
    """D1: a 4:2:2 frame of equal chroma rows decodes (new instance) to what the 4:2:0 frame of those rows decodes to (old instance).
    E1: a picture of equal row pairs encodes at 4:2:2 (new) to chroma rows 2j equal to the 4:2:0 encode's (old) row j."""
    rng = np.random.default_rng(H * W)
    geo = canvas_of(H, W)
    for siting, depth in itertools.product(("centre", "left"), (8, 10)):
        f0, f2 = yuv.Format(H, W, "bt709", False, siting, depth), yuv.Format(H, W, "bt709", False, siting, depth, "422")
        ch, cw = f0.chroma_shape
        top = 1 << depth
        Y, urow, vrow = rng.integers(0, top, H * W), rng.integers(0, top, cw), rng.integers(0, top, cw)
        b0 = np.concatenate([Y, np.tile(urow, ch), np.tile(vrow, ch)]).astype(f0.dtype)
        b2 = np.concatenate([Y, np.tile(urow, H), np.tile(vrow, H)]).astype(f0.dtype)
        for keep in ((False, True) if depth == 10 else (False,)):
            outs = []
            for buf, fmt, call in ((b0, f0, ops.yuv_surface_decode), (b2, f2, ops.yuv_sub_decode)):
                f = torch.full((3, geo[0], geo[1]), float("nan"), dtype=torch.float32, device=dev)
                call(to_dev(buf, dev), yuv.as_surface(fmt), dst=f, pad_top=geo[2], pad_left=geo[3], keep_depth=keep)
                outs.append(f)
            assert torch.equal(outs[0], outs[1]), (siting, depth, keep, "D1")
        half = rng.uniform(-0.05, 1.05, (3, ch, W)).astype(np.float32)
        x = np.full((3, geo[0], geo[1]), np.nan, np.float32)
        x[:, geo[2]:geo[2] + H, geo[3]:geo[3] + W] = np.repeat(half, 2, axis=1)[:, :H]
        o0 = torch.full((f0.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev)
        o2 = torch.full((f2.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev)
        ops.yuv_surface_encode(o0, yuv.Surface(f0), src=torch.from_numpy(x).to(dev), pad_top=geo[2], pad_left=geo[3])
        ops.yuv_sub_encode(o2, f2, src=torch.from_numpy(x).to(dev), pad_top=geo[2], pad_left=geo[3])
        (_, U0, V0), (_, U2, V2) = f0.planes(o0.cpu().numpy().view(f0.dtype)), f2.planes(o2.cpu().numpy().view(f2.dtype))
        assert np.array_equal(U2[0::2], U0) and np.array_equal(V2[0::2], V0), (siting, depth, "E1")


# ------------------------------------------------------------------------------------------------ a planned replay
@pytest.mark.parametrize("sub", SUBS)
def test_the_new_calls_record_into_launch_plans(ops, dev, sub):
    H, W = 8, 16
    fmt = yuv.Format(H, W, depth=10, subsampling=sub)
    geo = canvas_of(H, W)
    frames = [to_dev(fill(fmt, k, 0), dev) for k in range(2)]
    canvases = [torch.full((3, geo[0], geo[1]), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    outs = [torch.full((fmt.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]

    def both(buf, canvas, out):
        ops.yuv_sub_decode(buf, fmt, dst=canvas, pad_top=geo[2], pad_left=geo[3], keep_depth=True)
        ops.yuv_sub_encode(out, fmt, src=canvas, pad_top=geo[2], pad_left=geo[3])
    plan = ops.begin_plan([frames[0], canvases[0], outs[0]])
    try:
        both(frames[0], canvases[0], outs[0])
        assert len(plan.ops_list) == 2 and len(plan.patches) == 4
        plan = ops.end_plan(None)
    finally:
        ops.abort_plan()
    assert plan.run([frames[1], canvases[1], outs[1]], dev, ops._stream()) is None
    both(frames[1], canvases[0], outs[2])                                       # the direct launch of the same call
    assert torch.equal(outs[1], outs[2]) and torch.equal(canvases[1], canvases[0]) and not torch.equal(outs[1], outs[0])


def test_wrapper_refusals(ops, dev):
    f2, f4 = yuv.Format(16, 16, depth=10, subsampling="422"), yuv.Format(16, 16, subsampling="444")
    b2, b4 = (torch.zeros(f.frame_bytes, dtype=torch.uint8, device=dev) for f in (f2, f4))
    dst, u8 = torch.empty(3, 16, 16, device=dev), torch.empty(16, 16, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="yuv.Format or yuv.Surface expected"):
        ops.yuv_sub_decode(b2, "yuv422p10le", dst=dst)
    with pytest.raises(ValueError, match="buf must be"):
        ops.yuv_sub_decode(b2[:-1], f2, dst=dst)
    with pytest.raises(ValueError, match="even x0 for 4:2:2"):
        ops.yuv_sub_decode(b2, f2, dst=dst, window=(1, 3, 8, 8))
    ops.yuv_sub_decode(b2, f2, dst=dst, window=(1, 2, 8, 8), keep_depth=True)
    ops.yuv_sub_decode(b4, f4, dst=dst, dst_u8=u8[:8, :8].contiguous(), window=(1, 3, 8, 8))
    with pytest.raises(ValueError, match="must be tight"):
        ops.yuv_sub_encode(b4, yuv.Surface(f4, pitch=20), src=dst)
    with pytest.raises(ValueError, match="8-bit surfaces only"):
        ops.yuv_sub_encode(b2, f2, src_u8=u8)
    for call in (lambda: ops.yuv420_to_rgb(b4, f4, dst=dst), lambda: ops.rgb_to_yuv420(b4, f4, src=dst), lambda: ops.yuv420p10_to_f32(b2, f2, dst),
                 lambda: ops.f32_to_yuv420p10(b2, f2, dst), lambda: ops.yuv420_window(b4, f4, 0, 0, 0, 8, 8, dst=dst),
                 lambda: ops.yuv_surface_decode(b4, yuv.Surface(f4), dst=dst), lambda: ops.yuv_surface_encode(b4, yuv.Surface(f4), src=dst)):
        with pytest.raises(ValueError, match="4:2:0 frames only"):
            call()
    # the dispatchers send them to the new calls
    ops.yuv_decode(b4, f4, dst=dst)
    ops.yuv_encode(b4, f4, src=dst)
    ops.yuv_decode(b2, f2, dst=dst, window=(3, 0, 8, 16), pad_top=2, keep_depth=True)


# ------------------------------------------------------------------------------------------------ the loops
H, W = 64, 96


def shots(fmt, h=H, w=W):
    rgb = CS.shot(3, h, w, seed=11, tone=60) + CS.shot(2, h, w, seed=12, tone=190)
    if fmt.depth == 8:
        return [yuv.encode_numpy(f, fmt) for f in rgb]
    return [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt) | np.uint16(k % 4) for k, f in enumerate(rgb)]


class Encodes:
    """``HipOps.yuv_encode`` with every call's source kept: the predictions a loop encodes, as it hands them over"""

    def __init__(self, monkeypatch):
        self.calls, real = [], hip_ops.HipOps.yuv_encode

        def spy(ops, buf, fmt, src_u8=None, src=None, pad_top=0, pad_left=0):
            self.calls.append((fmt, None if src_u8 is None else src_u8.clone(), None if src is None else src.clone(), pad_top, pad_left))
            return real(ops, buf, fmt, src_u8=src_u8, src=src, pad_top=pad_top, pad_left=pad_left)
        monkeypatch.setattr(hip_ops.HipOps, "yuv_encode", spy)

    def expected(self):
        """``encode_numpy`` of every recorded source"""
        out = []
        for fmt, src_u8, src, pt, pl in self.calls:
            if src_u8 is not None:
                pic = src_u8.cpu().numpy()
            else:
                pic = src[:, pt:pt + fmt.height, pl:pl + fmt.width].permute(1, 2, 0).contiguous().cpu().numpy()
                if fmt.depth == 8:
                    pic = M.pixels(pic, 8).astype(np.uint8)
            out.append(yuv.encode_numpy(pic, fmt))
        return out


RUNS = {"2x": lambda fr, net, **kw: host_io.interpolate_video_2x(fr, net, divisor=32, **kw),
        "4x_pooled": lambda fr, net, **kw: host_io.interpolate_video_nx(fr, net, factor=4, divisor=32, pool=True, **kw),
        "4x_plain": lambda fr, net, **kw: host_io.interpolate_video_nx(fr, net, factor=4, divisor=32, pool=False, **kw),
        "retimed": lambda fr, net, **kw: host_io.interpolate_video_retimed(fr, net, 24, 60, levels=2, divisor=32, **kw)}
ORIGINALS = {"2x": (2, 1), "4x_pooled": (4, 1), "4x_plain": (4, 1), "retimed": (5, 2)}       # output k is input k // n * m when k % n == 0


def check_loop(net, monkeypatch, name, fmt, video, kw):
    """-> the frames; every produced frame is ``encode_numpy`` of a prediction the loop handed to the encode, originals pass through"""
    rec = Encodes(monkeypatch)
    got = list(RUNS[name](iter(video), net, pixfmt=fmt, **kw))
    monkeypatch.undo()
    n, m = ORIGINALS[name]
    assert len(got) == n * (len(video) - 1) // m + 1
    out_fmt = fmt if kw.get("keep_depth") else fmt.as_8bit()
    want = rec.expected()
    produced = []
    for k, g in enumerate(got):
        if k % n == 0:
            assert g is video[k // n * m]                       # originals are the caller's arrays
        else:
            assert g.dtype == out_fmt.dtype and g.size == out_fmt.frame_samples
            produced.append(g)
    assert len(want) == len(produced) and all(f == out_fmt for f, *_ in rec.calls)
    left = list(want)
    for g in produced:                                          # frame for frame, whatever order the levels were encoded in
        hit = next((i for i, e in enumerate(left) if np.array_equal(g, e)), None)
        assert hit is not None
        left.pop(hit)
    return got


@pytest.mark.parametrize("kind", ("8", "10keep"))
@pytest.mark.parametrize("sub", SUBS)
def test_loops_on_the_hip_path(net, dev, monkeypatch, sub, kind):
    depth, kw = (8, {}) if kind == "8" else (10, dict(keep_depth=True))
    fmt = yuv.Format(H, W, "bt709", False, "left" if sub == "422" else "centre", depth, sub)
    video = shots(fmt)
    runs = {name: check_loop(net, monkeypatch, name, fmt, video, kw) for name in RUNS}
    assert all(np.array_equal(a, b) for a, b in zip(runs["4x_pooled"], runs["4x_plain"]))          # pooled equal to plain
    if depth == 8:      # the RGB loop on the decoded pictures makes the same predictions: its uint8 frames are the encode's source pixels
        rgb = list(host_io.interpolate_video_nx(iter([yuv.decode_numpy(f, fmt) for f in video]), net, factor=4, divisor=32, pool=False, isBGR=False))
        assert all(np.array_equal(g, yuv.encode_numpy(r, fmt)) for k, (g, r) in enumerate(zip(runs["4x_plain"], rgb)) if k % 4)


def test_loops_with_a_crop_and_a_scene_cut(net, dev, monkeypatch):
    """An odd crop origin where the subsampling allows it: originals are ``crop`` of the caller's frames, a cut is copied as bytes,
    and what is produced is ``encode_numpy`` of the window's predictions."""
    scene = importlib.import_module("atm-vfi_amd.scene")
    centre_window = importlib.import_module("atm-vfi_amd.multiframe").centre_window
    for sub, crop, origin in (("422", (34, 64), (15, 16)), ("444", (32, 62), (16, 17))):
        fmt = yuv.Format(H, W, "bt709", False, "centre", 10, sub)
        video = shots(fmt)
        win = centre_window(H, W, crop)
        assert tuple(win[:2]) == origin
        sc = scene.SceneCuts()
        rec = Encodes(monkeypatch)
        got = list(host_io.interpolate_video_nx(iter(video), net, factor=2, divisor=32, pixfmt=fmt, keep_depth=True, crop=crop, scene=sc))
        monkeypatch.undo()
        assert len(got) == 9 and len(sc.cuts) == 1
        cropped = [yuv.crop(f, fmt, *win) for f in video]
        assert all(np.array_equal(got[2 * k], cropped[k]) for k in range(5))
        cut = sc.cuts[0]
        assert np.array_equal(got[2 * cut + 1], cropped[cut])
        want = rec.expected()
        made = [got[k] for k in range(1, 9, 2) if k != 2 * cut + 1]
        assert len(want) == len(made) == 3 and all(f == fmt.cropped(*win[2:]) for f, *_ in rec.calls)
        assert all(any(np.array_equal(g, e) for e in want) for g in made)
    with pytest.raises(ValueError, match="even x0 for 4:2:2"):
        list(host_io.interpolate_video_nx(iter(shots(yuv.Format(H, W, subsampling="422"))), net, factor=2, divisor=32,
                                          pixfmt=yuv.Format(H, W, subsampling="422"), crop=(32, 62)))


def test_network_base_128x192_once(dev, monkeypatch):
    base = make_net(dev, "base")
    fmt = yuv.Format(128, 192, "bt709", False, "left", 10, "422")
    video = shots(fmt, 128, 192)[:3]
    check_loop(base, monkeypatch, "4x_pooled", fmt, video, dict(keep_depth=True))
