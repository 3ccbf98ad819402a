"""Planar 4:2:2 / 4:4:4 frames on the host: the numpy twins against the per-sample loop model (tests/cpu_yuv_sub.py), the identities
that tie the three subsamplings together, the carried-over round-trip bounds, the refusals, Y4M tags, the loops through the numpy
path and the two new ABI calls' host-side checks.  No GPU."""
import ctypes
import importlib
import io
import itertools
import os
import re

import numpy as np
import pytest
import torch

import cpu_scene as CS
import cpu_yuv_sub as M

mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")
scene = importlib.import_module("atm-vfi_amd.scene")

SIZES = [(1, 1), (2, 2), (3, 5), (5, 3), (8, 16), (31, 41)]
SUBS = ("422", "444")
# windows per size: odd y0 everywhere (allowed for both), odd x0 for 4:4:4 only
WINDOWS = {(1, 1): [], (2, 2): [(1, 0, 1, 2)], (3, 5): [(1, 2, 2, 3), (2, 0, 1, 5)], (5, 3): [(3, 2, 2, 1), (1, 0, 3, 3)],
           (8, 16): [(3, 2, 5, 13), (1, 4, 7, 8)], (31, 41): [(7, 10, 20, 31), (29, 40, 2, 1)]}
WINDOWS_444 = {(1, 1): [], (2, 2): [(1, 1, 1, 1)], (3, 5): [(1, 3, 2, 2)], (5, 3): [(3, 1, 2, 2)], (8, 16): [(3, 5, 5, 11)], (31, 41): [(7, 9, 20, 31)]}


def sitings(sub):
    return ("centre", "left") if sub != "444" else ("centre",)


def surfaces(fmt):
    """tight; padded with a pitch that is no multiple of 4 and a chroma offset beyond pitch * H; padded with multiples of 4"""
    b, (H, W), (_, cw) = (2 if fmt.depth == 10 else 1), (fmt.height, fmt.width), fmt.chroma_shape
    odd = lambda n: next(p for p in range(n + b, n + 16, b) if p % 4)
    mul4 = lambda n: (n + 11) // 4 * 4
    return [yuv.Surface(fmt),
            yuv.Surface(fmt, pitch=odd(W * b), chroma_pitch=odd(cw * b), chroma_offset=odd(W * b) * H + 3 * b),
            yuv.Surface(fmt, pitch=mul4(W * b), chroma_pitch=mul4(cw * b), chroma_offset=mul4(W * b) * H + 8)]


def model_layout(s):
    s = yuv.as_surface(s)
    L = M.layout(s.height, s.width, s.depth, s.subsampling, s.pitch, s.chroma_pitch, s.chroma_offset)
    assert L["nbytes"] == s.nbytes and s.frame_samples * s.itemsize == s.nbytes and (L["ch"], L["cw"]) == s.chroma_shape
    return L


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rgb_picture(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the format
def test_format_and_surface_follow_the_subsampling():
    f0 = yuv.Format(5, 7)
    assert f0.subsampling == "420" and f0 == yuv.Format(5, 7, "auto", False, "centre", 8) and hash(f0) == hash(yuv.Format(5, 7, subsampling="420"))
    assert (f0.subsampling_id, f0.chroma_shape, f0.frame_samples) == (0, (3, 4), 35 + 24)
    f2, f4 = yuv.Format(5, 7, subsampling="422"), yuv.Format(5, 7, depth=10, subsampling="444")
    assert (f2.subsampling_id, f2.chroma_shape, f2.frame_samples, f2.frame_bytes) == (1, (5, 4), 35 + 40, 75)
    assert (f4.subsampling_id, f4.chroma_shape, f4.frame_samples, f4.frame_bytes) == (2, (5, 7), 105, 210)
    assert f2 != f0 and f2.cropped(3, 4) == yuv.Format(3, 4, "bt601", subsampling="422") and f4.as_8bit() == yuv.Format(5, 7, subsampling="444")
    buf = np.arange(75, dtype=np.uint8)
    Y, U, V = f2.planes(buf)
    assert Y.shape == (5, 7) and U.shape == V.shape == (5, 4) and U[0, 0] == 35 and V[0, 0] == 55 and V[4, 3] == 74
    with pytest.raises(ValueError, match="4:2:2"):
        f2.check(np.zeros(59, np.uint8))
    with pytest.raises(ValueError, match="unknown subsampling"):
        yuv.Format(4, 4, subsampling="411")
    with pytest.raises(ValueError, match="no meaning for subsampling 444"):
        yuv.Format(4, 4, siting="left", subsampling="444")
    assert yuv.CHROMAS == ("planar", "uv", "vu")
    for chroma in ("uv", "vu"):
        with pytest.raises(ValueError, match="4:2:0 only"):
            yuv.Surface(f2, chroma)
    s = yuv.Surface(f4, pitch=16, chroma_pitch=20, chroma_offset=100)
    assert (s.subsampling, s.subsampling_id, s.nbytes) == ("444", 2, 100 + 20 * 9 + 14) and not s.is_tight
    assert s.tight() == yuv.Surface(f4) and s.tight().nbytes == f4.frame_bytes and s.cropped(2, 3).fmt == f4.cropped(2, 3)
    assert yuv.out_format(f4, True) == f4 and yuv.out_format(f4, False) == f4.as_8bit() and yuv.out_format(s, False) == yuv.Surface(f4.as_8bit())
    assert yuv.passes_through(f2) and not yuv.passes_through(s) and yuv.passes_through(s.tight())


def test_surface_of_knows_the_four_names():
    for name, depth, sub in (("yuv422p", 8, "422"), ("yuv444p", 8, "444"), ("yuv422p10le", 10, "422"), ("yuv444p10le", 10, "444")):
        s = yuv.surface_of(name, 6, 10, matrix="bt709")
        assert s == yuv.Surface(yuv.Format(6, 10, "bt709", depth=depth, subsampling=sub)) and s.is_tight and s.chroma == "planar" and not s.msb
        b = depth // 8 if depth == 8 else 2
        p = yuv.surface_of(name, 6, 10, pitch=32)
        assert p.pitch == 32 and p.chroma_pitch == (32 if sub == "444" else 16) and p.chroma_pitch >= p.chroma_shape[1] * b
    assert yuv.surface_of("yuv420p", 6, 10) == yuv.Surface(yuv.Format(6, 10))
    with pytest.raises(ValueError, match="yuv444p10le"):
        yuv.surface_of("yuv440p", 6, 10)


# ------------------------------------------------------------------------------------------------ twins == loop model
@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_numpy_twins_are_the_loop_model(H, W, sub, depth):
    combos = list(itertools.product(("bt601", "bt709"), sitings(sub), (False, True) if depth == 8 else (False,)))
    windows = WINDOWS[H, W] + (WINDOWS_444[H, W] if sub == "444" else [])
    for k, (matrix, siting, full) in enumerate(combos):
        fmt = yuv.Format(H, W, matrix, full, siting, depth, sub)
        for n, s in enumerate([fmt] + surfaces(fmt)):
            if (H, W) == (31, 41) and (k + n) % 3:              # the largest size: every combination once over the three layouts
                continue
            L = model_layout(s)
            buf = M.random_frame(L, seed=100 * k + n)
            want = M.decode(buf, L, matrix, int(full), siting)
            assert np.array_equal(yuv.decode_numpy(buf, s), want.astype(np.uint8))
            assert np.array_equal(yuv.decode_numpy(buf, s, bgr=True), want[:, :, ::-1].astype(np.uint8))
            if depth == 10:
                keep = M.decode(buf, L, matrix, 0, siting, keep=True)
                assert same_bits(yuv.decode_numpy_f32(buf, s), keep.astype(np.float32) / np.float32(1023))
                for win in windows:
                    wk = M.decode(buf, L, matrix, 0, siting, window=win, keep=True)
                    assert same_bits(yuv.decode_numpy_f32(buf, s, window=win), wk.astype(np.float32) / np.float32(1023))
                    y0, x0, h, w = win
                    assert np.array_equal(wk, keep[y0:y0 + h, x0:x0 + w])          # a window of the whole frame's decode
            for win in windows:                                 # crop: the samples untouched, decodable on their own layout
                y0, x0, h, w = win
                c = yuv.crop(buf, s, *win)
                Lc = model_layout(s.cropped(h, w))
                assert c.dtype == s.dtype and c.size * L["b"] == Lc["nbytes"]
                for plane, (sy, sx) in (("y", (1, 1)), ("u", M.STEPS[sub]), ("v", M.STEPS[sub])):
                    rows, cols = (h, w) if plane == "y" else (Lc["ch"], Lc["cw"])
                    raw, rawc = M.raw_bytes(buf, L), M.raw_bytes(c, Lc)
                    assert all(M.value(rawc, Lc, plane, r, q) == M.value(raw, L, plane, y0 // sy + r, x0 // sx + q) for r in range(rows) for q in range(cols))
            if n == 0 or s.is_tight:                            # encodes write tight frames
                rng = np.random.default_rng(7 * k + n)
                if depth == 8:
                    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
                    assert np.array_equal(M.raw_bytes(yuv.encode_numpy(rgb, s), L), M.encode(M.pixels(rgb, 8), L, matrix, int(full), siting))
                    assert np.array_equal(yuv.encode_numpy(rgb[:, :, ::-1], s, bgr=True), yuv.encode_numpy(rgb, s))
                else:
                    x = rng.uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32)
                    x.reshape(-1)[::5] = (rng.integers(0, 1023, x.reshape(-1)[::5].size) + 0.5).astype(np.float32) / np.float32(1023)     # ties
                    got = yuv.encode_numpy(x, s)
                    assert got.dtype == np.uint16 and np.array_equal(M.raw_bytes(got.astype("<u2"), L), M.encode(M.pixels(x, 10), L, matrix, 0, siting))
            else:
                with pytest.raises(ValueError, match="tight"):
                    yuv.encode_numpy(np.zeros((H, W, 3), np.uint8 if depth == 8 else np.float32), s)


def test_repack_moves_samples_between_layouts_of_one_subsampling():
    for sub, depth in itertools.product(SUBS, (8, 10)):
        fmt = yuv.Format(6, 10, depth=depth, subsampling=sub)
        buf = M.random_frame(model_layout(fmt), seed=3)
        for s in surfaces(fmt):
            moved = yuv.repack(buf, fmt, s)
            assert np.array_equal(yuv.repack(moved, s, fmt), buf) and np.array_equal(yuv.decode_numpy(moved, s), yuv.decode_numpy(buf, fmt))
        with pytest.raises(ValueError, match="subsampling"):
            yuv.repack(buf, fmt, yuv.Format(6, 10, depth=depth))
        with pytest.raises(ValueError, match="subsampling"):
            yuv.repack(buf, fmt, yuv.Format(6, 10, depth=depth, subsampling="444" if sub == "422" else "422"))


# ------------------------------------------------------------------------------------------------ the identities
@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("H,W", [(2, 2), (5, 3), (8, 16), (31, 41)], ids=lambda v: str(v))
def test_identities_between_the_subsamplings(H, W, depth):
    rng, top = np.random.default_rng(H * W + depth), (1024 if depth == 10 else 256)
    dt = np.uint16 if depth == 10 else np.uint8
    for siting in ("centre", "left"):
        f0, f2 = yuv.Format(H, W, "bt709", False, siting, depth), yuv.Format(H, W, "bt709", False, siting, depth, "422")
        ch, cw = f0.chroma_shape
        # D1: a 4:2:2 frame whose chroma rows are all equal decodes to the pixels of the 4:2:0 frame that holds those rows
        Y, urow, vrow = rng.integers(0, top, (H, W)), rng.integers(0, top, cw), rng.integers(0, top, cw)
        b0 = np.concatenate([Y.reshape(-1), np.tile(urow, ch), np.tile(vrow, ch)]).astype(dt)
        b2 = np.concatenate([Y.reshape(-1), np.tile(urow, H), np.tile(vrow, H)]).astype(dt)
        assert np.array_equal(yuv.decode_numpy(b2, f2), yuv.decode_numpy(b0, f0))
        if depth == 10:
            assert same_bits(yuv.decode_numpy_f32(b2, f2), yuv.decode_numpy_f32(b0, f0))
        # E1: a picture whose rows 2j and 2j + 1 are equal has 4:2:2 chroma rows 2j equal to the 4:2:0 encode's row j
        half = rng.integers(0, 256, (ch, W, 3)).astype(np.uint8)
        rgb = np.repeat(half, 2, axis=0)[:H]
        src = rgb if depth == 8 else (rgb.astype(np.float32) * np.float32(4.0117) / np.float32(1023))
        (_, U0, V0), (_, U2, V2) = f0.planes(yuv.encode_numpy(src, f0)), f2.planes(yuv.encode_numpy(src, f2))
        assert np.array_equal(U2[0::2], U0) and np.array_equal(V2[0::2], V0)
    # D2: flat U and V planes decode to the same pixels under all three subsamplings
    f = {s: yuv.Format(H, W, "bt601", False, "centre", depth, s) for s in yuv.SUBSAMPLINGS}
    Y, u, v = rng.integers(0, top, H * W), int(rng.integers(0, top)), int(rng.integers(0, top))
    flat = {s: np.concatenate([Y, np.full(f[s].chroma_shape[0] * f[s].chroma_shape[1], u), np.full(f[s].chroma_shape[0] * f[s].chroma_shape[1], v)]).astype(dt)
            for s in f}
    assert np.array_equal(yuv.decode_numpy(flat["422"], f["422"]), yuv.decode_numpy(flat["420"], f["420"]))
    assert np.array_equal(yuv.decode_numpy(flat["444"], f["444"]), yuv.decode_numpy(flat["420"], f["420"]))
    assert np.array_equal(yuv.decode_numpy(flat["420"], yuv.Format(H, W, "bt601", False, "left", depth)), yuv.decode_numpy(flat["444"], f["444"]))
    # E2: with columns 2i and 2i + 1 equal and centre siting, the 4:4:4 chroma at column 2i equals the 4:2:2 sample i
    half = rng.integers(0, 256, (H, (W + 1) // 2, 3)).astype(np.uint8)
    rgb = np.repeat(half, 2, axis=1)[:, :W]
    src = rgb if depth == 8 else (rgb.astype(np.float32) * np.float32(4.0117) / np.float32(1023))
    (_, U2, V2), (_, U4, V4) = f["422"].planes(yuv.encode_numpy(src, f["422"])), f["444"].planes(yuv.encode_numpy(src, f["444"]))
    assert np.array_equal(U4[:, 0::2], U2) and np.array_equal(V4[:, 0::2], V2)


def test_444_round_trips_within_the_flat_colour_bounds_and_greys_hit_mid():
    """A 4:4:4 round trip of any pixel is the 4:2:0 round trip of that flat colour: the bounds tests/test_yuv_cpu.py and
    tests/test_yuv10_cpu.py hold for flat colours -- 2 levels limited, 1 level full range at 8 bit, 2 levels at 10 bit -- carry
    over to random per-pixel colours, with no new number."""
    H, W = 24, 40
    rgb = rgb_picture(H, W, 5)
    for matrix, full in itertools.product(("bt601", "bt709"), (False, True)):
        f4, f0 = yuv.Format(H, W, matrix, full, subsampling="444"), yuv.Format(2, 2, matrix, full)
        back = yuv.decode_numpy(yuv.encode_numpy(rgb, f4), f4)
        assert np.abs(back.astype(int) - rgb.astype(int)).max() <= (1 if full else 2)
        for y, x in ((0, 0), (7, 13), (23, 39)):                # the same pixel as a flat 4:2:0 picture
            flat = np.broadcast_to(rgb[y, x], (2, 2, 3)).copy()
            assert np.array_equal(yuv.decode_numpy(yuv.encode_numpy(flat, f0), f0)[0, 0], back[y, x])
        f2 = yuv.Format(H, W, matrix, full, "left", subsampling="422")
        cols = np.broadcast_to(rgb[:, :1], (H, W, 3)).copy()    # flat rows: 4:2:2 keeps them within the same bound
        assert np.abs(yuv.decode_numpy(yuv.encode_numpy(cols, f2), f2).astype(int) - cols.astype(int)).max() <= (1 if full else 2)
    x10 = np.random.default_rng(6).integers(0, 1024, (H, W, 3))
    for matrix in ("bt601", "bt709"):
        f4 = yuv.Format(H, W, matrix, depth=10, subsampling="444")
        back = np.rint(yuv.decode_numpy_f32(yuv.encode_numpy(x10.astype(np.float32) / np.float32(1023), f4), f4) * np.float32(1023)).astype(int)
        assert np.abs(back - x10).max() <= 2
    # grey ramps: U = V = mid exactly
    for sub, depth in itertools.product(SUBS, (8, 10)):
        top, mid = (1023, 512) if depth == 10 else (255, 128)
        ramp = np.broadcast_to((np.arange(H * W) % (top + 1)).reshape(H, W, 1), (H, W, 3))
        for matrix, full in itertools.product(("bt601", "bt709"), (False, True) if depth == 8 else (False,)):
            fmt = yuv.Format(H, W, matrix, full, depth=depth, subsampling=sub)
            src = ramp.astype(np.uint8) if depth == 8 else ramp.astype(np.float32) / np.float32(1023)
            _, U, V = fmt.planes(yuv.encode_numpy(src, fmt))
            assert (U == mid).all() and (V == mid).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_origin_rules_and_the_420_only_calls():
    f2, f4, f0 = (yuv.Format(8, 12, depth=10, subsampling=s) for s in ("422", "444", "420"))
    b2, b4, b0 = (np.zeros(f.frame_samples, np.uint16) for f in (f2, f4, f0))
    assert yuv.crop(b2, f2, 3, 2, 4, 6).size == f2.cropped(4, 6).frame_samples and yuv.crop(b4, f4, 3, 5, 4, 6).size == 3 * 24
    assert yuv.decode_numpy_f32(b2, f2, window=(3, 2, 4, 6)).shape == (4, 6, 3) and yuv.decode_numpy_f32(b4, f4, window=(3, 5, 4, 6)).shape == (4, 6, 3)
    with pytest.raises(ValueError, match=r"even x0 for 4:2:2"):
        yuv.crop(b2, f2, 2, 3, 4, 6)
    with pytest.raises(ValueError, match=r"even x0 for 4:2:2"):
        yuv.decode_numpy_f32(b2, f2, window=(0, 1, 4, 6))
    with pytest.raises(ValueError, match=r"must be even for 4:2:0 frames"):        # the 4:2:0 messages stay
        yuv.crop(b0, f0, 1, 0, 4, 6)
    with pytest.raises(ValueError, match=r"must be even for 4:2:0 frames"):
        yuv.decode_numpy_f32(b0, f0, window=(0, 1, 4, 6))
    for f, b in ((f2, b2), (f4, b4)):
        with pytest.raises(ValueError, match="subsampling " + f.subsampling):
            yuv.window_numpy(b, f, 0, 0, 0, 4, 4)
        with pytest.raises(ValueError, match="outside"):
            yuv.crop(b, f, 6, 0, 4, 6)
    # HipOps refuses a non-4:2:0 format in every 4:2:0 method before it looks at anything else (no device, no library needed)
    ops = hip_ops.HipOps.__new__(hip_ops.HipOps)
    for f in (f2, f4, yuv.Surface(f2)):
        for call in (lambda: ops.yuv420_to_rgb(None, f, dst=None), lambda: ops.yuv420_window(None, f, 0, 0, 0, 4, 4), lambda: ops.rgb_to_yuv420(None, f),
                     lambda: ops.yuv420p10_to_f32(None, f, None), lambda: ops.f32_to_yuv420p10(None, f, None),
                     lambda: ops.yuv_surface_decode(None, yuv.as_surface(f)), lambda: ops.yuv_surface_encode(None, yuv.as_surface(f))):
            with pytest.raises(ValueError, match="subsampling " + f.subsampling):
                call()


# ------------------------------------------------------------------------------------------------ Y4M
TAGS = {"422": ("422", 8, "left"), "444": ("444", 8, "centre"), "422p10": ("422", 10, "left"), "444p10": ("444", 10, "centre")}


@pytest.mark.parametrize("tag", list(TAGS))
def test_y4m_tags_round_trip_byte_for_byte(tag):
    sub, depth, siting = TAGS[tag]
    fmt = yuv.Format(6, 10, "bt601", False, siting, depth, sub)
    frames = [M.random_frame(model_layout(fmt), seed=k) for k in range(3)]
    out = io.BytesIO()
    wr = yuv.Y4MWriter(out, fmt, "30000/1001")
    assert wr.ctag == tag
    for f in frames:
        wr.write(f)
    wr.close()
    data = out.getvalue()
    assert data.startswith(b"YUV4MPEG2 W10 H6 F30000:1001 Ip A0:0 C" + tag.encode() + b" XCOLORRANGE=LIMITED\n")
    assert len(data) == data.index(b"\n") + 1 + 3 * (6 + fmt.frame_bytes)
    with pytest.raises(ValueError, match=f"tag C{tag}"):                         # the default reader refuses them, by name, as ever
        yuv.Y4MReader(io.BytesIO(data))
    with pytest.raises(ValueError, match=f"tag C{tag}"):
        yuv.Y4MReader(io.BytesIO(data), accept=("420", "444" if sub == "422" else "422"))
    rd = yuv.Y4MReader(io.BytesIO(data), matrix="bt601", accept=("420", "422", "444"))
    assert rd.fmt == fmt and rd.ctag == tag and len(rd) == 3
    got = list(rd)
    assert all(g.dtype == fmt.dtype and np.array_equal(g, f) for g, f in zip(got, frames))
    again = io.BytesIO()
    with yuv.Y4MWriter(again, rd.fmt, rd.fps, ctag=rd.ctag) as w2:
        for g in got:
            w2.write(g)
    assert again.getvalue() == data
    with pytest.raises(ValueError, match="does not describe"):
        yuv.Y4MWriter(io.BytesIO(), fmt, 24, ctag="420jpeg")
    with pytest.raises(ValueError, match="does not describe"):
        yuv.Y4MWriter(io.BytesIO(), yuv.Format(6, 10), 24, ctag=tag)
    if sub == "422":                                                            # C422 means co-sited chroma: no tag for a centre-sited frame
        with pytest.raises(ValueError, match="no Y4M tag"):
            yuv.Y4MWriter(io.BytesIO(), yuv.Format(6, 10, depth=depth, subsampling="422"), 24)
    with pytest.raises(ValueError, match="tag C420paldv"):
        yuv.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 F25:1 C420paldv\n"), accept=("420", "422", "444"))
    with pytest.raises(ValueError, match="unknown subsampling"):
        yuv.Y4MReader(io.BytesIO(data), accept=("411",))


# ------------------------------------------------------------------------------------------------ the loops, numpy path
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend (tests/test_yuv_surface_cpu.py's stand-in): the pair mean."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, a, b):
        return {"I_t": (a + b) / 2}


H, W = 24, 40
RGB = CS.shot(3, H, W, seed=1, tone=60) + CS.shot(2, H, W, seed=2, tone=190)
LOOPS = {"nx": (lambda frames, **kw: mf.interpolate_video_nx(frames, Mean(), factor=4, **kw), (4, 1)),
         "nx_tta": (lambda frames, **kw: mf.interpolate_video_nx(frames, Mean(), factor=2, tta=True, **kw), (2, 1)),
         "retimed": (lambda frames, **kw: rt.interpolate_video_retimed(frames, Mean(), 24, 60, levels=2, **kw), (5, 2))}
# (n, m): output k is an original when k % n == 0, input k // n * m; five inputs give 4 n / m + 1 outputs


def original_of(step, k):
    return k // step[0] * step[1] if k % step[0] == 0 else None



def formats(sub, depth):
    """the format of the tests' streams (left-sited where a siting exists) and the I420 format beside it"""
    siting = "left" if sub == "422" else "centre"
    return yuv.Format(H, W, "bt709", False, siting, depth, sub), yuv.Format(H, W, "bt709", False, siting, depth)


def video_of(fmt):
    if fmt.depth == 8:
        return [yuv.encode_numpy(f, fmt) for f in RGB]
    return [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt) | np.uint16(k % 4) for k, f in enumerate(RGB)]


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("crop", (None, (16, 32)), ids=("whole", "crop"))
@pytest.mark.parametrize("sub", SUBS)
def test_8bit_loops_encode_the_rgb_loops_predictions(sub, crop, loop):
    """8 bit, and 10 bit without keep_depth: the loop decodes to uint8 RGB, runs the RGB loop and encodes what that produces.  So the
    expectation is the RGB loop itself on ``decode_numpy`` of the frames -- what an I420 run of the same pictures encodes."""
    run, step = LOOPS[loop]
    kw = {} if crop is None else dict(crop=crop)
    win = mf.centre_window(H, W, crop)
    for depth in (8, 10):
        fmt, _ = formats(sub, depth)
        out_fmt = fmt.as_8bit().cropped(win[2], win[3])
        video = video_of(fmt)
        keep = [f.copy() for f in video]
        pictures = [yuv.decode_numpy(f, fmt) for f in video]
        for with_scene in (False, True):
            sc_rgb, sc_got = (scene.SceneCuts(), scene.SceneCuts()) if with_scene else (None, None)
            rgb = list(run(iter(pictures), isBGR=False, scene=sc_rgb, **kw))
            got = list(run(iter(video), pixfmt=fmt, scene=sc_got, **kw))
            assert len(got) == len(rgb) == step[0] * (len(video) - 1) // step[1] + 1
            copies = 0
            for k, (g, r) in enumerate(zip(got, rgb)):
                if original_of(step, k) is not None:            # an original: the caller's array, or its crop
                    src = video[original_of(step, k)]
                    assert (g is src) if crop is None else np.array_equal(g, yuv.crop(src, fmt, *win))
                    continue
                same = [j for j, p in enumerate(pictures) if np.array_equal(r, p[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])]
                if with_scene and same:                         # inside a cut the RGB loop copies a frame: this loop copies its bytes
                    assert np.array_equal(g, yuv.crop(video[same[0]], fmt, *win))
                    copies += 1
                else:
                    assert g.dtype == np.uint8 and np.array_equal(g, yuv.encode_numpy(r, out_fmt))
            if with_scene:
                assert sc_got.cuts == sc_rgb.cuts and len(sc_got.cuts) == 1 and copies >= 1
        assert all(np.array_equal(a, b) for a, b in zip(video, keep))


@pytest.mark.parametrize("sub", SUBS)
def test_the_synthetic_shutter_takes_the_new_formats(sub):
    """8 bit as ever: every output is the caller's frame where the RGB conversion passes a picture through, and ``encode_numpy`` of
    the RGB conversion's (blended) frame everywhere else."""
    fmt, _ = formats(sub, 8)
    video = video_of(fmt)
    pictures = [yuv.decode_numpy(f, fmt) for f in video]
    report = {}
    rgb = list(rt.interpolate_video_retimed(iter(pictures), Mean(), 60, 24, levels=2, shutter=360, isBGR=False))
    got = list(rt.interpolate_video_retimed(iter(video), Mean(), 60, 24, levels=2, shutter=360, pixfmt=fmt, report=report))
    assert len(got) == len(rgb) >= 2 and report["blended"] >= 1
    for g, r in zip(got, rgb):
        same = [j for j, p in enumerate(pictures) if np.array_equal(r, p)]
        assert np.array_equal(g, video[same[0]] if same else yuv.encode_numpy(r, fmt))
    with pytest.raises(ValueError):
        list(rt.interpolate_video_retimed(iter(video_of(formats(sub, 10)[0])), Mean(), 24, 60, levels=2, shutter=180, pixfmt=formats(sub, 10)[0],
                                          keep_depth=True))


class Recorder:
    """``yuv.encode_numpy`` with its fp32 sources kept: the predictions a keep_depth run encodes"""

    def __init__(self, monkeypatch):
        self.sources, real = [], yuv.encode_numpy

        def spy(rgb, fmt, bgr=False):
            self.sources.append(np.array(rgb, copy=True))
            return real(rgb, fmt, bgr)
        monkeypatch.setattr(yuv, "encode_numpy", spy)


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("crop", (None, (16, 32)), ids=("whole", "crop"))
@pytest.mark.parametrize("sub", SUBS)
def test_keep_depth_loops_encode_the_predictions_of_the_i420_run(sub, crop, loop, monkeypatch):
    """10 bit with keep_depth.  Frames with flat U and V planes decode to the same pixels under every subsampling (D2), so the I420
    run of the same luma makes the same fp32 predictions: produced frames are ``encode_numpy`` of exactly those, in this format."""
    run, step = LOOPS[loop]
    kw = dict(keep_depth=True) if crop is None else dict(keep_depth=True, crop=crop)
    win = mf.centre_window(H, W, crop)
    fmt, fmt0 = formats(sub, 10)
    out_fmt = fmt.cropped(win[2], win[3])
    luma = [fmt0.planes(yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt0))[0] for f in RGB]
    flat = lambda Y, f: np.concatenate([Y.reshape(-1), np.full(f.chroma_shape[0] * f.chroma_shape[1], 400), np.full(f.chroma_shape[0] * f.chroma_shape[1], 600)]).astype(np.uint16)
    video, video0 = [flat(Y, fmt) for Y in luma], [flat(Y, fmt0) for Y in luma]
    for with_scene in (False, True):
        sc0, sc1 = (scene.SceneCuts(), scene.SceneCuts()) if with_scene else (None, None)
        rec = Recorder(monkeypatch)
        ref = list(run(iter(video0), pixfmt=fmt0, scene=sc0, **kw))
        predictions = rec.sources
        monkeypatch.undo()
        got = list(run(iter(video), pixfmt=fmt, scene=sc1, **kw))
        assert len(got) == len(ref) == step[0] * (len(video) - 1) // step[1] + 1 and all(g.dtype == np.uint16 for g in got)
        made = iter(predictions)
        for k, (g, r) in enumerate(zip(got, ref)):
            if original_of(step, k) is not None:
                src = video[original_of(step, k)]
                assert (g is src) if crop is None else np.array_equal(g, yuv.crop(src, fmt, *win))
                continue
            same = [j for j, f in enumerate(video0) if np.array_equal(r, yuv.crop(f, fmt0, *win))]
            if with_scene and same:                             # a scene cut copies bytes
                assert np.array_equal(g, yuv.crop(video[same[0]], fmt, *win))
            else:
                assert np.array_equal(g, yuv.encode_numpy(next(made), out_fmt))
        assert next(made, None) is None
        if with_scene:
            assert sc1.cuts == sc0.cuts and len(sc1.cuts) == 1


def test_odd_crop_origins_follow_the_subsampling():
    for sub in SUBS:
        fmt, _ = formats(sub, 8)
        video = video_of(fmt)
        # a 14 x 32 window of 24 x 40 frames sits at (5, 4): odd y0, fine for both; 16 x 30 sits at (4, 5): 4:4:4 only
        got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=2, pixfmt=fmt, crop=(14, 32)))
        assert np.array_equal(got[0], yuv.crop(video[0], fmt, 5, 4, 14, 32))
        run = lambda: list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 48, levels=1, pixfmt=fmt, crop=(16, 30)))
        if sub == "444":
            assert np.array_equal(run()[0], yuv.crop(video[0], fmt, 4, 5, 16, 30))
        else:
            with pytest.raises(ValueError, match="even x0 for 4:2:2"):
                run()
    with pytest.raises(ValueError, match="must be even for 4:2:0 frames"):
        list(mf.interpolate_video_nx(iter([np.zeros(yuv.Format(H, W).frame_samples, np.uint8)] * 2), Mean(), factor=2, pixfmt=yuv.Format(H, W), crop=(14, 32)))


@pytest.mark.parametrize("tag", ("444p10", "422p10", "444", "422"))
def test_interpolate_y4m_keeps_the_layout(tag):
    sub, depth, siting = TAGS[tag]
    fmt = yuv.Format(H, W, "bt601", False, siting, depth, sub)
    video = video_of(fmt)
    src = io.BytesIO()
    with yuv.Y4MWriter(src, fmt, 24) as wr:
        for f in video:
            wr.write(f)
    data = src.getvalue()
    for kw in (dict(factor=2), dict(factor=4), dict(fps_out=60, levels=2)):
        for keep in ((False, True) if depth == 10 else (False,)):
            dst = io.BytesIO()
            info = yuv.interpolate_y4m(io.BytesIO(data), dst, Mean(), matrix="bt601", keep_depth=keep, **kw)
            rd = yuv.Y4MReader(io.BytesIO(dst.getvalue()), matrix="bt601", accept=yuv.SUBSAMPLINGS)
            deep = keep and depth == 10
            assert rd.fmt == (fmt if deep else fmt.as_8bit()) and rd.ctag == (tag if (deep or depth == 8) else sub)
            out = list(rd)
            assert len(out) == info["frames_out"] > len(video) and info["frames_in"] == len(video)
            if "factor" in kw:
                originals = out[::kw["factor"]]
                want = video if (deep or depth == 8) else [yuv.to_8bit(f, fmt) for f in video]
                assert len(originals) == len(video) and all(np.array_equal(a, b) for a, b in zip(originals, want))     # byte for byte
            else:
                first = video[0] if (deep or depth == 8) else yuv.to_8bit(video[0], fmt)
                assert np.array_equal(out[0], first) and rd.fps == 60


def test_raw_streams_take_the_new_surfaces():
    s = yuv.surface_of("yuv422p10le", H, W, pitch=2 * W + 16, matrix="bt709", siting="left")
    fmt = s.fmt
    frames = [yuv.repack(f, fmt, s) for f in video_of(fmt)]
    for keep in (False, True):
        dst = io.BytesIO()
        info = yuv.interpolate_raw(io.BytesIO(b"".join(f.astype("<u2").tobytes() for f in frames)), dst, Mean(), s, 24, factor=2, keep_depth=keep)
        want = list(mf.interpolate_video_nx(iter(frames), Mean(), factor=2, pixfmt=s, keep_depth=keep))
        if not keep:
            want = [yuv.to_8bit(f, s.tight()) if f.dtype == np.uint16 else f for f in want]
        assert dst.getvalue() == b"".join(f.astype("<u2" if keep else np.uint8).tobytes() for f in want) and info["frames_out"] == len(want) == 9
        assert len(dst.getvalue()) == 9 * (s.tight() if keep else s.as_8bit()).nbytes
    tools = os.path.join(CS.ROOT, "tools", "interp_raw.py")
    assert all(f'"{name}"' in open(tools).read() for name in yuv.PIX_FMTS_SUB)         # --pix-fmt takes the four names


# ------------------------------------------------------------------------------------------------ ABI
def test_sub_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    for name in ("atmvfi_yuv_decode", "atmvfi_yuv_encode"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
        assert lib.atmvfi_plan_fn_id(name.encode()) >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 29
    assert callable(hip_ops.HipOps.yuv_sub_decode) and callable(hip_ops.HipOps.yuv_sub_encode)
    # the subsampling is one int of the frame descriptor, after siting
    names = [n for n, _ in hip_ops.YuvDesc._fields_]
    assert names.index("subsampling") == names.index("siting") + 1 and re.search(r"int32_t siting;.*\n\s*int32_t subsampling;", hdr)
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error

    def dec(buf=P, H=64, W=96, depth=8, matrix=0, full=0, siting=0, sub=1, chroma=0, msb=0, pitch=0, cpitch=0, coff=0, keep=0, y0=0, x0=0, h=64,
            w=96, dst_u8=None, bgr=0, dst=P, Hp=64, Wp=96, pt=0, pl=0):
        d = hip_ops.YuvDesc(H=H, W=W, depth=depth, matrix=matrix, full_range=full, siting=siting, subsampling=sub, chroma=chroma, msb=msb,
                            pitch=pitch, chroma_pitch=cpitch, chroma_offset=coff)
        rc = lib.atmvfi_yuv_decode(ctypes.byref(d), buf, keep, 0, y0, x0, h, w, dst_u8, bgr, dst, Hp, Wp, pt, pl, None)
        assert rc == -1 and err().startswith(b"yuv_decode: ")      # one entry point for every subsampling
        return rc

    def enc(src_u8=None, bgr=0, src=P, Hp=64, Wp=96, pt=0, pl=0, H=64, W=96, depth=8, matrix=0, full=0, siting=0, sub=1, chroma=0, msb=0, buf=P):
        d = hip_ops.YuvDesc(H=H, W=W, depth=depth, matrix=matrix, full_range=full, siting=siting, subsampling=sub, chroma=chroma, msb=msb)
        rc = lib.atmvfi_yuv_encode(ctypes.byref(d), src_u8, bgr, src, Hp, Wp, pt, pl, buf, None)
        assert rc == -1 and err().startswith(b"yuv_encode: ")
        return rc
    for sub in (1, 2):
        assert dec(sub=sub, buf=None) == -1 and b"yuv_decode: null source" in err()
        assert dec(sub=sub, dst=None) == -1 and b"both outputs are null" in err()
        assert dec(sub=sub, H=0) == -1 and b"at least 1" in err()
        assert dec(sub=sub, depth=12) == -1 and b"depth must be 8 or 10" in err()
        assert dec(sub=sub, depth=10, full=1) == -1 and b"full range" in err()
        assert dec(sub=sub, matrix=2) == -1 and b"unknown matrix" in err()
        assert dec(sub=sub, siting=2) == -1
        for chroma in (1, 2):
            assert dec(sub=sub, chroma=chroma) == -1 and b"planar with LSB samples" in err()
            assert enc(sub=sub, chroma=chroma) == -1 and b"planar with LSB samples" in err()
        assert dec(sub=sub, depth=10, msb=1) == -1 and b"planar with LSB samples" in err()
        assert enc(sub=sub, depth=10, msb=1) == -1 and b"planar with LSB samples" in err()
        assert dec(sub=sub, pitch=95) == -1 and b"at least a luma row" in err()
        assert dec(sub=sub, keep=1) == -1 and b"keep_depth needs a 10-bit surface" in err()
        assert dec(sub=sub, keep=1, depth=10, dst_u8=P) == -1 and b"not with keep_depth" in err()
        assert dec(sub=sub, y0=2) == -1 and b"outside the" in err()
        assert dec(sub=sub, Hp=63) == -1 and b"smaller than the window" in err()
        assert dec(sub=sub, dst=P + 2) == -1 and b"4-byte aligned" in err()
        assert dec(sub=sub, H=100000, W=100000, h=100000, w=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()
        assert enc(sub=sub, buf=None) == -1 and b"yuv_encode: null destination" in err()
        assert enc(sub=sub, src=None) == -1 and b"exactly one" in err()
        assert enc(sub=sub, depth=10, src=None, src_u8=P) == -1 and b"fp32 canvas" in err()
        assert enc(sub=sub, Wp=95) == -1 and b"smaller than the frame" in err()
        assert enc(sub=sub, src=P + 1) == -1 and b"4-byte aligned" in err()
    for sub in (-1, 3):
        assert dec(sub=sub) == -1 and b"unknown subsampling" in err()
        assert enc(sub=sub) == -1 and b"unknown subsampling" in err()
    assert dec(sub=2, siting=1) == -1 and b"no meaning for 4:4:4" in err()
    assert enc(sub=2, siting=1) == -1 and b"no meaning for 4:4:4" in err()
    # chroma rows: (W + 1) / 2 samples at 4:2:2, W at 4:4:4
    assert dec(sub=1, cpitch=47) == -1 and b"at least a chroma row" in err()
    assert dec(sub=2, cpitch=95) == -1 and b"at least a chroma row" in err()
    # the window origin: a multiple of the subsampling step per axis
    assert dec(sub=1, x0=3, w=8) == -1 and b"even x0 for 4:2:2" in err()
    assert dec(sub=0, chroma=0, y0=1, h=8) == -1 and b"yuv_decode" in err() and b"must be even" in err()      # sub 0: the 4:2:0 rule
    assert dec(sub=0, chroma=3) == -1 and b"unknown chroma layout" in err()
    assert enc(sub=0, chroma=0, msb=1) == -1 and b"yuv_encode" in err() and b"msb needs depth 10" in err()
    # an odd y0 at 4:2:2 and any origin at 4:4:4 pass the origin rule (and fail the next check: the canvas)
    assert dec(sub=1, y0=1, h=8, Hp=4) == -1 and b"smaller than the window" in err()
    assert dec(sub=2, y0=1, x0=3, h=8, w=8, Hp=4) == -1 and b"smaller than the window" in err()
