"""CPU: deep RGB frames (``pixfmt.DeepRGB``, atm-vfi_amd/rgb16.py; csrc/rgb16.hip's definition) without a GPU: the vectorised twins against
the per-sample loop model of tests/cpu_rgb16.py, the round trip and the tie to the 8-bit path over every code, the kernel's
reciprocal form of q / top in exact rational arithmetic, ties and clamps of the encode, the descriptor, raw I/O, the ABI's host-side
checks, and the loops on a CPU stand-in model."""
import importlib
import io
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cpu_rgb16 as M
import cpu_scene as CS

mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
scene = importlib.import_module("atm-vfi_amd.scene")
yuv = importlib.import_module("atm-vfi_amd.yuv")
rgb16 = importlib.import_module("atm-vfi_amd.rgb16")
pixfmt = importlib.import_module("atm-vfi_amd.pixfmt")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
shutter = importlib.import_module("atm-vfi_amd.shutter")
active = importlib.import_module("atm-vfi_amd.active")

# (H, W, window or None, canvas or None, pad_top, pad_left): the GPU list of tests/test_gpu_rgb16.py without 2160 x 4096
GEOMETRIES = [
    (16, 16, None, None, 0, 0),
    (18, 22, None, None, 0, 0),
    (16, 16, None, (32, 32), 8, 8),
    (18, 22, (3, 5, 11, 13), (24, 32), 6, 9),       # odd origin and size, unequal pads on all four sides
    (18, 22, (0, 0, 18, 22), None, 0, 0),           # window == frame
    (18, 22, (17, 21, 1, 1), (3, 4), 1, 2),         # a 1 x 1 window
]


def padded(hw3, canvas, pad_top, pad_left):
    """[h,w,3] -> [3,Hp,Wp] with replicate padding, the picture at (pad_top, pad_left)"""
    h, w = hw3.shape[:2]
    Hp, Wp = (h, w) if canvas is None else canvas
    return np.pad(hw3.transpose(2, 0, 1), ((0, 0), (pad_top, Hp - h - pad_top), (pad_left, Wp - w - pad_left)), mode="edge")


# ------------------------------------------------------------------------------------------------ the twins are the loops
@pytest.mark.parametrize("depth", M.DEPTHS)
@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_twins_are_the_sample_loops(geo, layout, depth):
    H, W, window, canvas, pt, pl = geo
    rng = np.random.default_rng(H * 1000 + W + depth)
    fmt = yuv.DeepRGB(H, W, depth, layout)
    frame = M.random_frame(rng, H, W, depth, over=True)
    f32, u8 = M.decode_loop(frame, layout, depth, H, W, window, canvas, pt, pl)
    got = rgb16.decode_numpy_f32(frame, fmt, window=window)
    assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(padded(got, canvas, pt, pl), f32)
    probe = rgb16.probe_numpy(frame, fmt, window=window)
    assert probe.dtype == np.uint8 and np.array_equal(probe, u8)
    # the encode: the canvas of fp32 noise around [0, 1], the picture at the pads
    y0, x0, h, w = window or (0, 0, H, W)
    Hp, Wp = canvas or (h, w)
    src = rng.uniform(-0.1, 1.1, (3, Hp, Wp)).astype(np.float32)
    out = fmt.cropped(h, w)
    want = M.encode_loop(src, layout, depth, h, w, pt, pl)
    enc = rgb16.encode_numpy(np.ascontiguousarray(src[:, pt:pt + h, pl:pl + w].transpose(1, 2, 0)), out)
    assert enc.dtype == np.uint16 and enc.ndim == 1 and np.array_equal(enc, want)
    # crop: the samples of the window, as a frame of the cropped format
    c = rgb16.crop(frame, fmt, y0, x0, h, w)
    assert c.dtype == np.uint16 and c.shape == (3 * h * w,)
    for y, x, ch in ((0, 0, 0), (h - 1, w - 1, 2), (h // 2, w // 2, 1)):
        assert c[M.sample_index(layout, h, w, y, x, ch)] == frame[M.sample_index(layout, H, W, y0 + y, x0 + x, ch)]
    assert np.array_equal(rgb16.decode_numpy_f32(c, out), got)


def codes_frame(depth, layout):
    """every code of the depth, once per component: a frame of (top + 1) pixels"""
    n = M.top_of(depth) + 1
    fmt = yuv.DeepRGB(1, n, depth, layout)
    rgb = np.stack([np.arange(n), np.arange(n)[::-1], (np.arange(n) * 7) % n], axis=1).astype(np.uint16).reshape(1, n, 3)
    return fmt, rgb, rgb16._layout_of(rgb, fmt)


@pytest.mark.parametrize("depth", M.DEPTHS)
@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_round_trip_of_every_code(depth, layout):
    fmt, rgb, frame = codes_frame(depth, layout)
    x = rgb16.decode_numpy_f32(frame, fmt)
    assert np.array_equal(x, rgb.astype(np.float32) / np.float32(M.top_of(depth)))
    assert np.array_equal(rgb16.encode_numpy(x, fmt), frame)
    assert np.array_equal(rgb16.probe_numpy(frame, fmt), (rgb >> (depth - 8)).astype(np.uint8))


@pytest.mark.parametrize("depth", (10, 12))
def test_samples_above_the_depth_decode_as_top(depth):
    top = M.top_of(depth)
    fmt = yuv.DeepRGB(2, 4, depth, "rgb48")
    frame = np.array([top + 1, 65535, top, top - 1, 1 << 15, top + 7] * 4, np.uint16)
    want = np.minimum(frame, top).reshape(2, 4, 3)
    assert np.array_equal(rgb16.decode_numpy_f32(frame, fmt), want.astype(np.float32) / np.float32(top))
    assert np.array_equal(rgb16.probe_numpy(frame, fmt), (want >> (depth - 8)).astype(np.uint8))
    f32, u8 = M.decode_loop(frame, "rgb48", depth, 2, 4)
    assert f32.max() == np.float32(1) and u8.max() == 255


def test_depth_16_of_257_b_is_the_8_bit_value():
    b = np.arange(256)
    fmt = yuv.DeepRGB(1, 256, 16, "rgb48")
    frame = np.repeat((257 * b).astype(np.uint16), 3)
    x = rgb16.decode_numpy_f32(frame, fmt)
    assert np.array_equal(x[0, :, 0], b.astype(np.float32) / np.float32(255)) and np.array_equal(x[0, :, 0], x[0, :, 2])
    assert np.array_equal(rgb16.probe_numpy(frame, fmt)[0, :, 1], b.astype(np.uint8))


def fl32(v: Fraction) -> Fraction:
    """round to nearest even onto the fp32 grid (normal numbers: everything here lies above 2^-20)"""
    if v == 0:
        return v
    s, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    unit = Fraction(2) ** (e - 23)
    n, r = divmod(a, unit)
    n = int(n)
    if r * 2 > unit or (r * 2 == unit and n % 2):
        n += 1
    return s * n * unit


@pytest.mark.parametrize("depth", M.DEPTHS)
def test_the_kernels_reciprocal_form_is_the_division(depth):
    """csrc/rgb16.hip unit_of: y = fl(q r), r = fl(1 / top); fma(fma(-top, y, q), r, y) -- one rounding per fma -- equals
    fl(q / top) for every code, in exact rational arithmetic."""
    top = M.top_of(depth)
    r = fl32(Fraction(1, top))
    assert float(r) == float(np.float32(1.0) / np.float32(top))
    q = np.arange(top + 1)
    want = q.astype(np.float32) / np.float32(top)
    for k in range(top + 1):
        y = fl32(k * r)
        e = fl32(k - top * y)
        assert fl32(e * r + y) == Fraction(float(want[k])), (depth, k)


# ------------------------------------------------------------------------------------------------ the encode's rounding
@pytest.mark.parametrize("depth", M.DEPTHS)
def test_encode_ties_go_to_even_and_the_ends_clamp(depth):
    top = M.top_of(depth)
    t = M.ties(depth)
    assert len(t) == 8 and {k % 2 for _, k in t} == {0}
    assert any(np.float32(x * np.float32(top)) - np.floor(x * np.float32(top)) == 0.5 and int(np.floor(x * np.float32(top))) % 2 == 1 for x, _ in t)
    xs = np.array([x for x, _ in t] + [-0.0, 0.0, -1.0, -1e30, 1.0, 1.0 + 2.0 ** -20, 2.0, 1e30, 0.5 / top * 0.999, 1.0 - 0.25 / top], np.float32)
    want = np.array([k for _, k in t] + [0, 0, 0, 0, top, top, top, top, 0, top], np.uint16)
    n = xs.size
    fmt = yuv.DeepRGB(1, n, depth, "gbrp")
    src = np.stack([xs, xs[::-1], xs], axis=1).reshape(1, n, 3)
    got = rgb16.encode_numpy(np.ascontiguousarray(src), fmt).reshape(3, n)
    assert np.array_equal(got[2], want) and np.array_equal(got[0], want[::-1]) and np.array_equal(got[1], want)
    loop = M.encode_loop(np.ascontiguousarray(src.transpose(2, 0, 1)), "gbrp", depth, 1, n)
    assert np.array_equal(loop, got.reshape(-1))


# ------------------------------------------------------------------------------------------------ the descriptor
def test_deep_rgb_descriptor():
    f = yuv.DeepRGB(18, 22)
    assert (f.depth, f.layout, f.layout_id, f.steps, f.dtype, f.is_tight) == (16, "rgb48", 0, (1, 1), np.uint16, True)
    assert f.frame_samples == 3 * 18 * 22 and f.frame_bytes == f.nbytes == 6 * 18 * 22 and f.tight() is f
    assert f.cropped(4, 6) == yuv.DeepRGB(4, 6) and yuv.DeepRGB(4, 6, 10, "gbrp").layout_id == 2 and yuv.DeepRGB(4, 6, 12, "bgr48").layout_id == 1
    assert pixfmt.DeepRGB is yuv.DeepRGB and hash(f) == hash(yuv.DeepRGB(18, 22, 16, "rgb48"))
    for kw, msg in ((dict(depth=8), "depth must be 10, 12 or 16"), (dict(depth=14), "depth must be 10, 12 or 16"),
                    (dict(layout="rgb24"), "unknown layout 'rgb24'"), (dict(layout="gbrap"), "unknown layout")):
        with pytest.raises(ValueError, match=msg):
            yuv.DeepRGB(4, 6, **kw)
    for hw in ((0, 6), (4, 0), (-1, 3)):
        with pytest.raises(ValueError, match="at least 1"):
            yuv.DeepRGB(*hw)
    a = np.zeros((18, 22, 3), np.uint16)
    for shaped in (a, a.reshape(3, 18, 22), a.reshape(-1)):
        v = f.check(shaped, "t")
        assert v.shape == (f.frame_samples,) and np.shares_memory(v, a)
    for bad in (a.astype(np.uint8), a.reshape(-1)[:-1], np.zeros((18, 22, 4), np.uint16), a[:, ::2], np.zeros((18, 22, 3), np.int16)):
        with pytest.raises(ValueError, match="t: a contiguous uint16 rgb48 frame of 1188 samples"):
            f.check(bad, "t")
    assert yuv.out_format(f, True) is f and yuv.passes_through(f)


def test_surface_of_the_five_names():
    want = {"rgb48le": ("rgb48", 16), "bgr48le": ("bgr48", 16), "gbrp10le": ("gbrp", 10), "gbrp12le": ("gbrp", 12), "gbrp16le": ("gbrp", 16)}
    for name, (layout, depth) in want.items():
        assert yuv.surface_of(name, 18, 22) == yuv.DeepRGB(18, 22, depth, layout)
        with pytest.raises(ValueError, match="tight RGB"):
            yuv.surface_of(name, 18, 22, pitch=256)
    with pytest.raises(ValueError, match="gbrp12le"):
        yuv.surface_of("gbrp14le", 18, 22)
    assert yuv.surface_of("nv12", 18, 22).chroma == "uv"


def test_raw_reader_and_writer_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    fmt = yuv.surface_of("gbrp12le", 6, 10)
    frames = [M.random_frame(rng, 6, 10, 12) for _ in range(3)]
    path = tmp_path / "clip.gbrp12le"
    with yuv.RawWriter(path, fmt) as wr:
        for f in frames:
            wr.write(f.reshape(3, 6, 10))
    assert os.path.getsize(path) == 3 * fmt.nbytes
    raw = open(path, "rb").read()
    assert raw[:2] == int(frames[0][0]).to_bytes(2, "little")
    with yuv.RawReader(path, fmt, 24) as rd:
        assert len(rd) == 3
        got = list(rd)
    assert all(g.dtype == np.uint16 and np.array_equal(g, f) for g, f in zip(got, frames))
    with pytest.raises(ValueError, match="truncated"):
        list(yuv.RawReader(io.BytesIO(raw[:-1]), fmt, 24))
    with pytest.raises(ValueError, match="RawWriter.write"):
        yuv.RawWriter(io.BytesIO(), fmt).write(frames[0].astype(np.uint8))


# ------------------------------------------------------------------------------------------------ the loops, host backend
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend: the pair mean, counting the pairs it is asked for."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.pairs = 0

    def forward(self, a, b):
        self.pairs += a.shape[0]
        return {"I_t": (a + b) / 2}


H, W = 24, 40


def deep_video(fmt, rgb8, shaped=True):
    """uint8 RGB frames -> frames of ``fmt`` that use the depth's low bits; ``shaped``: as the caller would hold them ([H,W,3] / [3,H,W])"""
    rng = np.random.default_rng(17)
    out = []
    for f in rgb8:
        q = (f.astype(np.int64) * M.top_of(fmt.depth)) // 255
        q = np.clip(q + rng.integers(-3, 4, q.shape), 0, M.top_of(fmt.depth)).astype(np.uint16)
        flat = rgb16._layout_of(q, fmt)
        out.append(flat.reshape((3, fmt.height, fmt.width) if fmt.layout == "gbrp" else (fmt.height, fmt.width, 3)) if shaped else flat)
    return out


def mean_of(a, b):
    return (a + b) / np.float32(2)


def expected_nx(P, fmt, factor, window=None):
    """the N-x loop's frames for the stand-in: originals as objects, produced frames from the chained fp32 means"""
    out_fmt = fmt if window is None else fmt.cropped(*window[2:])
    out = []
    for a, b in zip(P, P[1:]):
        pos = {0: rgb16.decode_numpy_f32(a, fmt, window=window), factor: rgb16.decode_numpy_f32(b, fmt, window=window)}
        span = factor
        while span > 1:
            for lo in range(0, factor, span):
                pos[lo + span // 2] = mean_of(pos[lo], pos[lo + span])
            span //= 2
        out.append(a)
        out += [rgb16.encode_numpy(pos[k], out_fmt) for k in range(1, factor)]
    return out + [P[-1]]


def same_frames(got, want, P):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if any(w is p for p in P):
            assert g is w                                               # originals are the caller's objects
        else:
            assert g.dtype == np.uint16 and g.ndim == 1 and np.array_equal(g, w) and all(g is not p for p in P)


@pytest.mark.parametrize("layout,depth", [("rgb48", 16), ("bgr48", 16), ("gbrp", 10), ("gbrp", 12)])
@pytest.mark.parametrize("factor", (2, 4))
def test_nx_on_the_stand_in(layout, depth, factor):
    fmt = yuv.DeepRGB(H, W, depth, layout)
    P = deep_video(fmt, CS.shot(3, H, W, seed=3, tone=120))
    keep = [p.copy() for p in P]
    m = Mean()
    got = list(mf.interpolate_video_nx(iter(P), m, factor=factor, pixfmt=fmt, keep_depth=True))
    assert m.pairs == 2 * (factor - 1)
    same_frames(got, expected_nx(P, fmt, factor), P)
    assert all(np.array_equal(a, b) for a, b in zip(P, keep))          # the caller's buffers are untouched
    # tta of a symmetric stand-in is the prediction itself; a divisor pads with replicas: the same frames
    again = list(mf.interpolate_video_nx(iter(P), Mean(), factor=factor, pixfmt=fmt, keep_depth=True, tta=True, divisor=None))
    same_frames(again, got, P)


def test_nx_crop_at_an_odd_origin():
    fmt = yuv.DeepRGB(H, W, 12, "gbrp")
    P = deep_video(fmt, CS.shot(3, H, W, seed=4, tone=90))
    got = list(mf.interpolate_video_nx(iter(P), Mean(), factor=4, pixfmt=fmt, keep_depth=True, crop=(14, 30)))
    window = mf.centre_window(H, W, (14, 30))
    assert window == (5, 5, 14, 30)
    want = expected_nx(P, fmt, 4, window=window)
    assert len(got) == len(want) == 9
    for i, (g, w) in enumerate(zip(got, want)):
        if i % 4 == 0:                                                  # an original: rgb16.crop of the caller's array
            w = rgb16.crop(w, fmt, *window)
        assert g.dtype == np.uint16 and g.shape == (3 * 14 * 30,) and np.array_equal(g, w)


def test_scene_cut_on_a_two_shot_deep_video():
    fmt = yuv.DeepRGB(H, W, 16, "rgb48")
    rgb8 = CS.shot(3, H, W, seed=1, tone=60) + CS.shot(3, H, W, seed=2, tone=190)
    P = deep_video(fmt, rgb8)
    P8 = [rgb16.probe_numpy(p, fmt) for p in P]
    for run, run8 in ((lambda fr, m, **kw: mf.interpolate_video_nx(fr, m, factor=4, **kw), None),
                      (lambda fr, m, **kw: rt.interpolate_video_retimed(fr, m, 24, 60, levels=3, **kw), None)):
        s16, s8, m = scene.SceneCuts(), scene.SceneCuts(), Mean()
        got = list(run(iter(P), m, pixfmt=fmt, keep_depth=True, scene=s16))
        list(run(iter(P8), Mean(), isBGR=False, scene=s8))
        assert s16.cuts == s8.cuts == [2] and s16.stats == s8.stats    # the decisions of the truncated 8-bit picture
        # the cut segment's frames are copies of the caller's arrays, in their shape
        copies = [g for g in got if g.shape == P[0].shape and all(g is not p for p in P)]
        assert copies and all(any(np.array_equal(c, p) for p in (P[2], P[3])) for c in copies)
    full = list(mf.interpolate_video_nx(iter(P), m, factor=4, pixfmt=fmt, keep_depth=True, scene=scene.SceneCuts()))
    assert [np.array_equal(full[8 + k], P[2 if k <= 2 else 3]) for k in (1, 2, 3)] == [True] * 3


def test_retimed_24_to_60_on_the_stand_in():
    fmt = yuv.DeepRGB(H, W, 10, "gbrp")
    P = deep_video(fmt, CS.shot(4, H, W, seed=6, tone=140))
    m, report = Mean(), {}
    got = list(rt.interpolate_video_retimed(iter(P), m, 24, 60, levels=3, pixfmt=fmt, keep_depth=True, report=report))
    slots = list(rt.retime_slots(range(len(P)), 24, 60, 3))
    assert len(got) == len(slots) == report["outputs"] and m.pairs == report["forwards"] > 0
    dec = [rgb16.decode_numpy_f32(p, fmt) for p in P]

    def at(seg, p, n=8):
        """position p of n between frames seg and seg + 1, by the recursion: the chained means"""
        lo, hi, a, b = 0, n, dec[seg], dec[seg + 1] if seg + 1 < len(dec) else None
        while True:
            if p == lo:
                return a
            if p == hi:
                return b
            mid = (lo + hi) // 2
            c = mean_of(a, b)
            if p == mid:
                return c
            lo, hi, a, b = (lo, mid, a, c) if p < mid else (mid, hi, c, b)
    for g, (seg, p) in zip(got, slots):
        if p == 0 or p == 8:
            assert g is P[seg + (p == 8)]
        else:
            assert g.dtype == np.uint16 and np.array_equal(g, rgb16.encode_numpy(at(seg, p), fmt))
    # a repeated frame is dropped, as the probe pictures decide
    Pd = P[:2] + [P[1].copy()] + P[2:]
    d, d8 = rt.Duplicates(), rt.Duplicates()
    list(rt.interpolate_video_retimed(iter(Pd), Mean(), 24, 60, levels=3, pixfmt=fmt, keep_depth=True, dedup=d))
    list(rt.interpolate_video_retimed(iter([rgb16.probe_numpy(p, fmt) for p in Pd]), Mean(), 24, 60, levels=3, isBGR=False, dedup=d8))
    assert 2 in d.dropped and d.dropped == d8.dropped and d.stats == d8.stats


class Cap:
    """a ``cv2.VideoCapture`` stand-in over uint16 [H,W,3] frames (what OpenCV returns for a 16-bit image: B first)"""

    def __init__(self, frs, fps=24.0):
        self.frs, self.i, self.fps, self.open = frs, 0, fps, True

    def get(self, prop):
        return {host_io.CAP_PROP_FPS: self.fps, host_io.CAP_PROP_FRAME_WIDTH: float(W), host_io.CAP_PROP_FRAME_HEIGHT: float(H)}[prop]

    def isOpened(self):
        return self.open

    def read(self):
        self.i += 1
        return (True, self.frs[self.i - 1]) if self.i <= len(self.frs) else (False, None)

    def release(self):
        self.open = False


class Sink:
    def __init__(self, fps, size):
        self.fps, self.size, self.got = fps, size, []

    def write(self, f):
        self.got.append(f.copy())

    def release(self):
        pass


def test_the_capture_front_ends_hand_a_deep_pixfmt_on():
    fmt = yuv.DeepRGB(H, W, 16, "bgr48")
    P = deep_video(fmt, CS.shot(3, H, W, seed=3, tone=120))
    sinks = []
    mk = lambda fps, size: sinks.append(Sink(fps, size)) or sinks[-1]
    info = mf.video_nx(Cap(P), mk, Mean(), factor=4, pixfmt=fmt, keep_depth=True)
    assert info["frames_in"] == 3 and info["frames_out"] == 9 and sinks[0].size == (W, H) and sinks[0].fps == 96
    want = expected_nx(P, fmt, 4)
    assert all(np.array_equal(g.reshape(-1), w.reshape(-1)) for g, w in zip(sinks[0].got, want))
    info = rt.video_retimed(Cap(P), mk, Mean(), 60, levels=3, pixfmt=fmt, keep_depth=True)
    direct = list(rt.interpolate_video_retimed(iter(P), Mean(), 24, 60, levels=3, pixfmt=fmt, keep_depth=True))
    assert info["frames_out"] == len(direct) == len(sinks[1].got) and all(np.array_equal(g.reshape(-1), w.reshape(-1)) for g, w in zip(sinks[1].got, direct))
    with pytest.raises(ValueError, match="keep_depth"):
        mf.video_nx(Cap(P), mk, Mean(), factor=2, pixfmt=fmt)


def test_refusals_name_their_argument():
    fmt = yuv.DeepRGB(H, W, 10, "gbrp")
    P = deep_video(fmt, CS.shot(2, H, W, seed=3, tone=120))
    nx = lambda **kw: list(mf.interpolate_video_nx(iter(P), Mean(), factor=2, pixfmt=fmt, **kw))
    re_ = lambda **kw: list(rt.interpolate_video_retimed(iter(P), Mean(), 24, 60, pixfmt=fmt, **kw))
    for run in (nx, re_):
        with pytest.raises(ValueError, match="keep_depth"):
            run()
        with pytest.raises(ValueError, match="keep_depth"):
            run(keep_depth=False)
        with pytest.raises(ValueError, match="active"):
            run(keep_depth=True, active=(0, 0, 16, 32))
        with pytest.raises(ValueError, match="active"):
            run(keep_depth=True, active=active.ActiveArea())
    with pytest.raises(ValueError, match="shutter"):
        re_(keep_depth=True, shutter=180)
    with pytest.raises(ValueError, match="shutter"):
        re_(keep_depth=True, shutter=shutter.Shutter(180))
    with pytest.raises(ValueError, match="interpolate_video_nx: a contiguous uint16 gbrp frame"):
        list(mf.interpolate_video_nx(iter([P[0], P[1].astype(np.uint8)]), Mean(), factor=2, pixfmt=fmt, keep_depth=True))
    # the stream front end: the same texts, and both ends are closed
    src = io.BytesIO(b"".join(p.tobytes() for p in P))
    for kw, word in ((dict(), "keep_depth"), (dict(keep_depth=True, active=(0, 0, 16, 32)), "active"),
                     (dict(keep_depth=True, fps_out=60, shutter=180), "shutter")):
        with pytest.raises(ValueError, match=word):
            yuv.interpolate_raw(src, io.BytesIO(), Mean(), fmt, 24, **kw)
    src.seek(0)
    dst = io.BytesIO()
    info = yuv.interpolate_raw(src, dst, Mean(), fmt, 24, factor=2, keep_depth=True)
    assert info["frames_in"] == 2 and info["frames_out"] == 3 and len(dst.getvalue()) == 3 * fmt.nbytes
    back = np.frombuffer(dst.getvalue(), "<u2").reshape(3, -1)
    assert np.array_equal(back[0], P[0].reshape(-1)) and np.array_equal(back[2], P[1].reshape(-1))
    assert np.array_equal(back[1], expected_nx(P, fmt, 2)[1])


def test_interp_raw_tool_refuses_before_it_needs_a_gpu(tmp_path):
    import subprocess
    import sys
    tool = os.path.join(CS.ROOT, "tools", "interp_raw.py")
    base = [sys.executable, tool, str(tmp_path / "in.rgb"), str(tmp_path / "out.rgb"), "--pix-fmt", "gbrp12le", "--size", "40x24", "--fps", "24"]
    for extra, word in (([], "keep_depth"), (["--keep-depth", "--active"], "active"),
                        (["--keep-depth", "--fps-out", "60", "--shutter", "180"], "shutter"), (["--keep-depth", "--pitch", "128"], "tight RGB")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)


# ------------------------------------------------------------------------------------------------ ABI
def test_rgb16_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    for name in ("atmvfi_rgb16_decode", "atmvfi_rgb16_encode"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert (lib.atmvfi_version() >> 8) & 255 >= 25
    mk = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert " rgb16.hip" in mk
    assert callable(hip_ops.HipOps.rgb16_decode) and callable(hip_ops.HipOps.rgb16_encode)
    P, Q, U = 0x10000, 0x4000000000, 0x5000000000     # never dereferenced: every call below fails its host-side checks before a launch
    err = lambda: lib.atmvfi_last_error().decode()

    def dec(src=P, H=16, W=16, depth=16, layout=0, y0=0, x0=0, h=16, w=16, dst=Q, Hp=16, Wp=16, pt=0, pl=0, u8=U):
        return lib.atmvfi_rgb16_decode(src, H, W, depth, layout, y0, x0, h, w, dst, Hp, Wp, pt, pl, u8, None)

    def enc(src=Q, Hp=16, Wp=16, pt=0, pl=0, dst=P, H=16, W=16, depth=16, layout=0):
        return lib.atmvfi_rgb16_encode(src, Hp, Wp, pt, pl, dst, H, W, depth, layout, None)
    for kw, msg in ((dict(src=None), "null source"), (dict(dst=None, u8=None), "both outputs are null"), (dict(depth=8), "depth must be 10, 12 or 16"),
                    (dict(depth=14), "depth must be"), (dict(layout=3), "unknown layout 3"), (dict(layout=-1), "unknown layout"),
                    (dict(H=0), "zero size"), (dict(w=0), "zero size"), (dict(y0=-1), "zero size"), (dict(y0=1), "outside the 16 x 16 frame"),
                    (dict(x0=8, w=9), "outside"), (dict(Hp=15), "Hp 15 < h 16"), (dict(Wp=16, pl=1), "Wp 16 < w 16 + pad_left 1"),
                    (dict(pt=-1), "bad canvas"), (dict(src=P + 1), "2-byte aligned"), (dict(dst=Q + 2), "4-byte aligned"),
                    (dict(H=1 << 20, W=1 << 20, h=1 << 20, w=1 << 20, Hp=1 << 20, Wp=1 << 20), "too large")):
        assert dec(**kw) == -1 and "rgb16_decode" in err() and msg in err(), (kw, err())
    for kw, msg in ((dict(src=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(depth=11), "depth must be 10, 12 or 16"),
                    (dict(layout=3), "unknown layout 3"), (dict(H=0), "bad geometry"), (dict(Hp=15), "bad geometry"), (dict(pl=1), "bad geometry"),
                    (dict(pt=-1), "bad geometry"), (dict(dst=P + 1), "2-byte aligned"), (dict(src=Q + 1), "4-byte aligned"),
                    (dict(H=1 << 20, W=1 << 20, Hp=1 << 20, Wp=1 << 20), "too large")):
        assert enc(**kw) == -1 and "rgb16_encode" in err() and msg in err(), (kw, err())
