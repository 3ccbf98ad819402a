"""CPU: planar YUV 4:2:0 (atm-vfi_amd/yuv.py; include/atmvfi.h atmvfi_yuv_decode / atmvfi_yuv_encode): the coefficient table,
the vectorised numpy twins against the per-pixel model of tests/cpu_yuv.py, closed forms and round trips, float64 and PIL yardsticks,
Y4M files, the loops with ``pixfmt=`` through the generic (no-GPU) path, and the ABI's host-side checks."""
import ctypes
import importlib
import io
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cpu_scene as CS
import cpu_yuv as C

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")
yuv = importlib.import_module("atm-vfi_amd.yuv")

COMBOS = list(itertools.product(("bt601", "bt709"), (False, True), ("centre", "left")))
SIZES = [(1, 1), (2, 2), (3, 5), (16, 16), (17, 31), (37, 53)]


# ------------------------------------------------------------------------------------------------ coefficients
def test_coefficients_are_the_table_and_the_float64_derivation():
    assert set(yuv.COEFFS) == {(m, f) for m in ("bt601", "bt709") for f in (False, True)}
    for (m, f), (dec, enc) in yuv.COEFFS.items():
        assert list(dec) == C.TABLE[m, int(f)][0] and [list(r) for r in enc] == C.TABLE[m, int(f)][1]
        # from (Kr, Kb), written out once more here
        kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[m]
        kg = 1 - kr - kb
        sy, sc = (1.0, 1.0) if f else (219 / 255, 224 / 255)
        want_dec = [1 / sy, 2 * (1 - kr) / sc, -2 * (1 - kb) * kb / kg / sc, -2 * (1 - kr) * kr / kg / sc, 2 * (1 - kb) / sc]
        want_enc = [[kr * sy, kg * sy, kb * sy], [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc],
                    [0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]]
        assert list(dec) == [int(np.rint(v * 16384)) for v in want_dec]
        assert [list(r) for r in enc] == [[int(np.rint(v * 16384)) for v in r] for r in want_enc]
        assert yuv.derive_coeffs(m, f) == (list(dec), [list(r) for r in enc])
        assert [sum(r) for r in enc] == [16384 if f else 14071, 0, 0]


def test_the_kernels_8_bit_table_is_the_derivation():
    """kCoeffs[2][2] of csrc/yuv_common.h, [matrix][full_range], read from the source: yuv.COEFFS and the float64 derivation."""
    src = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "yuv_common.h")).read()
    table = re.search(r"kCoeffs\[2\]\[2\]\s*=\s*\{(.*?)\n\};", src, flags=re.S).group(1)
    rows = [[int(v) for v in re.findall(r"-?\d+", line.split("//")[0])] for line in table.splitlines() if re.search(r"\{\{", line)]
    assert len(rows) == 4 and all(len(r) == 14 for r in rows)
    for k, (m, f) in enumerate(itertools.product(("bt601", "bt709"), (False, True))):
        dec, enc = yuv.COEFFS[m, f]
        assert rows[k] == list(dec) + [v for r in enc for v in r], (m, f, rows[k])
        assert (rows[k][:5], [rows[k][5 + 3 * i:8 + 3 * i] for i in range(3)]) == yuv.derive_coeffs(m, f), (m, f)


def test_format():
    f = yuv.Format(1080, 1920)
    assert f.matrix == "bt709" and yuv.Format(719, 1280).matrix == "bt601" and yuv.Format(720, 2, "bt601").matrix == "bt601"
    assert f.frame_bytes == 1080 * 1920 * 3 // 2 and yuv.Format(3, 5).frame_bytes == 15 + 2 * 6
    assert yuv.Format(3, 5, depth=10).frame_bytes == 2 * 27 and yuv.Format(3, 5, depth=10).as_8bit().frame_bytes == 27
    with pytest.raises(Exception):
        f.height = 2                                        # frozen
    assert f == yuv.Format(1080, 1920, "bt709") and hash(f) == hash(yuv.Format(1080, 1920, "bt709"))
    for bad in (dict(matrix="bt2020"), dict(siting="top"), dict(depth=12), dict(depth=10, full_range=True)):
        with pytest.raises(ValueError):
            yuv.Format(4, 4, **bad)
    with pytest.raises(ValueError):
        yuv.Format(0, 4)
    buf = np.arange(27, dtype=np.uint8)
    Y, U, V = yuv.Format(3, 5).planes(buf)
    assert Y.shape == (3, 5) and U.shape == V.shape == (2, 3) and Y.base is not None and U[0, 0] == 15 and V[1, 2] == 26
    Y[0, 0] = 99
    assert buf[0] == 99                                     # views
    with pytest.raises(ValueError):
        yuv.Format(3, 5).planes(buf[:-1])
    with pytest.raises(ValueError):
        yuv.Format(3, 5).planes(buf.astype(np.uint16))


# ------------------------------------------------------------------------------------------------ twins
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_numpy_twins_are_the_loop_model(H, W):
    for k, (m, f, s) in enumerate(COMBOS):
        fmt = yuv.Format(H, W, m, f, s)
        buf = C.random_frame(H, W, 8, seed=H * W + k)
        rgb = np.random.default_rng(k).integers(0, 256, (H, W, 3)).astype(np.uint8)
        for bgr in (False, True):
            assert np.array_equal(yuv.decode_numpy(buf, fmt, bgr=bgr), C.decode(buf, H, W, m, int(f), s, 8, bgr))
            got = yuv.encode_numpy(rgb, fmt, bgr=bgr)
            assert got.dtype == np.uint8 and got.shape == (fmt.frame_bytes,) and np.array_equal(got, C.encode(rgb, m, int(f), s, bgr))
        if not f:
            b10 = C.random_frame(H, W, 10, seed=H * W + k)
            assert np.array_equal(yuv.decode_numpy(b10, yuv.Format(H, W, m, f, s, 10)), C.decode(b10, H, W, m, 0, s, 10))
    with pytest.raises(ValueError):
        yuv.encode_numpy(np.zeros((H, W, 3), np.uint8), yuv.Format(H, W, depth=10))
    with pytest.raises(ValueError):
        yuv.encode_numpy(np.zeros((H + 1, W, 3), np.uint8), yuv.Format(H, W))


def _upsampled(buf, fmt):
    """the definition's integer chroma upsampling, through the twin: decode with an identity-like trick is not possible, so redo it"""
    Y, U, V = (p.astype(np.int64) for p in fmt.planes(buf))
    H, W = fmt.height, fmt.width
    ch, cw = fmt.chroma_shape
    out = []
    for c in (U, V):
        up = np.zeros((H, W), np.int64)
        for y in range(H):
            r0 = y >> 1
            r1 = min(max(r0 + (1 if y & 1 else -1), 0), ch - 1)
            for x in range(W):
                q0 = x >> 1
                if fmt.siting == "centre":
                    q1, w0, w1 = min(max(q0 + (1 if x & 1 else -1), 0), cw - 1), 3, 1
                else:
                    q1 = min(q0 + 1, cw - 1)
                    w0, w1 = (2, 2) if x & 1 else (4, 0)
                up[y, x] = (3 * (w0 * c[r0, q0] + w1 * c[r0, q1]) + (w0 * c[r1, q0] + w1 * c[r1, q1]) + 8) >> 4
        out.append(up)
    return Y, out[0], out[1]


def _float_matrices(m, f):
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[m]
    kg = 1 - kr - kb
    sy, sc = (1.0, 1.0) if f else (219 / 255, 224 / 255)
    dec = np.array([[1 / sy, 0, 2 * (1 - kr) / sc], [1 / sy, -2 * (1 - kb) * kb / kg / sc, -2 * (1 - kr) * kr / kg / sc],
                    [1 / sy, 2 * (1 - kb) / sc, 0]])
    enc = np.array([[kr * sy, kg * sy, kb * sy], [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc],
                    [0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]])
    return dec, enc


def test_against_the_float64_matrices():
    """Seeded uniform-random 37 x 53 data: the 14-bit integer matrices against the float64 ones with rint, on the same upsampled /
    summed chroma.  At most 1 level apart, in at most 1 % of the samples."""
    H, W = 37, 53
    for k, (m, f, s) in enumerate(COMBOS):
        dec, enc = _float_matrices(m, f)
        for depth in ((8,) if f else (8, 10)):
            fmt = yuv.Format(H, W, m, f, s, depth)
            buf = C.random_frame(H, W, depth, seed=k)
            Y, U, V = _upsampled(buf, fmt)
            scale, yo, mid = (4.0, 64, 512) if depth == 10 else (1.0, 0 if f else 16, 128)
            yuvf = np.stack([(Y - yo) / scale, (U - mid) / scale, (V - mid) / scale], -1)
            want = np.clip(np.rint(yuvf @ dec.T), 0, 255)
            d = np.abs(yuv.decode_numpy(buf, fmt).astype(np.int64) - want)
            print(f"decode {m} full={f} {s} depth {depth}: max {d.max():.0f}, differing {100 * (d > 0).mean():.3f} %")
            assert d.max() <= 1 and (d > 0).mean() <= 0.01
        fmt = yuv.Format(H, W, m, f, s)
        rgb = np.random.default_rng(50 + k).integers(0, 256, (H, W, 3)).astype(np.uint8)
        p = rgb.astype(np.float64)
        ch, cw = fmt.chroma_shape
        ra, ca = 2 * np.arange(ch), 2 * np.arange(cw)
        rows = p[ra] + p[np.minimum(ra + 1, H - 1)]
        if s == "left":
            mean = (rows[:, np.maximum(ca - 1, 0)] + 2 * rows[:, ca] + rows[:, np.minimum(ca + 1, W - 1)]) / 8
        else:
            mean = (rows[:, ca] + rows[:, np.minimum(ca + 1, W - 1)]) / 4
        wy = np.clip(np.rint(p @ enc[0] + (0 if f else 16)), 0, 255)
        wu = np.clip(np.rint(mean @ enc[1] + 128), 0, 255)
        wv = np.clip(np.rint(mean @ enc[2] + 128), 0, 255)
        want = np.concatenate([wy.reshape(-1), wu.reshape(-1), wv.reshape(-1)])
        d = np.abs(yuv.encode_numpy(rgb, fmt).astype(np.int64) - want)
        print(f"encode {m} full={f} {s}: max {d.max():.0f}, differing {100 * (d > 0).mean():.3f} %")
        assert d.max() <= 1 and (d > 0).mean() <= 0.01


def test_grey_ramp():
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 4, 0).repeat(3, 2)          # [4,256,3]
    for m, f, s in COMBOS:
        fmt = yuv.Format(4, 256, m, f, s)
        enc = yuv.encode_numpy(ramp, fmt)
        Y, U, V = fmt.planes(enc)
        assert (U == 128).all() and (V == 128).all()
        flat = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None, None], 4, 1).repeat(4, 2).repeat(3, 3)      # 256 flat 4x4 greys
        for g in range(256):
            fm = yuv.Format(4, 4, m, f, s)
            back = yuv.decode_numpy(yuv.encode_numpy(flat[g], fm), fm).astype(int)
            assert np.abs(back - g).max() <= (0 if f else 1), (m, f, s, g)


def test_flat_colours_round_trip():
    rng = np.random.default_rng(2024)
    cols = rng.integers(0, 256, (200, 3)).astype(np.uint8)
    for m, f, s in COMBOS:
        fm = yuv.Format(4, 6, m, f, s)
        worst = 0
        for c in cols:
            img = np.broadcast_to(c, (4, 6, 3)).copy()
            back = yuv.decode_numpy(yuv.encode_numpy(img, fm), fm).astype(int)
            worst = max(worst, np.abs(back - c.astype(int)).max())
        assert worst <= (1 if f else 2), (m, f, s, worst)


def test_full_range_bt601_against_pil():
    from PIL import Image
    rng = np.random.default_rng(9)
    blocks = rng.integers(0, 256, (12, 20, 3)).astype(np.uint8)
    img = blocks.repeat(2, 0).repeat(2, 1)                                                       # every 2 x 2 block is flat
    ref = np.asarray(Image.fromarray(img, "RGB").convert("YCbCr")).astype(int)
    for s in ("centre",):
        fmt = yuv.Format(24, 40, "bt601", True, s)
        Y, U, V = (p.astype(int) for p in fmt.planes(yuv.encode_numpy(img, fmt)))
        d = max(np.abs(Y - ref[:, :, 0]).max(), np.abs(U - ref[::2, ::2, 1]).max(), np.abs(V - ref[::2, ::2, 2]).max())
        assert d <= 1, d


def test_crop():
    fmt = yuv.Format(10, 14)
    buf = C.random_frame(10, 14, seed=1)
    Y, U, V = fmt.planes(buf)
    got = yuv.crop(buf, fmt, 2, 4, 5, 7)
    cy, cu, cv = fmt.cropped(5, 7).planes(got)
    assert np.array_equal(cy, Y[2:7, 4:11]) and np.array_equal(cu, U[1:4, 2:6]) and np.array_equal(cv, V[1:4, 2:6])
    assert np.array_equal(yuv.crop(buf, fmt, 0, 0, 10, 14), buf)
    for y0, x0 in ((1, 0), (0, 3)):
        with pytest.raises(ValueError, match="even"):
            yuv.crop(buf, fmt, y0, x0, 4, 4)
    with pytest.raises(ValueError):
        yuv.crop(buf, fmt, 8, 0, 4, 4)


# ------------------------------------------------------------------------------------------------ Y4M
@pytest.mark.parametrize("H,W,kw,rate", [(24, 40, {}, Fraction(25)), (5, 7, dict(siting="left"), Fraction(30000, 1001)),
                                         (6, 10, dict(full_range=True), Fraction(24000, 1001)), (7, 9, dict(depth=10), Fraction(60))])
def test_y4m_write_then_read_is_identical(tmp_path, H, W, kw, rate):
    fmt = yuv.Format(H, W, **kw)
    frames = [C.random_frame(H, W, fmt.depth, seed=k) for k in range(3)]
    path = tmp_path / "a.y4m"
    with yuv.Y4MWriter(path, fmt, rate) as wr:
        for f in frames:
            wr.write(f)
    with yuv.Y4MReader(path) as rd:
        assert rd.fmt == fmt and rd.fps == rate and isinstance(rd.fps, Fraction) and len(rd) == 3
        got = list(rd)
    assert len(got) == 3 and all(g.dtype == fmt.dtype and g.ndim == 1 and np.array_equal(g, f) for g, f in zip(got, frames))
    # ... and the bytes: rewriting what was read gives the same file
    with yuv.Y4MReader(path) as rd, yuv.Y4MWriter(tmp_path / "b.y4m", rd.fmt, rd.fps, ctag=rd.ctag, aspect=rd.aspect) as wr:
        for f in rd:
            wr.write(f)
    assert (tmp_path / "a.y4m").read_bytes() == (tmp_path / "b.y4m").read_bytes()
    with pytest.raises(ValueError):
        yuv.Y4MWriter(io.BytesIO(), fmt, rate).write(frames[0][:-1])


def _stream(header, n, fmt_bytes):
    return io.BytesIO(header + b"\n" + b"".join(b"FRAME\n" + bytes(fmt_bytes) for _ in range(n)))


def test_y4m_headers():
    for tag, siting, depth in (("C420", "centre", 8), ("C420jpeg", "centre", 8), ("C420mpeg2", "left", 8), ("C420p10", "centre", 10), (None, "centre", 8)):
        nb = (8 * 6 + 2 * 12) * (2 if depth == 10 else 1)
        head = b"YUV4MPEG2 W6 H8 F30000:1001 Ip A1:1" + (b" " + tag.encode() if tag else b"") + b" XYSCSS=420JPEG"
        rd = yuv.Y4MReader(_stream(head, 2, nb))
        assert rd.fmt == yuv.Format(8, 6, "bt601", False, siting, depth) and rd.fps == Fraction(30000, 1001) and len(rd) == 2
        assert [f.dtype for f in rd] == [rd.fmt.dtype] * 2
    rd = yuv.Y4MReader(_stream(b"YUV4MPEG2 W2 H720 F25:1 C420jpeg XCOLORRANGE=FULL", 1, 720 * 2 + 2 * 360))
    assert rd.fmt == yuv.Format(720, 2, "bt709", True) and rd.fps == 25
    for tag in ("C420paldv", "C422", "C444", "Cmono", "C444p10", "C422p10", "C420p12"):
        with pytest.raises(ValueError, match=tag):
            yuv.Y4MReader(_stream(b"YUV4MPEG2 W6 H8 F25:1 Ip " + tag.encode(), 1, 72))
    for tag in ("It", "Ib", "Im"):
        with pytest.raises(ValueError, match=tag):
            yuv.Y4MReader(_stream(b"YUV4MPEG2 W6 H8 F25:1 " + tag.encode() + b" C420", 1, 72))
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        yuv.Y4MReader(io.BytesIO(b"RIFF....\n"))
    # a truncated last frame
    data = _stream(b"YUV4MPEG2 W6 H8 F25:1 Ip C420", 2, 72).getvalue()
    rd = yuv.Y4MReader(io.BytesIO(data[:-5]))
    with pytest.raises(ValueError, match="truncated"):
        list(rd)
    # FRAME lines may carry parameters
    rd = yuv.Y4MReader(io.BytesIO(b"YUV4MPEG2 W2 H2 F25:1\nFRAME Ip\n" + bytes(range(6))))
    assert [list(f) for f in rd] == [[0, 1, 2, 3, 4, 5]]


# ------------------------------------------------------------------------------------------------ the loops, generic path
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend (tests/test_scene_cpu.py's stand-in): the pair mean."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.pairs = 0

    def forward(self, a, b):
        self.pairs += a.shape[0]
        return {"I_t": (a + b) / 2}


H, W = 24, 40
FMT = yuv.Format(H, W, "bt709", False, "left")
SHOT_A = [yuv.encode_numpy(f, FMT) for f in CS.shot(5, H, W, seed=1, tone=60)]
SHOT_B = [yuv.encode_numpy(f, FMT) for f in CS.shot(5, H, W, seed=2, tone=190)]


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("kw", [dict(), dict(time_interval=2), dict(crop=(16, 32)), dict(tta=True), dict(time_interval=2, crop=(16, 32), tta=True)],
                         ids=lambda k: "-".join(k) or "plain")
def test_loops_with_pixfmt_through_the_generic_path(factor, kw):
    video = SHOT_A + SHOT_B
    keep = [v.copy() for v in video]
    y0, x0, h, w = mf.centre_window(H, W, kw.get("crop"))
    out_fmt = FMT.cropped(h, w)
    s = kw.get("time_interval", 1)
    for sc_yuv, sc_rgb in ((None, None), (scene.SceneCuts(), scene.SceneCuts())):
        model = Mean()
        got = list(mf.interpolate_video_nx(iter(video), model, factor=factor, pixfmt=FMT, scene=sc_yuv, isBGR=True, **kw))
        rgb_model = Mean()
        want = list(mf.interpolate_video_nx(iter([yuv.decode_numpy(v, FMT) for v in video]), rgb_model, factor=factor, isBGR=False,
                                            scene=sc_rgb, **kw))
        assert len(got) == len(want) == factor * ((len(video) - 1) // s) + 1 and model.pairs == rgb_model.pairs
        cut = set() if sc_yuv is None else set(sc_yuv.cuts)
        if sc_yuv is not None:
            assert sc_yuv.cuts == sc_rgb.cuts == [(len(SHOT_A) - 1) // s] and sc_yuv.stats == sc_rgb.stats
        for k, (g, wnt) in enumerate(zip(got, want)):
            assert g.dtype == np.uint8 and g.shape == (out_fmt.frame_bytes,)
            seg, pos = divmod(k, factor)
            if pos == 0:                                 # an original: the caller's bytes (its planes' crop), no colour round trip
                src = video[seg * s]
                assert np.array_equal(g, yuv.crop(src, FMT, y0, x0, h, w))
                if kw.get("crop") is None:
                    assert g is src
            elif seg in cut:                             # a cut copy: a copy of the nearer original's bytes
                src = video[seg * s] if pos <= factor // 2 else video[(seg + 1) * s]
                assert np.array_equal(g, yuv.crop(src, FMT, y0, x0, h, w)) and g is not src
            else:                                        # a produced frame: the RGB loop's frame, encoded
                assert np.array_equal(g, yuv.encode_numpy(wnt, out_fmt))
    assert all(np.array_equal(a, b) for a, b in zip(video, keep))        # the caller's buffers are untouched


def test_loops_with_pixfmt_refuse_an_odd_crop_origin_and_wrong_frames():
    with pytest.raises(ValueError, match="even"):
        list(mf.interpolate_video_nx(iter(SHOT_A), Mean(), factor=2, pixfmt=FMT, crop=(18, 32)))            # rows 3 .. 21
    with pytest.raises(ValueError, match="even"):
        list(mf.interpolate_video_nx(iter(SHOT_A), Mean(), factor=2, pixfmt=FMT, crop=(16, 30)))            # columns 5 .. 35
    with pytest.raises(ValueError):
        list(mf.interpolate_video_nx(iter([f[:-1] for f in SHOT_A]), Mean(), factor=2, pixfmt=FMT))
    import inspect
    for fn in (host_io.interpolate_video_2x, host_io.interpolate_video_nx, host_io.FramePipeline.__init__):
        assert inspect.signature(fn).parameters["pixfmt"].default is None


def test_ten_bit_input_through_the_generic_path():
    fmt = yuv.Format(H, W, depth=10)
    video = [(f.astype(np.uint16) << 2) for f in SHOT_A[:3]]
    got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=2, pixfmt=fmt))
    want = list(mf.interpolate_video_nx(iter([yuv.decode_numpy(v, fmt) for v in video]), Mean(), factor=2, isBGR=False))
    assert got[0] is video[0] and got[2] is video[1] and got[4] is video[2]
    for k in (1, 3):
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], yuv.encode_numpy(want[k], fmt.as_8bit()))


@pytest.mark.parametrize("factor,kw", [(2, {}), (4, {}), (2, dict(crop=(16, 32))), (4, dict(time_interval=2))])
def test_interpolate_y4m(tmp_path, factor, kw):
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    n = 5
    with yuv.Y4MWriter(src, FMT, Fraction(30000, 1001), aspect="1:1") as wr:
        for f in SHOT_A[:n]:
            wr.write(f)
    sc = scene.SceneCuts()
    info = yuv.interpolate_y4m(src, dst, Mean(), factor=factor, scene=sc, matrix="bt709", **kw)
    s = kw.get("time_interval", 1)
    _, _, h, w = mf.centre_window(H, W, kw.get("crop"))
    n_out = factor * ((n - 1) // s) + 1
    assert info == {"fps_in": Fraction(30000, 1001), "fps_out": Fraction(30000, 1001) * factor / s, "size": (w, h), "frames_in": n,
                    "frames_out": n_out, "cuts": []}
    with yuv.Y4MReader(dst, matrix="bt709") as rd:
        assert rd.fmt == FMT.cropped(h, w) and rd.fps == Fraction(30000 * factor, 1001 * s) and rd.ctag == "420mpeg2" and rd.aspect == "1:1"
        got = list(rd)
    want = list(mf.interpolate_video_nx(iter(SHOT_A[:n]), Mean(), factor=factor, pixfmt=FMT, **kw))
    assert len(got) == len(want) == n_out and all(np.array_equal(g, w_) for g, w_ in zip(got, want))
    if s == 1 and not kw:
        assert factor * (n - 1) + 1 == n_out


def test_interpolate_y4m_writes_ten_bit_input_back_as_eight_bit(tmp_path):
    fmt = yuv.Format(H, W, depth=10)
    video = [(f.astype(np.uint16) << 2) for f in SHOT_A[:3]]
    src, dst = io.BytesIO(), io.BytesIO()
    wr = yuv.Y4MWriter(src, fmt, 24)
    for f in video:
        wr.write(f)
    src.seek(0)
    info = yuv.interpolate_y4m(src, dst, Mean(), factor=2)
    assert info["frames_out"] == 5 and info["fps_out"] == 48
    dst.seek(0)
    rd = yuv.Y4MReader(dst)
    got = list(rd)
    assert rd.fmt == fmt.as_8bit() and rd.ctag == "420jpeg" and len(got) == 5
    assert np.array_equal(got[0], yuv.to_8bit(video[0], fmt)) and got[0].dtype == np.uint8


@pytest.mark.parametrize("kw", [{}, dict(fps_out=50)], ids=["factor", "fps_out"])
def test_interpolate_y4m_releases_its_reader_when_the_crop_is_refused(tmp_path, monkeypatch, kw):
    """A refusal between opening the reader and opening the writer leaves no handle of the source open, and no output file."""
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with yuv.Y4MWriter(src, FMT, 25) as wr:
        wr.write(SHOT_A[0])
    opened = []

    def tracking_open(*a, **k):
        opened.append(open(*a, **k))
        return opened[-1]
    monkeypatch.setattr(yuv, "open", tracking_open, raising=False)
    with pytest.raises(ValueError, match="does not fit"):
        yuv.interpolate_y4m(src, dst, Mean(), crop=(H + 2, W), **kw)
    assert len(opened) == 1 and str(opened[0].name) == str(src) and opened[0].closed and not dst.exists()


# ------------------------------------------------------------------------------------------------ ABI
def test_yuv_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    for name in ("atmvfi_yuv_decode", "atmvfi_yuv_encode"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
        assert lib.atmvfi_plan_fn_id(name.encode()) >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 29
    mk = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert " yuv.hip" in mk and " yuv_encode.hip" in mk
    assert callable(hip_ops.HipOps.yuv420_to_rgb) and callable(hip_ops.HipOps.rgb_to_yuv420)
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error

    def dec(yuv_=P, H=64, W=96, depth=8, matrix=0, full=0, siting=0, d8=P, bgr=0, dst=P, Hp=64, Wp=96, pt=0, pl=0):
        d = hip_ops.YuvDesc(H=H, W=W, depth=depth, matrix=matrix, full_range=full, siting=siting)     # the whole frame of a packed planar format
        rc = lib.atmvfi_yuv_decode(ctypes.byref(d), yuv_, 0, 0, 0, 0, H, W, d8, bgr, dst, Hp, Wp, pt, pl, None)
        assert rc == -1 and err().startswith(b"yuv_decode: ")           # the shared checks, under the entry point's own name
        return rc

    def enc(s8=P, bgr=0, src=None, Hp=64, Wp=96, pt=0, pl=0, H=64, W=96, matrix=0, full=0, siting=0, yuv_=P):
        d = hip_ops.YuvDesc(H=H, W=W, depth=8, matrix=matrix, full_range=full, siting=siting)
        rc = lib.atmvfi_yuv_encode(ctypes.byref(d), s8, bgr, src, Hp, Wp, pt, pl, yuv_, None)
        assert rc == -1 and err().startswith(b"yuv_encode: ")
        return rc
    assert dec(yuv_=None) == -1 and b"null source" in err()
    assert dec(d8=None, dst=None) == -1 and b"both outputs are null" in err()
    assert dec(H=0) == -1 and b"at least 1" in err()
    assert dec(W=0) == -1 and b"at least 1" in err()
    assert dec(depth=12) == -1 and b"depth must be 8 or 10" in err()
    assert dec(depth=10, full=1) == -1 and b"10-bit full range" in err()
    assert dec(matrix=2) == -1 and b"unknown matrix" in err()
    assert dec(siting=2) == -1 and b"unknown siting" in err()
    assert dec(Hp=63) == -1 and b"smaller than the window" in err()     # (one decode entry point: the whole frame is a window too)
    assert dec(pl=1) == -1 and b"smaller than the window" in err()
    assert dec(pt=-1) == -1 and b"smaller than the window" in err()
    assert dec(dst=P + 2) == -1 and b"4-byte aligned" in err()
    assert dec(H=100000, W=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()        # 1.25e9 work items
    assert dec(full=2) == -1 and b"full_range" in err()                                         # (asserted for its siblings before)
    assert dec(d8=None, dst=P + 2) == -1 and b"4-byte aligned" in err()
    assert enc(yuv_=None) == -1 and b"null destination" in err()
    assert enc(s8=None, src=None) == -1 and b"exactly one" in err() and b"neither" in err()
    assert enc(s8=P, src=P) == -1 and b"exactly one" in err() and b"both" in err()
    assert enc(H=0) == -1 and b"at least 1" in err()
    assert enc(H=100000, W=100000) == -1 and b"too large" in err()
    assert enc(matrix=-1) == -1 and b"unknown matrix" in err()
    assert enc(siting=3) == -1 and b"unknown siting" in err()
    assert enc(full=2) == -1 and b"full_range" in err()
    assert enc(s8=None, src=P, Wp=95) == -1 and b"smaller than the frame" in err()
    assert enc(s8=None, src=P, pt=1) == -1 and b"smaller than the frame" in err()
    assert enc(s8=None, src=P + 1) == -1 and b"4-byte aligned" in err()
    assert enc(W=0) == -1 and b"at least 1" in err()
    assert enc(s8=None, src=P, pl=-4) == -1 and b"smaller than the frame" in err()
    assert enc(s8=None, src=P, H=100000, W=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()


def test_the_kernels_multiply_add_form_of_q_over_255_is_the_fp32_division():
    """csrc/yuv_common.h writes q / 255 as y = fl(q r), fl(y + fl(q - 255 y) r) with r = fl(1 / 255) and fused multiply-adds (one rounding
    each).  In exact rational arithmetic, for every q in 0..255: the bits of the fp32 division (what frame_u8_to_f32 computes)."""
    from fractions import Fraction as Fr

    def fl(x):
        """the float32 nearest to the rational x, ties to even"""
        c = np.float32(float(x))
        best = None
        for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
            d = abs(Fr(float(cand)) - x)
            if best is None or d < best[0] or (d == best[0] and not (int(cand.view(np.uint32)) & 1)):
                best = (d, cand)
        return best[1]
    r = fl(Fr(1, 255))
    assert float(r).hex() == "0x1.0101020000000p-8"             # the kernel's constant
    plain = 0
    for q in range(256):
        want = np.float32(q) / np.float32(255)
        assert want.view(np.uint32) == fl(Fr(q, 255)).view(np.uint32)
        y = fl(q * Fr(float(r)))
        e = fl(q - 255 * Fr(float(y)))
        got = fl(Fr(float(y)) + Fr(float(e)) * Fr(float(r)))
        assert got.view(np.uint32) == want.view(np.uint32), q
        plain += int(y.view(np.uint32) != want.view(np.uint32))
    assert plain > 0                                            # the bare product is not enough: the correction step is needed
