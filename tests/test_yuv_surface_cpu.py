"""``yuv.Surface`` on the host: the numpy twins against the per-sample loop model (tests/cpu_yuv_surface.py), ``repack``, the
refusals, the raw reader / writer, the loops through the numpy path and the two new ABI calls' host-side checks.  No GPU."""
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
import cpu_yuv_surface as M

mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")

SIZES = [(1, 1), (2, 2), (3, 5), (8, 16), (6, 18)]
KINDS = {"8": (8, False), "10": (10, False), "10msb": (10, True)}
WINDOWS = {(1, 1): [], (2, 2): [(0, 0, 1, 1)], (3, 5): [(2, 2, 1, 3), (0, 2, 3, 3)], (8, 16): [(2, 2, 5, 13), (4, 0, 3, 15)],
           (6, 18): [(2, 4, 3, 11), (0, 2, 5, 15)]}


def surfaces(H, W, chroma, depth, msb, **fkw):
    """tight; padded with a pitch that is no multiple of 4 and a chroma offset beyond pitch * H; padded with multiples of 4"""
    fmt = yuv.Format(H, W, depth=depth, **fkw)
    b, cw = (2 if depth == 10 else 1), (W + 1) // 2
    crow = (cw if chroma == "planar" else 2 * cw) * b
    odd = lambda n: next(p for p in range(n + b, n + 16, b) if p % 4)
    mul4 = lambda n: (n + 11) // 4 * 4
    return [yuv.Surface(fmt, chroma, msb),
            yuv.Surface(fmt, chroma, msb, pitch=odd(W * b), chroma_pitch=odd(crow), chroma_offset=odd(W * b) * H + 3 * b),
            yuv.Surface(fmt, chroma, msb, pitch=mul4(W * b), chroma_pitch=mul4(crow), chroma_offset=mul4(W * b) * H + 8)]


def model_layout(s):
    L = M.layout(s.height, s.width, s.depth, s.chroma, s.msb, s.pitch, s.chroma_pitch, s.chroma_offset)
    assert L["nbytes"] == s.nbytes and s.frame_samples * s.itemsize == s.nbytes
    return L


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ twins == loop model
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("chroma", yuv.CHROMAS)
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_numpy_twins_are_the_loop_model(H, W, chroma, kind):
    depth, msb = KINDS[kind]
    combos = list(itertools.product(("bt601", "bt709"), ("centre", "left"), (False, True) if depth == 8 else (False,)))
    for k, (matrix, siting, full) in enumerate(combos):
        for n, s in enumerate(surfaces(H, W, chroma, depth, msb, matrix=matrix, siting=siting, full_range=full)):
            L = model_layout(s)
            assert s.is_tight == (n == 0) and s.tight() == surfaces(H, W, chroma, depth, msb, matrix=matrix, siting=siting, full_range=full)[0]
            buf = M.random_surface(L, seed=100 * k + n)
            kw = dict(matrix=matrix, full_range=int(full), siting=siting)
            want = M.decode(buf, L, **kw)
            assert np.array_equal(yuv.decode_numpy(buf, s), want.astype(np.uint8))
            assert np.array_equal(yuv.decode_numpy(buf, s, bgr=True), want[:, :, ::-1].astype(np.uint8))
            for win in WINDOWS[H, W]:
                assert np.array_equal(yuv.window_numpy(buf, s, 0, *win), M.decode(buf, L, window=win, **kw).astype(np.uint8)), win
            if depth == 10:
                for win in [None] + WINDOWS[H, W]:
                    want10 = M.decode(buf, L, window=win, keep=True, **kw).astype(np.float32) / np.float32(1023)
                    assert same_bits(yuv.decode_numpy_f32(buf, s, window=win), want10), win
            if msb:         # the low six bits of a stored sample do not matter
                clean = (buf & np.uint16(0xffc0)).astype(np.uint16)
                assert np.array_equal(yuv.decode_numpy(clean, s), yuv.decode_numpy(buf, s))
                assert same_bits(yuv.decode_numpy_f32(clean, s), yuv.decode_numpy_f32(buf, s))
            if n == 0:      # encodes write tight surfaces
                rng = np.random.default_rng(7 * k + 1)
                if depth == 8:
                    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
                    got = yuv.encode_numpy(rgb, s)
                    assert np.array_equal(yuv.encode_numpy(np.ascontiguousarray(rgb[:, :, ::-1]), s, bgr=True), got)
                else:
                    rgb = rng.uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32)
                    got = yuv.encode_numpy(rgb, s)
                assert got.dtype == s.dtype and got.shape == (s.frame_samples,)
                assert np.array_equal(got.astype("<u2" if depth == 10 else np.uint8).view(np.uint8), M.encode(M.pixels(rgb, depth), L, **kw))
            else:
                with pytest.raises(ValueError, match="tight"):
                    yuv.encode_numpy(np.zeros((H, W, 3), np.uint8 if depth == 8 else np.float32), s)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_repack_moves_samples_between_layouts(H, W, kind):
    depth, msb = KINDS[kind]
    fmt = yuv.Format(H, W, depth=depth, siting="left")
    rng = np.random.default_rng(H * 100 + W)
    f = rng.integers(0, 1024 if depth == 10 else 256, fmt.frame_samples).astype(fmt.dtype)
    assert np.array_equal(yuv.repack(f, fmt, yuv.Surface.i420(H, W, depth=depth, siting="left")), f)       # the same bytes
    rgb = yuv.decode_numpy(f, fmt)
    src = rgb if depth == 8 else rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    for chroma in yuv.CHROMAS:
        for s in surfaces(H, W, chroma, depth, msb, siting="left"):
            g = yuv.repack(f, fmt, s)
            assert g.dtype == s.dtype and g.shape == (s.frame_samples,)
            assert np.array_equal(yuv.repack(g, s, fmt), f)                                     # there and back
            assert np.array_equal(yuv.repack(yuv.repack(g, s, s.tight()), s.tight(), s), g)
            if msb:
                assert not (g & 63).any()                                                       # the low bits are written as zero
            assert np.array_equal(yuv.decode_numpy(g, s), rgb)
            if depth == 10:
                assert same_bits(yuv.decode_numpy_f32(g, s), yuv.decode_numpy_f32(f, fmt))
            assert np.array_equal(yuv.encode_numpy(src, s.tight()), yuv.repack(yuv.encode_numpy(src, fmt), fmt, s.tight()))
            assert np.array_equal(yuv.crop(g, s, 0, 0, H, W), yuv.repack(f, fmt, s.tight()))
            for y0, x0, h, w in WINDOWS[H, W]:
                assert np.array_equal(yuv.crop(g, s, y0, x0, h, w), yuv.repack(yuv.crop(f, fmt, y0, x0, h, w), fmt.cropped(h, w), s.cropped(h, w)))
            assert np.array_equal(yuv.to_8bit(g, s), g if depth == 8 else yuv.repack(yuv.to_8bit(f, fmt), fmt.as_8bit(), s.as_8bit()))
    with pytest.raises(ValueError, match="size or depth"):
        yuv.repack(f, fmt, yuv.Surface.nv12(H + 2, W))
    with pytest.raises(ValueError, match="size or depth"):
        yuv.repack(f, fmt, yuv.Surface(yuv.Format(H, W, depth=18 - depth), "uv"))


def test_constructors_and_sizes():
    s = yuv.Surface.nv12(1080, 1920, pitch=2048)
    assert (s.chroma, s.msb, s.depth, s.pitch, s.chroma_pitch, s.chroma_offset) == ("uv", False, 8, 2048, 2048, 2048 * 1080)
    assert s.nbytes == 2048 * 1080 + 2048 * 539 + 1920 and not s.is_tight and s.matrix == "bt709"
    assert s.tight() == yuv.Surface.nv12(1080, 1920) and s.tight().nbytes == 1080 * 1920 * 3 // 2
    assert s.cropped(720, 1280) == yuv.Surface.nv12(720, 1280, matrix="bt709")
    p = yuv.Surface.p010(1080, 1920, pitch=4096, chroma_offset=4096 * 1088, siting="left")
    assert (p.chroma, p.msb, p.depth, p.dtype, p.siting) == ("uv", True, 10, np.uint16, "left")
    assert p.nbytes == 4096 * 1088 + 4096 * 539 + 3840 and p.frame_samples == p.nbytes // 2
    assert p.as_8bit() == yuv.Surface.nv12(1080, 1920, siting="left") and p.tight().is_tight
    i = yuv.Surface.i420(5, 7)
    assert i.is_tight and i.nbytes == yuv.Format(5, 7).frame_bytes and i.fmt == yuv.Format(5, 7)
    assert yuv.Surface.i420(4, 8, pitch=16).chroma_pitch == 8
    assert yuv.Surface(yuv.Format(3, 5), "vu").nbytes == 15 + 2 * 6
    assert yuv.surface_of("p010le", 4, 6, pitch=16) == yuv.Surface.p010(4, 6, pitch=16)
    assert yuv.surface_of("nv21", 4, 6) == yuv.Surface(yuv.Format(4, 6), "vu")


def test_surface_refusals():
    f8, f10 = yuv.Format(4, 6), yuv.Format(4, 6, depth=10)
    with pytest.raises(ValueError, match="msb needs depth 10"):
        yuv.Surface(f8, "uv", msb=True)
    with pytest.raises(ValueError, match="at least a luma row"):
        yuv.Surface(f8, "uv", pitch=5)
    with pytest.raises(ValueError, match="at least a chroma row"):
        yuv.Surface(f8, "uv", chroma_pitch=5)                 # an interleaved row holds 2 cw samples
    with pytest.raises(ValueError, match="multiple of the sample size"):
        yuv.Surface(f10, "uv", msb=True, pitch=13)
    with pytest.raises(ValueError, match="multiple of the sample size"):
        yuv.Surface(f10, "planar", chroma_pitch=7)
    with pytest.raises(ValueError, match="at least pitch"):
        yuv.Surface(f8, "uv", pitch=8, chroma_offset=31)      # inside the luma plane
    with pytest.raises(ValueError, match="multiple of the sample size"):
        yuv.Surface(f10, "uv", chroma_offset=49)
    with pytest.raises(ValueError, match="unknown chroma"):
        yuv.Surface(f8, "nv12")
    with pytest.raises(ValueError, match="yuv.Format"):
        yuv.Surface((4, 6))
    s = yuv.Surface.nv12(4, 6, pitch=8)
    good = np.zeros(s.frame_samples, np.uint8)
    assert s.check(good) is not None
    for bad in (np.zeros(s.frame_samples + 1, np.uint8), np.zeros(s.frame_samples, np.uint16), np.zeros(s.tight().frame_samples, np.uint8),
                np.zeros(2 * s.frame_samples, np.uint8)[::2]):
        with pytest.raises(ValueError, match="expected"):
            yuv.decode_numpy(bad, s)
    with pytest.raises(ValueError, match="must be even"):
        yuv.crop(good, s, 1, 0, 2, 2)
    with pytest.raises(ValueError, match="outside"):
        yuv.crop(good, s, 2, 2, 4, 4)


# ------------------------------------------------------------------------------------------------ raw streams
class Dribble(io.RawIOBase):
    """A pipe that delivers at most ``n`` bytes per read and cannot seek."""

    def __init__(self, data, n):
        self.data, self.n, self.pos = data, n, 0

    def readable(self):
        return True

    def seekable(self):
        return False

    def read(self, size=-1):
        k = self.n if size is None or size < 0 else min(size, self.n)
        out = self.data[self.pos:self.pos + k]
        self.pos += len(out)
        return out


@pytest.mark.parametrize("s", [yuv.Surface.nv12(6, 10, pitch=12), yuv.Surface.p010(6, 10), yuv.Format(6, 10)], ids=["nv12p", "p010", "i420"])
def test_raw_reader_and_writer(s, tmp_path):
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 1024 if s.depth == 10 else 256, s.frame_samples).astype(s.dtype) for _ in range(5)]
    path = str(tmp_path / "clip.raw")
    with yuv.RawWriter(path, s) as wr:
        for f in frames:
            wr.write(f)
        assert wr.frames == 5
        with pytest.raises(ValueError, match="expected"):
            wr.write(frames[0][:-1])
    assert os.path.getsize(path) == 5 * s.frame_bytes
    with yuv.RawReader(path, s, "30000/1001") as rd:
        assert len(rd) == 5 and str(rd.fps) == "30000/1001" and rd.surface is s
        got = list(rd)
    assert len(got) == 5 and all(g.dtype == s.dtype and np.array_equal(g, f) for g, f in zip(got, frames))
    data = open(path, "rb").read()
    with yuv.RawReader(path, s, 25) as rd:                      # skip, seekable
        assert rd.skip(2) == 2 and np.array_equal(next(iter(rd)), frames[2]) and rd.skip(7) == 2
    rd = yuv.RawReader(Dribble(data, 7), s, 25)                 # a short-reading pipe: the same frames, no length
    with pytest.raises(TypeError):
        len(rd)
    assert rd.skip(1) == 1
    got = list(rd)
    assert len(got) == 4 and all(np.array_equal(g, f) for g, f in zip(got, frames[1:]))
    assert yuv.RawReader(Dribble(data, 7), s, 25).skip(9) == 5
    for src in (io.BytesIO(data[:-3]), Dribble(data[:-3], 11)):          # a truncated last frame
        it = iter(yuv.RawReader(src, s, 25))
        assert all(np.array_equal(next(it), f) for f in frames[:4])
        with pytest.raises(ValueError, match="truncated frame"):
            next(it)
    for src in (io.BytesIO(data[:-3]), Dribble(data[:-3], 11)):
        with pytest.raises(ValueError, match="truncated frame"):
            yuv.RawReader(src, s, 25).skip(5)
    out = io.BytesIO()
    wr = yuv.RawWriter(out, s)
    wr.write(frames[1])
    wr.close()
    assert out.getvalue() == data[s.frame_bytes:2 * s.frame_bytes]


# ------------------------------------------------------------------------------------------------ the loops, numpy path
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend (tests/test_yuv_cpu.py's stand-in): the pair mean."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, a, b):
        return {"I_t": (a + b) / 2}


H, W = 24, 40
FMT8, FMT10 = yuv.Format(H, W, "bt709", False, "left"), yuv.Format(H, W, "bt709", False, "left", 10)
RGB = CS.shot(3, H, W, seed=1, tone=60) + CS.shot(2, H, W, seed=2, tone=190)
VIDEO8 = [yuv.encode_numpy(f, FMT8) for f in RGB]
VIDEO10 = [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), FMT10) | np.uint16(k % 4) for k, f in enumerate(RGB)]
LOOPS = {"nx": lambda frames, **kw: mf.interpolate_video_nx(frames, Mean(), factor=4, **kw),
         "nx_tta": lambda frames, **kw: mf.interpolate_video_nx(frames, Mean(), factor=2, tta=True, **kw),
         "retimed": lambda frames, **kw: rt.interpolate_video_retimed(frames, Mean(), 24, 60, levels=2, **kw)}
CASES = {"nv12": (FMT8, yuv.Surface(FMT8, "uv"), {}),
         "nv12_padded_crop": (FMT8, yuv.Surface(FMT8, "uv", pitch=W + 6, chroma_pitch=W + 2, chroma_offset=(W + 6) * H + 10), dict(crop=(16, 32))),
         "nv21_padded": (FMT8, yuv.Surface(FMT8, "vu", pitch=W + 8, chroma_pitch=W + 8), {}),
         "p010": (FMT10, yuv.Surface(FMT10, "uv", True), {}),
         "p010_keep": (FMT10, yuv.Surface(FMT10, "uv", True), dict(keep_depth=True)),
         "p010_padded_keep_crop": (FMT10, yuv.Surface(FMT10, "uv", True, pitch=2 * W + 6, chroma_pitch=2 * W + 4), dict(keep_depth=True, crop=(16, 32)))}


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("case", list(CASES))
def test_loops_yield_the_repack_of_the_i420_run(case, loop):
    fmt, s, kw = CASES[case]
    video = VIDEO8 if fmt.depth == 8 else VIDEO10
    frames = [yuv.repack(f, fmt, s) for f in video]
    keep = [f.copy() for f in frames]
    for with_scene in (False, True):
        sc = (lambda: importlib.import_module("atm-vfi_amd.scene").SceneCuts()) if with_scene else (lambda: None)
        sc_ref, sc_got = sc(), sc()
        ref = list(LOOPS[loop](iter(video), pixfmt=fmt, scene=sc_ref, **kw))
        got = list(LOOPS[loop](iter(frames), pixfmt=s, scene=sc_got, **kw))
        assert len(got) == len(ref) > len(video)
        if with_scene:
            assert sc_got.cuts == sc_ref.cuts and len(sc_ref.cuts) == 1
        _, _, h, w = mf.centre_window(H, W, kw.get("crop"))
        shapes = set()
        for g, r in zip(got, ref):
            # an original of 10-bit input stays 10-bit; a produced frame has the output's depth: the rule Format follows
            rf = (fmt if r.dtype == np.uint16 else fmt.as_8bit()).cropped(h, w)
            rs = (s.tight() if r.dtype == np.uint16 else s.as_8bit()).cropped(h, w)
            assert g.dtype == r.dtype and np.array_equal(g, yuv.repack(r, rf, rs))
            shapes.add((g.dtype, g.shape))
        assert len(shapes) == (2 if (fmt.depth == 10 and not kw.get("keep_depth")) else 1)       # one stream, one buffer shape per depth
        if s.is_tight and "crop" not in kw:
            assert got[0] is frames[0] and got[-1] is frames[-1]           # originals are the caller's own objects
        else:
            assert got[0] is not frames[0] and np.array_equal(got[0], yuv.crop(frames[0], s, *mf.centre_window(H, W, kw.get("crop"))))
    assert all(np.array_equal(a, b) for a, b in zip(frames, keep))


def test_interpolate_raw_writes_what_the_loop_yields():
    s = yuv.Surface.nv12(H, W, pitch=W + 8, matrix="bt709", siting="left")
    frames = [yuv.repack(f, FMT8, s) for f in VIDEO8]
    src = io.BytesIO(b"".join(f.tobytes() for f in frames))
    dst = io.BytesIO()
    info = yuv.interpolate_raw(src, dst, Mean(), s, "24", factor=4)
    want = list(mf.interpolate_video_nx(iter(frames), Mean(), factor=4, pixfmt=s))
    assert dst.getvalue() == b"".join(f.tobytes() for f in want)
    assert info["frames_in"] == 5 and info["frames_out"] == 17 and info["fps_out"] == 96 and info["size"] == (W, H)
    p = yuv.Surface(FMT10, "uv", True)
    frames = [yuv.repack(f, FMT10, p) for f in VIDEO10]
    for keep in (False, True):
        dst = io.BytesIO()
        info = yuv.interpolate_raw(io.BytesIO(b"".join(f.astype("<u2").tobytes() for f in frames)), dst, Mean(), p, 24, fps_out=60, levels=2,
                                   keep_depth=keep)
        want = list(rt.interpolate_video_retimed(iter(frames), Mean(), 24, 60, levels=2, pixfmt=p, keep_depth=keep))
        if not keep:        # originals are converted on the host: one stream of NV12
            want = [yuv.to_8bit(f, p) if f.dtype == np.uint16 else f for f in want]
        assert dst.getvalue() == b"".join(f.astype("<u2" if keep else np.uint8).tobytes() for f in want) and info["frames_out"] == len(want)
    with pytest.raises(ValueError, match="needs fps_out"):
        yuv.interpolate_raw(io.BytesIO(b""), io.BytesIO(), Mean(), s, 24, shutter=180)


# ------------------------------------------------------------------------------------------------ ABI
def test_surface_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    for name in ("atmvfi_yuv_decode", "atmvfi_yuv_encode"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
        assert lib.atmvfi_plan_fn_id(name.encode()) >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 29
    assert callable(hip_ops.HipOps.yuv_surface_decode) and callable(hip_ops.HipOps.yuv_surface_encode)
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error

    def dec(buf=P, H=64, W=96, depth=8, matrix=0, full=0, siting=0, chroma=1, msb=0, pitch=0, cpitch=0, coff=0, keep=0, y0=0, x0=0, h=64, w=96,
            dst_u8=None, bgr=0, dst=P, Hp=64, Wp=96, pt=0, pl=0):
        d = hip_ops.YuvDesc(H=H, W=W, depth=depth, matrix=matrix, full_range=full, siting=siting, chroma=chroma, msb=msb, pitch=pitch,
                            chroma_pitch=cpitch, chroma_offset=coff)
        rc = lib.atmvfi_yuv_decode(ctypes.byref(d), buf, keep, 0, y0, x0, h, w, dst_u8, bgr, dst, Hp, Wp, pt, pl, None)
        assert rc == -1 and err().startswith(b"yuv_decode: ")
        return rc

    def enc(src_u8=None, bgr=0, src=P, Hp=64, Wp=96, pt=0, pl=0, H=64, W=96, depth=8, matrix=0, full=0, siting=0, chroma=1, msb=0, buf=P):
        d = hip_ops.YuvDesc(H=H, W=W, depth=depth, matrix=matrix, full_range=full, siting=siting, chroma=chroma, msb=msb)
        rc = lib.atmvfi_yuv_encode(ctypes.byref(d), src_u8, bgr, src, Hp, Wp, pt, pl, buf, None)
        assert rc == -1 and err().startswith(b"yuv_encode: ")
        return rc
    assert dec(buf=None) == -1 and b"null source" in err()
    assert dec(dst=None) == -1 and b"both outputs are null" in err()
    assert dec(H=0) == -1 and b"at least 1" in err()
    assert dec(depth=12) == -1 and b"depth must be 8 or 10" in err()
    assert dec(depth=10, full=1) == -1 and b"full range" in err()
    assert dec(matrix=2) == -1 and b"unknown matrix" in err()
    assert dec(siting=2) == -1 and b"unknown siting" in err()
    assert dec(chroma=3) == -1 and b"unknown chroma layout" in err()
    assert dec(msb=1) == -1 and b"msb needs depth 10" in err()
    assert dec(msb=2, depth=10) == -1 and b"msb must be 0 or 1" in err()
    assert dec(pitch=95) == -1 and b"at least a luma row" in err()
    assert dec(depth=10, pitch=193) == -1 and b"multiple of the sample size" in err()
    assert dec(cpitch=95) == -1 and b"at least a chroma row" in err()
    assert dec(chroma=0, cpitch=47) == -1 and b"at least a chroma row" in err()
    assert dec(depth=10, cpitch=195) == -1 and b"multiple of the sample size" in err()
    assert dec(pitch=128, coff=128 * 64 - 1) == -1 and b"at least pitch * H" in err()
    assert dec(depth=10, coff=192 * 64 + 1) == -1 and b"multiple of the sample size" in err()
    assert dec(keep=1) == -1 and b"keep_depth needs a 10-bit surface" in err()
    assert dec(keep=2, depth=10) == -1 and b"keep_depth must be 0 or 1" in err()
    assert dec(keep=1, depth=10, dst_u8=P) == -1 and b"not with keep_depth" in err()
    assert dec(h=0) == -1 and b"at least 1" in err()
    assert dec(y0=2) == -1 and b"outside the" in err()
    assert dec(x0=-2, w=8) == -1 and b"outside the" in err()
    assert dec(y0=1, h=8) == -1 and b"must be even" in err()
    assert dec(x0=3, w=8) == -1 and b"must be even" in err()
    assert dec(Hp=63) == -1 and b"smaller than the window" in err()
    assert dec(pl=1) == -1 and b"smaller than the window" in err()
    assert dec(dst=P + 2) == -1 and b"4-byte aligned" in err()
    assert dec(H=100000, W=100000, h=100000, w=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()
    assert enc(buf=None) == -1 and b"null destination" in err()
    assert enc(src=None) == -1 and b"exactly one" in err()
    assert enc(src_u8=P) == -1 and b"exactly one" in err()
    assert enc(W=0) == -1 and b"at least 1" in err()
    assert enc(depth=9) == -1 and b"depth must be 8 or 10" in err()
    assert enc(chroma=-1) == -1 and b"unknown chroma layout" in err()
    assert enc(msb=1) == -1 and b"msb needs depth 10" in err()
    assert enc(depth=10, src=None, src_u8=P) == -1 and b"fp32 canvas" in err()
    assert enc(Wp=95) == -1 and b"smaller than the frame" in err()
    assert enc(src=P + 1) == -1 and b"4-byte aligned" in err()
    assert enc(H=100000, W=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()
    assert dec(pt=-1) == -1 and b"smaller than the window" in err()                             # (asserted for its siblings before)
    assert dec(full=2) == -1 and b"full_range" in err()
    assert enc(src=None, src_u8=None) == -1 and b"exactly one" in err() and b"neither" in err()
    assert enc(src_u8=P) == -1 and b"both" in err()
    assert enc(siting=3) == -1 and b"unknown siting" in err()
    assert enc(pl=-4) == -1 and b"smaller than the frame" in err()


# ------------------------------------------------------------------------------------------------ the frame descriptor
_DESC_GROUPS = {
    "size": [(dict(H=0), b"H and W must be at least 1 (got 0 x 16)"), (dict(W=0), b"H and W must be at least 1 (got 8 x 0)"),
             (dict(H=3, W=5, y0=2), b"at (2, 0) of a 3 x 5 frame")],
    "colour": [(dict(depth=12), b"depth must be 8 or 10 (got 12)"), (dict(matrix=7), b"unknown matrix 7"),
               (dict(full_range=5), b"full_range must be 0 or 1 (got 5)"), (dict(siting=3), b"unknown siting 3")],
    "layout": [(dict(subsampling=9), b"unknown subsampling 9"), (dict(chroma=4), b"unknown chroma layout 4"),
               (dict(depth=10, msb=6), b"msb must be 0 or 1 (got 6)"), (dict(subsampling=2, siting=1), b"siting 1 has no meaning for 4:4:4")],
    "strides": [(dict(pitch=15), b"pitch 15 must be"), (dict(chroma_pitch=7), b"chroma_pitch 7 must be"),
                (dict(chroma_offset=127), b"chroma_offset 127 must be"), (dict(pitch=32, chroma_offset=255), b"at least pitch * H = 256")],
}


@pytest.mark.parametrize("group", list(_DESC_GROUPS))
def test_yuv_desc_layout_matches_the_header(group):
    """hip_ops.YuvDesc against the C struct: one wrong field at a time on an otherwise valid 8 x 16 block (3 x 5 where the frame's size is
    the point), each refused before any launch with the message of exactly that field and its value -- a ctypes field that sits
    elsewhere than its C counterpart makes the library read another value there and report something else (or nothing)."""
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    P = 0x10000       # never dereferenced
    assert ctypes.sizeof(hip_ops.YuvDesc) == 64 and hip_ops.YuvDesc.pitch.offset == 40          # nine int32, padding, three int64
    for wrong, text in _DESC_GROUPS[group]:
        kw = {**dict(H=8, W=16, depth=8, matrix=0), **wrong}
        y0 = kw.pop("y0", 0)
        d = hip_ops.YuvDesc(**kw)
        assert lib.atmvfi_yuv_decode(ctypes.byref(d), P, 0, 0, y0, 0, 2, 4, None, 0, P, 2, 4, 0, 0, None) == -1
        assert lib.atmvfi_last_error().startswith(b"yuv_decode: ") and text in lib.atmvfi_last_error(), (wrong, lib.atmvfi_last_error())
        if "pitch" in "".join(wrong) or "chroma_offset" in wrong or "y0" in wrong or "H" in wrong and "W" in wrong:
            continue                                        # (an encode reads no stride and has no window)
        assert lib.atmvfi_yuv_encode(ctypes.byref(d), None, 0, P, kw["H"], kw["W"], 0, 0, P, None) == -1
        assert lib.atmvfi_last_error().startswith(b"yuv_encode: ") and text in lib.atmvfi_last_error(), (wrong, lib.atmvfi_last_error())
    assert lib.atmvfi_yuv_decode(None, P, 0, 0, 0, 0, 2, 4, None, 0, P, 2, 4, 0, 0, None) == -1 and b"null descriptor" in lib.atmvfi_last_error()
