"""CPU: the Xiph evaluation on Y4M clips -- ``yuv.window_numpy`` against the per-pixel model (tests/cpu_yuv_window.py), the ABI's
host-side checks of ``atmvfi_yuv_decode`` (``mode``), finding a clip and choosing its source (``evaluate.xiph_y4m_file`` / ``xiph_sources``),
``Y4MReader.skip`` and the reader thread's errors on tiny files written with ``Y4MWriter``."""
import ctypes
import importlib
import io
import os
import re

import numpy as np
import pytest

import cpu_scene as CS
import cpu_yuv_window as CW

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
evaluate = importlib.import_module("atm-vfi_amd.evaluate")
yuv = importlib.import_module("atm-vfi_amd.yuv")


# ------------------------------------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fmt", CW.FORMATS, ids=[f[0] for f in CW.FORMATS])
@pytest.mark.parametrize("geom", [CW.WHOLE_16, CW.INNER_40x56], ids=["whole16", "inner40x56"])
def test_window_numpy_is_the_loop_model(geom, fmt, mode):
    (H, W), windows = geom
    _, depth, matrix, full, siting = fmt
    f = yuv.Format(H, W, matrix, bool(full), siting, depth)
    got = yuv.window_numpy(CW.frame(H, W, depth), f, mode, *windows[mode])
    want = CW.window_u8(CW.decoded(H, W, depth, matrix, full, siting), mode, *windows[mode])
    assert got.dtype == np.uint8 and got.shape == want.shape and got.flags.c_contiguous and np.array_equal(got, want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fmt", [CW.FORMATS[0], CW.FORMATS[-1]], ids=[CW.FORMATS[0][0], CW.FORMATS[-1][0]])
def test_window_numpy_on_an_odd_frame_and_a_wide_one(fmt, mode):
    _, depth, matrix, full, siting = fmt
    (H, W), windows = CW.ODD_37x53
    f = yuv.Format(H, W, matrix, bool(full), siting, depth)
    assert np.array_equal(yuv.window_numpy(CW.frame(H, W, depth), f, mode, *windows[mode]),
                          CW.window_u8(CW.decoded(H, W, depth, matrix, full, siting), mode, *windows[mode]))
    # the wide frame against the vectorised decode (itself held to the loops by tests/test_yuv_cpu.py) and the window model
    (H, W), windows = CW.WIDE_16x4200
    f = yuv.Format(H, W, matrix, bool(full), siting, depth)
    assert np.array_equal(yuv.window_numpy(CW.frame(H, W, depth), f, mode, *windows[mode]),
                          CW.window_u8(yuv.decode_numpy(CW.frame(H, W, depth), f), mode, *windows[mode]))


def test_window_numpy_refuses_what_the_call_refuses():
    f = yuv.Format(16, 16)
    buf = CW.frame(16, 16, 8)
    with pytest.raises(ValueError, match="must be even"):
        yuv.window_numpy(buf, f, 0, 1, 0, 4, 4)
    with pytest.raises(ValueError, match="must be even"):
        yuv.window_numpy(buf, f, 1, 0, 3, 4, 4)
    with pytest.raises(ValueError, match="outside the frame"):
        yuv.window_numpy(buf, f, 1, 0, 0, 9, 8)
    with pytest.raises(ValueError, match="outside the frame"):
        yuv.window_numpy(buf, f, 0, 2, 2, 15, 4)
    with pytest.raises(ValueError, match="unknown mode"):
        yuv.window_numpy(buf, f, 2, 0, 0, 4, 4)


# ------------------------------------------------------------------------------------------------ ABI
def test_yuv420_window_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    name = "atmvfi_yuv_decode"                      # the window with its area mode is `mode` of the one decode entry point
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert lib.atmvfi_plan_fn_id(name.encode()) >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 29
    assert " yuv.hip" in open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert callable(hip_ops.HipOps.yuv420_window) and callable(yuv.window_numpy)
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error

    def win(yuv_=P, H=64, W=96, depth=8, matrix=0, full=0, siting=0, mode=0, y0=0, x0=0, h=32, w=48, dst=P, Hp=32, Wp=48, pt=0, pl=0, d8=P):
        d = hip_ops.YuvDesc(H=H, W=W, depth=depth, matrix=matrix, full_range=full, siting=siting)
        rc = lib.atmvfi_yuv_decode(ctypes.byref(d), yuv_, 0, mode, y0, x0, h, w, d8, 0, dst, Hp, Wp, pt, pl, None)
        assert rc == -1 and err().startswith(b"yuv_decode: ")           # the shared checks, under the entry point's own name
        return rc
    assert win(yuv_=None) == -1 and b"null source" in err()
    assert win(dst=None, d8=None) == -1 and b"both outputs are null" in err()
    assert win(mode=2) == -1 and b"unknown mode" in err()
    assert win(mode=-1) == -1 and b"unknown mode" in err()
    assert win(y0=34) == -1 and b"window outside the frame" in err()                    # 34 + 32 > 64
    assert win(x0=50) == -1 and b"window outside the frame" in err()
    assert win(mode=1, h=33, Hp=33) == -1 and b"window outside the frame" in err() and b"66 x 96" in err()    # 2h x 2w source pixels
    assert win(mode=1, w=49, Wp=49) == -1 and b"window outside the frame" in err()
    assert win(y0=1) == -1 and b"must be even" in err()
    assert win(x0=3) == -1 and b"must be even" in err()
    assert win(depth=10, full=1) == -1 and b"10-bit full range" in err()
    assert win(depth=12) == -1 and b"depth must be 8 or 10" in err()
    assert win(Hp=31) == -1 and b"smaller than the window" in err()
    assert win(Wp=47) == -1 and b"smaller than the window" in err()
    assert win(pt=1) == -1 and b"smaller than the window" in err()
    assert win(pl=4) == -1 and b"smaller than the window" in err()
    assert win(pt=-1) == -1 and b"smaller than the window" in err()
    assert win(h=0) == -1 and b"negative or zero" in err()
    assert win(x0=-2) == -1 and b"negative or zero" in err()
    assert win(H=0) == -1 and b"at least 1" in err()
    assert win(matrix=2) == -1 and b"unknown matrix" in err()
    assert win(siting=2) == -1 and b"unknown siting" in err()
    assert win(full=2) == -1 and b"full_range" in err()
    assert win(dst=P + 2) == -1 and b"4-byte aligned" in err()
    assert win(W=0) == -1 and b"at least 1" in err()                                            # (asserted for its siblings before)
    assert win(mode=1, y0=2) == -1 and b"window outside the frame" in err() and b"64 x 96" in err()     # 2 + 2 * 32 > 64
    assert win(mode=1, x0=2) == -1 and b"window outside the frame" in err()
    assert win(mode=1, y0=1, h=8, w=8, Hp=8, Wp=8) == -1 and b"must be even" in err()
    assert win(mode=1, Hp=31) == -1 and b"smaller than the window" in err()
    for mode in (0, 1):         # 1.25e9 and 2.5e9 work items
        assert win(mode=mode, H=200000, W=200000, h=100000, w=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()


# ------------------------------------------------------------------------------------------------ finding a clip, choosing its source
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()
    return path


def test_clip_lookup(tmp_path):
    root = str(tmp_path)
    plain = _touch(os.path.join(root, "Tango.y4m"))
    down = _touch(os.path.join(root, "Netflix_FoodMarket2_4096x2160_60fps_10bit_420.y4m"))
    assert evaluate.xiph_y4m_file(root, "Tango") == plain                   # the plain name
    assert evaluate.xiph_y4m_file(root, "FoodMarket2") == down              # the download name
    assert evaluate.xiph_y4m_file(root, "FoodMarket") is None               # FoodMarket does not match FoodMarket2
    assert evaluate.xiph_y4m_file(root, "Crosswalk") is None
    fm = _touch(os.path.join(root, "Netflix_FoodMarket_4096x2160_60fps_10bit_420.y4m"))
    assert evaluate.xiph_y4m_file(root, "FoodMarket") == fm and evaluate.xiph_y4m_file(root, "FoodMarket2") == down
    other = _touch(os.path.join(root, "Copy_FoodMarket_4096x2160.y4m"))
    with pytest.raises(ValueError) as e:                                    # ambiguity: both files are named
        evaluate.xiph_y4m_file(root, "FoodMarket")
    assert fm in str(e.value) and other in str(e.value)
    _touch(os.path.join(root, "FoodMarket.y4m"))                            # the plain name settles it
    assert evaluate.xiph_y4m_file(root, "FoodMarket") == os.path.join(root, "FoodMarket.y4m")


def test_sources_auto_png_y4m_and_the_missing_clip(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "ClipA"))
    a4 = _touch(os.path.join(root, "ClipA.y4m"))
    b4 = _touch(os.path.join(root, "Netflix_ClipB_384x216_60fps_10bit_420.y4m"))
    # auto: the PNG directory takes precedence where it exists
    assert evaluate.xiph_sources(root, ("ClipA", "ClipB")) == {"ClipA": ("png", os.path.join(root, "ClipA")), "ClipB": ("y4m", b4)}
    assert evaluate.xiph_sources(root, ("ClipA", "ClipB"), "y4m") == {"ClipA": ("y4m", a4), "ClipB": ("y4m", b4)}
    assert evaluate.xiph_sources(root, ("ClipA", "ClipB"), "png")["ClipB"] == ("png", os.path.join(root, "ClipB"))
    with pytest.raises(FileNotFoundError) as e:
        evaluate.xiph_sources(root, ("ClipA", "ClipC"))
    msg = str(e.value)
    assert "ClipC" in msg and os.path.join(root, "ClipC") + os.sep in msg and os.path.join(root, "ClipC.y4m") in msg and "*_ClipC_*.y4m" in msg
    with pytest.raises(FileNotFoundError, match=r"ClipC\.y4m"):
        evaluate.xiph_sources(root, ("ClipC",), "y4m")
    with pytest.raises(ValueError, match="unknown Xiph source"):
        evaluate.xiph_sources(root, ("ClipA",), "mp4")
    # forcing PNG on a clip without a directory fails in the lister, naming the first missing frame
    with pytest.raises(FileNotFoundError, match="001.png"):
        evaluate.xiph(root, ("ClipB",), range(2, 7, 2))
    # PNG number k is stream frame k - 1
    s = evaluate.xiph_y4m(b4, "ClipB", range(2, 7, 2))
    assert [x.name for x in s] == ["ClipB/002", "ClipB/004", "ClipB/006"] and s[0].frames == ((b4, 0), (b4, 1), (b4, 2))
    assert s[2].frames == ((b4, 4), (b4, 5), (b4, 6)) and all(x.level == "xiph" for x in s)


# ------------------------------------------------------------------------------------------------ the reader
def _write_clip(path, h, w, frames, depth=8):
    fmt = yuv.Format(h, w, depth=depth)
    with yuv.Y4MWriter(path, fmt, 60) as wr:
        for k in range(frames):
            wr.write(CW.frame(h, w, depth, seed=100 + k))
    return fmt


class _Pipe(io.RawIOBase):
    """A stream that cannot seek, and counts the bytes it hands out."""

    def __init__(self, data):
        self.data, self.pos = data, 0

    def readable(self):
        return True

    def seekable(self):
        return False

    def readinto(self, b):
        n = min(len(b), len(self.data) - self.pos)
        b[:n] = self.data[self.pos:self.pos + n]
        self.pos += n
        return n


@pytest.mark.parametrize("depth", [8, 10])
def test_reader_skip_seeks_or_drops(tmp_path, depth):
    path = str(tmp_path / "c.y4m")
    fmt = _write_clip(path, 16, 24, 5, depth)
    with yuv.Y4MReader(path) as rd:                     # seekable
        it = iter(rd)
        assert rd.skip(2) == 2
        assert np.array_equal(next(it), CW.frame(16, 24, depth, seed=102))
        assert rd.skip(1) == 1
        assert np.array_equal(next(it), CW.frame(16, 24, depth, seed=104))
        assert rd.skip(3) == 0 and next(it, None) is None
    pipe = _Pipe(open(path, "rb").read())
    rd = yuv.Y4MReader(io.BufferedReader(pipe))         # not seekable: read and dropped
    it = iter(rd)
    assert rd.skip(3) == 3
    assert np.array_equal(next(it), CW.frame(16, 24, depth, seed=103))
    assert rd.skip(9) == 1 and rd.skip(1) == 0
    with open(path, "r+b") as f:                        # a truncated last frame is an error, not a short count
        f.truncate(os.path.getsize(path) - 7)
    with yuv.Y4MReader(path) as rd:
        assert rd.skip(4) == 4
        with pytest.raises(ValueError, match="truncated"):
            rd.skip(1)
    assert fmt.frame_bytes == (16 * 24 * 3 // 2) * (2 if depth == 10 else 1)


def test_feed_reads_each_needed_frame_once_in_order_and_stops(tmp_path, monkeypatch):
    a, b = str(tmp_path / "A.y4m"), str(tmp_path / "B.y4m")
    _write_clip(a, 16, 24, 9)
    _write_clip(b, 16, 24, 9, depth=10)
    reads = []

    class Counting(yuv.Y4MReader):
        def __iter__(self):
            for fr in super().__iter__():
                reads.append(self.f.name)
                yield fr
    monkeypatch.setattr(evaluate.yuv, "Y4MReader", Counting)
    feed = evaluate._Y4MFeed([("A", a, [1, 2, 3, 5]), ("B", b, [0, 6])], "auto")
    try:
        for file, k, depth in [(a, 1, 8), (a, 2, 8), (a, 3, 8), (a, 5, 8), (b, 0, 10), (b, 6, 10)]:
            fr, fmt, dt = feed.get((file, k))
            assert np.array_equal(fr, CW.frame(16, 24, depth, seed=100 + k)) and fmt.depth == depth and fmt.matrix == "bt601" and dt >= 0
    finally:
        feed.close()
    assert reads == [a] * 4 + [b] * 2 and not feed.thread.is_alive()       # skipped frames are never read; nothing after the last one


def test_feed_errors_short_stream_and_size(tmp_path):
    short = str(tmp_path / "Short.y4m")
    _write_clip(short, 16, 24, 3)
    feed = evaluate._Y4MFeed([("Short", short, [1, 2, 5])], "auto")
    try:
        feed.get((short, 1))
        feed.get((short, 2))
        with pytest.raises(ValueError) as e:
            feed.get((short, 5))
    finally:
        feed.close()
    assert "Short" in str(e.value) and "frame 5" in str(e.value) and "only 3 frames" in str(e.value)
    for h, w in [(20, 24), (16, 28)]:                   # H % 8 / W % 8: the centre-crop origin would be odd
        odd = str(tmp_path / f"Odd{h}x{w}.y4m")
        _write_clip(odd, h, w, 3)
        feed = evaluate._Y4MFeed([("Odd", odd, [0])], "auto")
        try:
            with pytest.raises(ValueError, match=r"H % 8 == 0 and W % 8 == 0.*" + f"{h}x{w}"):
                feed.get((odd, 0))
        finally:
            feed.close()
    assert evaluate.xiph_geometry(24, 40, "cropped-4k")[1:3] == (6, 10)     # why: % 4 alone gives an even origin only by luck


def test_frames_that_do_not_ascend_are_refused_before_anything_is_read(tmp_path):
    """A Y4M stream is walked forward once: a descending range (valid for a PNG tree) must raise, not leave the consumer waiting."""
    a, b = str(tmp_path / "A.y4m"), str(tmp_path / "B.y4m")
    up = evaluate.xiph_y4m(a, "A", range(2, 7, 2))
    assert evaluate._y4m_jobs(up) == [("A", a, [0, 1, 2, 3, 4, 5, 6])]
    assert evaluate._y4m_jobs(up[:1] + up[2:]) == [("A", a, [0, 1, 2, 4, 5, 6])]              # a gap is fine, and is skipped
    assert evaluate._y4m_jobs(up + evaluate.xiph_y4m(b, "B", [3])) == [("A", a, [0, 1, 2, 3, 4, 5, 6]), ("B", b, [1, 2, 3])]
    assert evaluate._y4m_jobs(up + up) == [("A", a, [0, 1, 2, 3, 4, 5, 6])]                   # frames already wanted are not read again
    with pytest.raises(ValueError, match=r"A/004.*stream frame 2 .*after frame 6.*must ascend"):
        evaluate._y4m_jobs(evaluate.xiph_y4m(a, "A", range(6, 1, -2)))
    with pytest.raises(ValueError, match="must ascend"):
        evaluate._y4m_jobs(evaluate.xiph_y4m(a, "A", [6, 2]))
    with pytest.raises(ValueError, match="wanted again after another clip"):
        evaluate._y4m_jobs(evaluate.xiph_y4m(a, "A", [2]) + evaluate.xiph_y4m(b, "B", [2]) + evaluate.xiph_y4m(a, "A", [6]))
    with pytest.raises(ValueError, match="start at 001"):
        evaluate._y4m_jobs(evaluate.xiph_y4m(a, "A", [1]))
    # PNG frames never enter a job
    assert evaluate._y4m_jobs([evaluate.Sample("C/002", "xiph", ("r/C/001.png", "r/C/002.png", "r/C/003.png"))]) == []


def test_feed_asked_for_more_than_its_jobs_raises_instead_of_waiting(tmp_path):
    path = str(tmp_path / "A.y4m")
    _write_clip(path, 16, 24, 4)
    feed = evaluate._Y4MFeed([("A", path, [1, 2])], "auto")
    try:
        feed.get((path, 1))
        feed.get((path, 2))
        for _ in range(2):
            with pytest.raises(RuntimeError, match="after the reader had delivered every frame"):
                feed.get((path, 0))
    finally:
        feed.close()


def test_samples_helper_is_what_the_lister_and_the_cli_share(tmp_path):
    root = str(tmp_path)
    b4 = _touch(os.path.join(root, "Netflix_ClipB_384x216_60fps_10bit_420.y4m"))
    samples, where = evaluate.xiph_samples(root, ("ClipB",), range(2, 5, 2))
    assert where == {"ClipB": "y4m"} and samples == evaluate.xiph_y4m(b4, "ClipB", range(2, 5, 2))
    with pytest.raises(FileNotFoundError, match="001.png"):
        evaluate.xiph_samples(root, ("ClipB",), range(2, 5, 2), "png")
