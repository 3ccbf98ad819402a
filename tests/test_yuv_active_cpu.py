"""CPU: the active picture on YUV streams and in the retimed loop (atm-vfi_amd/active.py: bar_code, yuv_borders_numpy,
yuv_compose_numpy; ``active=`` of ``interpolate_video_nx`` with a ``pixfmt`` and of ``interpolate_video_retimed``; atmvfi_yuv_borders /
atmvfi_yuv_compose) without a GPU: the host twins against the per-sample models, the sample code of the ``peak`` default against the
canvases of tests/golden/active_ref.npz, letterboxed videos through the host backend of both loops, the refusals, and the ABI's
host-side checks."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cpu_active as C
import cpu_yuv_active as Y

active = importlib.import_module("atm-vfi_amd.active")
mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
yuv = importlib.import_module("atm-vfi_amd.yuv")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")


def surface_of(L, **fmt_kw):
    """the yuv.Surface of a model layout"""
    f = yuv.Format(L["H"], L["W"], depth=L["depth"], subsampling=L["sub"], **fmt_kw)
    return yuv.Surface(f, {"planar": "planar", "uv": "uv", "vu": "vu"}[L["chroma"]], L["msb"], L["pitch"], L["chroma_pitch"], L["chroma_offset"])


LAYOUTS = {
    "i420 16x16": Y.layout(16, 16),
    "i420 18x22": Y.layout(18, 22),
    "p10 21x37": Y.layout(21, 37, depth=10),
    "p010 pitch": Y.layout(18, 22, depth=10, chroma="uv", msb=True, pitch=64, chroma_pitch=64, chroma_offset=64 * 18 + 128),
    "nv21 pitch": Y.layout(20, 26, chroma="vu", pitch=32, chroma_pitch=32),
    "422 10 bit": Y.layout(17, 23, depth=10, sub="422", pitch=48, chroma_pitch=26),
    "444": Y.layout(16, 19, sub="444"),
}


# ------------------------------------------------------------------------------------------------ twins
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_yuv_borders_numpy_is_the_sample_loop(name):
    L = LAYOUTS[name]
    s = surface_of(L)
    buf = Y.random_frame(L, seed=3, poison=0xFF)               # padding at the largest byte: it must never be read
    for y, x in ((0, 0), (0, L["W"] - 1), (L["H"] - 1, 0), (L["H"] - 1, L["W"] - 1)):
        Y.set_luma(buf, L, y, x, 1023 if L["depth"] == 10 else 255)
    got = active.yuv_borders_numpy(buf, s)
    assert got.dtype == np.int32 and got.shape == (L["H"] + L["W"],)
    assert np.array_equal(got, Y.borders_model(buf, L)) and np.array_equal(got, Y.borders_model_lines(buf, L))
    if s.is_tight and s.chroma == "planar":                    # a Format's frame is its tight planar surface's
        assert np.array_equal(active.yuv_borders_numpy(buf, s.fmt), got)
    with pytest.raises(ValueError, match="16 x 16"):
        active.yuv_borders_numpy(np.zeros(yuv.Format(15, 16).frame_samples, np.uint8), yuv.Format(15, 16))


WINDOWS = {
    "i420 18x22": [(4, 6, 8, 10), (0, 0, 18, 22), (0, 0, 2, 2), (16, 20, 2, 2), (0, 4, 18, 8), (6, 0, 4, 22)],
    "p10 21x37": [(10, 20, 11, 17), (0, 0, 20, 36), (20, 36, 1, 1)],
    "p010 pitch": [(2, 4, 10, 12)],
    "nv21 pitch": [(8, 2, 12, 24)],
    "422 10 bit": [(3, 4, 7, 10), (5, 20, 12, 3)],
    "444": [(1, 3, 5, 7)],
}


@pytest.mark.parametrize("name,siting", [(n, s) for n in WINDOWS for s in ("centre", "left") if not (n == "444" and s == "left")])
def test_yuv_compose_numpy_is_the_sample_loop(name, siting):
    L = LAYOUTS[name]
    s = surface_of(L, siting=siting)
    border = Y.random_frame(L, seed=5, poison=0xEE)
    rng = np.random.default_rng(11)
    for win in WINDOWS[name]:
        y0, x0, h, w = win
        if L["depth"] == 10:
            src = rng.uniform(-0.1, 1.1, (h, w, 3)).astype(np.float32)
        else:
            src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        frame = yuv.encode_numpy(src, s.tight().cropped(h, w))
        want = Y.compose_model(border, L, win, Y.encode_window(Y.cpu_yuv_sub.pixels(src, L["depth"]), L, h, w, s.matrix, 0, siting))
        got = active.yuv_compose_numpy(border, s, win, frame)
        assert got.dtype == s.dtype and got.size == s.tight().frame_samples
        assert np.array_equal(got.view(np.uint8), want), win
        # the two equalities of the definition
        assert np.array_equal(yuv.crop(got, s.tight(), y0, x0, h, w), frame)
        if (h, w) == (L["H"], L["W"]):
            assert np.array_equal(got, frame)
    for bad in ((1, 0, 4, 4), (0, 1, 4, 4), (0, 0, 3, 4), (0, 0, 4, 3)):
        if Y.window_ok(L, bad):
            continue
        with pytest.raises(ValueError, match="subsampling step"):
            active.yuv_compose_numpy(border, s, bad, np.zeros(1, s.dtype))
    assert host_io.yuv_borders_numpy is active.yuv_borders_numpy and host_io.yuv_compose_numpy is active.yuv_compose_numpy
    assert host_io.bar_code is active.bar_code


# ------------------------------------------------------------------------------------------------ the policy's threshold
def test_bar_code_values():
    assert active.bar_code(yuv.Format(64, 64), 24) == 36
    assert active.bar_code(yuv.Format(64, 64, depth=10), 24) == 146
    assert active.bar_code(yuv.Surface.p010(64, 64), 24) == 146 and active.bar_code(yuv.Surface.nv12(64, 64), 24) == 36
    for peak in (0, 24, 200, 255):
        assert active.bar_code(yuv.Format(64, 64, full_range=True), peak) == peak
    assert active.bar_code(yuv.Format(64, 64), 0) == 16 and active.bar_code(yuv.Format(64, 64), 255) == 235
    assert active.bar_code(yuv.Format(64, 64, depth=10), 0) == 64 and active.bar_code(yuv.Format(64, 64, depth=10), 255) == 940
    assert all(active.bar_code(yuv.Format(64, 64), p) <= active.bar_code(yuv.Format(64, 64), p + 1) for p in range(255))      # monotone


def test_default_peak_keeps_its_margins_in_sample_codes():
    """README "Active picture": every canvas of the fixture encoded to limited range, bt601 and bt709, at 8 and 10 bits; the lines of
    ``cpu_active.fixture_statistics``; margins above the black code yo."""
    canv = C.decoded_canvases()
    peak = active.ActiveArea().peak
    for depth in (8, 10):
        yo = 16 << (depth - 8)
        for matrix in ("bt601", "bt709"):
            bar_max, content_min, by_black = 0, 1 << 16, {0: 0, 16: 0}
            for (name, black, q), c in canv.items():
                H, W = c.shape[:2]
                fmt = yuv.Format(H, W, matrix=matrix, depth=depth)
                frame = yuv.encode_numpy(c.astype(np.float32) / np.float32(255) if depth == 10 else c, fmt)
                prof = active.yuv_borders_numpy(frame, fmt)
                rows, cols = prof[:H], prof[H:]
                far = np.concatenate([rows[:C.BAR_ROWS - C.KEEP], rows[H - C.BAR_ROWS + C.KEEP:], cols[:C.BAR_COLS - C.KEEP],
                                      cols[W - C.BAR_COLS + C.KEEP:]])
                edge = np.concatenate([rows[C.BAR_ROWS:C.BAR_ROWS + C.KEEP], rows[H - C.BAR_ROWS - C.KEEP:H - C.BAR_ROWS],
                                       cols[C.BAR_COLS:C.BAR_COLS + C.KEEP], cols[W - C.BAR_COLS - C.KEEP:W - C.BAR_COLS]])
                bar_max, content_min = max(bar_max, int(far.max())), min(content_min, int(edge.min()))
                by_black[black] = max(by_black[black], int(far.max()))
                T = active.bar_code(fmt, peak)
                y0, x0, y1, x1 = active.rect_of(prof, H, W, T)
                assert C.BAR_ROWS - C.KEEP <= y0 <= C.BAR_ROWS + C.KEEP and C.BAR_COLS - C.KEEP <= x0 <= C.BAR_COLS + C.KEEP, (name, black, q)
                assert H - C.BAR_ROWS - C.KEEP <= y1 <= H - C.BAR_ROWS + C.KEEP and W - C.BAR_COLS - C.KEEP <= x1 <= W - C.BAR_COLS + C.KEEP
            T = active.bar_code(yuv.Format(64, 64, matrix=matrix, depth=depth), peak)
            print(f"{depth:2d}-bit {matrix}: T {T}, largest far-bar line maximum {bar_max} (black 0: {by_black[0]}, black 16: {by_black[16]}), "
                  f"smallest content-edge maximum {content_min}; (T - yo) / (bar - yo) = {(T - yo) / (bar_max - yo):.2f}, "
                  f"(content - yo) / (T - yo) = {(content_min - yo) / (T - yo):.2f}")
            assert T == (36 if depth == 8 else 146)
            assert T - yo >= 1.3 * (bar_max - yo)
            assert content_min - yo >= 1.9 * (T - yo)


# ------------------------------------------------------------------------------------------------ the loops, host backend
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend: the pair mean, recording the frame sizes it is asked for."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.shapes = []

    def forward(self, a, b):
        self.shapes.append(tuple(a.shape[-2:]))
        return {"I_t": (a + b) / 2}


H, W, WIN = 128, 96, (32, 0, 64, 96)
L5, PIC = C.letterboxed(5, H, W, (32, 96), seed=1)
KW = dict(divisor=16)                     # 64 rows pad to 64 against 128: the window gains
FORMATS = {
    "i420": (yuv.Format(H, W), {}),
    "422p10": (yuv.Format(H, W, depth=10, subsampling="422", siting="left"), dict(keep_depth=True)),
    "nv12 pitch": (yuv.Surface.nv12(H, W, pitch=128), {}),
}


def _out(fmt):
    return yuv.out_format(fmt, fmt.depth == 10)


@pytest.mark.parametrize("name", list(FORMATS))
def test_letterboxed_yuv_through_the_nx_loop(name):
    fmt, kw = FORMATS[name]
    video = Y.letterboxed_yuv(yuv, fmt, L5)
    model, area = Mean(), active.ActiveArea()
    got = list(mf.interpolate_video_nx(iter(video), model, factor=4, pixfmt=fmt, active=area, **KW, **kw))
    cropped = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, pixfmt=fmt, crop=(64, 96), **KW, **kw))
    assert len(got) == len(cropped) == 17 and area.window == WIN and area.probed == 5 and area.fallback_at is None
    assert area.code == active.bar_code(fmt, area.peak) and len(area.stats) == 5 + 5
    Y.check_nx(yuv, fmt, _out(fmt), WIN, got, video, cropped, 4)
    assert set(model.shapes) == {(64, 96)}                                     # the forwards ran on the window
    # a fixed window: never probed, never checked
    got2 = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, pixfmt=fmt, active=WIN, **KW, **kw))
    assert all(np.array_equal(a, b) for a, b in zip(got, got2))


@pytest.mark.parametrize("name", list(FORMATS))
def test_letterboxed_yuv_through_the_retimed_loop(name):
    fmt, kw = FORMATS[name]
    video = Y.letterboxed_yuv(yuv, fmt, L5)
    model, area, rep = Mean(), active.ActiveArea(), {}
    got = list(rt.interpolate_video_retimed(iter(video), model, 24, 60, levels=3, pixfmt=fmt, active=area, report=rep, **KW, **kw))
    cropped = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60, levels=3, pixfmt=fmt, crop=(64, 96), **KW, **kw))
    slots = list(rt.retime_slots(range(5), 24, 60, 3))
    assert area.window == WIN and area.fallback_at is None and rep["outputs"] == len(slots) == 11
    Y.check_retimed(yuv, fmt, _out(fmt), WIN, got, video, cropped, slots, 8)
    assert set(model.shapes) == {(64, 96)}


def test_retimed_active_on_rgb_frames():
    model, area = Mean(), active.ActiveArea()
    got = list(rt.interpolate_video_retimed(iter(L5), model, 24, 60, levels=3, active=area, **KW))
    alone = list(rt.interpolate_video_retimed(iter(PIC), Mean(), 24, 60, levels=3, **KW))
    slots = list(rt.retime_slots(range(5), 24, 60, 3))
    assert area.window == WIN and len(got) == len(alone) == len(slots) and set(model.shapes) == {(64, 96)}
    for g, a, (j, p) in zip(got, alone, slots):
        if p in (0, 8):
            assert g is L5[j + (p == 8)]
            continue
        near = L5[j] if p <= 4 else L5[j + 1]
        assert np.array_equal(g[32:96], a) and np.array_equal(g[:32], near[:32]) and np.array_equal(g[96:], near[96:])
    p = inspect.signature(rt.interpolate_video_retimed).parameters
    assert "active" in p and p["active"].default is None


@pytest.mark.parametrize("name", ["i420", "422p10"])
def test_a_lit_bar_sample_sends_both_loops_back_to_the_whole_frame(name):
    fmt, kw = FORMATS[name]
    k = 3
    video = Y.letterboxed_yuv(yuv, fmt, L5)
    video[k] = video[k].copy()
    fmt.planes(video[k])[0][5, 7] = 1023 if fmt.depth == 10 else 255           # a luma sample of frame 3, inside the top bar
    area = active.ActiveArea(probe=2)
    got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, pixfmt=fmt, active=area, **KW, **kw))
    plain = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, pixfmt=fmt, **KW, **kw))
    cropped = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, pixfmt=fmt, crop=(64, 96), **KW, **kw))
    assert area.window == WIN and area.probed == 2 and area.fallback_at == k - 1 and len(got) == len(plain)
    Y.check_nx(yuv, fmt, _out(fmt), WIN, got, video, cropped, 4, segments=k - 1)
    at = (k - 1) * 4
    assert all(np.array_equal(got[i], plain[i]) for i in range(at, len(got)))
    assert not np.array_equal(got[at - 1], plain[at - 1])                      # (the bars of a windowed frame are an original's)
    area, model = active.ActiveArea(probe=2), Mean()
    got = list(rt.interpolate_video_retimed(iter(video), model, 24, 60, levels=3, pixfmt=fmt, active=area, **KW, **kw))
    plain = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60, levels=3, pixfmt=fmt, **KW, **kw))
    cropped = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60, levels=3, pixfmt=fmt, crop=(64, 96), **KW, **kw))
    slots = list(rt.retime_slots(range(5), 24, 60, 3))
    assert area.fallback_at == k - 1 and len(got) == len(plain)
    first = min(i for i, (j, p) in enumerate(slots) if j >= k - 1)
    Y.check_retimed(yuv, fmt, _out(fmt), WIN, got, video, cropped, slots, 8, upto=first)
    assert all(np.array_equal(got[i], plain[i]) for i in range(first, len(got)))
    assert (64, 96) in model.shapes and (128, 96) in model.shapes


def test_a_dropped_duplicate_is_examined_too():
    fmt, kw = FORMATS["i420"]
    video = Y.letterboxed_yuv(yuv, fmt, L5)
    dup = video[2].copy()
    fmt.planes(dup)[0][5, 7] = 60                                              # a repeat of frame 2 but for one bar sample above the code 36
    video = video[:3] + [dup] + video[3:]
    area, dd = active.ActiveArea(probe=2), rt.Duplicates(cell=2.0, peak=60)
    got = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60, levels=3, pixfmt=fmt, active=area, dedup=dd, **KW))
    plain = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60, levels=3, pixfmt=fmt, dedup=rt.Duplicates(cell=2.0, peak=60), **KW))
    assert dd.dropped == [3] and area.fallback_at == 2 and len(got) == len(plain)      # the widened segment 2 ends at frame 4
    slots = list(rt.retime_slots([0, 1, 2, 4, 5], 24, 60, 3))
    first = min(i for i, (j, p) in enumerate(slots) if j >= 2)
    assert all(np.array_equal(got[i], plain[i]) for i in range(first, len(got)))
    assert not all(np.array_equal(got[i], plain[i]) for i in range(first))


def test_windows_that_gain_nothing_are_the_plain_loops():
    fmt, kw = FORMATS["i420"]
    full = Y.letterboxed_yuv(yuv, fmt, C.cpu_scene.shot(5, H, W, seed=4, tone=150))
    boxed = Y.letterboxed_yuv(yuv, fmt, L5)
    for video, d, shape in ((full, 16, (128, 96)), (boxed, 128, (128, 128))):  # no bars; bars that gain nothing under divisor 128
        for loop, a in ((mf.interpolate_video_nx, dict(factor=4)), (lambda f, m, **k: rt.interpolate_video_retimed(f, m, 24, 60, levels=3, **k), {})):
            area, model = active.ActiveArea(), Mean()
            got = list(loop(iter(video), model, pixfmt=fmt, active=area, divisor=d, **a))
            plain = list(loop(iter(video), Mean(), pixfmt=fmt, divisor=d, **a))
            assert area.window == (0, 0, H, W) and area.fallback_at is None and len(got) == len(plain)
            assert all(np.array_equal(g, p) for g, p in zip(got, plain)) and set(model.shapes) == {shape}


def test_refusals():
    f8, f10 = yuv.Format(H, W), yuv.Format(H, W, depth=10)
    v8, v10 = Y.letterboxed_yuv(yuv, f8, L5[:3]), Y.letterboxed_yuv(yuv, f10, L5[:3])
    retimed = lambda frames, **k: rt.interpolate_video_retimed(frames, Mean(), 24, 60, **k)
    for loop in (lambda frames, **k: mf.interpolate_video_nx(frames, Mean(), **k), retimed):
        with pytest.raises(ValueError, match="keep_depth=True"):
            list(loop(iter(v10), pixfmt=f10, active=active.ActiveArea()))
        with pytest.raises(ValueError, match="crop"):
            list(loop(iter(v8), pixfmt=f8, active=active.ActiveArea(), crop=(64, 64)))
        with pytest.raises(ValueError, match=r"pixfmt expects frames of the format, got uint8 \(128, 96, 3\)"):
            list(loop(iter(L5), pixfmt=f8, active=WIN))
        assert list(loop(iter([]), pixfmt=f8, active=active.ActiveArea())) == []
    with pytest.raises(ValueError, match="shutter"):
        list(retimed(iter(v8), pixfmt=f8, active=active.ActiveArea(), shutter=180))
    with pytest.raises(ValueError, match="shutter"):
        list(retimed(iter(L5), active=WIN, shutter=180))


# ------------------------------------------------------------------------------------------------ ABI
def test_yuv_active_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(C.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    assert re.search(r"\bint\s+atmvfi_yuv_borders\s*\(", hdr) and re.search(r"\bint64_t\s+atmvfi_yuv_borders_workspace_ints\s*\(", hdr)
    assert re.search(r"\bint\s+atmvfi_yuv_compose\s*\(", hdr)
    for name in ("atmvfi_yuv_borders", "atmvfi_yuv_borders_workspace_ints", "atmvfi_yuv_compose"):
        assert name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert (lib.atmvfi_version() >> 8) & 255 >= 29
    for name in ("yuv_borders", "yuv_borders_workspace", "yuv_compose"):
        assert callable(getattr(hip_ops.HipOps, name))
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err, ws_ints = lib.atmvfi_last_error, lib.atmvfi_yuv_borders_workspace_ints

    def borders(src=P, H=64, W=96, depth=8, msb=0, pitch=0, out=P, ws=P, n=None):
        n = max(ws_ints(H, W), 0) if n is None else n
        return lib.atmvfi_yuv_borders(ctypes.byref(hip_ops.YuvDesc(H=H, W=W, depth=depth, msb=msb, pitch=pitch)), src, out, ws, n, None)
    assert borders(src=None) == -1 and b"null pointer" in err()
    assert borders(out=None) == -1 and b"null pointer" in err()
    assert borders(ws=None) == -1 and b"null pointer" in err()
    assert borders(H=15) == -1 and b"at least 16 x 16" in err()
    assert borders(W=15) == -1 and b"at least 16 x 16" in err()
    assert borders(H=60000, W=60000, n=1 << 40) == -1 and b"too large" in err()
    assert borders(depth=12) == -1 and b"depth must be 8 or 10" in err()
    assert borders(msb=1) == -1 and b"needs depth 10" in err()
    assert borders(pitch=95) == -1 and b"pitch" in err()
    assert borders(depth=10, pitch=193) == -1 and b"pitch" in err()
    assert borders(out=P + 2) == -1 and b"4-byte aligned" in err()
    assert borders(n=ws_ints(64, 96) - 1) == -1 and b"workspace of" in err()
    # the 8-bit partials of frame_borders plus a second word per group of four columns and chunk
    assert ws_ints(64, 96) == 4 * 64 + 2 * 8 * 24 and ws_ints(2160, 4096) == 16 * 2160 + 2 * 270 * 1024
    assert ws_ints(15, 96) == -1 and b"at least 16 x 16" in err()

    def compose(dst=P, border=4 * P, H=64, W=96, depth=8, matrix=0, fr=0, siting=0, sub=0, chroma=0, msb=0, bp=0, bcp=0, bco=0, y0=8, x0=4,
                h=32, w=40, src=8 * P, Hp=64, Wp=64, pt=0, pl=0, u8=None):
        d = hip_ops.YuvDesc(H=H, W=W, depth=depth, matrix=matrix, full_range=fr, siting=siting, subsampling=sub, chroma=chroma, msb=msb, pitch=bp,
                            chroma_pitch=bcp, chroma_offset=bco)
        return lib.atmvfi_yuv_compose(ctypes.byref(d), dst, border, y0, x0, h, w, src, Hp, Wp, pt, pl, u8, None)
    assert compose(dst=None) == -1 and b"null pointer" in err()
    assert compose(border=None) == -1 and b"null pointer" in err()
    assert compose(u8=9 * P) == -1 and b"exactly one" in err()
    assert compose(src=None) == -1 and b"exactly one" in err()
    assert compose(matrix=2) == -1 and b"unknown matrix" in err()
    assert compose(depth=9) == -1 and b"depth must be 8 or 10" in err()
    assert compose(sub=3) == -1 and b"unknown subsampling" in err()
    assert compose(sub=1, chroma=1) == -1 and b"planar" in err()
    assert compose(msb=1) == -1 and b"msb needs depth 10" in err()
    assert compose(bp=95) == -1 and b"pitch" in err()
    assert compose(y0=40) == -1 and b"window outside the frame" in err()
    assert compose(h=0) == -1 and b"window outside the frame" in err()
    assert compose(y0=7) == -1 and b"subsampling step" in err()
    assert compose(x0=5) == -1 and b"subsampling step" in err()
    assert compose(h=31) == -1 and b"subsampling step" in err()
    assert compose(border=P) == -1 and b"must not overlap" in err()
    assert compose(border=P + 64 * 96 * 3 // 2 - 1) == -1 and b"must not overlap" in err()           # the last byte overlaps
    assert compose(border=P - 64 * 96 * 3 // 2 + 1) == -1 and b"must not overlap" in err()
    assert compose(Hp=31) == -1 and b"canvas" in err()
    assert compose(depth=10, src=None, u8=9 * P) == -1 and b"10-bit" in err()
