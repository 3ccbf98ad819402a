"""CPU: the active picture of letterboxed video (atm-vfi_amd/active.py, the ``active=`` argument of ``interpolate_video_nx``,
atmvfi_frame_borders / atmvfi_frame_compose) without a GPU: the host twins against the loop models, the policy's pure functions on
hand-made profiles, the ``peak`` default against the canvases of tests/golden/active_ref.npz with the margins it was placed with, the
ABI's host-side checks, and letterboxed videos through the generic path of the loop."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cpu_active as C

active = importlib.import_module("atm-vfi_amd.active")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")

MARGIN = 1.5          # the margin the default must keep to both sides (README "Active picture")


# ------------------------------------------------------------------------------------------------ twins
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W", [(16, 16), (18, 22), (33, 47), (40, 130)])
def test_borders_numpy_is_the_loop_model(H, W, bgr):
    rng = np.random.default_rng(H * 1000 + W)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frame[rng.integers(0, H, 5)] //= 16                        # some dark rows and columns: the maxima differ from line to line
    frame[:, rng.integers(0, W, 5)] //= 16
    got = active.borders_numpy(frame, bgr=bgr)
    assert got.dtype == np.int32 and got.shape == (H + W,)
    assert np.array_equal(got, C.borders_model(frame, bgr)) and np.array_equal(got, C.borders_model_pixels(frame, bgr))
    pure = np.zeros((H, W, 3), np.uint8)
    pure[3, 5] = (255, 0, 0)                                   # one pixel, byte 0 lit: luma 77 as RGB, 29 as BGR
    want = np.zeros(H + W, np.int32)
    want[3] = want[H + 5] = (29 * 255 + 128) >> 8 if bgr else (77 * 255 + 128) >> 8
    assert np.array_equal(active.borders_numpy(pure, bgr=bgr), want)


def test_borders_numpy_refusals():
    for bad in ((15, 40), (40, 15)):
        with pytest.raises(ValueError):
            active.borders_numpy(np.zeros(bad + (3,), np.uint8))
    with pytest.raises(ValueError):
        active.borders_numpy(np.zeros((16, 16, 3), np.float32))
    with pytest.raises(ValueError):
        active.borders_numpy(np.zeros((16, 16), np.uint8))


def _tie(k: int) -> np.float32:
    """an fp32 x whose fp32 product x * 255 is exactly k + 0.5"""
    x = np.float32((k + 0.5) / 255.0)
    for cand in (x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-1))):
        if np.float32(cand) * np.float32(255.0) == np.float32(k + 0.5):
            return np.float32(cand)
    raise AssertionError(k)


TIES = np.array([_tie(k) for k in range(255)], np.float32)


def _canvas_values(rng, shape):
    """fp32 values with exact .5 ties of x * 255, values outside [0, 1] and ordinary ones"""
    ties = TIES[rng.integers(0, 255, shape)]
    plain = rng.uniform(-0.3, 1.3, shape).astype(np.float32)
    pick = rng.integers(0, 3, shape)
    return np.where(pick == 0, ties, np.where(pick == 1, plain, rng.uniform(0, 1, shape).astype(np.float32))).astype(np.float32)


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,win,pad", [(3, 5, (1, 2, 1, 1), (0, 0)), (8, 12, (0, 0, 8, 12), (2, 3)), (9, 14, (0, 3, 4, 11), (1, 0)),
                                         (9, 14, (5, 0, 4, 7), (0, 5)), (10, 16, (3, 5, 5, 7), (3, 4)), (12, 16, (2, 4, 8, 8), (4, 4))])
def test_compose_numpy_is_the_loop_model(H, W, win, pad, bgr):
    rng = np.random.default_rng(H * 100 + W + win[0])
    border = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    h, w = win[2:]
    src = _canvas_values(rng, (3, h + pad[0] + 2, w + pad[1] + 3))
    got = active.compose_numpy(border, win, src=src, pad_top=pad[0], pad_left=pad[1], bgr=bgr)
    assert got.dtype == np.uint8 and np.array_equal(got, C.compose_model(border, win, src=src, pad_top=pad[0], pad_left=pad[1], bgr=bgr))
    inside = lambda f: f[win[0]:win[0] + h, win[1]:win[1] + w]
    rgb = active.compose_numpy(border, win, src=src, pad_top=pad[0], pad_left=pad[1])
    assert got is not border and np.array_equal(inside(got)[..., ::-1] if bgr else inside(got), inside(rgb))
    u8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = active.compose_numpy(border, win, win_u8=u8, bgr=bgr)                    # already in output order: bgr changes nothing
    assert np.array_equal(got, C.compose_model(border, win, win_u8=u8)) and np.array_equal(got[win[0]:win[0] + h, win[1]:win[1] + w], u8)


def test_compose_rounds_half_to_even_and_clamps():
    src = np.zeros((3, 1, 4), np.float32)
    src[:, 0] = TIES[[0, 1, 2, 254]]
    assert (src[0, 0] * np.float32(255.0)).tolist() == [0.5, 1.5, 2.5, 254.5]                 # exact ties in fp32
    got = active.compose_numpy(np.zeros((1, 4, 3), np.uint8), (0, 0, 1, 4), src=src)
    assert got[0, :, 0].tolist() == [0, 2, 2, 254]
    src[:, 0] = (-1.0, 1.0 + 2.0 ** -20, 7.0, -2.0 ** -30)
    assert active.compose_numpy(np.zeros((1, 4, 3), np.uint8), (0, 0, 1, 4), src=src)[0, :, 1].tolist() == [0, 255, 255, 0]
    with pytest.raises(ValueError):
        active.compose_numpy(np.zeros((4, 4, 3), np.uint8), (0, 0, 2, 2))                     # neither source
    with pytest.raises(ValueError):
        active.compose_numpy(np.zeros((4, 4, 3), np.uint8), (0, 0, 2, 2), src=np.zeros((3, 2, 2), np.float32), win_u8=np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ValueError):
        active.compose_numpy(np.zeros((4, 4, 3), np.uint8), (3, 0, 2, 2), win_u8=np.zeros((2, 2, 3), np.uint8))      # outside the frame
    with pytest.raises(ValueError):
        active.compose_numpy(np.zeros((4, 4, 3), np.uint8), (0, 0, 2, 2), src=np.zeros((3, 2, 2), np.float32), pad_left=1)


# ------------------------------------------------------------------------------------------------ policy
def profile(H, W, rows=None, cols=None, lit=200, dark=0):
    """line maxima of a frame whose rows ``rows[0] .. rows[1] - 1`` and columns ``cols[0] .. cols[1] - 1`` hold the picture"""
    r0, r1 = rows or (0, H)
    c0, c1 = cols or (0, W)
    p = np.full(H + W, dark, np.int32)
    p[r0:r1] = lit
    p[H + c0:H + c1] = lit
    return p


def test_rect_of_snaps_outward_to_even_and_ignores_dark_lines_inside():
    H, W = 100, 160
    assert active.rect_of(profile(H, W), H, W, 24) == (0, 0, H, W)
    assert active.rect_of(profile(H, W, rows=(10, 90)), H, W, 24) == (10, 0, 90, W)
    assert active.rect_of(profile(H, W, rows=(5, 97)), H, W, 24) == (4, 0, 98, W)                  # top 5 -> 4, bottom 3 -> 2
    assert active.rect_of(profile(H, W, rows=(1, 99), cols=(7, 151)), H, W, 24) == (0, 6, 100, 152)
    p = profile(H, W, rows=(10, 90))
    p[40:50] = 0                                                                                   # a dark band inside the picture
    p[H + 30] = 3
    assert active.rect_of(p, H, W, 24) == (10, 0, 90, W)
    # the threshold is inclusive: a line whose maximum is peak is a bar line, peak + 1 is picture
    assert active.rect_of(profile(H, W, rows=(10, 90), dark=24), H, W, 24) == (10, 0, 90, W)
    assert active.rect_of(profile(H, W, rows=(10, 90), dark=25), H, W, 24) == (0, 0, H, W)
    assert active.rect_of(profile(H, W, rows=(10, 90), lit=24), H, W, 24) == (100, 160, 0, 0)      # all bars: empty
    with pytest.raises(ValueError):
        active.rect_of(np.zeros(H + W + 1, np.int32), H, W, 24)


def test_undecided_frames():
    H, W = 100, 160
    assert active.decided((10, 0, 90, W), H, W) and active.decided((0, 0, 25, 40), H, W)
    assert not active.decided((0, 0, 24, W), H, W) and not active.decided((0, 0, H, 38), H, W)     # fewer than H / 4 rows, W / 4 columns
    assert not active.decided(active.rect_of(np.zeros(H + W, np.int32), H, W, 24), H, W)           # a black frame
    assert not active.decided((50, 0, 50, W), H, W) and not active.decided((60, 0, 40, W), H, W)


def test_lock_takes_the_union_and_applies_the_gain_rule():
    H, W = 1080, 1920
    whole = (0, 0, H, W)
    assert active.lock([], H, W, 64) == whole
    assert active.lock([(0, 0, 10, 10)], H, W, 64) == whole                                        # undecided rects do not count
    # bars of 4 rows: 1072 rows pad to 1088 as 1080 do -> nothing gained; bars of 138 rows: 804 rows pad to 832
    assert active.lock([active.rect_of(profile(H, W, rows=(4, 1076)), H, W, 24)], H, W, 64) == whole
    assert active.lock([active.rect_of(profile(H, W, rows=(138, 942)), H, W, 24)], H, W, 64) == (138, 0, 804, 1920)
    assert active.padded_area(804, 1920, 64) == 832 * 1920 and active.padded_area(1080, 1920, 64) == 1088 * 1920
    # the union of two rects, a third undecided one left out
    assert active.lock([(140, 0, 940, 1920), (138, 20, 900, 1900), (500, 500, 510, 510)], H, W, 64) == (138, 0, 802, 1920)
    assert active.lock([(138, 0, 942, 1920), (0, 240, 1080, 1680)], H, W, 64) == whole             # letterbox + pillarbox: the whole frame
    # no padding: the area itself decides, and the sides must be multiples of what the network needs
    assert active.lock([(138, 0, 942, 1920)], H, W, None, 1) == (138, 0, 804, 1920)
    assert active.lock([(138, 0, 942, 1920)], H, W, None, 16) == whole
    assert active.lock([(140, 0, 940, 1920)], H, W, None, 16) == (140, 0, 800, 1920)
    # divisor 16: 1080 rows pad to 1088, and so do 1076; 1072 stay
    assert active.lock([(2, 0, 1078, 1920)], H, W, 16) == whole and active.lock([(4, 0, 1076, 1920)], H, W, 16) == (4, 0, 1072, 1920)


def test_violates():
    H, W = 100, 160
    win = (10, 20, 80, 120)
    inside = profile(H, W, rows=(10, 90), cols=(20, 140))
    assert not active.violates(inside, win, H, W, 24)
    assert not active.violates(np.zeros(H + W, np.int32), win, H, W, 24)                           # a black frame violates nothing
    for at in (9, 90, H + 19, H + 140):
        p = inside.copy()
        p[at] = 25
        assert active.violates(p, win, H, W, 24), at
        p[at] = 24
        assert not active.violates(p, win, H, W, 24), at
    assert not active.violates(np.full(H + W, 255, np.int32), (0, 0, H, W), H, W, 24)              # nothing lies outside the whole frame
    with pytest.raises(ValueError):
        active.violates(np.zeros(3, np.int32), win, H, W, 24)


def test_fixed_window_and_policy_arguments():
    assert active.fixed_window((2, 4, 10, 20), 16, 32) == (2, 4, 10, 20)
    for bad in ((1, 4, 10, 20), (2, 4, 9, 20), (2, 4, 16, 20), (-2, 4, 10, 20), (2, 4, 10), "abcd", (2, 14, 10, 20)):
        with pytest.raises(ValueError):
            active.fixed_window(bad, 16, 32)
    a = active.ActiveArea()
    assert (a.peak, a.probe, a.patience) == (active.DEFAULT_PEAK, 8, 48) and a.window is None and a.fallback_at is None and a.stats == []
    for kw in (dict(peak=-1), dict(peak=256), dict(probe=0), dict(patience=0)):
        with pytest.raises(ValueError):
            active.ActiveArea(**kw)


def test_probe_stream_stops_at_probe_patience_or_the_end():
    H, W = 64, 48
    lit, black = np.full((H, W, 3), 0, np.uint8), np.zeros((H, W, 3), np.uint8)
    lit[16:48] = 200
    prof = lambda f: active.borders_numpy(f, bgr=False)
    a = active.ActiveArea(probe=3, patience=10)
    held = a.probe_stream(iter([lit] * 20), H, W, 16, 16, 1, prof)
    assert len(held) == 3 and a.probed == 3 and a.window == (16, 0, 32, 48) and len(a.stats) == 3
    a.begin()
    held = a.probe_stream(iter([black] * 20), H, W, 16, 16, 1, prof)                                # never decided: patience ends it
    assert len(held) == 10 and a.probed == 10 and a.window == (0, 0, H, W)
    a.begin()
    held = a.probe_stream(iter([black] * 4 + [lit] * 20), H, W, 16, 16, 1, prof)
    assert len(held) == 7 and a.window == (16, 0, 32, 48)
    a.begin()
    held = a.probe_stream(iter([black, lit]), H, W, 16, 16, 1, prof)                                # the stream ends first
    assert len(held) == 2 and a.probed == 2 and a.window == (16, 0, 32, 48)
    a.begin()
    wide = lit.copy()
    wide[10:16] = 90
    held = a.probe_stream(iter([lit, black, wide, black, lit, lit]), H, W, 16, 16, 2, prof)         # step 2: frames 0, 2, 4 are examined
    assert len(held) == 5 and len(a.stats) == 3 and a.window == (10, 0, 38, 48)
    with pytest.raises(ValueError):
        a.probe_stream(iter([lit[:32]]), H, W, 16, 16, 1, prof)


# ------------------------------------------------------------------------------------------------ the default
def test_default_peak_keeps_its_margins_on_the_fixture():
    assert os.path.getsize(C.ACTIVE_REF) < (1 << 20)
    canv = C.decoded_canvases()
    assert len(canv) == 5 * len(C.BLACKS) * len(C.QUALITIES) and all(c.shape == (380, 281, 3) and c.dtype == np.uint8 for c in canv.values())
    bars, content = C.fixture_statistics()
    for (label, b), (_, c) in zip(bars, content):
        print("%-44s bar maximum %3d   smallest content-edge maximum %3d" % (label, b, c))
    bar_max, content_min = max(b for _, b in bars), min(c for _, c in content)
    peak = active.ActiveArea().peak
    print(f"peak {peak}: {peak / bar_max:.3f} x the bars' {bar_max}, the content's {content_min} is {content_min / peak:.3f} x peak")
    assert peak == active.DEFAULT_PEAK
    assert peak >= MARGIN * bar_max
    assert peak <= content_min / MARGIN
    # and the policy finds every canvas's picture to within the 8 lines JPEG ringing may take, never less than the picture
    for (name, black, q), c in canv.items():
        H, W = c.shape[:2]
        y0, x0, y1, x1 = active.rect_of(active.borders_numpy(c, bgr=False), H, W, peak)
        assert C.BAR_ROWS - C.KEEP <= y0 <= C.BAR_ROWS + C.KEEP and C.BAR_COLS - C.KEEP <= x0 <= C.BAR_COLS + C.KEEP, (name, black, q)
        assert H - C.BAR_ROWS - C.KEEP <= y1 <= H - C.BAR_ROWS + C.KEEP and W - C.BAR_COLS - C.KEEP <= x1 <= W - C.BAR_COLS + C.KEEP


# ------------------------------------------------------------------------------------------------ the loop, generic path
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend: the pair mean, recording the frame sizes it is asked for."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.shapes = []

    def forward(self, a, b):
        self.shapes.append(tuple(a.shape[-2:]))
        return {"I_t": (a + b) / 2}


H, W, ROWS = 64, 48, (16, 48)
WIN = (16, 0, 32, 48)
L, PIC = C.letterboxed(6, H, W, ROWS, seed=1)
KW = dict(divisor=16)                     # 32 rows pad to 32 against 64: the window gains; under 64 it would not


def _check_windowed(got, video, alone, factor, win=WIN, first_segment=0, segments=None):
    """``got``: the frames of segments ``first_segment ...`` of the letterboxed ``video``; ``alone``: the loop's frames on the pictures"""
    y0, x0, h, w = win
    n_seg = len(video) - 1 if segments is None else segments
    for s in range(first_segment, first_segment + n_seg):
        for k in range(factor):
            g = got[(s - first_segment) * factor + k]
            if k == 0:
                assert g is video[s], (s, k)
                continue
            assert g.dtype == np.uint8 and g.shape == video[s].shape
            assert np.array_equal(g[y0:y0 + h, x0:x0 + w], alone[s * factor + k]), (s, k)
            bars = video[s] if k <= factor // 2 else video[s + 1]
            mask = np.ones(g.shape[:2], bool)
            mask[y0:y0 + h, x0:x0 + w] = False
            assert np.array_equal(g[mask], bars[mask]), (s, k)


@pytest.mark.parametrize("factor", [2, 4, 8])
@pytest.mark.parametrize("kw", [dict(), dict(tta=True), dict(isBGR=False)], ids=lambda k: "-".join(k) or "plain")
def test_letterboxed_video_through_the_generic_path(factor, kw):
    model, area = Mean(), active.ActiveArea()
    got = list(mf.interpolate_video_nx(iter(L), model, factor=factor, active=area, **KW, **kw))
    alone = list(mf.interpolate_video_nx(iter(PIC), Mean(), factor=factor, **KW, **kw))
    assert len(got) == len(alone) == 5 * factor + 1 and got[-1] is L[-1]
    _check_windowed(got, L, alone, factor)
    assert area.window == WIN and area.probed == 6 and area.fallback_at is None and len(area.stats) == 6 + 6
    assert set(model.shapes) == {(32, 48)}                                     # the forwards ran on the window
    # the record is per run
    list(mf.interpolate_video_nx(iter(L[:3]), Mean(), factor=factor, active=area, **KW, **kw))
    assert area.probed == 3 and len(area.stats) == 6


def test_a_lit_pixel_in_a_bar_sends_the_loop_back_to_the_whole_frame():
    factor, k = 4, 3
    video = [f.copy() for f in L]
    video[k][5, 7] = 255                                                       # frame 3, inside the top bar
    area = active.ActiveArea(probe=2)
    model = Mean()
    got = list(mf.interpolate_video_nx(iter(video), model, factor=factor, active=area, **KW))
    assert area.window == WIN and area.probed == 2 and area.fallback_at == k - 1
    alone = list(mf.interpolate_video_nx(iter(PIC), Mean(), factor=factor, **KW))
    plain = list(mf.interpolate_video_nx(iter(video), Mean(), factor=factor, **KW))
    _check_windowed(got[:(k - 1) * factor], video, alone, factor, segments=k - 1)
    at = (k - 1) * factor
    assert len(got) == len(plain)
    for i in range(at, len(got)):
        assert np.array_equal(got[i], plain[i]), i
    assert not np.array_equal(got[at - 1], plain[at - 1])                      # (the bars of a windowed frame are an original's)
    per = len(mf.nx_levels(factor))                                            # forward calls per segment: one batch per level
    assert model.shapes[:per * (k - 1)] == [(32, 48)] * per * (k - 1) and set(model.shapes[per * (k - 1):]) == {(64, 48)}
    # with scene= the cut segments are watched too: the cut at segment 2 is also where the violating frame arrives
    other, _ = C.letterboxed(3, H, W, ROWS, seed=9, tone=60, span=20)
    video = L[:3] + other
    video[3] = video[3].copy()
    video[3][60, 2] = 255
    area, sc = active.ActiveArea(probe=2), scene.SceneCuts()
    got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=factor, active=area, scene=sc, **KW))
    plain = list(mf.interpolate_video_nx(iter(video), Mean(), factor=factor, scene=scene.SceneCuts(), **KW))
    assert sc.cuts == [2] and area.fallback_at == 2
    for i in range(2 * factor, len(got)):
        assert np.array_equal(got[i], plain[i]), i


def test_black_frames_first_still_lock_the_window():
    black = [np.zeros((H, W, 3), np.uint8) for _ in range(3)]
    video = black + L
    area = active.ActiveArea()
    got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=2, active=area, **KW))
    alone = list(mf.interpolate_video_nx(iter([b[16:48] for b in black] + PIC), Mean(), factor=2, **KW))
    assert area.window == WIN and area.fallback_at is None
    _check_windowed(got, video, alone, 2)


def test_no_bars_or_no_gain_is_the_plain_loop():
    full = C.cpu_scene.shot(5, H, W, seed=4, tone=150)
    for video, kw in ((full, KW), (L, dict(divisor=64))):                      # no bars; bars that gain nothing under divisor 64
        area, model = active.ActiveArea(), Mean()
        got = list(mf.interpolate_video_nx(iter(video), model, factor=4, active=area, **kw))
        plain = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, **kw))
        assert area.window == (0, 0, H, W) and area.fallback_at is None and len(got) == len(plain)
        assert all(np.array_equal(g, p) for g, p in zip(got, plain)) and all(got[4 * i] is video[i] for i in range(len(video)))
        assert set(model.shapes) == {(64, 48) if kw["divisor"] == 16 else (64, 64)}


def test_time_interval_examines_the_uploaded_frames_only():
    video = [f.copy() for f in L[:5]]
    video[1][2, 2] = video[3][2, 2] = 255                                      # frames the stride drops: never looked at
    area = active.ActiveArea(probe=2)
    got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=2, time_interval=2, active=area, **KW))
    assert area.window == WIN and area.fallback_at is None and len(got) == 5 and area.probed == 3
    alone = list(mf.interpolate_video_nx(iter(PIC[:5]), Mean(), factor=2, time_interval=2, **KW))
    assert np.array_equal(got[1][16:48], alone[1]) and np.array_equal(got[1][:16], video[0][:16])


def test_fixed_window_scene_cuts_and_refusals():
    # a fixed window: never probed, never checked -- a lit bar pixel changes nothing
    video = [f.copy() for f in L]
    video[2][1, 1] = 255
    got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, active=WIN, **KW))
    _check_windowed(got, video, list(mf.interpolate_video_nx(iter(PIC), Mean(), factor=4, **KW)), 4)
    with pytest.raises(ValueError, match="even"):
        list(mf.interpolate_video_nx(iter(L), Mean(), active=(15, 0, 32, 48), **KW))
    with pytest.raises(ValueError, match="outside"):
        list(mf.interpolate_video_nx(iter(L), Mean(), active=(40, 0, 32, 48), **KW))
    # scene cuts work on the whole frame and yield copies of the originals
    other, other_pic = C.letterboxed(4, H, W, ROWS, seed=7, tone=60, span=20)
    area, sc = active.ActiveArea(), scene.SceneCuts()
    video = L[:4] + other
    got = list(mf.interpolate_video_nx(iter(video), Mean(), factor=4, active=area, scene=sc, **KW))
    assert sc.cuts == [3] and area.window == WIN and area.fallback_at is None
    alone = list(mf.interpolate_video_nx(iter(PIC[:4] + other_pic), Mean(), factor=4, scene=scene.SceneCuts(), **KW))
    _check_windowed(got[:12], video, alone, 4, segments=3)
    assert [np.array_equal(got[12 + k], video[3 if k <= 2 else 4]) for k in range(4)] == [True] * 4
    _check_windowed(got[16:], video, alone, 4, first_segment=4, segments=3)
    # refusals
    with pytest.raises(ValueError, match="crop"):
        list(mf.interpolate_video_nx(iter(L), Mean(), active=active.ActiveArea(), crop=(32, 32)))
    yuv = importlib.import_module("atm-vfi_amd.yuv")
    with pytest.raises(ValueError, match="pixfmt"):
        list(mf.interpolate_video_nx(iter(L), Mean(), active=WIN, pixfmt=yuv.Format(H, W)))
    assert list(mf.interpolate_video_nx(iter([]), Mean(), active=active.ActiveArea())) == []
    p = inspect.signature(mf.interpolate_video_nx).parameters
    assert "active" in p and p["active"].default is None
    assert host_io.ActiveArea is active.ActiveArea and host_io.borders_numpy is active.borders_numpy and host_io.compose_numpy is active.compose_numpy


def test_video_nx_passes_active_through():
    class Cap:
        def __init__(self):
            self.i, self.open = 0, True

        def get(self, prop):
            return {host_io.CAP_PROP_FPS: 25.0, host_io.CAP_PROP_FRAME_WIDTH: float(W), host_io.CAP_PROP_FRAME_HEIGHT: float(H)}[prop]

        def isOpened(self):
            return self.open

        def read(self):
            self.i += 1
            return (True, L[self.i - 1]) if self.i <= len(L) else (False, None)

        def release(self):
            self.open = False

    class Sink:
        def __init__(self):
            self.got = []

        def write(self, f):
            self.got.append(f.copy())

        def release(self):
            pass
    sink, area = Sink(), active.ActiveArea()
    info = host_io.video_nx(Cap(), lambda fps, size: sink, Mean(), factor=4, active=area, **KW)
    assert info == {"fps_in": 25, "fps_out": 100, "size": (W, H), "frames_in": 6, "frames_out": 21} and area.window == WIN
    want = list(mf.interpolate_video_nx(iter(L), Mean(), factor=4, active=active.ActiveArea(), **KW))
    assert all(np.array_equal(g, w) for g, w in zip(sink.got, want))


# ------------------------------------------------------------------------------------------------ ABI
def test_active_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(C.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    assert re.search(r"\bint\s+atmvfi_frame_borders\s*\(", hdr) and re.search(r"\bint64_t\s+atmvfi_frame_borders_workspace_ints\s*\(", hdr)
    assert re.search(r"\bint\s+atmvfi_frame_compose\s*\(", hdr)
    for name in ("atmvfi_frame_borders", "atmvfi_frame_borders_workspace_ints", "atmvfi_frame_compose"):
        assert name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert lib.atmvfi_plan_fn_id(b"atmvfi_frame_borders") >= 0 and lib.atmvfi_plan_fn_id(b"atmvfi_frame_compose") >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 21
    assert "active.hip" in open(os.path.join(C.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    for name in ("frame_borders", "frame_borders_workspace", "frame_compose"):
        assert callable(getattr(hip_ops.HipOps, name))
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error
    ws_ints = lib.atmvfi_frame_borders_workspace_ints

    def borders(src=P, H=64, W=96, bgr=0, out=P, ws=P, n=None):
        n = max(ws_ints(H, W), 0) if n is None else n
        return lib.atmvfi_frame_borders(src, H, W, bgr, out, ws, n, None)
    assert borders(src=None) == -1 and b"null pointer" in err()
    assert borders(out=None) == -1 and b"null pointer" in err()
    assert borders(ws=None) == -1 and b"null pointer" in err()
    assert borders(H=15) == -1 and b"at least 16 x 16" in err()
    assert borders(W=15) == -1 and b"at least 16 x 16" in err()
    assert borders(H=-64) == -1 and b"at least 16 x 16" in err()
    assert borders(H=60000, W=60000, n=1 << 40) == -1 and b"too large" in err()                      # 3.6e9 pixels
    assert borders(H=100000000, W=17, n=1 << 40) == -1 and b"too large" in err()                     # H * W fits; 390 625 row chunks do not
    assert borders(out=P + 2) == -1 and b"4-byte aligned" in err()
    assert borders(ws=P + 1) == -1 and b"4-byte aligned" in err()
    assert borders(n=ws_ints(64, 96) - 1) == -1 and b"workspace of" in err()
    # the workspace query: H words per wave that sees a row (4 per column tile) + W / 4 words per row chunk; -1 for a frame the call refuses
    assert ws_ints(64, 96) == 4 * 64 + 8 * 24 and ws_ints(1080, 1920) == 8 * 1080 + 135 * 480 and ws_ints(2160, 4096) == 16 * 2160 + 270 * 1024
    assert ws_ints(18, 22) == 4 * 18 + 3 * 6
    assert ws_ints(15, 96) == -1 and b"at least 16 x 16" in err()
    assert ws_ints(60000, 60000) == -1

    def compose(dst=P, border=2 * P, H=64, W=96, y0=8, x0=4, h=32, w=40, src=3 * P, Hp=64, Wp=64, pt=0, pl=0, win=None, bgr=0):
        return lib.atmvfi_frame_compose(dst, border, H, W, y0, x0, h, w, src, Hp, Wp, pt, pl, win, bgr, None)
    assert compose(dst=None) == -1 and b"null pointer" in err()
    assert compose(border=None) == -1 and b"null pointer" in err()
    assert compose(win=4 * P) == -1 and b"exactly one" in err()
    assert compose(src=None) == -1 and b"exactly one" in err()
    assert compose(y0=40) == -1 and b"window outside the frame" in err()
    assert compose(x0=-4) == -1 and b"window outside the frame" in err()
    assert compose(h=0) == -1 and b"window outside the frame" in err()
    assert compose(w=97, x0=0) == -1 and b"window outside the frame" in err()
    assert compose(border=P) == -1 and b"must not alias" in err()
    assert compose(border=P + 3 * 64 * 96 - 1) == -1 and b"must not alias" in err()                  # the last byte overlaps
    assert compose(border=P - 3 * 64 * 96 + 1) == -1 and b"must not alias" in err()
    assert compose(Hp=31) == -1 and b"bad geometry" in err()
    assert compose(Wp=40, pl=1) == -1 and b"bad geometry" in err()
    assert compose(pt=-1) == -1 and b"bad geometry" in err()
    assert compose(H=1 << 16, W=1 << 17, h=32, w=40) == -1 and b"too large" in err()
