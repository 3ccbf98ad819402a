"""CPU: frame-rate conversion (atm-vfi_amd/retime.py) without a GPU: the timeline and the sparse schedule against the table of README
"Frame-rate conversion", the host difference against the pixel-loop model of tests/cpu_framediff.py, the duplicate policy and its
default thresholds against tests/golden/dedup_ref.npz with the margins they were placed with, the whole loop through the generic path
with a toy model, the adapters, and the ABI's host-side checks."""
import ctypes
import importlib
import inspect
import io
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cpu_framediff as D
import cpu_scene as C

rt = importlib.import_module("atm-vfi_amd.retime")
mf = importlib.import_module("atm-vfi_amd.multiframe")
scene = importlib.import_module("atm-vfi_amd.scene")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")

MARGIN = 1.5          # the margin the defaults must keep to both sets (README "Frame-rate conversion")


# ------------------------------------------------------------------------------------------------ timeline and schedule
def tally(fps_in, fps_out, levels, kept=range(25)):
    """(outputs, interpolated, forwards without TTA, the slots) of a conversion"""
    slots, n = list(rt.retime_slots(kept, fps_in, fps_out, levels)), 1 << levels
    per_segment = {}
    for j, p in slots:
        if 0 < p < n:
            per_segment.setdefault(j, set()).add(p)
    forwards = sum(len(lv) for ps in per_segment.values() for lv in rt.sparse_levels(sorted(ps), levels))
    return len(slots), sum(0 < p < n for _, p in slots), forwards, slots


TABLE = [      # fps_in, fps_out, levels -> outputs, interpolated, forwards, the first slots (25 source frames)
    (24, 60, 3, 61, 48, 96, [(0, 0), (0, 3), (0, 6), (1, 2), (1, 5), (2, 0), (2, 3), (2, 6)]),
    (25, 60, 3, 58, 53, 110, [(0, 0), (0, 3), (0, 7), (1, 2), (1, 5), (2, 1), (2, 4), (2, 7)]),
    (Fraction(30000, 1001), 60, 3, 49, 24, 24, [(0, 0), (0, 4), (0, 8), (1, 4), (1, 8)]),
    ("30000/1001", "60", 3, 49, 24, 24, [(0, 0), (0, 4), (0, 8), (1, 4), (1, 8)]),
    (24, 60, 4, 61, 48, 144, [(0, 0), (0, 6), (0, 13), (1, 3), (1, 10)]),
    (24, 120, 3, 121, 96, 120, [(0, 0), (0, 2), (0, 3), (0, 5), (0, 6), (1, 0)]),
    (60, 24, 3, 10, 5, 5, [(0, 0), (2, 4), (5, 0), (7, 4)]),
    (24, 48, 3, 49, 24, 24, [(0, 0), (0, 4), (1, 0)]),
    (30, 60, 1, 49, 24, 24, [(0, 0), (0, 1), (1, 0)]),
]


@pytest.mark.parametrize("fi,fo,levels,outputs,interpolated,forwards,head", TABLE, ids=lambda v: str(v).replace(" ", "")[:24])
def test_the_schedule_table(fi, fo, levels, outputs, interpolated, forwards, head):
    n_out, n_int, n_fwd, slots = tally(fi, fo, levels)
    assert (n_out, n_int, n_fwd) == (outputs, interpolated, forwards)
    assert slots[:len(head)] == head
    n = 1 << levels
    assert all(0 <= p <= n and 0 <= j < 24 for j, p in slots)
    if (24 * Fraction(fo) / Fraction(fi)).denominator == 1:          # an output falls on the last frame
        assert slots[-1] == (23, n)
    assert slots == sorted(slots)                                     # time order; no position repeats in a span-1 segment
    assert len(set(slots)) == len(slots)
    # the definition, output by output, and the documented timing error
    fi, fo = Fraction(fi), Fraction(fo)
    for m, (j, p) in enumerate(slots):
        u = m * fi / fo
        assert j <= u <= j + 1 and abs((j + Fraction(p, n)) - u) <= Fraction(1, 2 * n)
    assert (len(slots)) / fo > 24 / fi                                # the next output would lie behind the last frame


def test_timelines_with_dropped_frames():
    assert list(rt.retime_slots([0, 2, 4, 6], 24, 24, 3)) == [(0, 0), (0, 4), (1, 0), (1, 4), (2, 0), (2, 4), (2, 8)]
    assert list(rt.retime_slots([0, 3, 6], 24, 24, 3)) == [(0, 0), (0, 3), (0, 5), (1, 0), (1, 3), (1, 5), (1, 8)]
    # a widened segment can map two outputs to one position (g = 2, 24 -> 120: ten outputs on eight positions)
    slots = list(rt.retime_slots([0, 2], 24, 120, 3))
    assert [p for _, p in slots] == [0, 1, 2, 2, 3, 4, 5, 6, 6, 7, 8] and {j for j, _ in slots} == {0}
    assert list(rt.retime_slots([0], 24, 60, 3)) == [(0, 0)] and list(rt.retime_slots([], 24, 60, 3)) == []
    assert list(rt.retime_slots(range(3), 24, 24, 2)) == [(0, 0), (1, 0), (1, 4)]        # the same rate: the frames


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_sparse_levels_of_everything_is_the_full_recursion(levels):
    n = 1 << levels
    assert rt.sparse_levels(range(1, n), levels) == mf.nx_levels(n)
    assert rt.sparse_levels(range(0, n + 1), levels) == mf.nx_levels(n)          # 0 and N need nothing
    assert rt.sparse_levels([], levels) == [[] for _ in range(levels)]


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 6])
def test_sparse_levels_are_closed(levels):
    n = 1 << levels
    rng = np.random.default_rng(levels)
    subsets = [[p] for p in range(1, n)] + [sorted(set(rng.integers(1, n, 3).tolist())) for _ in range(8)]
    for want in subsets:
        lv = rt.sparse_levels(want, levels)
        assert len(lv) == levels
        have = {0, n}
        for li, level in enumerate(lv):
            assert level == sorted(level, key=lambda t: t[2])
            for left, right, out in level:
                half = out & -out
                assert (left, right) == (out - half, out + half) and li + 1 == levels - (half.bit_length() - 1)
                assert left in have and right in have, (want, out)     # parents: 0, N or outputs of an EARLIER level
            have |= {o for _, _, o in level}
        made = have - {0, n}
        assert set(want) <= made
        # nothing but ancestors: every node is wanted or a parent of another node
        parents = {x for level in lv for l, r, _ in level for x in (l, r)}
        assert made <= set(want) | parents
    assert rt.sparse_levels([3, 6], 3) == [[(0, 8, 4)], [(0, 4, 2), (4, 8, 6)], [(2, 4, 3)]]
    assert rt.sparse_levels([4], 3) == [[(0, 8, 4)], [], []]
    assert rt.sparse_levels([5], 3) == [[(0, 8, 4)], [(4, 8, 6)], [(4, 6, 5)]]


def test_refusals():
    for bad in (dict(fps_in=0), dict(fps_in=-24), dict(fps_out=0), dict(fps_out=Fraction(-1, 2)), dict(levels=0), dict(levels=7),
                dict(levels=2.0), dict(levels=True), dict(fps_in=24, fps_out=60, levels=1), dict(fps_in=1, fps_out=9, levels=3),
                dict(fps_in=29.97), dict(fps_out="fast"), dict(fps_out=None)):
        kw = dict(dict(fps_in=24, fps_out=60, levels=3), **bad)
        with pytest.raises(ValueError):
            rt.retime_slots(range(5), **kw)
        with pytest.raises(ValueError):
            rt.interpolate_video_retimed(iter([]), Mean(), **kw)
    list(rt.retime_slots(range(5), 1, 8, 3))                         # 2**levels * fps_in == fps_out is allowed
    list(rt.retime_slots(range(5), 24.0, 60, 3))                     # a whole-number float is exact
    for kept in ([1, 2], [0, 2, 2], [0, 3, 1]):
        with pytest.raises(ValueError):
            list(rt.retime_slots(kept, 24, 60, 3))
    for bad in ([9], [-1], [1.5]):
        with pytest.raises(ValueError):
            rt.sparse_levels(bad, 3)
    with pytest.raises(ValueError):
        rt.sparse_levels([1], 7)


def test_retime_slots_streams():
    asked = []

    def kept():
        for k in range(6):
            asked.append(k)
            yield k
    seen = []
    for j, p in rt.retime_slots(kept(), 24, 60, 3):
        seen.append((j, p))
        assert max(asked) <= j + 1, (j, p, asked)                     # output m comes before kept[j + 2] is requested
    assert seen == list(rt.retime_slots(range(6), 24, 60, 3)) and asked == list(range(6))


# ------------------------------------------------------------------------------------------------ the difference
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,win", [(16, 16, None), (40, 52, (3, 5, 33, 47)), (33, 47, None), (17, 130, None)])
def test_difference_numpy_is_the_loop_model(H, W, win, bgr):
    rng = np.random.default_rng(H * 1000 + W)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = np.where(rng.random((H, W, 1)) < 0.3, a, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).astype(np.uint8)
    y0, x0, h, w = win or (0, 0, H, W)
    want = D.difference_model(a, b, y0, x0, h, w, bgr)
    got = rt.difference_numpy(a, b, win, bgr=bgr)
    assert got.dtype == np.int32 and got.shape == (258,) and np.array_equal(got, want)
    assert np.array_equal(rt.difference_numpy(b, a, win, bgr=bgr), want)                  # symmetric
    assert np.array_equal(D.difference_fast(a, b, y0, x0, h, w, bgr), want)               # the yardstick of the large GPU cases
    assert 0 < want[257] < h * w and want[:256].sum() >= want[257] and want[256] <= 255
    assert not np.array_equal(got, rt.difference_numpy(a, b, win, bgr=not bgr))           # the channel order matters
    assert not rt.difference_numpy(a, a, win, bgr=bgr).any()


def test_difference_closed_forms_and_refusals():
    a = np.zeros((32, 64, 3), np.uint8)
    b = a.copy()
    b[5, 9] = (0, 255, 0)                                             # luma (150 * 255 + 128) >> 8 = 149, in cell (2, 2)
    d = rt.difference_numpy(a, b)
    assert d[16 * 2 + 2] == 149 and d[:256].sum() == 149 and d[256] == 149 and d[257] == 1
    assert rt.duplicate_statistics(d, 32, 64) == (149 / 8, 149)       # a cell of a 32 x 64 window has 2 x 4 pixels
    white = np.full_like(a, 255)
    d = rt.difference_numpy(a, white)
    assert np.all(d[:256] == 255 * 8) and d[256] == 255 and d[257] == 32 * 64
    assert rt.duplicate_statistics(d, 32, 64) == (255.0, 255)
    for bad in (lambda: rt.difference_numpy(a[:15], b[:15]), lambda: rt.difference_numpy(a, b[:, :40]),
                lambda: rt.difference_numpy(a, b, (0, 40, 32, 32)), lambda: rt.difference_numpy(a.astype(np.float32), b),
                lambda: rt.duplicate_statistics(np.zeros(288), 32, 64)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the policy
def words(d_cell_num=0, peak=0):
    """a difference of a 16 x 16 window (one pixel per cell) with the given largest cell SAD and peak"""
    d = np.zeros(258, np.int32)
    d[7], d[256], d[257] = d_cell_num, peak, int(d_cell_num > 0)
    return d


def test_duplicates_drop_rule():
    dd = rt.Duplicates(cell=9.0, peak=40, max_run=3)
    assert (dd.cell, dd.peak, dd.max_run) == (rt.DEFAULT_CELL, rt.DEFAULT_PEAK, 3) == (9.0, 40, 3)
    dup, moved = words(), words(100, 100)
    # frames 1..8: d d d d m d m d -- max_run: the fourth duplicate in a row is kept, and the run starts again behind it
    drops = [dd.judge(x, 16, 16) for x in (dup, dup, dup, dup, moved, dup, moved, dup)]
    assert drops == [True, True, True, False, False, True, False, True]
    assert dd.dropped == [1, 2, 3, 6, 8] and len(dd.stats) == 8 and dd.stats[0] == (0.0, 0) and dd.stats[4] == (100.0, 100)
    # the last frame of the stream is kept: the frame held back as a duplicate comes back
    assert dd.finish() is True and dd.dropped == [1, 2, 3, 6]
    assert dd.finish() is False and dd.dropped == [1, 2, 3, 6]
    dd.begin()
    assert dd.dropped == [] and dd.stats == []
    assert [dd.judge(x, 16, 16) for x in (dup, moved)] == [True, False] and dd.finish() is False and dd.dropped == [1]
    # both tests must pass; the bounds are inclusive
    edge = rt.Duplicates(cell=9.0, peak=40)
    assert edge.is_duplicate(9.0, 40) and not edge.is_duplicate(9.01, 40) and not edge.is_duplicate(9.0, 41)
    assert edge.judge(words(9, 40), 16, 16) and not edge.judge(words(10, 10), 16, 16) and not edge.judge(words(1, 41), 16, 16)
    never = rt.Duplicates(max_run=0)
    assert [never.judge(dup, 16, 16) for _ in range(3)] == [False] * 3 and never.dropped == []


def _stats(a, b):
    return rt.duplicate_statistics(D.difference_model(a, b, bgr=False), *a.shape[:2])


@pytest.fixture(scope="module")
def fixture_statistics():
    """(duplicates, motion): lists of (label, d_cell, d_peak) on the pictures of scene_ref.npz / dedup_ref.npz, by the loop model."""
    return ([(label,) + _stats(a, b) for label, a, b in D.duplicate_pairs()], [(label,) + _stats(a, b) for label, a, b in D.motion_pairs()])


def test_default_thresholds_keep_their_margins_on_the_fixture(fixture_statistics):
    assert os.path.getsize(D.DEDUP_REF) < (1 << 20)
    P, R = C.pictures(), D.reencodes()
    assert len(R) == 2 * len(P) == 10 and all(r.dtype == np.uint8 and r.shape == (300, 207, 3) for r in R.values())
    dups, moves = fixture_statistics
    assert len(dups) == 25 and len(moves) == 5
    for row in dups + moves:
        print("%-48s d_cell %7.3f  d_peak %3d" % row)
    pair = _stats(P["frame0"], P["frame1"])
    print("%-48s d_cell %7.3f  d_peak %3d" % (("frame0 / frame1",) + pair))
    dd = rt.Duplicates()
    for label, dc, dp in dups:
        assert dd.is_duplicate(dc, dp), label
    for label, dc, dp in moves + [("frame0 / frame1",) + pair]:
        assert not dd.is_duplicate(dc, dp), label
        assert dc > dd.cell and dp > dd.peak, label                    # either test alone tells motion
    assert dd.cell >= MARGIN * max(dc for _, dc, _ in dups) and dd.cell <= min(dc for _, dc, _ in moves) / MARGIN
    assert dd.peak >= MARGIN * max(dp for _, _, dp in dups) and dd.peak <= min(dp for _, _, dp in moves) / MARGIN
    # the statistics the README quotes
    assert round(max(dc for _, dc, _ in dups), 2) == 2.99 and max(dp for _, _, dp in dups) == 16
    assert round(min(dc for _, dc, _ in moves), 2) == 29.27 and min(dp for _, _, dp in moves) == 110
    assert round(pair[0], 1) == 181.8 and pair[1] == 237
    # the policy's stated limit: a small low-contrast change passes both tests
    f = P["frame0"]
    g = f.copy()
    g[100:108, 100:108] = np.clip(g[100:108, 100:108].astype(np.int64) + 40, 0, 255)
    assert dd.is_duplicate(*_stats(f, g))


# ------------------------------------------------------------------------------------------------ the loop, generic path
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend: the pair mean, counting the pairs it is asked for."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.pairs = 0

    def forward(self, a, b):
        self.pairs += a.shape[0]
        return {"I_t": (a + b) / 2}


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k


H, W = 24, 40
VIDEO = C.shot(5, H, W, seed=1, tone=60)
# five pictures that are no duplicates of each other (the shot above drifts so gently that its neighbours ARE within the duplicate set)
MOVING = [C.shot(1, H, W, seed=20 + k, tone=tone)[0] for k, tone in enumerate((40, 90, 140, 190, 230))]


@pytest.mark.parametrize("kw", [dict(), dict(crop=(16, 32)), dict(tta=True), dict(max_batch=1)], ids=lambda k: "-".join(k) or "plain")
def test_four_times_the_rate_is_interpolate_video_nx(kw):
    model, report = Mean(), {}
    got = list(rt.interpolate_video_retimed(iter(VIDEO), model, 6, 24, levels=2, report=report, **kw))
    _same(got, list(mf.interpolate_video_nx(iter(VIDEO), Mean(), factor=4, **kw)))
    t = 2 if kw.get("tta") else 1
    assert model.pairs == 4 * 3 * t and report == {"outputs": 17, "interpolated": 12, "forwards": 12}
    if "crop" not in kw:
        assert all(got[4 * i] is VIDEO[i] for i in range(5))          # originals are the caller's own arrays


def test_the_same_rate_yields_the_input_and_runs_no_forward():
    model = Mean()
    got = list(rt.interpolate_video_retimed(iter(VIDEO), model, 25, 25, levels=3))
    assert len(got) == 5 and all(g is f for g, f in zip(got, VIDEO)) and model.pairs == 0
    assert list(rt.interpolate_video_retimed(iter([]), model, 25, 25)) == []
    one = list(rt.interpolate_video_retimed(iter(VIDEO[:1]), model, 24, 60, dedup=rt.Duplicates(), scene=scene.SceneCuts()))
    assert len(one) == 1 and one[0] is VIDEO[0] and model.pairs == 0


def test_24_to_60_evaluates_only_what_it_shows():
    model, report = Mean(), {}
    got = list(rt.interpolate_video_retimed(iter(VIDEO), model, 24, 60, levels=3, report=report))
    full = list(mf.interpolate_video_nx(iter(VIDEO), Mean(), factor=8))
    slots = list(rt.retime_slots(range(5), 24, 60, 3))
    assert len(got) == len(slots) == 11
    _same(got, [full[8 * j + p] for j, p in slots])
    assert model.pairs == report["forwards"] == 2 * report["interpolated"] == 16
    # downwards: two of five frames are shown, one midpoint between them
    model = Mean()
    got = list(rt.interpolate_video_retimed(iter(VIDEO), model, 60, 24, levels=3))
    assert list(rt.retime_slots(range(5), 60, 24, 3)) == [(0, 0), (2, 4)] and model.pairs == 1
    _same(got, [VIDEO[0], full[8 * 2 + 4]])


@pytest.mark.parametrize("crop", [None, (16, 32)])
def test_duplicates_are_dropped_and_their_segments_widen(crop):
    A, B, Cc = MOVING[:3]
    video = [A, D.primed(A, 1), B, D.primed(B, 2), Cc]
    model, dd = Mean(), rt.Duplicates()
    got = list(rt.interpolate_video_retimed(iter(video), model, 24, 24, levels=3, dedup=dd, crop=crop))
    assert dd.dropped == [1, 3] and len(dd.stats) == 4 and len(got) == 5 and model.pairs == 2
    y0, x0, h, w = mf.centre_window(H, W, crop)
    assert dd.stats == [rt.duplicate_statistics(D.difference_model(video[i - 1], video[i], y0, x0, h, w, True), h, w) for i in range(1, 5)]
    want = list(mf.interpolate_video_nx(iter([A, B, Cc]), Mean(), factor=2, crop=crop))          # A mid B mid C
    _same(got, want)
    # the same frames as the loop on A B C at half the rate
    _same(got, list(rt.interpolate_video_retimed(iter([A, B, Cc]), Mean(), 12, 24, levels=3, crop=crop)))
    # a trailing duplicate is the last frame: kept (held back until the stream ends behind it)
    dd2 = rt.Duplicates()
    tail = list(rt.interpolate_video_retimed(iter(video[:4]), Mean(), 24, 24, dedup=dd2))
    assert dd2.dropped == [1] and len(tail) == 4 and tail[3] is video[3] and tail[2] is video[2]
    # max_run: of four copies in a row only three go
    run = [A] + [D.primed(A, k) for k in range(4)] + [B]
    dd3 = rt.Duplicates(max_run=3)
    out = list(rt.interpolate_video_retimed(iter(run), Mean(), 24, 24, dedup=dd3))
    assert dd3.dropped == [1, 2, 3] and len(out) == 6 and out[4] is run[4] and out[5] is run[5]
    # widened to g = 2 at 24 -> 120: two outputs of one position -- the second a copy of the same frame, not the same array
    dd4, model = rt.Duplicates(), Mean()
    wide = list(rt.interpolate_video_retimed(iter([A, D.primed(A, 1), B]), model, 24, 120, levels=3, dedup=dd4))
    slots = list(rt.retime_slots([0, 2], 24, 120, 3))
    assert dd4.dropped == [1] and len(wide) == len(slots) == 11 and model.pairs == 7
    twice = [k for k in range(1, 11) if slots[k] == slots[k - 1]]
    assert twice == [3, 8] and all(np.array_equal(wide[k], wide[k - 1]) and wide[k] is not wide[k - 1] for k in twice)
    full = list(mf.interpolate_video_nx(iter([A, B]), Mean(), factor=8))
    _same(wide, [full[p] for _, p in slots])
    # without dedup nothing is compared or dropped
    plain = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 24))
    assert all(g is f for g, f in zip(plain, video))


def test_a_cut_segment_is_filled_with_copies():
    A, B = C.shot(3, H, W, seed=1, tone=60), C.shot(3, H, W, seed=2, tone=190)
    model, sc = Mean(), scene.SceneCuts()
    got = list(rt.interpolate_video_retimed(iter(A + B), model, 24, 60, levels=3, scene=sc))
    slots = list(rt.retime_slots(range(6), 24, 60, 3))
    assert sc.cuts == [2] and len(sc.stats) == 5 and len(got) == len(slots) == 13
    free = list(rt.interpolate_video_retimed(iter(A + B), Mean(), 24, 60, levels=3))
    video = A + B
    for k, (j, p) in enumerate(slots):
        if j != 2 or p in (0, 8):
            assert np.array_equal(got[k], free[k]), k
        else:
            src = video[2] if p <= 4 else video[3]
            assert np.array_equal(got[k], src) and got[k] is not src, k
    cut_nodes = sum(len(lv) for lv in rt.sparse_levels([p for j, p in slots if j == 2], 3))
    assert model.pairs == 2 * 10 - cut_nodes and cut_nodes > 0


def test_i420_frames_through_the_generic_path():
    fmt = yuv.Format(H, W)
    video = [yuv.encode_numpy(f, fmt) for f in VIDEO]
    got = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60, levels=3, pixfmt=fmt))
    full = list(mf.interpolate_video_nx(iter(video), Mean(), factor=8, pixfmt=fmt))
    slots = list(rt.retime_slots(range(5), 24, 60, 3))
    _same(got, [full[8 * j + p] for j, p in slots])
    assert got[0] is video[0] and got[5] is video[2]
    dd = rt.Duplicates()
    dup = [video[0], video[0].copy(), video[2]]
    out = list(rt.interpolate_video_retimed(iter(dup), Mean(), 24, 24, dedup=dd, pixfmt=fmt))
    assert dd.dropped == [1] and dd.stats[0] == (0.0, 0) and len(out) == 3 and out[0] is dup[0] and out[2] is dup[2]
    _same(out[1:2], list(mf.interpolate_video_nx(iter([video[0], video[2]]), Mean(), factor=2, pixfmt=fmt))[1:2])
    fmt10 = yuv.Format(H, W, depth=10)
    v10 = [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt10) for f in VIDEO[:3]]
    deep = list(rt.interpolate_video_retimed(iter(v10), Mean(), 24, 60, levels=3, pixfmt=fmt10, keep_depth=True))
    full = list(mf.interpolate_video_nx(iter(v10), Mean(), factor=8, pixfmt=fmt10, keep_depth=True))
    _same(deep, [full[8 * j + p] for j, p in rt.retime_slots(range(3), 24, 60, 3)])
    assert all(f.dtype == np.uint16 for f in deep)


# ------------------------------------------------------------------------------------------------ adapters
def test_video_retimed_and_interpolate_y4m():
    video = [MOVING[0], D.primed(MOVING[0], 1), MOVING[2], MOVING[3], MOVING[4]]

    class Cap:
        def __init__(self):
            self.i, self.open = 0, True

        def get(self, prop):
            return {host_io.CAP_PROP_FPS: 24.0, host_io.CAP_PROP_FRAME_WIDTH: float(W), host_io.CAP_PROP_FRAME_HEIGHT: float(H)}[prop]

        def isOpened(self):
            return self.open

        def read(self):
            self.i += 1
            return (True, video[self.i - 1]) if self.i <= len(video) else (False, None)

        def release(self):
            self.open = False

    class Sink:
        def __init__(self):
            self.got, self.opened = [], None

        def write(self, f):
            self.got.append(f.copy())

        def release(self):
            pass

    def run(fps_out, **kw):
        sink = Sink()

        def make(fps, size):
            sink.opened = (fps, size)
            return sink
        return host_io.video_retimed(Cap(), make, Mean(), fps_out, **kw), sink
    info, sink = run(60)
    assert info == {"fps_in": 24, "fps_out": 60, "size": (W, H), "frames_in": 5, "frames_out": 11, "forwards": 16}
    assert sink.opened == (60, (W, H))
    _same(sink.got, list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60)))
    dd, sc = rt.Duplicates(), scene.SceneCuts(hist=2.0)               # d_hist <= 1: never a cut
    info, sink = run("60000/1001", dedup=dd, scene=sc, levels=4, crop=(16, 32))
    assert info["dropped"] == [1] and info["cuts"] == [] and info["size"] == (32, 16) and info["fps_out"] == pytest.approx(59.94, abs=0.01)
    assert "dropped" not in run(60)[0] and "cuts" not in run(60)[0]
    assert info["frames_out"] == len(list(rt.retime_slots([0, 2, 3, 4], 24, Fraction(60000, 1001), 4))) == len(sink.got)
    with pytest.raises(ValueError):
        run(60, levels=1)

    # Y4M: the header carries exactly the requested rate; fps_out=None is the path of before
    fmt = yuv.Format(H, W)
    src = io.BytesIO()
    wr = yuv.Y4MWriter(src, fmt, Fraction(24000, 1001))
    frames = [yuv.encode_numpy(f, fmt) for f in VIDEO]
    for f in frames:
        wr.write(f)
    wr.close()
    data = src.getvalue()
    dst = io.BytesIO()
    info = yuv.interpolate_y4m(io.BytesIO(data), dst, Mean(), fps_out="60000/1001", levels=3)
    assert info["fps_in"] == Fraction(24000, 1001) and info["fps_out"] == Fraction(60000, 1001) and info["frames_in"] == 5
    assert info["frames_out"] == 11 and info["forwards"] == 16 and "dropped" not in info
    rd = yuv.Y4MReader(io.BytesIO(dst.getvalue()))
    assert rd.fps == Fraction(60000, 1001)
    _same(list(rd), list(rt.interpolate_video_retimed(iter(frames), Mean(), 24, 60, pixfmt=fmt)))
    info = yuv.interpolate_y4m(io.BytesIO(data), io.BytesIO(), Mean(), fps_out=24, dedup=rt.Duplicates(max_run=0))
    assert info["dropped"] == [] and info["frames_out"] == 5 and info["fps_out"] == 24 and info["forwards"] == 0    # 24000/1001 -> 24: every output rounds to an original
    dd = rt.Duplicates()                                             # this shot drifts within the duplicate set: runs of three go
    info = yuv.interpolate_y4m(io.BytesIO(data), io.BytesIO(), Mean(), fps_out=24, dedup=dd)
    assert info["dropped"] == dd.dropped == [1, 2, 3] and info["frames_out"] == 5
    plain, again = io.BytesIO(), io.BytesIO()
    a = yuv.interpolate_y4m(io.BytesIO(data), plain, Mean(), factor=2)
    b = yuv.interpolate_y4m(io.BytesIO(data), again, Mean(), factor=2, fps_out=None)
    assert a == b and plain.getvalue() == again.getvalue() and "forwards" not in a


def test_arguments_and_exports():
    p = inspect.signature(rt.interpolate_video_retimed).parameters
    assert list(p)[:4] == ["frames", "model", "fps_in", "fps_out"] and "time_interval" not in p
    want = dict(levels=3, dedup=None, crop=None, isBGR=True, divisor=64, tta=False, max_batch=4, pool=True, scene=None, pixfmt=None,
                keep_depth=False)
    assert {k: p[k].default for k in want} == want
    for mod in (host_io, yuv):
        assert mod.interpolate_video_retimed is rt.interpolate_video_retimed and mod.Duplicates is rt.Duplicates
    assert host_io.video_retimed is rt.video_retimed and host_io.retime_slots is rt.retime_slots and host_io.sparse_levels is rt.sparse_levels
    q = inspect.signature(yuv.interpolate_y4m).parameters
    assert q["fps_out"].default is None and q["levels"].default == 3 and q["dedup"].default is None
    # the loops of before know nothing of this
    for fn in (host_io.interpolate_video_2x, host_io.FramePipeline.__init__, mf.interpolate_video_nx, host_io.interpolate_video_2x_distributed):
        assert not {"dedup", "fps_out", "levels"} & set(inspect.signature(fn).parameters), fn
    assert inspect.signature(mf._SegmentRunner.run).parameters["levels"].default is None
    assert inspect.signature(mf._Uploader.__init__).parameters["difference"].default is None


# ------------------------------------------------------------------------------------------------ ABI
def test_frame_difference_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(C.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    assert re.search(r"\bint\s+atmvfi_frame_difference\s*\(", hdr) and re.search(r"\bint64_t\s+atmvfi_frame_difference_workspace_ints\s*\(", hdr)
    for name in ("atmvfi_frame_difference", "atmvfi_frame_difference_workspace_ints"):
        assert name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert (lib.atmvfi_version() >> 8) & 255 >= 16
    assert "framediff.hip" in open(os.path.join(C.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert callable(getattr(hip_ops.HipOps, "frame_difference")) and callable(getattr(hip_ops.HipOps, "frame_difference_workspace"))
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error
    ws_ints = lib.atmvfi_frame_difference_workspace_ints

    def call(a=P, b=P, H=64, W=96, bgr=0, y0=0, x0=0, h=64, w=96, out=P, ws=P, n=None):
        n = max(ws_ints(h, w), 0) if n is None else n
        return lib.atmvfi_frame_difference(a, b, H, W, bgr, y0, x0, h, w, out, ws, n, None)
    # the refusals of atmvfi_frame_signature
    for null in ("a", "b", "out", "ws"):
        assert call(**{null: None}) == -1 and b"null pointer" in err()
    assert call(y0=1) == -1 and b"window outside the frame" in err()
    assert call(x0=1) == -1 and b"window outside the frame" in err()
    assert call(x0=-1, w=90) == -1 and b"window outside the frame" in err()
    assert call(H=0) == -1 and b"window outside the frame" in err()
    assert call(h=15) == -1 and b"at least 16 x 16" in err()
    assert call(w=15) == -1 and b"at least 16 x 16" in err()
    assert call(H=60000, W=60000, h=60000, w=60000) == -1 and b"too large" in err()
    assert call(H=100000000, W=17, h=100000000, w=17) == -1 and b"too large" in err()
    assert call(out=P + 2) == -1 and b"4-byte aligned" in err()
    assert call(n=ws_ints(64, 96) - 1) == -1 and b"workspace of" in err()
    # the workspace query: 18 words per workgroup, 16 cell rows x column tiles x row chunks; -1 for a window the call refuses
    assert ws_ints(64, 96) == 18 * 16 and ws_ints(1080, 1920) == 18 * 16 * 2 * 9 and ws_ints(2160, 4096) == 18 * 16 * 4 * 17
    assert ws_ints(15, 96) == -1 and b"at least 16 x 16" in err()
    assert ws_ints(60000, 60000) == -1
