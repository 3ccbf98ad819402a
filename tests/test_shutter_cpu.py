"""CPU: the synthetic shutter (atm-vfi_amd/shutter.py; ``interpolate_video_retimed(shutter=)``) without a GPU: the light tables against
their float64 derivation, ``blend_numpy`` and ``shutter_slots`` against the loop model of tests/cpu_shutter.py and the table of README
"Synthetic shutter", the whole loop through the generic path with a toy model against ``blend_numpy`` of the N-x run's frames, and the
ABI's host-side checks."""
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
import cpu_shutter as S

sh = importlib.import_module("atm-vfi_amd.shutter")
rt = importlib.import_module("atm-vfi_amd.retime")
mf = importlib.import_module("atm-vfi_amd.multiframe")
scene = importlib.import_module("atm-vfi_amd.scene")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")

LIGHTS = ("code", "linear")


# ------------------------------------------------------------------------------------------------ tables and arithmetic
def test_the_literal_tables_are_the_float64_derivation():
    assert set(sh.SHUTTER_TABLES) == set(LIGHTS) and sh.LIGHTS == LIGHTS
    for light in LIGHTS:
        assert list(sh.SHUTTER_TABLES[light]) == S.derived_table(light), light
    lin = sh.SHUTTER_TABLES["linear"]
    assert list(lin[:6]) == [0, 20, 40, 60, 80, 99] and lin[-1] == 65535
    assert min(b - a for a, b in zip(lin, lin[1:])) == 19              # strictly increasing
    assert S.tie_margin() > 1.6e-3                                     # no 65535 eotf near a rounding tie: the literals are not fragile


def test_the_kernel_files_literals_are_the_derivation():
    src = open(os.path.join(C.ROOT, "atm-vfi_amd", "csrc", "shutter.hip")).read()
    for light, name in (("code", "SHUTTER_LUT_CODE"), ("linear", "SHUTTER_LUT_LINEAR")):
        body = re.search(r"#define " + name + r" \\\n((?:.*\\\n)*.*)\n", src).group(1)
        assert [int(v) for v in re.findall(r"\d+", body)] == S.derived_table(light), light
    assert re.search(r"kShutterLut\[2\]\[256\]\s*=\s*\{\{SHUTTER_LUT_CODE\},\s*\{SHUTTER_LUT_LINEAR\}\}", src)
    assert re.search(r"kShutterLutDev\[2\]\[256\]\s*=\s*\{\{SHUTTER_LUT_CODE\},\s*\{SHUTTER_LUT_LINEAR\}\}", src)


@pytest.mark.parametrize("light", LIGHTS)
def test_the_inverse_returns_every_code(light):
    lut = S.derived_table(light)
    assert [S.inverse_value(lut[q], lut) for q in range(256)] == list(range(256))
    assert S.inverse_table(lut)[:1] == [0] and S.inverse_table(lut)[65535] == 255
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(sh.blend_numpy([ramp], [1], light), ramp)
    assert np.array_equal(sh.blend_numpy([ramp, ramp, ramp], [3, 1, 2], light), ramp)


def test_the_mean_of_black_and_white():
    a, b = np.zeros((2, 3), np.uint8), np.full((2, 3), 255, np.uint8)
    assert (sh.blend_numpy([a, b], [1, 1], "linear") == 188).all() and (sh.blend_numpy([a, b], [1, 1], "code") == 128).all()
    assert (S.blend_model([a, b], [1, 1], "linear") == 188).all() and (S.blend_model([a, b], [1, 1], "code") == 128).all()


@pytest.mark.parametrize("light", LIGHTS)
@pytest.mark.parametrize("shape", [(7, 5, 3), (16, 16, 3)], ids=str)
def test_blend_numpy_is_the_loop_model(shape, light):
    rng = np.random.default_rng(sum(shape) + len(light))
    for count in (1, 2, 3, 5, 8, 13, 20):
        frames = [rng.integers(0, 256, shape).astype(np.uint8) for _ in range(count)]
        weights = [int(w) for w in rng.integers(1, 4, count)]
        got = sh.blend_numpy(frames, weights, light)
        assert got.dtype == np.uint8 and np.array_equal(got, S.blend_model(frames, weights, light)), (count, weights)


@pytest.mark.parametrize("light", LIGHTS)
def test_the_largest_total_weight_does_not_overflow(light):
    white = np.full((3, 4, 3), 255, np.uint8)
    assert (sh.blend_numpy([white] * 7, [4681] * 7, light) == 255).all()                         # 7 x 4681 = 32767
    assert (sh.blend_numpy([white, np.zeros_like(white)], [32766, 1], light) == 255).all()
    assert 65535 * sh.MAX_WEIGHT + (sh.MAX_WEIGHT >> 1) < 2 ** 31
    with pytest.raises(ValueError):
        sh.blend_numpy([white] * 2, [32767, 1], light)
    with pytest.raises(ValueError):
        sh.blend_numpy([white], [0], light)
    with pytest.raises(ValueError):
        sh.blend_numpy([white, white[:2]], [1, 1], light)
    with pytest.raises(ValueError):
        sh.blend_numpy([white], [1], "gamma")


# ------------------------------------------------------------------------------------------------ timeline
def tally(fi, fo, levels, angle, kept=range(25)):
    outs, n = list(sh.shutter_slots(kept, fi, fo, levels, sh.Shutter(angle))), 1 << levels
    per_segment = {}
    for _, _, samples in outs:
        for j, p, _ in samples:
            if 0 < p < n:
                per_segment.setdefault(j, set()).add(p)
    forwards = sum(len(lv) for ps in per_segment.values() for lv in rt.sparse_levels(sorted(ps), levels))
    sizes = [len(s) for _, _, s in outs]
    return len(outs), sum(sizes), min(sizes), max(sizes), forwards, outs


def span(j, lo, hi):
    return [(j, p) for p in range(lo, hi + 1)]


TABLE = [      # fps_in, fps_out, levels, angle -> outputs, samples, min / max per output, forwards, {m: sample set} (25 source frames)
    (60, 60, 3, 180, 25, 97, 2, 4, 120, {0: [(0, 0), (0, 1)], 1: [(0, 6), (0, 7), (1, 0), (1, 1)]}),
    (60, 60, 3, 360, 25, 193, 4, 8, 168, {1: span(0, 4, 7) + span(1, 0, 3)}),
    (60, 60, 3, 90, 25, 49, 1, 2, 72, {1: [(0, 7), (1, 0)]}),
    (60, 60, 3, 45, 25, 25, 1, 1, 0, {}),
    (60, 24, 2, 180, 10, 48, 3, 5, 33, {1: [(2, 0), (2, 1), (2, 2), (2, 3), (3, 0)]}),
    (60, 24, 3, 360, 10, 190, 10, 20, 167, {0: span(0, 0, 7) + [(1, 0), (1, 1)]}),
    (24, 60, 3, 180, 61, 97, 1, 2, 120, {0: [(0, 0)], 1: [(0, 3)], 2: [(0, 6), (0, 7)]}),
    (120, 30, 1, 360, 7, 49, 4, 8, 24, {1: [(2, 0), (2, 1), (3, 0), (3, 1), (4, 0), (4, 1), (5, 0), (5, 1)]}),
]


@pytest.mark.parametrize("fi,fo,levels,angle,outputs,samples,least,most,forwards,heads", TABLE, ids=lambda v: str(v).replace(" ", "")[:16])
def test_the_timeline_table(fi, fo, levels, angle, outputs, samples, least, most, forwards, heads):
    n_out, n_samples, lo, hi, n_fwd, outs = tally(fi, fo, levels, angle)
    assert (n_out, n_samples, lo, hi, n_fwd) == (outputs, samples, least, most, forwards)
    for m, want in heads.items():
        assert [(j, p) for j, p, _ in outs[m][2]] == want, m
    # the outputs are retime_slots' outputs, unchanged in number and position; every weight is the span
    assert [pos for _, pos, _ in outs] == list(rt.retime_slots(range(25), fi, fo, levels)) and [m for m, _, _ in outs] == list(range(n_out))
    assert all(w == 1 for _, _, s in outs for _, _, w in s)
    # and the whole of it is the brute-force model
    assert outs == S.slots_model(range(25), fi, fo, levels, angle)
    if angle == 45:                                                   # every output single: equals shutter=None
        assert all(s == [(j, p, 1)] for _, (j, p), s in outs)


def test_the_two_listed_cases():
    outs = list(sh.shutter_slots([0, 2, 3, 4], 24, 24, 2, sh.Shutter(360)))
    assert [s for _, _, s in outs] == [[(0, 0, 2)], [(0, 1, 2), (0, 2, 2)], [(0, 3, 2), (1, 0, 1), (1, 1, 1)],
                                       [(1, 2, 1), (1, 3, 1), (2, 0, 1), (2, 1, 1)], [(2, 2, 1), (2, 3, 1), (2, 4, 1)]]
    assert outs == S.slots_model([0, 2, 3, 4], 24, 24, 2, 360)
    cut = list(sh.shutter_slots(range(5), 24, 24, 2, 360, cuts=[1]))
    assert [(j, p) for j, p, _ in cut[1][2]] == [(0, 2), (0, 3), (1, 0), (1, 1)]
    assert [(j, p) for j, p, _ in cut[2][2]] == [(1, 3), (2, 0), (2, 1)]                  # output 2 belongs to the second shot
    assert cut == S.slots_model(range(5), 24, 24, 2, 360, cuts=[1])


@pytest.mark.parametrize("kept,fi,fo,levels,angle,cuts", [
    (range(9), 25, 60, 3, 360, ()), (range(9), 24, 60, 3, 7, ()), (range(9), 24, 60, 3, "22.5", ()), (range(12), 120, 30, 1, 360, (3,)),
    (range(12), 120, 30, 2, 360, (4, 5)), ([0, 1, 4, 5, 7, 8], 24, 60, 3, 270, (1,)), ([0, 3, 4, 8], 30, 24, 2, 360, (0, 2)),
    (range(8), 60, 24, 3, Fraction(355, 2), (2, 6)), ([0], 24, 60, 3, 180, ()), ([0, 1], 24, 24, 1, 360, (0,)), (range(7), 50, 60, 2, 1, ()),
], ids=lambda v: str(v).replace(" ", "")[:12])
def test_shutter_slots_is_the_brute_force_model(kept, fi, fo, levels, angle, cuts):
    assert list(sh.shutter_slots(kept, fi, fo, levels, sh.Shutter(angle), cuts=cuts)) == S.slots_model(kept, fi, fo, levels, angle, cuts)
    assert list(sh.shutter_slots(iter(kept), fi, fo, levels, angle, cuts=cuts)) == S.slots_model(kept, fi, fo, levels, angle, cuts)


@pytest.mark.parametrize("fi,fo", [(60, 60), (60, 24), (24, 60), (25, 60)])
def test_windows_are_disjoint_at_360_degrees(fi, fo):
    outs = list(sh.shutter_slots(range(25), fi, fo, 3, sh.Shutter(360)))
    seen = [(j, p) for _, _, s in outs for j, p, _ in s]
    assert len(seen) == len(set(seen))
    assert seen == sorted(seen)                                       # in time order, across outputs too
    if fo == fi:                                                      # 360 degrees at the same rate: no sample is left out
        assert len(seen) == 24 * 8 + 1                                # (downwards the samples behind the last output's window are)


def test_it_streams():
    """an output is yielded as soon as the last kept frame its window can reach has been read"""
    read = []

    def kept():
        for k in range(25):
            read.append(k)
            yield k
    it = sh.shutter_slots(kept(), 60, 60, 3, sh.Shutter(180))
    assert next(it)[0] == 0 and read == [0, 1]
    assert next(it)[0] == 1 and read == [0, 1, 2]


def test_refusals():
    for bad in (0, -1, 361, "360.5", 0.5, None, True, "x"):
        with pytest.raises(ValueError, match="angle"):
            sh.Shutter(bad)
    assert sh.Shutter(360).angle == 360 and sh.Shutter("22.5").angle == Fraction(45, 2) and sh.Shutter().light == "linear"
    assert sh.Shutter(Fraction(1, 1000)).angle == Fraction(1, 1000) and sh.Shutter(180.0).angle == 180
    with pytest.raises(ValueError, match="light"):
        sh.Shutter(180, "gamma")
    with pytest.raises(ValueError, match="angle"):
        list(sh.shutter_slots(range(3), 24, 24, 3, 400))
    # the total weight: named with rates, levels and angle, at the call
    with pytest.raises(ValueError, match=r"40000 -> 1 fps with 1 levels at 360 degrees"):
        sh.shutter_slots(range(3), 40000, 1, 1, sh.Shutter(360))
    with pytest.raises(ValueError, match=r"40000 -> 1 fps"):
        rt.interpolate_video_retimed(iter(VIDEO), Mean(), 40000, 1, levels=1, shutter=sh.Shutter(360))
    sh.shutter_slots(range(3), 16383, 1, 1, sh.Shutter(360))          # 32766 samples: allowed
    with pytest.raises(ValueError):
        sh.shutter_slots(range(3), 24, 60, 1, sh.Shutter(180))        # retime_slots' own refusals stay
    # a 10-bit blend is out of scope
    fmt10 = yuv.Format(H, W, depth=10)
    with pytest.raises(ValueError, match="10-bit"):
        rt.interpolate_video_retimed(iter([]), Mean(), 60, 60, pixfmt=fmt10, keep_depth=True, shutter=sh.Shutter(180))
    with pytest.raises(ValueError, match="angle"):
        rt.interpolate_video_retimed(iter(VIDEO), Mean(), 60, 60, shutter=0)
    with pytest.raises(ValueError, match="fps_out"):
        yuv.interpolate_y4m(io.BytesIO(b""), io.BytesIO(), Mean(), factor=2, shutter=sh.Shutter(180))


# ------------------------------------------------------------------------------------------------ the loop, generic path
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend (tests/test_yuv_cpu.py's stand-in): the pair mean, counting the pairs it is asked for."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.pairs = 0

    def forward(self, a, b):
        self.pairs += a.shape[0]
        return {"I_t": (a + b) / 2}


H, W = 24, 40
VIDEO = C.shot(5, H, W, seed=1, tone=60)          # a two-tone pattern that drifts
MOVING = [C.shot(1, H, W, seed=20 + k, tone=tone)[0] for k, tone in enumerate((40, 90, 140, 190, 230))]


def blurred(frames, fi, fo, levels, shutter, **kw):
    report, model = {}, Mean()
    got = list(rt.interpolate_video_retimed(iter(frames), model, fi, fo, levels=levels, shutter=shutter, report=report, **kw))
    return got, report, model


def check_against_the_nx_run(got, outs, sample_frame, light, encode=None):
    """every multi-sample output is blend_numpy of the frames at its samples; a single-sample one is that frame"""
    assert len(got) == len(outs)
    for g, (m, pos, samples) in zip(got, outs):
        frames = [sample_frame(j, p) for j, p, _ in samples]
        if len(samples) == 1:
            want = frames[0]
        else:
            want = sh.blend_numpy(frames, [w for _, _, w in samples], light)
            want = encode(want) if encode else want
        assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want), m


@pytest.mark.parametrize("fi,fo,levels,angle,light,kw", [
    (60, 60, 3, 180, "linear", {}), (60, 60, 3, 180, "code", {}), (60, 24, 2, 180, "linear", {}), (24, 60, 3, 180, "linear", {}),
    (120, 30, 1, 360, "linear", {}), (60, 60, 3, 360, "linear", dict(crop=(16, 32))), (60, 60, 2, 180, "linear", dict(tta=True)),
    (60, 60, 3, 180, "linear", dict(isBGR=False, max_batch=1)),
], ids=lambda v: str(v).replace(" ", "")[:14])
def test_blurred_outputs_are_blends_of_the_nx_runs_frames(fi, fo, levels, angle, light, kw):
    n = 1 << levels
    got, report, model = blurred(VIDEO, fi, fo, levels, sh.Shutter(angle, light), **kw)
    full = list(rt.interpolate_video_retimed(iter(VIDEO), Mean(), fi, n * fi, levels=levels, **kw))
    outs = list(sh.shutter_slots(range(5), fi, fo, levels, sh.Shutter(angle)))
    check_against_the_nx_run(got, outs, lambda j, p: full[n * j + p], light)
    need = {}
    for _, _, samples in outs:
        for j, p, _ in samples:
            if 0 < p < n:
                need.setdefault(j, set()).add(p)
    forwards = sum(len(lv) for ps in need.values() for lv in rt.sparse_levels(sorted(ps), levels))
    assert report == {"outputs": len(outs), "interpolated": sum(0 < p < n for _, (_, p), _ in outs), "forwards": forwards,
                      "blended": sum(len(s) > 1 for _, _, s in outs), "samples": sum(len(s) for _, _, s in outs)}
    assert model.pairs == forwards * (2 if kw.get("tta") else 1) and report["blended"] > 0
    if (fi, fo, levels, angle) == (60, 60, 3, 180):
        assert forwards == 5 * 4 and report["samples"] == 2 + 3 * 4 + 3


def test_single_sample_outputs_are_what_the_unblurred_loop_yields():
    plain = list(rt.interpolate_video_retimed(iter(VIDEO), Mean(), 60, 60, levels=3))
    got, report, model = blurred(VIDEO, 60, 60, 3, sh.Shutter(45))
    assert len(got) == 5 and all(g is f for g, f in zip(got, VIDEO)) and all(g is p for g, p in zip(got, plain))
    assert model.pairs == 0 and report == {"outputs": 5, "interpolated": 0, "forwards": 0, "blended": 0, "samples": 5}
    # upwards at a small angle: frame for frame the unblurred conversion, originals as the caller's own arrays
    plain = list(rt.interpolate_video_retimed(iter(VIDEO), Mean(), 24, 60, levels=3))
    got, report, model = blurred(VIDEO, 24, 60, 3, sh.Shutter(45))
    slots = list(rt.retime_slots(range(5), 24, 60, 3))
    assert report["blended"] == 0 and report["samples"] == len(slots) == len(got) and report["forwards"] == 16 == model.pairs
    for g, p, (j, pos) in zip(got, plain, slots):
        assert np.array_equal(g, p) and (g is VIDEO[j] if pos == 0 else True)
    # 24 -> 60 at 180 degrees mixes singles and pairs: the singles are the unblurred frames
    got, report, _ = blurred(VIDEO, 24, 60, 3, sh.Shutter(180))
    outs = list(sh.shutter_slots(range(5), 24, 60, 3, 180))
    for g, p, (_, pos, samples) in zip(got, plain, outs):
        if samples == [(pos[0], pos[1], 1)]:
            assert np.array_equal(g, p)
    assert got[0] is VIDEO[0] and report["blended"] == sum(len(s) > 1 for _, _, s in outs) > 0
    # a one-frame stream and an empty one
    assert list(rt.interpolate_video_retimed(iter([]), Mean(), 60, 60, shutter=180)) == []
    one = list(rt.interpolate_video_retimed(iter(VIDEO[:1]), Mean(), 60, 60, shutter=180, scene=scene.SceneCuts(), dedup=rt.Duplicates()))
    assert len(one) == 1 and one[0] is VIDEO[0]
    # a cropped original is its crop
    got, _, _ = blurred(VIDEO, 60, 60, 3, sh.Shutter(45), crop=(16, 32))
    y0, x0, h, w = mf.centre_window(H, W, (16, 32))
    assert all(np.array_equal(g, f[y0:y0 + h, x0:x0 + w]) for g, f in zip(got, VIDEO))


def test_dropped_duplicates_widen_the_segments_and_weigh_their_samples():
    A, B, Cc = MOVING[:3]
    video = [A, D.primed(A, 1), B, D.primed(B, 2), Cc]
    dd = rt.Duplicates()
    got, report, model = blurred(video, 24, 24, 2, sh.Shutter(360), dedup=dd)
    assert dd.dropped == [1, 3]
    outs = list(sh.shutter_slots([0, 2, 4], 24, 24, 2, 360))
    assert all(w == 2 for _, _, s in outs for _, _, w in s) and len(outs) == 5
    full = list(mf.interpolate_video_nx(iter([A, B, Cc]), Mean(), factor=4))
    check_against_the_nx_run(got, outs, lambda j, p: full[4 * j + p], "linear")
    assert got[0] is A and report["blended"] == 4 and model.pairs == 6
    # unequal spans: the samples of the widened segment count double
    video = [A, D.primed(A, 1), B, Cc]
    dd = rt.Duplicates()
    got, report, _ = blurred(video, 24, 24, 2, sh.Shutter(360), dedup=dd)
    outs = list(sh.shutter_slots([0, 2, 3], 24, 24, 2, 360))
    assert dd.dropped == [1] and outs[2][2] == [(0, 3, 2), (1, 0, 1), (1, 1, 1)]
    full = list(mf.interpolate_video_nx(iter([A, B, Cc]), Mean(), factor=4))
    check_against_the_nx_run(got, outs, lambda j, p: full[4 * j + p], "linear")


def shared_positions(kept, fi, fo, levels, angle):
    """the (segment, interior position) pairs that more than one output shows"""
    seen, twice = set(), set()
    for _, _, samples in sh.shutter_slots(kept, fi, fo, levels, angle):
        for j, p, _ in samples:
            if 0 < p < (1 << levels):
                (twice if (j, p) in seen else seen).add((j, p))
    return twice


@pytest.mark.parametrize("fi,fo,levels,angle,dups,kept", [
    (24, 60, 2, 180, (1, 0), [0, 2, 3]), (24, 60, 2, 360, (1, 0), [0, 2, 3]), (24, 60, 3, 180, (3, 0, 3), [0, 4, 5, 9]),
    (24, 60, 3, 45, (3, 0, 3), [0, 4, 5, 9]), (60, 60, 1, 180, (2, 0), [0, 3, 4]), (1, 8, 3, 90, (1, 0), [0, 2, 3]),
], ids=lambda v: str(v).replace(" ", "")[:12])
def test_a_widened_segment_shows_one_position_in_two_outputs(fi, fo, levels, angle, dups, kept):
    """Where dropped frames stretch a segment's positions further apart than the outputs, two outputs have one nearest position: one
    takes it through its window and the other as the position of an empty window, or both do.  Each gets the frame."""
    n = 1 << levels
    pictures = [C.shot(1, H, W, seed=40 + k, tone=tone)[0] for k, tone in enumerate((40, 100, 160, 220))][:len(dups) + 1]
    video = []
    for k, f in enumerate(pictures):
        video += [f] + [D.primed(f, 10 * k + r + 1) for r in range(dups[k] if k < len(dups) else 0)]
    assert shared_positions(kept, fi, fo, levels, angle)
    dd = rt.Duplicates()
    got, report, model = blurred(video, fi, fo, levels, sh.Shutter(angle), dedup=dd)
    assert [i for i in range(len(video)) if i not in dd.dropped] == kept
    outs = list(sh.shutter_slots(kept, fi, fo, levels, angle))
    assert outs == S.slots_model(kept, fi, fo, levels, angle)
    full = list(mf.interpolate_video_nx(iter(pictures), Mean(), factor=n))
    check_against_the_nx_run(got, outs, lambda j, p: full[n * j + p], "linear")
    plain = list(rt.interpolate_video_retimed(iter(video), Mean(), fi, fo, levels=levels, dedup=rt.Duplicates()))
    for g, p, (_, pos, samples) in zip(got, plain, outs):
        if [(j, q) for j, q, _ in samples] == [pos]:
            assert np.array_equal(g, p)                               # a single sample: the unblurred loop's frame


@pytest.mark.parametrize("fi,fo,levels", [(24, 24, 2), (24, 60, 3), (120, 30, 1)])
def test_no_output_mixes_the_two_shots_of_a_cut(fi, fo, levels):
    n = 1 << levels
    A, B = C.shot(3, H, W, seed=1, tone=60), C.shot(3, H, W, seed=2, tone=190)
    sc = scene.SceneCuts()
    got, report, model = blurred(A + B, fi, fo, levels, sh.Shutter(360), scene=sc)
    assert sc.cuts == [2]
    outs = list(sh.shutter_slots(range(6), fi, fo, levels, 360, cuts=sc.cuts))
    full = list(rt.interpolate_video_retimed(iter(A + B), Mean(), fi, n * fi, levels=levels, scene=scene.SceneCuts()))
    check_against_the_nx_run(got, outs, lambda j, p: full[n * j + p], "linear")
    first = lambda j, p: j < 2 or (j == 2 and 2 * p <= n)
    assert all(len({first(j, p) for j, p, _ in s}) == 1 for _, _, s in outs)
    if levels > 1:                                                    # the cut segment's copies take part, on their own side
        assert any(j == 2 and 0 < p < n for _, _, s in outs for j, p, _ in s)
    else:                                                             # N = 2: position 1 still shows the first frame, which output 1 leaves out
        assert [(j, p) for j, p, _ in outs[1][2]] == [(3, 0), (3, 1), (4, 0), (4, 1), (4, 2)] and outs[1][1] == (4, 0)
    # the cut segment runs no forward
    assert model.pairs == report["forwards"] == sum(len(lv) for j in range(5) if j != 2 for lv in rt.sparse_levels(
        sorted({p for _, _, s in outs for jj, p, _ in s if jj == j and 0 < p < n}), levels))


def test_i420_frames_through_the_generic_path():
    fmt = yuv.Format(H, W, "bt709", False, "left")
    video = [yuv.encode_numpy(f, fmt) for f in VIDEO]
    got, report, _ = blurred(video, 60, 60, 3, sh.Shutter(180), pixfmt=fmt)
    rgb = [yuv.decode_numpy(v, fmt) for v in video]
    full = list(rt.interpolate_video_retimed(iter(rgb), Mean(), 60, 480, levels=3, isBGR=False))
    outs = list(sh.shutter_slots(range(5), 60, 60, 3, 180))
    assert report["blended"] == 5
    check_against_the_nx_run(got, outs, lambda j, p: full[8 * j + p], "linear", encode=lambda f: yuv.encode_numpy(f, fmt))
    # at a small angle the originals are the caller's own bytes
    got, _, _ = blurred(video, 60, 60, 3, sh.Shutter(45), pixfmt=fmt)
    assert all(g is v for g, v in zip(got, video))
    # upwards at a small angle: produced single-sample outputs are the unblurred loop's bytes too
    got, report, _ = blurred(video, 24, 60, 3, sh.Shutter(45), pixfmt=fmt)
    plain = list(rt.interpolate_video_retimed(iter(video), Mean(), 24, 60, levels=3, pixfmt=fmt))
    assert report["blended"] == 0 and report["interpolated"] == 8 and len(got) == len(plain) == 11
    assert all(g.dtype == p.dtype and np.array_equal(g, p) for g, p in zip(got, plain))
    # 10-bit input without keep_depth: its 8-bit picture is blended
    fmt10 = yuv.Format(H, W, depth=10)
    v10 = [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt10) for f in VIDEO[:3]]
    got, _, _ = blurred(v10, 60, 60, 2, sh.Shutter(360), pixfmt=fmt10)
    rgb = [yuv.decode_numpy(v, fmt10) for v in v10]
    full = list(rt.interpolate_video_retimed(iter(rgb), Mean(), 60, 240, levels=2, isBGR=False))
    outs = list(sh.shutter_slots(range(3), 60, 60, 2, 360))
    assert all(len(s) > 1 for _, _, s in outs)
    check_against_the_nx_run(got, outs, lambda j, p: full[4 * j + p], "linear", encode=lambda f: yuv.encode_numpy(f, fmt10.as_8bit()))


def test_adapters_and_exports():
    p = inspect.signature(rt.interpolate_video_retimed).parameters
    assert list(p)[:4] == ["frames", "model", "fps_in", "fps_out"] and list(p)[-1] == "shutter" and p["shutter"].default is None
    for mod in (host_io, yuv):
        assert mod.Shutter is sh.Shutter and mod.shutter_slots is sh.shutter_slots and mod.blend_numpy is sh.blend_numpy
    assert inspect.signature(yuv.interpolate_y4m).parameters["shutter"].default is None
    run = inspect.signature(mf._SegmentRunner.run).parameters
    assert run["levels"].default is None and run["blend"].default is None
    for fn in (host_io.interpolate_video_2x, host_io.FramePipeline.__init__, mf.interpolate_video_nx, host_io.interpolate_video_2x_distributed):
        assert "shutter" not in inspect.signature(fn).parameters, fn
    tool = open(os.path.join(C.ROOT, "tools", "interp_y4m.py")).read()
    assert "--shutter" in tool and "--light" in tool

    # video_retimed hands the keyword on
    class Cap:
        def __init__(self):
            self.i = 0

        def get(self, prop):
            return {host_io.CAP_PROP_FPS: 60.0, host_io.CAP_PROP_FRAME_WIDTH: float(W), host_io.CAP_PROP_FRAME_HEIGHT: float(H)}[prop]

        def isOpened(self):
            return True

        def read(self):
            self.i += 1
            return (True, VIDEO[self.i - 1]) if self.i <= len(VIDEO) else (False, None)

        def release(self):
            pass

    class Sink:
        got = []

        def write(self, f):
            self.got.append(f.copy())

        def release(self):
            pass
    report = {}
    info = host_io.video_retimed(Cap(), lambda fps, size: Sink(), Mean(), 60, shutter=sh.Shutter(180), report=report)
    assert info["frames_out"] == 5 and info["forwards"] == 20 and report["blended"] == 5
    want, _, _ = blurred(VIDEO, 60, 60, 3, sh.Shutter(180))
    assert all(np.array_equal(g, w) for g, w in zip(Sink.got, want))
    # Y4M
    fmt = yuv.Format(H, W)
    src = io.BytesIO()
    wr = yuv.Y4MWriter(src, fmt, Fraction(60))
    frames = [yuv.encode_numpy(f, fmt) for f in VIDEO]
    for f in frames:
        wr.write(f)
    wr.close()
    dst = io.BytesIO()
    info = yuv.interpolate_y4m(io.BytesIO(src.getvalue()), dst, Mean(), fps_out=24, levels=2, shutter=sh.Shutter(180, "code"))
    assert info["frames_out"] == 2 and info["blended"] == 2 and info["forwards"] == 5
    want, _, _ = blurred(frames, 60, 24, 2, sh.Shutter(180, "code"), pixfmt=fmt)
    assert all(np.array_equal(g, w) for g, w in zip(yuv.Y4MReader(io.BytesIO(dst.getvalue())), want))


# ------------------------------------------------------------------------------------------------ ABI
def test_shutter_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(C.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    for name in ("atmvfi_shutter_accumulate", "atmvfi_shutter_resolve", "atmvfi_shutter_table"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert (lib.atmvfi_version() >> 8) & 255 >= 18
    assert "shutter.hip" in open(os.path.join(C.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    for name in ("shutter_accumulate", "shutter_resolve", "shutter_table"):
        assert callable(getattr(hip_ops.HipOps, name))
    # the library's literal tables
    for k, light in enumerate(LIGHTS):
        out = (ctypes.c_uint16 * 256)()
        assert lib.atmvfi_shutter_table(k, out) == 0 and tuple(out) == tuple(sh.SHUTTER_TABLES[light]), light
    err = lib.atmvfi_last_error
    assert lib.atmvfi_shutter_table(2, (ctypes.c_uint16 * 256)()) == -1 and b"unknown light" in err()
    assert lib.atmvfi_shutter_table(0, None) == -1 and b"null" in err()
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch

    def acc(acc=P, h=8, w=16, src=P, Hp=8, Wp=16, pad_top=0, pad_left=0, src_u8=None, bgr=0, weight=1, light=1, first=1):
        return lib.atmvfi_shutter_accumulate(acc, h, w, src, Hp, Wp, pad_top, pad_left, src_u8, bgr, weight, light, first, None)
    assert acc(acc=None) == -1 and b"null accumulator" in err()
    assert acc(src=None) == -1 and b"exactly one of src and src_u8" in err()
    assert acc(src_u8=P) == -1 and b"exactly one of src and src_u8" in err()
    assert acc(h=0) == -1 and b"zero size" in err()
    assert acc(w=-3) == -1 and b"zero size" in err()
    assert acc(pad_left=1) == -1 and b"window outside the canvas" in err()
    assert acc(pad_top=-1) == -1 and b"window outside the canvas" in err()
    assert acc(Hp=7) == -1 and b"window outside the canvas" in err()
    assert acc(Wp=0) == -1 and b"window outside the canvas" in err()
    assert acc(weight=0) == -1 and b"weight 0" in err()
    assert acc(weight=32768) == -1 and b"weight 32768" in err()
    assert acc(light=2) == -1 and b"unknown light" in err()
    assert acc(light=-1) == -1 and b"unknown light" in err()
    assert acc(acc=P + 2) == -1 and b"4-byte aligned" in err()
    assert acc(src=P + 1) == -1 and b"4-byte aligned" in err()
    assert acc(h=1 << 30, w=4, Hp=1 << 30, Wp=4) == -1 and b"too large" in err()
    assert acc(src=None, src_u8=P, h=1 << 29, w=8) == -1 and b"too large" in err()

    def res(acc=P, h=8, w=16, total=4, light=1, dst=P, bgr=0):
        return lib.atmvfi_shutter_resolve(acc, h, w, total, light, dst, bgr, None)
    assert res(acc=None) == -1 and b"null pointer" in err()
    assert res(dst=None) == -1 and b"null pointer" in err()
    assert res(h=0) == -1 and b"zero size" in err()
    assert res(total=0) == -1 and b"total_weight 0" in err()
    assert res(total=32768) == -1 and b"total_weight 32768" in err()
    assert res(light=5) == -1 and b"unknown light" in err()
    assert res(acc=P + 1) == -1 and b"4-byte aligned" in err()
    assert res(h=1 << 30, w=4) == -1 and b"too large" in err()
