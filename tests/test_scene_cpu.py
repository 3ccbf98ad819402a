"""CPU: scene-cut detection (atm-vfi_amd/scene.py, the ``scene=`` argument of the video loops, atmvfi_frame_signature) without a GPU: the
host signature against the loop model, the default thresholds against the pictures of tests/golden/scene_ref.npz with the margins they
were placed with, two-shot videos through the generic path of ``interpolate_video_nx``, the adapters on a fake codec and the ABI's
host-side checks."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cpu_scene as C

scene = importlib.import_module("atm-vfi_amd.scene")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")

MARGIN = 1.5          # the margin the defaults must keep to both sides (README "Scene cuts")


# ------------------------------------------------------------------------------------------------ signature
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,win", [(16, 16, None), (33, 47, None), (64, 96, (3, 5, 31, 41)), (40, 52, (1, 7, 33, 17)),
                                     (300, 207, None), (17, 130, None)])
def test_signature_numpy_is_the_loop_model(H, W, win, bgr):
    rng = np.random.default_rng(H * 1000 + W)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = scene.signature_numpy(frame, win, bgr=bgr)
    y0, x0, h, w = win or (0, 0, H, W)
    want = C.signature_model(frame, y0, x0, h, w, bgr)
    assert got.dtype == np.int32 and got.shape == (288,)
    assert np.array_equal(got, want)
    if frame[..., 0].sum() != frame[..., 2].sum():
        assert not np.array_equal(got, scene.signature_numpy(frame, win, bgr=not bgr))      # the channel order matters


def test_signature_closed_forms():
    # a constant frame: every cell is luma * its pixel count, one bin holds everything
    f = np.empty((37, 50, 3), np.uint8)
    f[...] = (200, 100, 50)                                   # RGB
    y = (77 * 200 + 150 * 100 + 29 * 50 + 128) >> 8
    sig = scene.signature_numpy(f, bgr=False)
    n = np.outer(np.diff(np.arange(17) * 37 // 16), np.diff(np.arange(17) * 50 // 16)).reshape(-1)
    assert n.sum() == 37 * 50 and np.array_equal(sig[:256], y * n)
    hist = np.zeros(32, np.int64); hist[y >> 3] = 37 * 50
    assert np.array_equal(sig[256:], hist)
    yb = (77 * 50 + 150 * 100 + 29 * 200 + 128) >> 8          # the same bytes read as BGR
    assert yb != y and np.array_equal(scene.signature_numpy(f, bgr=True)[:256], yb * n)
    # two tones, split at a cell boundary of a 32 x 64 frame: left cells 16 * 2 * 4 pixels of luma 0, right ones of luma 255
    g = np.zeros((32, 64, 3), np.uint8)
    g[:, 32:] = 255
    sig = scene.signature_numpy(g)
    cells = sig[:256].reshape(16, 16)
    assert np.all(cells[:, :8] == 0) and np.all(cells[:, 8:] == 255 * 2 * 4)
    assert sig[256] == 32 * 32 and sig[256 + 31] == 32 * 32 and sig[257:287].sum() == 0
    assert scene.cut_statistics(sig, sig, 32, 64) == (0.0, 0.0)
    black, white = scene.signature_numpy(np.zeros_like(g)), scene.signature_numpy(np.full_like(g, 255))
    assert scene.cut_statistics(black, white, 32, 64) == (1.0, 255.0)
    assert scene.cut_statistics(sig, black, 32, 64) == (0.5, 127.5)
    for bad in ((15, 40), (40, 15)):
        with pytest.raises(ValueError):
            scene.signature_numpy(np.zeros(bad + (3,), np.uint8))
    with pytest.raises(ValueError):
        scene.signature_numpy(g, (0, 40, 32, 32))               # window outside the frame
    with pytest.raises(ValueError):
        scene.signature_numpy(g.astype(np.float32))


# ------------------------------------------------------------------------------------------------ thresholds
def _stats(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return scene.cut_statistics(C.signature_model(a), C.signature_model(b), *a.shape[:2])


def fixture_statistics():
    """(continuous, unrelated): lists of (label, d_hist, d_grid) on the pictures of scene_ref.npz.  Continuous: the consecutive pair
    and, on every picture, 128-pixel windows panned by 1/8 and 1/4 of their side.  Unrelated: every pair of pictures except the
    consecutive one."""
    P = C.pictures()
    cont = [("frame0 / frame1",) + _stats(P["frame0"], P["frame1"])]
    for name, f in P.items():
        for frac in (0.125, 0.25):
            cont.append((f"pan {frac} of {name}",) + _stats(*C.pan_windows(f, frac)))
    names = list(P)
    unrel = [(f"{a} / {b}",) + _stats(P[a], P[b]) for i, a in enumerate(names) for b in names[i + 1:] if {a, b} != {"frame0", "frame1"}]
    return cont, unrel


def test_default_thresholds_keep_their_margins_on_the_fixture():
    assert os.path.getsize(C.SCENE_REF) < (1 << 20)
    P = C.pictures()
    assert set(P) >= {"frame0", "frame1"} and len(P) >= 4 and all(p.shape == P["frame0"].shape and p.dtype == np.uint8 for p in P.values())
    cont, unrel = fixture_statistics()
    assert len(unrel) == len(P) * (len(P) - 1) // 2 - 1
    for row in cont + unrel:
        print("%-48s d_hist %.4f  d_grid %6.2f" % row)
    sc = scene.SceneCuts()
    assert (sc.hist, sc.grid) == (scene.DEFAULT_HIST, scene.DEFAULT_GRID)
    for label, dh, dg in cont:
        assert not sc.is_cut(dh, dg), label
    for label, dh, dg in unrel:
        assert sc.is_cut(dh, dg), label
    assert sc.hist >= MARGIN * max(dh for _, dh, _ in cont)
    assert sc.hist <= min(dh for _, dh, _ in unrel) / MARGIN
    assert sc.grid <= min(dg for _, _, dg in unrel) / MARGIN
    # the grid term: a brightness step of 10 levels moves many bins and is still no cut
    f0 = P["frame0"]
    dh, dg = _stats(f0, np.clip(f0.astype(np.int32) + 10, 0, 255).astype(np.uint8))
    assert dg < sc.grid and not sc.is_cut(dh, dg)
    # judge() keeps the record, begin() forgets it
    a, b, c = (C.signature_model(P[k]) for k in ("frame0", "frame1", "other.davis-motor"))
    h, w = f0.shape[:2]
    assert [sc.judge(a, b, h, w), sc.judge(b, c, h, w), sc.judge(c, c, h, w)] == [False, True, False]
    assert sc.cuts == [1] and len(sc.stats) == 3 and sc.stats[2] == (0.0, 0.0) and sc.stats[0] == _stats(P["frame0"], P["frame1"])
    sc.begin()
    assert sc.cuts == [] and sc.stats == []


# ------------------------------------------------------------------------------------------------ the loops, generic path
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
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), k


H, W = 24, 40
SHOT_A = C.shot(5, H, W, seed=1, tone=60)
SHOT_B = C.shot(5, H, W, seed=2, tone=190)
SHOT_C = C.shot(1, H, W, seed=3, tone=120, span=20)


@pytest.mark.parametrize("factor", [2, 4, 8])
@pytest.mark.parametrize("kw", [dict(), dict(time_interval=2), dict(crop=(16, 32)), dict(tta=True), dict(time_interval=2, crop=(16, 32), tta=True)],
                         ids=lambda k: "-".join(k) or "plain")
def test_two_shot_video_through_the_generic_path(factor, kw):
    s = kw.get("time_interval", 1)
    y0, x0, h, w = mf.centre_window(H, W, kw.get("crop"))
    crop_of = lambda f: f[y0:y0 + h, x0:x0 + w]
    nx = lambda shot: mf.interpolate_video_nx(iter(shot), Mean(), factor=factor, **kw)
    model, sc = Mean(), scene.SceneCuts()
    got = list(mf.interpolate_video_nx(iter(SHOT_A + SHOT_B), model, factor=factor, scene=sc, **kw))
    # with time_interval 2 the segments are (0,2) (2,4) | (4,6) | (6,8): A's frames 0 2 4, B's frames 1 3 (video index 6, 8)
    A, B = (SHOT_A, SHOT_B) if s == 1 else (SHOT_A, SHOT_B[1:4])
    want = C.expected_two_shot(nx, A, B, factor, s, crop_of)
    _same(got, want)
    n_seg = (len(SHOT_A + SHOT_B) - 1) // s
    assert sc.cuts == [(len(SHOT_A) - 1) // s] and len(sc.stats) == n_seg
    assert model.pairs == (n_seg - 1) * (factor - 1) * (2 if kw.get("tta") else 1)        # no forward for the cut segment


@pytest.mark.parametrize("factor", [2, 4, 8])
def test_one_frame_shot_and_cuts_in_the_first_and_last_segment(factor):
    nx = lambda shot: list(mf.interpolate_video_nx(iter(shot), Mean(), factor=factor))
    fill = lambda a, b: [a] * (factor // 2) + [b] * (factor // 2 - 1)
    # a one-frame shot between two shots: two cuts in a row
    model, sc = Mean(), scene.SceneCuts()
    got = list(mf.interpolate_video_nx(iter(SHOT_A + SHOT_C + SHOT_B), model, factor=factor, scene=sc))
    want = nx(SHOT_A) + fill(SHOT_A[-1], SHOT_C[0]) + [SHOT_C[0]] + fill(SHOT_C[0], SHOT_B[0]) + nx(SHOT_B)
    _same(got, want)
    assert sc.cuts == [4, 5] and model.pairs == 8 * (factor - 1)
    # a cut in the first segment and one in the last: C | A... | C
    model = Mean()
    got = list(mf.interpolate_video_nx(iter(SHOT_C + SHOT_A + SHOT_C), model, factor=factor, scene=sc))
    want = [SHOT_C[0]] + fill(SHOT_C[0], SHOT_A[0]) + nx(SHOT_A) + fill(SHOT_A[-1], SHOT_C[0]) + [SHOT_C[0]]
    _same(got, want)
    assert sc.cuts == [0, 5] and len(sc.stats) == 6 and model.pairs == 4 * (factor - 1)          # .cuts / .stats were reset by the run
    # nothing but a cut
    got = list(mf.interpolate_video_nx(iter([SHOT_A[0], SHOT_B[0]]), model, factor=factor, scene=sc))
    _same(got, [SHOT_A[0]] + fill(SHOT_A[0], SHOT_B[0]) + [SHOT_B[0]])
    assert sc.cuts == [0] and model.pairs == 4 * (factor - 1)
    assert all(f is not SHOT_A[0] and f is not SHOT_B[0] for f in got[1:-1])                    # copies, not the caller's arrays


@pytest.mark.parametrize("kw", [dict(factor=4), dict(factor=8, time_interval=2, crop=(16, 32), tta=True)], ids=["4x", "8x-s2-crop-tta"])
def test_settings_that_never_cut_change_nothing(kw):
    video = SHOT_A + SHOT_B
    plain = list(mf.interpolate_video_nx(iter(video), Mean(), **kw))
    _same(list(mf.interpolate_video_nx(iter(video), Mean(), scene=None, **kw)), plain)
    never = scene.SceneCuts(hist=2.0)                          # d_hist <= 1: can never fire
    _same(list(mf.interpolate_video_nx(iter(video), Mean(), scene=never, **kw)), plain)
    assert never.cuts == [] and len(never.stats) == (len(video) - 1) // kw.get("time_interval", 1)
    assert max(dh for dh, _ in never.stats) > scene.DEFAULT_HIST                                 # ... though the cut is there
    # a cut-free video with the defaults
    sc = scene.SceneCuts()
    _same(list(mf.interpolate_video_nx(iter(SHOT_A), Mean(), scene=sc, **kw)), list(mf.interpolate_video_nx(iter(SHOT_A), Mean(), **kw)))
    assert sc.cuts == []


def test_arguments_and_exports():
    for fn in (host_io.interpolate_video_2x, host_io.FramePipeline.__init__, mf.interpolate_video_nx):
        p = inspect.signature(fn).parameters
        assert "scene" in p and p["scene"].default is None, fn
    assert "scene" not in inspect.signature(host_io.interpolate_video_2x_distributed).parameters
    assert host_io.SceneCuts is scene.SceneCuts and host_io.signature_numpy is scene.signature_numpy
    assert list(mf.interpolate_video_nx(iter([]), Mean(), scene=scene.SceneCuts())) == []
    with pytest.raises(ValueError):                            # a window under 16 x 16 has no signature
        list(mf.interpolate_video_nx(iter([np.zeros((12, 40, 3), np.uint8)] * 2), Mean(), factor=2, divisor=None, scene=scene.SceneCuts()))


def test_video_adapters_report_cuts_only_when_asked():
    video = SHOT_A + SHOT_B

    class Cap:
        def __init__(self):
            self.i, self.open = 0, True

        def get(self, prop):
            return {host_io.CAP_PROP_FPS: 25.0, host_io.CAP_PROP_FRAME_WIDTH: float(W), host_io.CAP_PROP_FRAME_HEIGHT: float(H)}[prop]

        def isOpened(self):
            return self.open

        def read(self):
            self.i += 1
            return (True, video[self.i - 1]) if self.i <= len(video) else (False, None)

        def release(self):
            self.open = False

    class Sink:
        def __init__(self):
            self.got = []

        def write(self, f):
            self.got.append(f.copy())

        def release(self):
            pass

    def run_nx(**kw):
        sink = Sink()
        return host_io.video_nx(Cap(), lambda fps, size: sink, Mean(), factor=4, **kw), sink.got
    base = {"fps_in": 25, "fps_out": 100, "size": (W, H), "frames_in": 10, "frames_out": 37}
    info, plain = run_nx()
    assert info == base
    info, got = run_nx(scene=None)
    assert info == base
    _same(got, plain)
    sc = scene.SceneCuts()
    info, got = run_nx(scene=sc)
    assert info == dict(base, cuts=[4]) and sc.cuts == [4]
    _same(got[:17], plain[:17]); _same(got[17:20], [video[4], video[4], video[5]]); _same(got[20:], plain[20:])
    info, got = run_nx(scene=scene.SceneCuts(hist=2.0))
    assert info == dict(base, cuts=[])
    _same(got, plain)

    # video_2x hands ``scene`` to its interpolator and reports what it recorded (the pipelined interpolator itself needs the GPU)
    seen = {}

    def interp(frames, model, isBGR=True, divisor=64, depth=3, **kw):
        seen.update(kw)
        return mf.interpolate_video_nx(frames, model, factor=2, isBGR=isBGR, divisor=divisor, **kw)

    def run_2x(**kw):
        sink = Sink()
        return host_io.video_2x(Cap(), lambda fps, size: sink, Mean(), interpolator=interp, **kw), sink.got
    base2 = {"fps_in": 25, "fps_out": 50, "size": (W, H), "frames_in": 10, "frames_out": 19}
    info, plain = run_2x()
    assert info == base2 and "scene" not in seen
    info, got = run_2x(scene=sc)
    assert info == dict(base2, cuts=[4]) and seen["scene"] is sc
    _same(got[:9], plain[:9]); _same(got[9:10], [video[4]]); _same(got[10:], plain[10:])


# ------------------------------------------------------------------------------------------------ ABI
def test_frame_signature_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(C.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    assert re.search(r"\bint\s+atmvfi_frame_signature\s*\(", hdr) and re.search(r"\bint64_t\s+atmvfi_frame_signature_workspace_ints\s*\(", hdr)
    for name in ("atmvfi_frame_signature", "atmvfi_frame_signature_workspace_ints"):
        assert name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert lib.atmvfi_plan_fn_id(b"atmvfi_frame_signature") >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 13
    assert "scene.hip" in open(os.path.join(C.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert callable(getattr(hip_ops.HipOps, "frame_signature"))
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error
    ws_ints = lib.atmvfi_frame_signature_workspace_ints

    def call(src=P, H=64, W=96, bgr=0, y0=0, x0=0, h=64, w=96, sig=P, ws=P, n=None):
        n = max(ws_ints(h, w), 0) if n is None else n
        return lib.atmvfi_frame_signature(src, H, W, bgr, y0, x0, h, w, sig, ws, n, None)
    assert call(src=None) == -1 and b"null pointer" in err()
    assert call(sig=None) == -1 and b"null pointer" in err()
    assert call(ws=None) == -1 and b"null pointer" in err()
    assert call(y0=1) == -1 and b"window outside the frame" in err()
    assert call(x0=1) == -1 and b"window outside the frame" in err()
    assert call(x0=-1, w=90) == -1 and b"window outside the frame" in err()
    assert call(H=0) == -1 and b"window outside the frame" in err()
    assert call(h=15) == -1 and b"at least 16 x 16" in err()
    assert call(w=15) == -1 and b"at least 16 x 16" in err()
    assert call(H=60000, W=60000, h=60000, w=60000) == -1 and b"too large" in err()         # 3.6e9 pixels: a bin count overflows
    assert call(H=100000000, W=17, h=100000000, w=17) == -1 and b"too large" in err()       # h * w fits; a 2-wide cell of 6.25e6 rows does not
    assert call(sig=P + 2) == -1 and b"4-byte aligned" in err()
    assert call(n=ws_ints(64, 96) - 1) == -1 and b"workspace of" in err()
    # the workspace query: 48 words per workgroup, 16 cell rows x column tiles x row chunks; -1 for a window the call refuses
    assert ws_ints(64, 96) == 48 * 16 and ws_ints(1080, 1920) == 48 * 16 * 2 * 9 and ws_ints(2160, 4096) == 48 * 16 * 4 * 17
    assert ws_ints(15, 96) == -1 and b"at least 16 x 16" in err()
    assert ws_ints(60000, 60000) == -1
