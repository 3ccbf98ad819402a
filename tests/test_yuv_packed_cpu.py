"""CPU: packed 4:2:2 capture frames (atm-vfi_amd/pixfmt.py Packed: uyvy, yuy2, y210, v210; yuv.unpack_numpy / pack_numpy; ``pixfmt=Packed``
of ``interpolate_video_nx`` / ``interpolate_video_retimed`` / ``interpolate_raw``; atmvfi_yuv_unpack / atmvfi_yuv_pack) without a GPU: the
twins against the per-sample loop model of tests/cpu_yuv_packed.py, the padding rule, hand-written vectors, the descriptor's refusals,
raw I/O, the ABI's host-side checks, and both loops on a CPU stand-in model: a packed stream gives the packed form of what its planar
stream gives."""
import ctypes
import importlib
import io
import os
import re

import numpy as np
import pytest
import torch

import cpu_active as CA
import cpu_scene as CS
import cpu_yuv_packed as M

active = importlib.import_module("atm-vfi_amd.active")
mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
scene = importlib.import_module("atm-vfi_amd.scene")
yuv = importlib.import_module("atm-vfi_amd.yuv")
pixfmt = importlib.import_module("atm-vfi_amd.pixfmt")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")

SHAPES = [(1, 2), (3, 6), (2, 8), (3, 46), (2, 48), (2, 50), (5, 98)]


def packed_of(layout, H, W, pitch=None, **kw):
    return yuv.Packed(yuv.Format(H, W, depth=M.DEPTH[layout], subsampling="422", **kw), layout, pitch)


def custom_pitches(layout, W):
    """pitches that are not the default: the row's own bytes rounded up to the unit (v210: below the default), and beyond the default"""
    unit = 16 if layout == "v210" else 4
    row, d = M.row_bytes(layout, W), M.default_pitch(layout, W)
    return sorted({p for p in (-(-row // unit) * unit, row + unit, d + unit, d + 5 * unit) if p != d})


def as_frame(k, raw):
    """model bytes -> a frame of ``k``"""
    return np.ascontiguousarray(raw).view(k.dtype)


# ------------------------------------------------------------------------------------------------ the twins
@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_twins_are_the_sample_loop(layout, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    k = packed_of(layout, H, W)
    assert k.pitch == M.default_pitch(layout, W) and k.nbytes == k.pitch * H and k.is_tight and k.planar == k.fmt
    p = M.random_planar(rng, layout, H, W)
    raw = M.pack_loop(p, layout, H, W)
    f = yuv.pack_numpy(p, k)
    assert f.dtype == k.dtype and f.shape == (k.frame_samples,) and np.array_equal(f.view(np.uint8), raw)
    assert not (raw & ~M.sample_mask(layout, H, W)).any()                    # zeros in every padding position
    u = yuv.unpack_numpy(f, k)
    assert u.dtype == k.planar.dtype and np.array_equal(u, M.unpack_loop(raw, layout, H, W)) and np.array_equal(u, p)
    assert np.array_equal(yuv.pack_numpy(u, k), f)                           # both round trips
    # a frame of arbitrary bytes: the twin reads what the loop reads
    noise = rng.integers(0, 256, k.nbytes).astype(np.uint8)
    assert np.array_equal(yuv.unpack_numpy(as_frame(k, noise), k), M.unpack_loop(noise, layout, H, W))


@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_padding_is_never_interpreted(layout, H, W):
    rng = np.random.default_rng(H * 77 + W)
    p = M.random_planar(rng, layout, H, W)
    raw = M.pack_loop(p, layout, H, W)
    d = M.default_pitch(layout, W)
    for pitch in [d] + custom_pitches(layout, W):
        k = packed_of(layout, H, W, pitch)
        assert k.is_tight == (pitch == d) and k.tight() == packed_of(layout, H, W)
        bad = M.poisoned(raw, layout, H, W, pitch)
        if pitch > M.row_bytes(layout, W):
            assert bad.reshape(H, pitch)[0, -1] == 0xFF
        assert np.array_equal(M.unpack_loop(bad, layout, H, W, pitch), p)
        assert np.array_equal(yuv.unpack_numpy(as_frame(k, bad), k), p)
        assert np.array_equal(yuv.pack_numpy(yuv.unpack_numpy(as_frame(k, bad), k), k).view(np.uint8), raw)      # the tight repack


def test_hand_written_vectors():
    group = bytes([0x01, 0x08, 0x30, 0x00,      # w0 = Cb0 1 | Y0 2 << 10 | Cr0 3 << 20
                   0x04, 0x14, 0x60, 0x00,      # w1 = Y1 4 | Cb1 5 << 10 | Y2 6 << 20
                   0x07, 0x20, 0x90, 0x00,      # w2 = Cr1 7 | Y3 8 << 10 | Cb2 9 << 20
                   0x0A, 0x2C, 0xF0, 0x3F])     # w3 = Y4 10 | Cr2 11 << 10 | Y5 1023 << 20
    want = [2, 4, 6, 8, 10, 1023, 1, 5, 9, 3, 7, 11]
    k = packed_of("v210", 1, 6, pitch=16)
    f = np.frombuffer(group, np.uint8)
    assert yuv.unpack_numpy(f, k).tolist() == want and M.unpack_loop(f, "v210", 1, 6, 16).tolist() == want
    tight = yuv.pack_numpy(np.array(want, np.uint16), k)
    assert tight.shape == (128,) and tight[:16].tobytes() == group and not tight[16:].any()
    # bits 30-31 set: the same samples
    hot = f.copy()
    hot[3::4] |= 0xC0
    assert yuv.unpack_numpy(hot, k).tolist() == want
    pair = np.array([10, 20, 30, 40], np.uint8)
    assert yuv.unpack_numpy(pair, packed_of("uyvy", 1, 2)).tolist() == [20, 40, 10, 30]        # U0 Y0 V0 Y1
    assert yuv.unpack_numpy(pair, packed_of("yuy2", 1, 2)).tolist() == [10, 30, 20, 40]        # Y0 U0 Y1 V0
    deep = np.array([5 << 6 | 63, 6 << 6, 7 << 6 | 1, 1023 << 6], np.uint16)
    assert yuv.unpack_numpy(deep, packed_of("y210", 1, 2)).tolist() == [5, 7, 6, 1023]
    assert yuv.pack_numpy(np.array([5, 7, 6, 1023], np.uint16), packed_of("y210", 1, 2)).tolist() == [5 << 6, 6 << 6, 7 << 6, 1023 << 6]


def test_surface_of_names_and_as_8bit():
    for name, layout in (("uyvy422", "uyvy"), ("yuyv422", "yuy2"), ("y210le", "y210"), ("v210", "v210")):
        k = yuv.surface_of(name, 6, 50, matrix="bt709", siting="left")
        assert isinstance(k, yuv.Packed) and k == packed_of(layout, 6, 50, matrix="bt709", siting="left") and k.layout_id == M.LAYOUTS.index(layout)
        assert (k.height, k.width, k.depth, k.siting, k.matrix) == (6, 50, M.DEPTH[layout], "left", "bt709")
    assert yuv.surface_of("v210", 4, 96, pitch=384).pitch == 384 and yuv.surface_of("v210", 4, 96).pitch == 256
    with pytest.raises(ValueError, match="unknown pixel format.*uyvy422, yuyv422, y210le, v210"):
        yuv.surface_of("nv16", 4, 4)
    assert yuv.surface_of("nv12", 4, 4) == yuv.Surface.nv12(4, 4) and yuv.surface_of("yuv422p", 4, 4) == yuv.Surface(yuv.Format(4, 4, subsampling="422"))
    v, y = packed_of("v210", 4, 50, pitch=272), packed_of("y210", 4, 50, pitch=208)
    assert v.as_8bit() == packed_of("uyvy", 4, 50) and y.as_8bit() == packed_of("yuy2", 4, 50)
    u = packed_of("uyvy", 4, 50, pitch=104)
    assert u.as_8bit() == u.tight() == packed_of("uyvy", 4, 50) and u.cropped(2, 8) == packed_of("uyvy", 2, 8)
    assert yuv.out_format(v, True) == v.tight() and yuv.out_format(v, False) == v.as_8bit()
    assert yuv.passes_through(v.tight()) and not yuv.passes_through(v) and yuv.Packed is pixfmt.Packed
    assert (v.dtype, v.itemsize, y.dtype, y.itemsize) == (np.uint8, 1, np.uint16, 2) and y.frame_samples * 2 == y.nbytes == y.frame_bytes


def test_packed_refusals():
    f8, f10 = yuv.Format(4, 8, subsampling="422"), yuv.Format(4, 8, depth=10, subsampling="422")
    with pytest.raises(ValueError, match="even"):
        yuv.Packed(yuv.Format(4, 7, subsampling="422"), "uyvy")
    for layout, fmt in (("uyvy", f10), ("yuy2", f10), ("y210", f8), ("v210", f8)):
        with pytest.raises(ValueError, match=layout):                                   # the wrong depth, naming the layout
            yuv.Packed(fmt, layout)
    for sub in ("420", "444"):
        with pytest.raises(ValueError, match="uyvy.*4:2:2"):
            yuv.Packed(yuv.Format(4, 8, subsampling=sub), "uyvy")
    with pytest.raises(ValueError, match="unknown layout"):
        yuv.Packed(f8, "nv16")
    for layout, fmt, bad in (("uyvy", f8, (12, 18, 15)), ("yuy2", f8, (12, 18)), ("y210", f10, (28, 34)), ("v210", f10, (16, 40, 36))):
        for pitch in bad:                                                               # short, or not a multiple of 4 (v210: 16)
            with pytest.raises(ValueError, match="pitch"):
                yuv.Packed(fmt, layout, pitch)
    assert yuv.Packed(f10, "v210", 32).pitch == 32 and yuv.Packed(f8, "uyvy", 20).pitch == 20
    with pytest.raises(ValueError, match="yuv.Format"):
        yuv.Packed("uyvy", "uyvy")
    k = yuv.Packed(f8, "uyvy")
    for bad in (np.zeros(63, np.uint8), np.zeros(64, np.uint16), np.zeros(128, np.uint8)[::2]):
        with pytest.raises(ValueError, match="uyvy frame"):
            k.check(bad, "x")
    # what existing tests pin stays refused
    with pytest.raises(ValueError, match="4:2:0 only"):
        yuv.Surface(f8, "uv")


def test_crop_of_a_packed_frame():
    rng = np.random.default_rng(5)
    for layout in M.LAYOUTS:
        k = packed_of(layout, 6, 20, pitch=M.default_pitch(layout, 20) + 16)
        p = M.random_planar(rng, layout, 6, 20)
        f = as_frame(k, M.poisoned(M.pack_loop(p, layout, 6, 20), layout, 6, 20, k.pitch))
        got = yuv.crop(f, k, 2, 4, 3, 10)
        assert np.array_equal(got, yuv.pack_numpy(yuv.crop(p, k.planar, 2, 4, 3, 10), k.cropped(3, 10))) and got.size == k.cropped(3, 10).frame_samples
        with pytest.raises(ValueError, match="even x0"):
            yuv.crop(f, k, 2, 3, 3, 10)


@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_raw_reader_and_writer(layout):
    rng = np.random.default_rng(9)
    k = packed_of(layout, 3, 50)
    frames = [yuv.pack_numpy(M.random_planar(rng, layout, 3, 50), k) for _ in range(3)]
    f = io.BytesIO()
    with yuv.RawWriter(f, k) as wr:
        for fr in frames:
            wr.write(fr)
        with pytest.raises(ValueError):
            wr.write(frames[0][:-1])
    assert f.tell() == 3 * k.nbytes
    f.seek(0)
    rd = yuv.RawReader(f, k, 25)
    assert len(rd) == 3
    got = list(rd)
    assert len(got) == 3 and all(g.dtype == k.dtype and np.array_equal(g, w) for g, w in zip(got, frames))
    with pytest.raises(ValueError, match="truncated"):
        list(yuv.RawReader(io.BytesIO(f.getvalue()[:-1]), k, 25))


# ------------------------------------------------------------------------------------------------ the loops, host backend
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend (tests/test_yuv_cpu.py's stand-in): the pair mean, recording the sizes it is asked for."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.pairs, self.shapes = 0, []

    def forward(self, a, b):
        self.pairs += a.shape[0]
        self.shapes.append(tuple(a.shape[-2:]))
        return {"I_t": (a + b) / 2}


H, W = 24, 40                # (v210: six whole groups and one of four pixels)


def planar_video(fmt, rgb):
    return [yuv.encode_numpy(f.astype(np.float32) / np.float32(255) if fmt.depth == 10 else f, fmt) for f in rgb]


def packed_video(k, Q):
    """the planar frames as frames of ``k``, everything that holds no sample set"""
    return [as_frame(k, M.poisoned(yuv.pack_numpy(q, k).view(np.uint8), k.layout, k.height, k.width, k.pitch)) for q in Q]


def check_identity(k, P, Q, got, want):
    """``got``: a loop's frames for the packed video P; ``want``: the same loop's for its planar video Q.  Originals are the caller's
    own objects at the default pitch; everything else is the packed form of the planar loop's frame, in the layout of its depth."""
    assert len(got) == len(want) and len(got) > len(P)
    seen = 0
    for g, w in zip(got, want):
        i = next((i for i, q in enumerate(Q) if w is q), None)
        if i is not None and k.is_tight:
            assert g is P[i]
            seen += 1
            continue
        out = k.tight() if w.dtype == k.planar.dtype else k.as_8bit()
        assert g.dtype == out.dtype and np.array_equal(g, yuv.pack_numpy(w, out)) and all(g is not p for p in P)
    return seen


def loops():
    nx = lambda frames, model, **kw: mf.interpolate_video_nx(frames, model, factor=4, **kw)
    retimed = lambda frames, model, **kw: rt.interpolate_video_retimed(frames, model, 24, 60, levels=3, **kw)
    return {"nx4": nx, "retimed": retimed}


CASES = {
    "uyvy": ("uyvy", None, {}),
    "yuy2 pitch": ("yuy2", 2 * W + 12, {}),
    "y210 keep": ("y210", None, dict(keep_depth=True)),
    "v210 keep": ("v210", None, dict(keep_depth=True)),
    "v210 keep pitch": ("v210", 112, dict(keep_depth=True)),        # (the row's own bytes: below the default 128)
    "v210": ("v210", None, {}),
    "uyvy tta": ("uyvy", None, dict(tta=True)),
    "uyvy crop": ("uyvy", None, dict(crop=(16, 32))),
}


@pytest.mark.parametrize("loop", ["nx4", "retimed"])
@pytest.mark.parametrize("case", list(CASES))
def test_a_packed_stream_gives_the_packed_form_of_its_planar_stream(loop, case):
    layout, pitch, kw = CASES[case]
    k = packed_of(layout, H, W, pitch, matrix="bt709", siting="left")
    Q = planar_video(k.planar, CS.shot(4, H, W, seed=3, tone=120))
    P = packed_video(k, Q)
    keep = [p.copy() for p in P]
    run = loops()[loop]
    m1, m2 = Mean(), Mean()
    got, want = list(run(iter(P), m1, pixfmt=k, **kw)), list(run(iter(Q), m2, pixfmt=k.planar, **kw))
    assert m1.pairs == m2.pairs > 0
    if "crop" in kw:
        ck = k.cropped(16, 32)
        assert all(g.size == ck.frame_samples for g in got)
        Qc = [w for w in want]
        assert all(np.array_equal(g, yuv.pack_numpy(w, ck)) for g, w in zip(got, Qc))
    else:
        originals = sum(any(w is q for q in Q) for w in want)       # (every frame under 4x; those on the output grid when retimed)
        assert originals >= 2 and (loop != "nx4" or originals == len(P))
        assert check_identity(k, P, Q, got, want) == (originals if k.is_tight else 0)
    assert all(np.array_equal(a, b) for a, b in zip(P, keep))          # the caller's buffers are untouched


def test_scene_dedup_and_shutter_on_uyvy():
    k = packed_of("uyvy", H, W, matrix="bt709", siting="left")
    rgb = CS.shot(3, H, W, seed=1, tone=60) + CS.shot(3, H, W, seed=2, tone=190)
    Q = planar_video(k.planar, rgb)
    P = packed_video(k, Q)
    for name, run in loops().items():
        s1, s2 = scene.SceneCuts(), scene.SceneCuts()
        got, want = list(run(iter(P), Mean(), pixfmt=k, scene=s1)), list(run(iter(Q), Mean(), pixfmt=k.planar, scene=s2))
        assert s1.cuts == s2.cuts == [2] and s1.stats == s2.stats
        check_identity(k, P, Q, got, want)
    # a repeated frame is dropped from both timelines alike
    Qd = Q[:2] + [Q[1].copy()] + Q[2:3]
    Pd = packed_video(k, Qd)
    d1, d2 = rt.Duplicates(), rt.Duplicates()
    got, want = (list(loops()["retimed"](iter(v), Mean(), pixfmt=f, dedup=d)) for v, f, d in ((Pd, k, d1), (Qd, k.planar, d2)))
    assert d1.dropped == d2.dropped and 2 in d1.dropped and d1.stats == d2.stats
    check_identity(k, Pd, Qd, got, want)
    r1, r2 = {}, {}
    got, want = (list(loops()["retimed"](iter(v), Mean(), pixfmt=f, shutter=180, report=r)) for v, f, r in ((P[:3], k, r1), (Q[:3], k.planar, r2)))
    assert r1 == r2 and r1["blended"] > 0
    check_identity(k, P[:3], Q[:3], got, want)


@pytest.mark.parametrize("layout,kw", [("uyvy", {}), ("v210", dict(keep_depth=True))])
def test_active_on_a_letterboxed_packed_clip(layout, kw):
    AH, AW, WIN = 128, 96, (32, 0, 64, 96)
    L5, _ = CA.letterboxed(5, AH, AW, (32, 96), seed=1)
    k = packed_of(layout, AH, AW, siting="left")
    Q = planar_video(k.planar, L5)
    P = packed_video(k, Q)
    for name, run in loops().items():
        m, a1, a2 = Mean(), active.ActiveArea(), active.ActiveArea()
        got = list(run(iter(P), m, pixfmt=k, active=a1, divisor=16, **kw))
        want = list(run(iter(Q), Mean(), pixfmt=k.planar, active=a2, divisor=16, **kw))
        assert a1.window == a2.window == WIN and a1.fallback_at is None and set(m.shapes) == {(64, 96)}     # the forwards ran on the window
        assert check_identity(k, P, Q, got, want) >= 3
        if name == "nx4":       # the bars of a produced frame are the nearer original's own bytes
            rows = np.r_[0:32, 96:128]
            for i, g in enumerate(got):
                near = Q[i // 4 + (i % 4 > 2)]
                for a, b in zip(k.planar.planes(yuv.unpack_numpy(g, k)), k.planar.planes(near)):
                    assert np.array_equal(a[rows], b[rows])
    got = list(loops()["nx4"](iter(P), Mean(), pixfmt=k, active=WIN, divisor=16, **kw))           # a fixed window: never probed
    want = list(loops()["nx4"](iter(Q), Mean(), pixfmt=k.planar, active=WIN, divisor=16, **kw))
    check_identity(k, P, Q, got, want)


def test_the_pinned_refusals_hold_with_a_packed_format():
    k8, k10 = packed_of("uyvy", H, W), packed_of("v210", H, W)
    P8 = packed_video(k8, planar_video(k8.planar, CS.shot(3, H, W, seed=1, tone=100)))
    P10 = packed_video(k10, planar_video(k10.planar, CS.shot(3, H, W, seed=1, tone=100)))
    nx, retimed = loops()["nx4"], loops()["retimed"]
    for run in (nx, retimed):
        with pytest.raises(ValueError, match="keep_depth=True"):
            list(run(iter(P10), Mean(), pixfmt=k10, active=active.ActiveArea()))
        with pytest.raises(ValueError, match="active does not go with crop"):
            list(run(iter(P8), Mean(), pixfmt=k8, active=active.ActiveArea(), crop=(16, 32)))
        with pytest.raises(ValueError, match="uyvy frame"):
            list(run(iter([p[:-1] for p in P8]), Mean(), pixfmt=k8))
        with pytest.raises(ValueError, match="frames of the format"):
            list(run(iter(P10), Mean(), pixfmt=k8, active=active.ActiveArea()))
        with pytest.raises(ValueError, match="even x0"):
            list(run(iter(P8), Mean(), pixfmt=k8, crop=(16, 30)))
    with pytest.raises(ValueError, match="shutter blends 8-bit pixels"):
        list(retimed(iter(P10), Mean(), pixfmt=k10, keep_depth=True, shutter=180))
    with pytest.raises(ValueError, match="active does not go with shutter"):
        list(retimed(iter(P8), Mean(), pixfmt=k8, active=active.ActiveArea(), shutter=180))
    with pytest.raises(ValueError, match="packed 4:2:2"):
        host_io.FramePipeline(Mean(), H, W, pixfmt=k8)


@pytest.mark.parametrize("layout,keep,kw", [("v210", True, {}), ("v210", False, {}), ("y210", False, dict(fps_out=60)), ("uyvy", False, dict(crop=(16, 32)))])
def test_interpolate_raw_with_a_packed_format(layout, keep, kw):
    k = packed_of(layout, H, W, pitch=M.default_pitch(layout, W) + 16, siting="left")
    Q = planar_video(k.planar, CS.shot(4, H, W, seed=4, tone=140))
    P = packed_video(k, Q)
    src, dst = io.BytesIO(b"".join(p.tobytes() for p in P)), io.BytesIO()
    info = yuv.interpolate_raw(src, dst, Mean(), k, 24, factor=2, keep_depth=keep, **kw)
    out = (k.tight() if keep else k.as_8bit()).cropped(*kw.get("crop", (H, W)))
    dst.seek(0)
    got = list(yuv.RawReader(dst, out, info["fps_out"]))
    assert info["frames_in"] == 4 and info["frames_out"] == len(got) and info["size"] == (out.width, out.height)
    if "fps_out" in kw:
        want = list(rt.interpolate_video_retimed(iter(P), Mean(), 24, 60, pixfmt=k, keep_depth=keep))
    else:
        want = list(mf.interpolate_video_nx(iter(P), Mean(), factor=2, pixfmt=k, keep_depth=keep, **kw))
    assert len(got) == len(want) > 4
    for g, w in zip(got, want):       # (10-bit originals of an 8-bit output: converted on the host, v210 -> uyvy, y210 -> yuy2)
        w = w if (w.dtype == out.dtype and w.size == out.frame_samples) else yuv.to_8bit(w, k.cropped(out.height, out.width))
        assert g.dtype == out.dtype and np.array_equal(g, w)
    if not keep and k.depth == 10:
        want0 = yuv.pack_numpy(yuv.to_8bit(Q[0], k.planar), out)
        assert np.array_equal(got[0], want0)


# ------------------------------------------------------------------------------------------------ ABI
def test_packed_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    for name in ("atmvfi_yuv_unpack", "atmvfi_yuv_pack"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
    assert (lib.atmvfi_version() >> 8) & 255 >= 23
    mk = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert " yuv_packed.hip" in mk
    assert callable(hip_ops.HipOps.yuv_unpack) and callable(hip_ops.HipOps.yuv_pack)
    assert "((W + 47) / 48) * 128" in hdr and "WRITTEN AS ZERO" in hdr and "NEVER INTERPRETED" in hdr
    P, Q = 0x10000, 0x4000000000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lambda: lib.atmvfi_last_error().decode()
    unpack = lambda packed=P, H=4, W=8, layout=0, pitch=0, planar=Q: lib.atmvfi_yuv_unpack(packed, H, W, layout, pitch, planar, None)
    pack = lambda planar=Q, H=4, W=8, layout=0, packed=P: lib.atmvfi_yuv_pack(planar, H, W, layout, packed, None)
    for call, who in ((unpack, "yuv_unpack"), (pack, "yuv_pack")):
        for kw, msg in ((dict(packed=None), "null pointer"), (dict(planar=None), "null pointer"), (dict(H=0), "H must be at least 1"),
                        (dict(W=0), "W even and at least 2"), (dict(W=7), "W even and at least 2"), (dict(layout=4), "unknown layout 4"),
                        (dict(layout=-1), "unknown layout"), (dict(layout=2, packed=P + 1), "2-byte aligned"),
                        (dict(layout=2, planar=Q + 1), "2-byte aligned"), (dict(layout=3, packed=P + 2), "4-byte aligned"),
                        (dict(layout=3, planar=Q + 1), "2-byte aligned"), (dict(planar=P + 16), "overlap"), (dict(packed=Q + 60), "overlap"),
                        (dict(H=1 << 24, W=4096), "too large"), (dict(H=1 << 22, W=1 << 14, layout=3), "too large")):
            assert call(**kw) != 0 and who in err() and msg in err(), (who, kw, err())
    for kw in (dict(pitch=12), dict(pitch=18), dict(pitch=-16), dict(layout=1, pitch=15), dict(layout=2, pitch=28), dict(layout=2, pitch=34),
               dict(layout=3, pitch=16), dict(layout=3, pitch=40), dict(layout=3, W=50, pitch=128)):
        assert unpack(**kw) != 0 and "yuv_unpack" in err() and "pitch" in err(), (kw, err())
