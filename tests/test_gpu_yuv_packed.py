"""GPU: packed 4:2:2 capture frames on the device (csrc/yuv_packed.hip atmvfi_yuv_unpack / atmvfi_yuv_pack; ``pixfmt=Packed`` of the video
loops): both kernels bit for bit against the per-sample loop model of tests/cpu_yuv_packed.py -- every layout, the aligned and the
general path reached by pointer offsets, pitched and poisoned sources, poisoned destinations with guards, the grid stride at 2160 x
4096 -- the host refusals, the composition with the 4:2:2 decode and encode, and the HIP loops: a packed stream gives the packed form
of what its planar stream gives."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cpu_active as CA
import cpu_scene as CS
import cpu_yuv_packed as M

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")
active = importlib.import_module("atm-vfi_amd.active")
rt = importlib.import_module("atm-vfi_amd.retime")

GUARD, POISON = 64, 0xA5
SHAPES = [(1, 2), (3, 6), (2, 8), (3, 46), (2, 48), (2, 50), (5, 98), (16, 1920), (4, 4096)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


def make_net(dev, kind):
    torch.set_grad_enabled(False)
    n = pkg.NetworkLite() if kind == "lite" else pkg.Network()
    n.load_state_dict(pkg.synthetic_state_dict(kind, seed=1), strict=True)
    n = n.to(dev).eval()
    n.global_motion, n.ensemble_global_motion = True, False
    return n


@pytest.fixture(scope="module")
def net(dev):
    return make_net(dev, "lite")


def packed_of(layout, H, W, pitch=None, **kw):
    return yuv.Packed(yuv.Format(H, W, depth=M.DEPTH[layout], subsampling="422", **kw), layout, pitch)


def sample_offsets(layout):
    """(packed, planar) pointer offsets of one sample (v210's packed frame: 4 bytes): the general path"""
    return {"uyvy": (1, 1), "yuy2": (1, 1), "y210": (2, 2), "v210": (4, 2)}[layout]


def on_dev(raw, dev, offset=0):
    """the bytes on the device, ``offset`` bytes past an allocation's start"""
    raw = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1))
    buf = torch.empty(raw.numel() + offset, dtype=torch.uint8, device=dev)
    buf[offset:].copy_(raw)
    return buf[offset:]


def poisoned_dst(n, dev, offset=0):
    """(the whole buffer, its n-byte view at ``offset``): POISON everywhere, GUARD bytes behind the view"""
    buf = torch.full((offset + n + GUARD,), POISON, dtype=torch.uint8, device=dev)
    return buf, buf[offset:offset + n]


def guards_intact(buf, offset, n):
    return bool((buf[:offset] == POISON).all()) and bool((buf[offset + n:] == POISON).all())


def unpack_on(ops, dev, k, raw, offsets=(0, 0)):
    src = on_dev(raw, dev, offsets[0])
    n = k.planar.frame_bytes
    buf, dst = poisoned_dst(n, dev, offsets[1])
    assert ops.yuv_unpack(src, k, dst=dst) is dst
    torch.cuda.synchronize()
    assert guards_intact(buf, offsets[1], n)
    return dst.cpu().numpy().view(k.planar.dtype)


def pack_on(ops, dev, k, planar, offsets=(0, 0)):
    src = on_dev(planar, dev, offsets[1])
    buf, dst = poisoned_dst(k.nbytes, dev, offsets[0])
    assert ops.yuv_pack(src, k, dst=dst) is dst
    torch.cuda.synchronize()
    assert guards_intact(buf, offsets[0], k.nbytes)
    return dst.cpu().numpy()


def custom_pitches(layout, W):
    """one pitch that keeps the 16-byte rows (the aligned path at a pitch) and one that does not (v210: every pitch does)"""
    d = M.default_pitch(layout, W)
    return [d + 32, M.row_bytes(layout, W) + (16 if layout == "v210" else 4)]


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_both_kernels_are_the_sample_loop(ops, dev, layout, H, W):
    rng = np.random.default_rng(H * 131 + W)
    k = packed_of(layout, H, W)
    p = M.random_planar(rng, layout, H, W)
    raw = M.pack_loop(p, layout, H, W)
    assert np.array_equal(M.unpack_loop(raw, layout, H, W), p)
    off = sample_offsets(layout)
    packs = [pack_on(ops, dev, k, p, o) for o in ((0, 0), off, (off[0], 0), (0, off[1]))]
    assert all(np.array_equal(g, raw) for g in packs)                  # every byte written, the zero padding included; both paths alike
    noise = rng.integers(0, 256, k.nbytes).astype(np.uint8)            # arbitrary bytes: padding, spare slots and bits set at random
    want = M.unpack_loop(noise, layout, H, W)
    for o in ((0, 0), off, (off[0], 0), (0, off[1])):
        assert np.array_equal(unpack_on(ops, dev, k, raw, o), p)
        assert np.array_equal(unpack_on(ops, dev, k, noise, o), want)
    for pitch in custom_pitches(layout, W):                            # a pitched source, everything that holds no sample set
        kp = packed_of(layout, H, W, pitch)
        bad = M.poisoned(raw, layout, H, W, pitch)
        for o in ((0, 0), off):
            assert np.array_equal(unpack_on(ops, dev, kp, bad, o), p)


@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_2160x4096_the_grid_stride(ops, dev, layout):
    H, W = 2160, 4096
    rng = np.random.default_rng(7)
    k = packed_of(layout, H, W)
    p = M.tall_planar(rng, layout, H, W)
    raw = M.pack_loop(p, layout, H, W, memo={})
    assert raw.size == k.nbytes and np.array_equal(M.unpack_loop(raw, layout, H, W, memo={}), p)
    off = sample_offsets(layout)
    for o in ((0, 0), off):
        assert np.array_equal(pack_on(ops, dev, k, p, o), raw)
        assert np.array_equal(unpack_on(ops, dev, k, raw, o), p)


def test_host_refusals(ops, dev):
    k = packed_of("y210", 4, 8)
    src, dst = on_dev(np.zeros(k.nbytes, np.uint8), dev), torch.empty(k.planar.frame_bytes, dtype=torch.uint8, device=dev)
    for bad in (dst[:-1], dst.cpu(), dst.view(torch.int16)):
        with pytest.raises(ValueError, match="planar 4:2:2 frame"):
            ops.yuv_unpack(src, k, dst=bad)
        with pytest.raises(ValueError, match="planar 4:2:2 frame"):
            ops.yuv_pack(bad, k)
    with pytest.raises(ValueError, match="y210 frame"):
        ops.yuv_unpack(src[:-2], k)
    with pytest.raises(ValueError, match="yuv.Packed expected"):
        ops.yuv_unpack(src, k.planar)
    with pytest.raises(ValueError, match="default pitch"):
        ops.yuv_pack(dst, packed_of("y210", 4, 8, pitch=48))
    assert ops.yuv_unpack(src, k).shape == (k.planar.frame_bytes,) and ops.yuv_pack(dst, k).shape == (k.nbytes,)
    # the library's own checks, reached through the wrapper: nothing is launched
    both = torch.zeros(1024, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.yuv_unpack(both[:k.nbytes], k, dst=both[k.nbytes - 16:k.nbytes - 16 + k.planar.frame_bytes])
    with pytest.raises(RuntimeError, match="overlap"):
        ops.yuv_pack(both[:k.planar.frame_bytes], k, dst=both[16:16 + k.nbytes])
    with pytest.raises(RuntimeError, match="2-byte aligned"):
        ops.yuv_unpack(both[1:1 + k.nbytes], k, dst=dst)
    with pytest.raises(RuntimeError, match="2-byte aligned"):
        ops.yuv_pack(both[1:1 + k.planar.frame_bytes], k, dst=src)
    v = packed_of("v210", 4, 8)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        ops.yuv_unpack(both[2:2 + v.nbytes], v, dst=dst)
    assert ops.recording is None
    lib = ops.lib
    for args, msg in (((src.data_ptr(), 4, 7, 0, 0, dst.data_ptr(), None), "W even"), ((src.data_ptr(), 0, 8, 0, 0, dst.data_ptr(), None), "H must"),
                      ((src.data_ptr(), 4, 8, 9, 0, dst.data_ptr(), None), "unknown layout"), ((None, 4, 8, 0, 0, dst.data_ptr(), None), "null"),
                      ((src.data_ptr(), 4, 8, 0, 14, dst.data_ptr(), None), "pitch"), ((src.data_ptr(), 4, 8, 3, 24, dst.data_ptr(), None), "pitch"),
                      ((src.data_ptr(), 1 << 24, 4096, 0, 0, dst.data_ptr() + (1 << 40), None), "too large")):
        assert lib.atmvfi_yuv_unpack(*args) != 0 and msg in lib.atmvfi_last_error().decode()


@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_composition_with_the_422_decode_and_encode(ops, dev, layout):
    H, W = 18, 50
    k = packed_of(layout, H, W, pitch=M.default_pitch(layout, W) + 16, matrix="bt709", siting="left")
    fmt = k.planar
    rgb = CS.shot(1, H, W, seed=5, tone=120)[0]
    planar = yuv.encode_numpy(rgb.astype(np.float32) / np.float32(255) if fmt.depth == 10 else rgb, fmt)
    frame = M.poisoned(yuv.pack_numpy(planar, k).view(np.uint8), layout, H, W, k.pitch)
    keep = fmt.depth == 10
    mk = lambda: (torch.empty(3, H, W, dtype=torch.float32, device=dev) if keep else torch.empty(H, W, 3, dtype=torch.uint8, device=dev))
    a, b = mk(), mk()
    dst = dict(dst=a, keep_depth=True) if keep else dict(dst_u8=a)
    ops.yuv_decode(ops.yuv_unpack(on_dev(frame, dev), k), fmt, **dst)
    dst = dict(dst=b, keep_depth=True) if keep else dict(dst_u8=b)
    ops.yuv_decode(on_dev(yuv.unpack_numpy(frame.view(k.dtype), k), dev), fmt, **dst)
    assert torch.equal(a, b)
    # the other way: the encode's planes, packed
    enc = torch.empty(fmt.frame_bytes, dtype=torch.uint8, device=dev)
    ops.yuv_encode(enc, fmt, **(dict(src=a) if keep else dict(src_u8=a)))
    got = ops.yuv_pack(enc, k.tight()).cpu().numpy()
    assert np.array_equal(got, yuv.pack_numpy(enc.cpu().numpy().view(fmt.dtype), k).view(np.uint8))


# ------------------------------------------------------------------------------------------------ the loops
H, W = 64, 96
RUNS = {"4x_pooled": lambda fr, net, **kw: host_io.interpolate_video_nx(fr, net, factor=4, divisor=32, pool=True, **kw),
        "4x_plain": lambda fr, net, **kw: host_io.interpolate_video_nx(fr, net, factor=4, divisor=32, pool=False, **kw),
        "4x_tta": lambda fr, net, **kw: host_io.interpolate_video_nx(fr, net, factor=4, divisor=32, tta=True, **kw),
        "retimed_dedup": lambda fr, net, **kw: host_io.interpolate_video_retimed(fr, net, 24, 60, levels=2, divisor=32, dedup=rt.Duplicates(), **kw)}
_planar_runs = {}


def shots(fmt, h=H, w=W, n=3):
    rgb = CS.shot(n, h, w, seed=11, tone=100)
    return [yuv.encode_numpy(f.astype(np.float32) / np.float32(255) if fmt.depth == 10 else f, fmt) for f in rgb]


def packed_video(k, Q):
    return [np.ascontiguousarray(M.poisoned(yuv.pack_numpy(q, k).view(np.uint8), k.layout, k.height, k.width, k.pitch)).view(k.dtype) for q in Q]


def planar_run(net, name, fmt, keep, key="shots"):
    """the planar loop's frames, computed once per (loop, format, depth kept) and left unchanged"""
    at = (name, fmt, keep, key)
    if at not in _planar_runs:
        Q = shots(fmt)
        if name == "retimed_dedup":
            Q = Q[:2] + [Q[1].copy()] + Q[2:]
        _planar_runs[at] = (Q, list(RUNS[name](iter(Q), net, pixfmt=fmt, keep_depth=keep)))
    return _planar_runs[at]


def check_identity(k, P, Q, got, want):
    assert len(got) == len(want) > len(P)
    originals = 0
    for g, w in zip(got, want):
        i = next((i for i, q in enumerate(Q) if w is q), None)
        if i is not None and k.is_tight:
            assert g is P[i]                                            # originals are the caller's objects
            originals += 1
            continue
        out = k.tight() if w.dtype == k.planar.dtype else k.as_8bit()
        assert g.dtype == out.dtype and g.size == out.frame_samples and np.array_equal(g, yuv.pack_numpy(w, out))
    return originals


LOOP_CASES = {
    "uyvy": ("uyvy", None, False),
    "yuy2": ("yuy2", None, False),
    "y210 keep": ("y210", None, True),
    "v210 keep": ("v210", None, True),
    "v210": ("v210", None, False),                     # 8-bit frames out, in uyvy
    "v210 keep pitch 256": ("v210", 256, True),        # given, and the default of W = 96
    "v210 keep pitch 384": ("v210", 384, True),
}


# (the retimed loop: one layout per depth and a pitched one)
LOOP_RUNS = [(c, n) for n in RUNS for c in LOOP_CASES if n != "retimed_dedup" or c in ("uyvy", "v210 keep", "v210 keep pitch 384")]


@pytest.mark.parametrize("case,name", LOOP_RUNS, ids=lambda v: str(v))
def test_a_packed_stream_gives_the_packed_form_of_its_planar_stream(net, dev, case, name):
    layout, pitch, keep = LOOP_CASES[case]
    k = packed_of(layout, H, W, pitch, matrix="bt709", siting="left")
    Q, want = planar_run(net, name, k.planar, keep)
    P = packed_video(k, Q)
    got = list(RUNS[name](iter(P), net, pixfmt=k, keep_depth=keep))
    originals = check_identity(k, P, Q, got, want)
    assert originals == (sum(any(w is q for q in Q) for w in want) if k.is_tight else 0) and (not k.is_tight or originals >= 2)


@pytest.mark.parametrize("layout,keep", [("uyvy", False), ("v210", True)])
def test_active_on_a_letterboxed_packed_clip(net, dev, monkeypatch, layout, keep):
    HL, WL, WIN = 128, 96, (32, 0, 64, 96)
    L5, _ = CA.letterboxed(3, HL, WL, (32, 96), seed=21, tone=150)
    k = packed_of(layout, HL, WL, siting="left")
    Q = [yuv.encode_numpy(f.astype(np.float32) / np.float32(255) if keep else f, k.planar) for f in L5]
    P = packed_video(k, Q)
    kw = dict(factor=4, max_batch=4, keep_depth=keep)
    want = list(host_io.interpolate_video_nx(iter(Q), net, pixfmt=k.planar, active=active.ActiveArea(), **kw))
    sizes = []
    for fn in ("forward", "forward_pooled"):
        klass = next(c for c in type(net).__mro__ if fn in c.__dict__)

        def wrapper(self, *a, _orig=klass.__dict__[fn], _fn=fn, **kws):
            sizes.append((a[0].hp, a[0].wp) if _fn == "forward_pooled" else tuple(a[0].shape[-2:]))
            return _orig(self, *a, **kws)
        monkeypatch.setattr(klass, fn, wrapper)
    area = active.ActiveArea()
    got = list(host_io.interpolate_video_nx(iter(P), net, pixfmt=k, active=area, **kw))
    monkeypatch.undo()
    assert area.window == WIN and area.fallback_at is None and sizes and set(sizes) == {(64, 128)}       # the window's padded size
    assert check_identity(k, P, Q, got, want) == 3
    rows = np.r_[0:32, 96:128]
    for i, g in enumerate(got):                                         # the bars: the nearer original's own samples
        near = Q[i // 4 + (i % 4 > 2)]
        for a, b in zip(k.planar.planes(yuv.unpack_numpy(g, k)), k.planar.planes(near)):
            assert np.array_equal(a[rows], b[rows])


def test_network_base_128x192_once(dev):
    base = make_net(dev, "base")
    k = packed_of("v210", 128, 192, matrix="bt709", siting="left")
    Q = shots(k.planar, 128, 192)
    P = packed_video(k, Q)
    run = RUNS["4x_pooled"]
    want = list(run(iter(Q), base, pixfmt=k.planar, keep_depth=True))
    got = list(run(iter(P), base, pixfmt=k, keep_depth=True))
    assert check_identity(k, P, Q, got, want) == 3


def test_interp_raw_tool_on_a_v210_file(dev, tmp_path):
    k = packed_of("v210", H, W, siting="left")
    P = packed_video(k, shots(k.planar, n=4))
    src, dst = tmp_path / "in.v210", tmp_path / "out.v210"
    with yuv.RawWriter(src, k) as wr:
        for p in P:
            wr.write(p)
    assert os.path.getsize(src) == 4 * k.nbytes
    tool = os.path.join(CS.ROOT, "tools", "interp_raw.py")
    r = subprocess.run([sys.executable, tool, str(src), str(dst), "--pix-fmt", "v210", "--keep-depth", "--size", f"{W}x{H}", "--fps", "24",
                        "--model", "lite", "--factor", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(dst) == 7 * k.nbytes
    with yuv.RawReader(dst, k, 48) as rd:
        got = list(rd)
    torch.set_grad_enabled(False)
    n = pkg.NetworkLite()                                               # the tool's model: synthetic weights, the defaults
    n.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    n = n.to(dev).eval()
    want = list(host_io.interpolate_video_nx(iter(P), n, factor=2, pixfmt=k, keep_depth=True))
    assert len(got) == len(want) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
