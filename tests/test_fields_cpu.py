"""Interlaced input on the host (atm-vfi_amd/fields.py): the twins against the per-pixel models of tests/cpu_fields.py, the loop on a
stand-in model against frames made by hand from the definition, the refusals, the Y4M / raw plumbing and the ABI's host checks."""
import ctypes
import importlib
import io

import numpy as np
import pytest
import torch

import cpu_fields as M
import cpu_scene as CS

fields = importlib.import_module("atm-vfi_amd.fields")
yuv = importlib.import_module("atm-vfi_amd.yuv")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
segments = importlib.import_module("atm-vfi_amd.segments")
F32 = np.float32
SHAPES = ((2, 1), (3, 5), (5, 4), (16, 32), (21, 37))


# ------------------------------------------------------------------------------------------------ the twins
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("p", (0, 1))
def test_bob_twin_is_the_model_bit_for_bit(h, w, p):
    S = M.hostile((2, h, w), seed=h * 100 + w)
    want = M.bob_model(S, p)
    got = fields.bob_numpy(S, p)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # field p's rows are kept bit for bit, and bob is idempotent
    assert np.array_equal(got[:, p::2].view(np.uint32), S[:, p::2].view(np.uint32))
    assert np.array_equal(fields.bob_numpy(got, p).view(np.uint32), got.view(np.uint32))
    top, left, hp, wp = 3, 5, h + 3 + 2, w + 5 + 6                     # unequal pads on the four sides
    can = fields.bob_numpy(S, p, canvas=(top, left, hp, wp))
    assert can.shape == (2, hp, wp) and np.array_equal(can.view(np.uint32), M.canvas_model(S, p, top, left, hp, wp).view(np.uint32))
    assert fields.bob_numpy(S[0], p).shape == (h, w)                   # a single plane


def test_bob_twin_refusals_and_parity():
    with pytest.raises(ValueError, match="h >= 2"):
        fields.bob_numpy(np.zeros((1, 1, 4), F32), 0)
    with pytest.raises(ValueError, match="float32"):
        fields.bob_numpy(np.zeros((1, 4, 4)), 0)
    with pytest.raises(ValueError, match="parity"):
        fields.bob_numpy(np.zeros((1, 4, 4), F32), 2)
    with pytest.raises(ValueError, match="does not fit"):
        fields.bob_numpy(np.zeros((1, 4, 4), F32), 0, canvas=(1, 1, 4, 8))
    for order in ("tff", "bff"):
        for k in range(6):
            assert fields.field_parity(k, order) == M.parity_model(k, order) == (k + (order == "bff")) % 2
    with pytest.raises(ValueError, match="unknown field order"):
        fields.field_parity(0, "top")
    assert host_io.deinterlace_video is fields.deinterlace_video and yuv.bob_numpy is fields.bob_numpy and yuv.weave_numpy is fields.weave_numpy


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("p", (0, 1))
def test_rows_twin_touches_no_row_of_the_other_parity(h, w, p):
    rng = np.random.default_rng(h + w + p)
    src = rng.integers(0, 256, (h, 3 * w), dtype=np.uint8)
    dst = np.full((h, 3 * w), 0xA5, np.uint8)                          # poisoned
    want = M.rows_model(dst, src, p)
    got = fields.rows_numpy(dst.copy(), src, p)
    assert np.array_equal(got, want)
    assert np.all(got[1 - p::2] == 0xA5) and np.array_equal(got[p::2], src[p::2])
    with pytest.raises(ValueError, match="one shape and type"):
        fields.rows_numpy(dst, src[:, :-1], p)


# ------------------------------------------------------------------------------------------------ the loop on a stand-in model
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend: the pair mean, counting its calls."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = 0

    def forward(self, a, b):
        self.calls += 1
        return {"I_t": (a + b) / 2}


H, W, DIV = 18, 24, 16
CANVAS = segments._canvas(H, W, DIV)                                  # (pad_top, pad_left, Hp, Wp)


def mean_forward(a, b):
    return ((torch.from_numpy(a) + torch.from_numpy(b)) / 2).numpy()


def rgb_video(n, seed=5, tone=120):
    return M.interlaced_video(n, H, W, seed=seed, tone=tone)


def fmt_video(fmt, rgb):
    """the RGB frames as frames of a planar format (10 bit: from their fp32 picture)"""
    return [yuv.encode_numpy(f.astype(F32) / F32(255) if fmt.depth == 10 else f, fmt) for f in rgb]


def stream_of(kind, rgb):
    """-> (pixfmt, frames, keywords of the loop)"""
    if kind == "rgb":
        return None, [f.copy() for f in rgb], dict(isBGR=False)
    if kind == "bgr":
        return None, [np.ascontiguousarray(f[:, :, ::-1]) for f in rgb], {}
    if kind == "i422":
        fmt = yuv.Format(H, W, "bt601", False, "left", 8, "422")
        return fmt, fmt_video(fmt, rgb), {}
    if kind == "444p10":
        fmt = yuv.Format(H, W, "bt709", False, "centre", 10, "444")
        return fmt, fmt_video(fmt, rgb), dict(keep_depth=True)
    if kind == "i422 pitch":
        fmt = yuv.Format(H, W, "bt601", False, "left", 8, "422")
        s = yuv.Surface(fmt, "planar", False, W + 8, W // 2 + 4, (W + 8) * H + 16)
        return s, [yuv.repack(f, fmt, s) for f in fmt_video(fmt, rgb)], {}
    layout, depth = {"uyvy": ("uyvy", 8), "v210": ("v210", 10)}[kind]
    k = yuv.Packed(yuv.Format(H, W, "bt709", False, "left", depth, "422"), layout)
    return k, [yuv.pack_numpy(f, k) for f in fmt_video(k.planar, rgb)], (dict(keep_depth=True) if depth == 10 else {})


def picture_of(frame, pixfmt, bgr):
    """the woven picture the network's canvas is made of: float32 [3,h,w]"""
    if isinstance(pixfmt, yuv.Packed):
        frame, pixfmt = yuv.unpack_numpy(frame, pixfmt), pixfmt.planar
    if pixfmt is not None and pixfmt.depth == 10:
        return np.ascontiguousarray(yuv.decode_numpy_f32(frame, pixfmt).transpose(2, 0, 1))
    img = frame if pixfmt is None else yuv.decode_numpy(frame, pixfmt)
    if pixfmt is None and bgr:
        img = img[:, :, ::-1]
    return (torch.tensor(np.ascontiguousarray(img.transpose(2, 0, 1))) / 255.).numpy()


def way_out(P, pixfmt, bgr):
    """the loops' ordinary way out of a prediction canvas: a frame of the output format"""
    top, left, _, _ = CANVAS
    p = np.ascontiguousarray(P[:, top:top + H, left:left + W].transpose(1, 2, 0))
    packed = pixfmt if isinstance(pixfmt, yuv.Packed) else None
    planar = pixfmt.planar if packed is not None else pixfmt
    if planar is not None and planar.depth == 10:
        out = yuv.encode_numpy(p, yuv.out_format(planar, True))
    else:
        u8 = np.round(p * 255).astype(np.uint8)
        if planar is None:
            return np.ascontiguousarray(u8[:, :, ::-1]) if bgr else u8
        out = yuv.encode_numpy(u8, yuv.out_format(planar, False))
    return out if packed is None else yuv.pack_numpy(out, packed.tight())


def by_hand(frames, pixfmt, order, mode, bgr, cuts=()):
    pics = [picture_of(f, pixfmt, bgr) for f in frames]
    preds = M.predictions_model(pics, order, mode, mean_forward, CANVAS, cuts)
    return [fields.weave_numpy(frames[k // 2], pixfmt, par, way_out(P, pixfmt, bgr)) for k, (P, par, _) in enumerate(preds)], preds


def real_rows_are_the_source(out, frame, pixfmt, par):
    if isinstance(pixfmt, yuv.Packed):
        out, frame, pixfmt = yuv.unpack_numpy(out, pixfmt.tight()), yuv.unpack_numpy(frame, pixfmt), pixfmt.planar
    if pixfmt is None:
        return np.array_equal(out[par::2], frame[par::2])
    dst = yuv.out_format(pixfmt, pixfmt.depth > 8)
    return all(np.array_equal(d[par::2], s[par::2]) for d, s in zip(dst.planes(out), pixfmt.planes(frame)))


@pytest.mark.parametrize("kind", ("rgb", "bgr", "i422", "444p10", "i422 pitch", "uyvy", "v210"))
@pytest.mark.parametrize("order", ("tff", "bff"))
def test_the_loop_gives_the_frames_made_by_hand(kind, order):
    pixfmt, frames, kw = stream_of(kind, rgb_video(3))
    bgr = kw.get("isBGR", True) and pixfmt is None
    keep = [f.copy() for f in frames]
    model = Mean()
    got = list(fields.deinterlace_video(iter(frames), model, order=order, divisor=DIV, pixfmt=pixfmt, **kw))
    want, preds = by_hand(frames, pixfmt, order, "mc", bgr)
    assert len(got) == 6 and model.calls == 4
    out_fmt = None if pixfmt is None else yuv.out_format(pixfmt, pixfmt.depth > 8)
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g.dtype == w_.dtype and g.shape == w_.shape and np.array_equal(g, w_), (kind, order, k)
        if out_fmt is not None:
            out_fmt.check(g, "test")                                   # a frame of out_format
        assert real_rows_are_the_source(g, frames[k // 2], pixfmt, preds[k][1])
    assert [b for _, _, b in preds] == [True, False, False, False, False, True]       # first and last fields are bob
    assert all(np.array_equal(a, b) for a, b in zip(frames, keep))                     # the caller's frames are untouched


def test_tff_and_bff_differ_and_bob_runs_no_forward():
    frames = rgb_video(3)
    run = lambda **kw: list(fields.deinterlace_video(frames, Mean(), divisor=DIV, isBGR=False, **kw))
    t, b = run(order="tff"), run(order="bff")
    assert any(not np.array_equal(x, y) for x, y in zip(t, b))
    assert np.array_equal(t[0][0::2], frames[0][0::2]) and np.array_equal(b[0][1::2], frames[0][1::2])
    model = Mean()
    got = list(fields.deinterlace_video(frames, model, mode="bob", divisor=DIV, isBGR=False))
    want, preds = by_hand(frames, None, "tff", "bob", False)
    assert model.calls == 0 and len(got) == 6 and all(np.array_equal(g, w_) for g, w_ in zip(got, want)) and all(b for _, _, b in preds)
    # the bob prediction of an RGB frame is the line average of its own field, rounded once more by the way out
    pic = picture_of(frames[1], None, False)
    assert np.array_equal(got[2], fields.weave_numpy(frames[1], None, 0, way_out(fields.bob_numpy(pic, 0, CANVAS), None, False)))


@pytest.mark.parametrize("n", (0, 1, 2))
def test_short_streams(n):
    frames = rgb_video(max(n, 1))[:n]
    model = Mean()
    got = list(fields.deinterlace_video(frames, model, divisor=DIV, isBGR=False))
    assert len(got) == 2 * n and model.calls == max(2 * n - 2, 0)
    if n:
        want, _ = by_hand(frames, None, "tff", "mc", False)
        assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))


def test_a_scene_cut_makes_the_fields_either_side_bob():
    A, B = rgb_video(3, seed=5, tone=70), rgb_video(2, seed=9, tone=190)
    cuts, model = host_io.SceneCuts(), Mean()
    got = list(fields.deinterlace_video(A + B, model, divisor=DIV, isBGR=False, scene=cuts))
    one = lambda v: list(fields.deinterlace_video(v, Mean(), divisor=DIV, isBGR=False))
    want = one(A) + one(B)
    assert cuts.cuts == [len(A) - 1] and len(cuts.stats) == len(A) + len(B) - 1
    assert len(got) == len(want) == 10 and all(np.array_equal(g, w_) for g, w_ in zip(got, want))
    assert model.calls == 2 * 5 - 2 - 2                                # minus two per cut
    by, _ = by_hand(A + B, None, "tff", "mc", False, cuts=(len(A) - 1,))
    assert all(np.array_equal(g, w_) for g, w_ in zip(got, by))
    # without scene= no signature is made and the pair across the cut is interpolated
    plain = list(fields.deinterlace_video(A + B, Mean(), divisor=DIV, isBGR=False))
    assert not np.array_equal(plain[5], got[5])


def test_every_refusal_gives_its_reason():
    frames, m = rgb_video(1), Mean()
    run = lambda f=frames, **kw: list(fields.deinterlace_video(f, m, divisor=DIV, **kw))
    with pytest.raises(ValueError, match=r"unknown field order 'top' \(tff, bff\)"):
        run(order="top")
    with pytest.raises(ValueError, match=r"unknown mode 'weave' \(mc, bob\)"):
        run(mode="weave")
    f420 = yuv.Format(H, W)
    for fmt in (f420, yuv.Surface.nv12(H, W), yuv.Surface.p010(H, W), yuv.Surface.i420(H, W, pitch=W + 8)):
        with pytest.raises(ValueError, match="interlaced 4:2:0 is not supported in any layout .*shared between the two fields"):
            run(pixfmt=fmt, keep_depth=True)
    f10 = yuv.Format(H, W, depth=10, subsampling="422", siting="left")
    for fmt in (f10, yuv.Packed(f10, "v210"), yuv.Packed(f10, "y210")):
        with pytest.raises(ValueError, match="10-bit pixfmt needs the depth kept: pass keep_depth=True"):
            run(pixfmt=fmt)
    with pytest.raises(ValueError, match="DeepRGB pixfmt is not deinterlaced"):
        run(pixfmt=yuv.DeepRGB(H, W, 10, "gbrp"), keep_depth=True)
    with pytest.raises(ValueError, match=r"1 row\(s\) has no two fields"):
        run([np.zeros((1, W, 3), np.uint8)])
    with pytest.raises(ValueError, match=r"1 row\(s\) has no two fields"):
        run(pixfmt=yuv.Format(1, W, subsampling="444"))
    with pytest.raises(ValueError, match=r"uint8 \[H,W,3\] frames expected"):
        run([np.zeros((4, W), np.uint8)])
    assert m.calls == 0


# ------------------------------------------------------------------------------------------------ Y4M and raw plumbing
def y4m_bytes(fmt, frames, itag, fps="25:1", ctag="422"):
    head = f"YUV4MPEG2 W{fmt.width} H{fmt.height} F{fps}" + (f" I{itag}" if itag else "") + f" A1:1 C{ctag}\n"
    return head.encode() + b"".join(b"FRAME\n" + f.tobytes() for f in frames)


def test_y4m_reader_takes_interlaced_tags_only_when_told_to():
    fmt = yuv.Format(H, W, "bt601", False, "left", 8, "422")
    frames = fmt_video(fmt, rgb_video(2))
    for tag in ("t", "b", "m"):
        with pytest.raises(ValueError, match=rf"^Y4MReader: interlaced streams are not supported \(tag I{tag}\)$"):
            yuv.Y4MReader(io.BytesIO(y4m_bytes(fmt, frames, tag)), accept=("422",))
    for tag in ("t", "b"):
        rd = yuv.Y4MReader(io.BytesIO(y4m_bytes(fmt, frames, tag)), accept=("422",), interlaced=True)
        assert rd.interlace == tag and all(np.array_equal(a, b) for a, b in zip(rd, frames))
    with pytest.raises(ValueError, match=r"mixed-mode interlacing is not supported \(tag Im"):
        yuv.Y4MReader(io.BytesIO(y4m_bytes(fmt, frames, "m")), accept=("422",), interlaced=True)
    for tag in ("p", "?", None):
        for il in (False, True):
            assert yuv.Y4MReader(io.BytesIO(y4m_bytes(fmt, frames, tag)), accept=("422",), interlaced=il).interlace == tag


def test_interpolate_y4m_deinterlaces_by_the_header_tag():
    fmt = yuv.Format(H, W, "bt601", False, "left", 8, "422")
    frames = fmt_video(fmt, rgb_video(3))
    want = list(fields.deinterlace_video(frames, Mean(), order="bff", divisor=64, pixfmt=fmt))
    dst = io.BytesIO()
    info = yuv.interpolate_y4m(io.BytesIO(y4m_bytes(fmt, frames, "b", fps="30000:1001")), dst, Mean(), interlaced="auto", deint_only=True,
                               matrix="bt601")
    assert info["frames_in"] == 3 and info["frames_out"] == 6 and str(info["fps_out"]) == "60000/1001"
    head = dst.getvalue().split(b"\n", 1)[0]
    assert b" Ip " in head and b"F60000:1001" in head
    got = list(yuv.Y4MReader(io.BytesIO(dst.getvalue()), matrix="bt601", accept=("422",)))
    assert len(got) == 6 and all(np.array_equal(g, w_) for g, w_ in zip(got, want))
    # a progressive header with "auto": the plain loop; no interlaced=: the tag is refused as ever
    info = yuv.interpolate_y4m(io.BytesIO(y4m_bytes(fmt, frames, "p")), io.BytesIO(), Mean(), interlaced="auto", matrix="bt601")
    assert info["frames_out"] == 5 and str(info["fps_out"]) == "50"
    with pytest.raises(ValueError, match=r"interlaced streams are not supported \(tag Ib\)"):
        yuv.interpolate_y4m(io.BytesIO(y4m_bytes(fmt, frames, "b")), io.BytesIO(), Mean())
    with pytest.raises(ValueError, match="unknown interlaced"):
        yuv.interpolate_y4m(io.BytesIO(b""), io.BytesIO(), Mean(), interlaced="top")
    with pytest.raises(ValueError, match="deint_only needs interlaced"):
        yuv.interpolate_y4m(io.BytesIO(y4m_bytes(fmt, frames, "p")), io.BytesIO(), Mean(), deint_only=True)


def test_interpolate_raw_on_an_interlaced_uyvy_file():
    k, frames, _ = stream_of("uyvy", rgb_video(3))
    raw = b"".join(f.tobytes() for f in frames)
    want = list(fields.deinterlace_video(frames, Mean(), divisor=64, pixfmt=k))
    dst = io.BytesIO()
    info = yuv.interpolate_raw(io.BytesIO(raw), dst, Mean(), k, 25, interlaced="tff", deint_only=True)
    assert info["frames_in"] == 3 and info["frames_out"] == 6 and info["fps_out"] == 50
    got = list(yuv.RawReader(io.BytesIO(dst.getvalue()), k, 50))
    assert len(got) == 6 and all(np.array_equal(g, w_) for g, w_ in zip(got, want))
    # the chained form: the N-x loop on the deinterlaced frames, at twice the rate
    dst = io.BytesIO()
    info = yuv.interpolate_raw(io.BytesIO(raw), dst, Mean(), k, 25, factor=2, interlaced="tff")
    chained = list(host_io.interpolate_video_nx(want, Mean(), factor=2, pixfmt=k))
    got = list(yuv.RawReader(io.BytesIO(dst.getvalue()), k, 100))
    assert info["frames_out"] == 11 and info["fps_out"] == 100 and len(got) == 11 and all(np.array_equal(g, w_) for g, w_ in zip(got, chained))
    with pytest.raises(ValueError, match="no tag for auto"):
        yuv.interpolate_raw(io.BytesIO(raw), io.BytesIO(), Mean(), k, 25, interlaced="auto")
    with pytest.raises(ValueError, match="interlaced 4:2:0 is not supported"):
        yuv.interpolate_raw(io.BytesIO(b""), io.BytesIO(), Mean(), yuv.Surface.nv12(H, W), 25, interlaced="tff")
    with pytest.raises(ValueError, match="keep_depth=True"):
        yuv.interpolate_raw(io.BytesIO(b""), io.BytesIO(), Mean(), stream_of("v210", rgb_video(1))[0], 25, interlaced="tff")


def test_weave_and_geometry_helpers():
    fmt = yuv.Format(H, W, "bt601", False, "left", 10, "422")
    s = yuv.Surface(fmt, "planar", False, 2 * W + 16, W + 8, (2 * W + 16) * H + 32)
    g = fields.plane_geometry(s.tight(), s)
    ch, cw = fmt.chroma_shape
    assert g == [(0, 0, 2 * W, 2 * W + 16, 2 * W, H), (2 * W * H, s.chroma_offset, W, W + 8, W, H),
                 (2 * W * H + W * H, s.chroma_offset + (W + 8) * H, W, W + 8, W, H)] and (ch, cw) == (H, W // 2)
    assert fields.plane_geometry(None, None, 5, 7) == [(0, 0, 21, 21, 21, 5)]
    rng = np.random.default_rng(3)
    src = yuv.repack(rng.integers(0, 1024, fmt.frame_samples).astype(np.uint16), fmt, s)
    produced = rng.integers(0, 1024, fmt.frame_samples).astype(np.uint16)
    out = fields.weave_numpy(src, s, 1, produced)
    flat = M.rows_bytes_model(produced.view(np.uint8), src.view(np.uint8), g, 1)
    assert np.array_equal(out.view(np.uint8), flat) and out is not produced


# ------------------------------------------------------------------------------------------------ the ABI
P = 1 << 30                                                           # a fake, 16-byte aligned device address: refusals come before any launch


def test_abi_version_symbols_and_refusals():
    lib = hip_ops.load_library()
    assert (lib.atmvfi_version() >> 8) & 255 >= 27
    for name in ("atmvfi_field_bob", "atmvfi_field_rows"):
        assert hasattr(lib, name) and name in hip_ops.SIGNATURES
        assert lib.atmvfi_plan_fn_id(name.encode()) >= 0
    assert hip_ops.FIELD_BOB_STRIP == 16
    err = lambda: lib.atmvfi_last_error()
    n = 3 * 32 * 48 * 4
    E, O = P + (1 << 20), P + (2 << 20)
    for args, word in (((None, E, O, 3, 32, 48, 3, 5, 21, 37), b"null"), ((P, None, None, 3, 32, 48, 3, 5, 21, 37), b"null"),
                       ((P, E, O, 0, 32, 48, 3, 5, 21, 37), b"bad shape"), ((P, E, O, 3, 32, 48, 3, 5, 1, 37), b"no two fields"),
                       ((P, E, O, 3, 32, 48, 3, 5, 30, 37), b"outside"), ((P, E, O, 3, 32, 48, 3, 12, 21, 37), b"outside"),
                       ((P, E, O, 3, 32, 48, -1, 5, 21, 37), b"outside"), ((P, E, O, 3, 32, 48, 3, 5, 21, 0), b"outside"),
                       ((P, P + n - 4, O, 3, 32, 48, 3, 5, 21, 37), b"overlaps the source"), ((P, E, P, 3, 32, 48, 3, 5, 21, 37), b"overlaps the source"),
                       ((P, E, E + n - 4, 3, 32, 48, 3, 5, 21, 37), b"two destinations overlap"), ((P, E, E, 3, 32, 48, 3, 5, 21, 37), b"two destinations overlap")):
        assert lib.atmvfi_field_bob(*args, None) == -1 and word in err(), (args, err())
    geo = lambda *planes: (ctypes.c_int64 * (6 * len(planes)))(*[v for p in planes for v in p])
    ok = (0, 0, 64, 64, 48, 8)
    for args, word in (((None, E, 1, geo(ok), 0), b"null"), ((P, None, 1, geo(ok), 0), b"null"), ((P, E, 1, None, 0), b"null"),
                       ((P, E, 0, geo(ok), 0), b"plane count"), ((P, E, 4, geo(ok, ok, ok), 0), b"plane count"),
                       ((P, E, 1, geo(ok), 2), b"parity"), ((P, E, 1, geo(ok), -1), b"parity"),
                       ((P, E, 1, geo((0, 0, 40, 64, 48, 8)), 0), b"above a pitch"), ((P, E, 1, geo((0, 0, 64, 32, 48, 8)), 0), b"above a pitch"),
                       ((P, E, 1, geo((-1, 0, 64, 64, 48, 8)), 0), b"bad geometry"), ((P, E, 1, geo((0, 0, 64, 64, 0, 8)), 0), b"bad geometry"),
                       ((P, E, 1, geo((0, 0, 64, 64, 48, 0)), 0), b"bad geometry"),
                       ((P, P, 1, geo(ok), 0), b"overlap the rows read"), ((P, P, 1, geo((0, 400, 64, 64, 48, 8)), 1), b"overlap the rows read"),
                       ((P, E, 2, geo(ok, (100, 4096, 64, 64, 48, 8)), 0), b"rows written of planes 0 and 1 overlap")):
        assert lib.atmvfi_field_rows(*args, None) == -1 and word in err(), (args, err())
    # one row and the odd parity: nothing to move, no launch, no error
    assert lib.atmvfi_field_rows(P, E, 1, geo((0, 0, 64, 64, 48, 1)), 1, None) == 0


def test_hipops_wrappers_refuse_on_the_host():
    ops = hip_ops.HipOps.__new__(hip_ops.HipOps)                      # no device: every refusal below comes before the library is touched
    ops.recording = None
    with pytest.raises(ValueError, match="contiguous CUDA fp32"):
        ops.field_bob(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="at least one of"):
        ops.field_bob(torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="contiguous CUDA uint8"):
        ops.field_rows(torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), [(0, 0, 4, 4, 4, 2)], 0)
