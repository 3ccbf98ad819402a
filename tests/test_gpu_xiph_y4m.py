"""GPU: the fused decode-window kernel (atm-vfi_amd/csrc/yuv.hip, atmvfi_yuv_decode with mode) bit for bit against the two-call
composition it replaces (``yuv420_to_rgb`` -> uint8, then ``frame_u8_window``) and against the per-pixel model
(tests/cpu_yuv_window.py), on both of its paths; and the Xiph evaluation on Y4M clips (evaluate.evaluate_xiph, benchmark/evaluate.py
--dataset xiph --source y4m) against the same evaluation on a PNG tree holding ``yuv.decode_numpy`` of the same frames."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import cpu_yuv_window as CW

pytestmark = pytest.mark.gpu
evaluate = importlib.import_module("atm-vfi_amd.evaluate")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")
pkg = importlib.import_module("atm-vfi_amd")

SENTINEL_F, SENTINEL_U = -7.0, 201
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


def _fmt(H, W, f):
    _, depth, matrix, full, siting = f
    return yuv.Format(H, W, matrix, bool(full), siting, depth)


def _upload(frame, dev, offset=0):
    """The frame's bytes on the device, ``offset`` bytes into a larger buffer."""
    b = torch.from_numpy(np.array(frame).view(np.uint8))          # (a writable copy of the shared frame)
    big = torch.zeros(b.numel() + 16, dtype=torch.uint8, device=dev)
    view = big[offset:offset + b.numel()]
    view.copy_(b.to(dev))
    assert view.data_ptr() % 4 == offset % 4
    return view


def _composition(ops, dev, src, fmt, mode, y0, x0, h, w, hp, wp, top, left):
    """The yardstick: the whole frame decoded to uint8 RGB, then frame_u8_window (from aligned memory)."""
    rgb = torch.empty(fmt.height, fmt.width, 3, dtype=torch.uint8, device=dev)
    ops.yuv420_to_rgb(src, fmt, dst_u8=rgb)
    dst = torch.empty(3, hp, wp, dtype=torch.float32, device=dev)
    u8 = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    ops.frame_u8_window(rgb, mode, y0, x0, h, w, dst=dst, dst_u8=u8, pad_top=top, pad_left=left)
    return dst, u8


def _check(ops, dev, src, fmt, mode, win, hp, wp, top, left, want, outputs="both", f32_offset=0):
    """One call into poisoned, guard-banded outputs: both outputs bit for bit ``want`` (dst, dst_u8); an output that was not asked
    for and the guard bands keep their sentinel, and no poison survives inside an output."""
    y0, x0, h, w = win
    fbuf = torch.full((3 * hp * wp + 2 * GUARD,), SENTINEL_F, dtype=torch.float32, device=dev)
    ubuf = torch.full((3 * h * w + 2 * GUARD,), SENTINEL_U, dtype=torch.uint8, device=dev)
    g = GUARD + f32_offset
    dst = fbuf[g:g + 3 * hp * wp].view(3, hp, wp) if outputs in ("both", "f32") else None
    u8 = ubuf[GUARD:GUARD + 3 * h * w].view(h, w, 3) if outputs in ("both", "u8") else None
    ops.yuv420_window(src, fmt, mode, y0, x0, h, w, dst=dst, dst_u8=u8, pad_top=top, pad_left=left)
    torch.cuda.synchronize()
    what = (fmt, mode, win, hp, wp, top, left, outputs, f32_offset)
    if dst is not None:
        assert torch.equal(dst, want[0]), what
    else:
        assert bool((fbuf == SENTINEL_F).all()), what
    if u8 is not None:
        assert torch.equal(u8, want[1]), what
    else:
        assert bool((ubuf == SENTINEL_U).all()), what
    assert bool((fbuf[:g] == SENTINEL_F).all()) and bool((fbuf[g + 3 * hp * wp:] == SENTINEL_F).all()), what
    assert bool((ubuf[:GUARD] == SENTINEL_U).all()) and bool((ubuf[-GUARD:] == SENTINEL_U).all()), what


def _paddings(h, w):
    """(Hp, Wp, pad_top, pad_left): none; (3, 4) with the canvas larger below and on the right; pad_left = 5 (the general path)."""
    return [(h, w, 0, 0), (h + 3 + 2, w + 4 + 4, 3, 4), (h + 1, w + 5 + 2, 0, 5)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("f", CW.FORMATS, ids=[f[0] for f in CW.FORMATS])
@pytest.mark.parametrize("geom", [CW.WHOLE_16, CW.INNER_40x56], ids=["whole16", "inner40x56"])
def test_kernel_equals_composition_and_model(geom, f, mode, ops, dev):
    (H, W), windows = geom
    fmt, win = _fmt(H, W, f), windows[mode]
    frame = CW.frame(H, W, fmt.depth)
    src = _upload(frame, dev)
    rgb = CW.decoded(H, W, fmt.depth, fmt.matrix, int(fmt.full_range), fmt.siting)
    for hp, wp, top, left in _paddings(*win[2:]):
        want = _composition(ops, dev, src, fmt, mode, *win, hp, wp, top, left)
        assert torch.equal(want[0].cpu(), torch.from_numpy(CW.window_f32(rgb, mode, *win, hp, wp, top, left)))      # the loop model
        assert torch.equal(want[1].cpu(), torch.from_numpy(CW.window_u8(rgb, mode, *win)))
        assert np.array_equal(want[1].cpu().numpy(), yuv.window_numpy(frame, fmt, mode, *win))
        for outputs in ("both", "f32", "u8"):
            _check(ops, dev, src, fmt, mode, win, hp, wp, top, left, want, outputs)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("f", [CW.FORMATS[0], CW.FORMATS[-1]], ids=[CW.FORMATS[0][0], CW.FORMATS[-1][0]])
@pytest.mark.parametrize("geom", [CW.ODD_37x53, CW.WIDE_16x4200], ids=["odd37x53", "wide16x4200"])
def test_odd_and_wide_frames(geom, f, mode, ops, dev):
    (H, W), windows = geom
    fmt, win = _fmt(H, W, f), windows[mode]
    frame = CW.frame(H, W, fmt.depth)
    src = _upload(frame, dev)
    for hp, wp, top, left in _paddings(*win[2:]):
        want = _composition(ops, dev, src, fmt, mode, *win, hp, wp, top, left)
        if H * W <= 40 * 56:
            rgb = CW.decoded(H, W, fmt.depth, fmt.matrix, int(fmt.full_range), fmt.siting)
            assert torch.equal(want[0].cpu(), torch.from_numpy(CW.window_f32(rgb, mode, *win, hp, wp, top, left)))
            assert torch.equal(want[1].cpu(), torch.from_numpy(CW.window_u8(rgb, mode, *win)))
        for outputs in ("both", "f32", "u8"):
            _check(ops, dev, src, fmt, mode, win, hp, wp, top, left, want, outputs)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("f", [CW.FORMATS[1], CW.FORMATS[-2]], ids=[CW.FORMATS[1][0], CW.FORMATS[-2][0]])
def test_misaligned_pointers_take_the_general_path_and_agree(f, mode, ops, dev):
    """The source one byte into its buffer, then the fp32 destination 4 bytes off a 16-byte boundary: the bits of the aligned call."""
    (H, W), windows = CW.INNER_40x56
    fmt, win = _fmt(H, W, f), windows[mode]
    frame = CW.frame(H, W, fmt.depth)
    src = _upload(frame, dev)
    h, w = win[2:]
    hp, wp, top, left = h + 5, w + 8, 3, 4
    want = _composition(ops, dev, src, fmt, mode, *win, hp, wp, top, left)
    _check(ops, dev, src, fmt, mode, win, hp, wp, top, left, want)                                    # aligned
    _check(ops, dev, _upload(frame, dev, offset=1), fmt, mode, win, hp, wp, top, left, want)          # source + 1 byte
    _check(ops, dev, src, fmt, mode, win, hp, wp, top, left, want, f32_offset=1)                      # fp32 destination + 4 bytes


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("f", [CW.FORMATS[2], CW.FORMATS[-1]], ids=[CW.FORMATS[2][0], CW.FORMATS[-1][0]])
def test_an_origin_of_two_mod_four_takes_the_general_path_and_agrees(f, mode, ops, dev):
    """W = 8 * odd: the centre crop starts at x0 = W / 4 with x0 % 4 == 2 while everything else is aligned.  Chroma pairs would straddle
    there, so the call must take the general path: the dispatch boundary, held to the composition and the loop model."""
    (H, W), windows = CW.CROP_24x72
    assert evaluate.xiph_geometry(H, W, "cropped-4k") == (0,) + windows[0] and windows[0][1] % 4 == 2 and windows[0][3] % 4 == 0
    fmt, win = _fmt(H, W, f), windows[mode]
    src = _upload(CW.frame(H, W, fmt.depth), dev)
    rgb = CW.decoded(H, W, fmt.depth, fmt.matrix, int(fmt.full_range), fmt.siting)
    for hp, wp, top, left in _paddings(*win[2:])[:2]:
        want = _composition(ops, dev, src, fmt, mode, *win, hp, wp, top, left)
        assert torch.equal(want[0].cpu(), torch.from_numpy(CW.window_f32(rgb, mode, *win, hp, wp, top, left)))
        assert torch.equal(want[1].cpu(), torch.from_numpy(CW.window_u8(rgb, mode, *win)))
        for outputs in ("both", "f32", "u8"):
            _check(ops, dev, src, fmt, mode, win, hp, wp, top, left, want, outputs)


@pytest.mark.parametrize("category", evaluate.XIPH_CATEGORIES)
def test_full_size_frame(category, ops, dev):
    """2160 x 4096, 10 bit, bt709 -> 1080 x 2048 padded to 1088 x 2048 (InputPadder(32)), as both Xiph categories need it."""
    fmt = yuv.Format(2160, 4096, depth=10)
    assert fmt.matrix == "bt709"
    gen = torch.Generator(device=dev).manual_seed(31)
    src = torch.randint(0, 1024, (fmt.frame_samples,), dtype=torch.int16, device=dev, generator=gen).view(torch.uint8)
    mode, y0, x0, h, w = evaluate.xiph_geometry(2160, 4096, category)
    want = _composition(ops, dev, src, fmt, mode, y0, x0, h, w, 1088, 2048, 4, 0)
    _check(ops, dev, src, fmt, mode, (y0, x0, h, w), 1088, 2048, 4, 0, want)


def test_binding_rejects_bad_tensors(ops, dev):
    fmt = yuv.Format(16, 16)
    src = torch.zeros(fmt.frame_bytes, dtype=torch.uint8, device=dev)
    ok = torch.zeros(8, 8, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="dst, dst_u8 or both"):
        ops.yuv420_window(src, fmt, 0, 0, 0, 8, 8)
    with pytest.raises(ValueError, match="uint8 tensor of 384 bytes"):                  # dtype
        ops.yuv420_window(src.view(torch.int8), fmt, 0, 0, 0, 8, 8, dst_u8=ok)
    with pytest.raises(ValueError, match="uint8 tensor of 384 bytes"):                  # shape
        ops.yuv420_window(src.view(24, 16), fmt, 0, 0, 0, 8, 8, dst_u8=ok)
    with pytest.raises(ValueError, match="uint8 tensor of 384 bytes"):                  # device
        ops.yuv420_window(src.cpu(), fmt, 0, 0, 0, 8, 8, dst_u8=ok)
    with pytest.raises(ValueError, match="uint8 tensor of 384 bytes"):                  # byte count
        ops.yuv420_window(src[:-1], fmt, 0, 0, 0, 8, 8, dst_u8=ok)
    with pytest.raises(ValueError, match="uint8 tensor of 768 bytes"):                  # an 8-bit frame for a 10-bit format
        ops.yuv420_window(src, yuv.Format(16, 16, depth=10), 0, 0, 0, 8, 8, dst_u8=ok)
    with pytest.raises(ValueError, match="must be even"):
        ops.yuv420_window(src, fmt, 0, 1, 0, 8, 8, dst_u8=ok)
    with pytest.raises(ValueError, match="must be even"):
        ops.yuv420_window(src, fmt, 1, 0, 3, 4, 4, dst_u8=ok[:4, :4].contiguous())
    with pytest.raises(ValueError, match=r"\[8,8,3\]"):
        ops.yuv420_window(src, fmt, 0, 0, 0, 8, 8, dst_u8=torch.zeros(8, 9, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="fp32"):
        ops.yuv420_window(src, fmt, 0, 0, 0, 8, 8, dst=torch.zeros(3, 8, 8, dtype=torch.float16, device=dev))
    with pytest.raises(RuntimeError, match="window outside the frame"):
        ops.yuv420_window(src, fmt, 1, 0, 0, 9, 8, dst=torch.zeros(3, 9, 8, device=dev))
    with pytest.raises(RuntimeError, match="smaller than the window"):
        ops.yuv420_window(src, fmt, 0, 0, 0, 8, 8, dst=torch.zeros(3, 8, 8, device=dev), pad_left=4)


# ---------------------------------------------------------------------------------------- evaluation
CLIPS = ("ClipA", "ClipB")
FRAMES = range(2, 7, 2)          # frames 001-007: middle frames 2, 4, 6
H, W = 216, 384


def _scene(ci):
    """Seven fp32 [H,W,3] frames in [0, 1]: a smooth scene drifting a little, plus per-pixel noise so that the 2x2 rule sees ties."""
    import pairs
    a, b = pairs.smooth_pair(1, H, W, 70 + ci)
    rng = np.random.default_rng(80 + ci)
    out = []
    for k in range(7):
        t = k / 6.0
        fr = ((1 - t) * a + t * b)[0].permute(1, 2, 0).numpy() * 255 + rng.integers(-3, 4, size=(H, W, 3))
        out.append(np.clip(np.round(fr), 0, 255).astype(np.float32) / np.float32(255))
    return out


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """(Y4M root, PNG root, mixed root): ClipA as C420jpeg under its plain name, ClipB as C420p10 under a download-style name, both
    through Y4MWriter; the PNG tree holds yuv.decode_numpy of those same frames; the mixed root has ClipA as a directory and ClipB as Y4M."""
    from PIL import Image
    base = tmp_path_factory.mktemp("xiph_y4m")
    y4m, png, mixed = (str(base / n) for n in ("y4m", "png", "mixed"))
    for d in (y4m, png, mixed):
        os.makedirs(d)
    fmts = {"ClipA": yuv.Format(H, W), "ClipB": yuv.Format(H, W, depth=10)}
    names = {"ClipA": "ClipA.y4m", "ClipB": f"Netflix_ClipB_{W}x{H}_60fps_10bit_420.y4m"}
    for ci, clip in enumerate(CLIPS):
        fmt = fmts[clip]
        frames = [yuv.encode_numpy(fr if fmt.depth == 10 else np.rint(fr * 255).astype(np.uint8), fmt) for fr in _scene(ci)]
        for root in (y4m, mixed) if clip == "ClipB" else (y4m,):
            with yuv.Y4MWriter(os.path.join(root, names[clip]), fmt, 60) as wr:
                assert wr.ctag == ("420p10" if fmt.depth == 10 else "420jpeg")
                for fr in frames:
                    wr.write(fr)
        for root in (png, mixed) if clip == "ClipA" else (png,):
            os.makedirs(os.path.join(root, clip))
            for k, fr in enumerate(frames):
                Image.fromarray(yuv.decode_numpy(fr, fmt)).save(os.path.join(root, clip, f"{k + 1:03d}.png"))
    return y4m, png, mixed


@pytest.fixture(scope="module")
def lite(dev):
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def png_result(roots, lite):
    """The reference of every comparison below, computed once: the PNG path of today on the decoded frames."""
    return evaluate.evaluate_xiph(lite, roots[1], clips=CLIPS, frames=FRAMES, keep_predictions=True)


def _key(r):
    return [(x["level"], x["name"], x["psnr"], x["ssim"]) for x in r.records]


def test_y4m_root_scores_exactly_as_the_png_tree(roots, lite, png_result):
    src = {}
    res = evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS, frames=FRAMES, keep_predictions=True, sources=src)
    assert src == {"ClipA": "y4m", "ClipB": "y4m"}
    assert len(res.records) == 12 and _key(res) == _key(png_result)                   # PSNR and SSIM compared with ==
    assert res.levels == png_result.levels and list(res.levels) == list(evaluate.XIPH_CATEGORIES)
    for got, want in zip(res.predictions, png_result.predictions):
        assert got.shape == (3, 108, 192) and torch.equal(got, want)
    # K forwards in flight; limit counts triplets per category; one category alone
    assert _key(evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS, frames=FRAMES, streams=2)) == _key(png_result)
    assert _key(evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS, frames=FRAMES, limit=4)) == _key(png_result)[:4] + _key(png_result)[6:10]
    one = evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS, frames=FRAMES, categories=("cropped-4k",))
    assert _key(one) == _key(png_result)[6:] and list(one.levels) == ["cropped-4k"]
    # forcing the source; a forced source that is not there
    assert _key(evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS[:1], frames=FRAMES, source="y4m")) == \
        [k for k in _key(png_result) if k[1].startswith("ClipA/")]
    with pytest.raises(FileNotFoundError, match="001.png"):
        evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS, frames=FRAMES, source="png")


def test_y4m_tta_is_the_png_tree_tta(roots, lite):
    want = evaluate.evaluate_xiph(lite, roots[1], clips=CLIPS[1:], frames=FRAMES, tta=True, keep_predictions=True)
    got = evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS[1:], frames=FRAMES, tta=True, keep_predictions=True)
    assert _key(got) == _key(want) and len(got.records) == 6
    for a, b in zip(got.predictions, want.predictions):
        assert torch.equal(a, b)


def test_every_frame_is_read_once_uploaded_once_and_never_decoded_to_rgb(roots, lite, png_result, monkeypatch):
    reads, uploads = [], []

    class Counting(yuv.Y4MReader):
        def __iter__(self):
            for fr in super().__iter__():
                reads.append((self.f.name, self.fmt.depth))
                yield fr
    real_upload = evaluate._upload_i420

    def upload(frame, dev):
        uploads.append(frame.nbytes)
        return real_upload(frame, dev)

    def never(*a, **k):
        raise AssertionError("the Y4M path must not decode to an RGB frame")
    monkeypatch.setattr(evaluate.yuv, "Y4MReader", Counting)
    monkeypatch.setattr(evaluate, "_upload_i420", upload)
    monkeypatch.setattr(hip_ops.HipOps, "yuv420_to_rgb", never)
    monkeypatch.setattr(hip_ops.HipOps, "frame_u8_window", never)
    res = evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS, frames=FRAMES)
    assert _key(res) == _key(png_result)
    assert len(reads) == 14 and [d for _, d in reads] == [8] * 7 + [10] * 7           # 2 clips x 7 frames, each clip walked once
    assert uploads == [H * W * 3 // 2] * 7 + [H * W * 3] * 7                         # the I420 bytes: 1.5 B/px, 3 B/px at 10 bit


def test_mixed_root_reports_its_sources(roots, lite, png_result):
    src = {}
    res = evaluate.evaluate_xiph(lite, roots[2], clips=CLIPS, frames=FRAMES, sources=src)
    assert src == {"ClipA": "png", "ClipB": "y4m"} and _key(res) == _key(png_result)
    with pytest.raises(FileNotFoundError, match="ClipA.y4m"):
        evaluate.evaluate_xiph(lite, roots[2], clips=CLIPS, frames=FRAMES, source="y4m")


def test_short_stream_raises(roots, lite):
    with pytest.raises(ValueError, match=r"ClipB.*frame 7.*only 7 frames"):
        evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS[1:], frames=range(2, 9, 2))


def test_descending_frames_are_refused_on_y4m_and_still_scored_from_png(roots, lite):
    """``frames=range(6, 1, -2)`` is a valid range: the PNG tree scores it, a Y4M stream (read forward once) refuses it at once."""
    with pytest.raises(ValueError, match="must ascend"):
        evaluate.evaluate_xiph(lite, roots[0], clips=CLIPS[:1], frames=range(6, 1, -2))
    res = evaluate.evaluate_xiph(lite, roots[1], clips=CLIPS[:1], frames=range(6, 1, -2), categories=("cropped-4k",))
    assert [r["name"] for r in res.records] == ["ClipA/006", "ClipA/004", "ClipA/002"]


def test_cli_on_y4m_root(roots, tmp_path, dev, capsys):
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    ck = str(tmp_path / "ck.pt")
    host_io.save_checkpoint(net, ck)
    cli = importlib.import_module("benchmark.evaluate")
    out_json = str(tmp_path / "r.json")
    res = cli.main(["--dataset", "xiph", "--path", roots[0], "--clips", ",".join(CLIPS), "--frames", "2:7:2", "--ckpt", ck, "--model", "lite",
                    "--limit", "3", "--json", out_json, "--timings", "--source", "y4m"])
    out = capsys.readouterr().out
    for cat in evaluate.XIPH_CATEGORIES:
        assert any(cat in line and "Avg PSNR: " in line and "SSIM: " in line for line in out.splitlines()), out
    assert "decode_wait" in out and "decode_cpu" in out and "forward" in out
    rec = json.load(open(out_json))
    assert rec["sources"] == {"ClipA": "y4m", "ClipB": "y4m"}
    assert [r["level"] for r in rec["records"]] == ["resized-2k"] * 3 + ["cropped-4k"] * 3 and len(res.records) == 6
    assert set(rec["levels"]) == set(evaluate.XIPH_CATEGORIES) and rec["global_motion"] is True
