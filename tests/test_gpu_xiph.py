"""GPU: the frame-preparation kernel (atm-vfi_amd/csrc/frames.hip) bit for bit against its numpy model (tests/cpu_frames.py) on both of
its paths, and the Xiph evaluation (evaluate.evaluate_xiph, benchmark/evaluate.py --dataset xiph) end to end on a tree written here."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import cpu_frames as CF

pytestmark = pytest.mark.gpu
metrics = importlib.import_module("atm-vfi_amd.metrics")
evaluate = importlib.import_module("atm-vfi_amd.evaluate")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
pkg = importlib.import_module("atm-vfi_amd")

TOL_CPU = 2e-6         # kernel vs the fp64 restatement (tests/test_gpu_metrics.py)
TOL_PSNR = 1e-5
SENTINEL_F, SENTINEL_U = -7.0, 201


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _check(ops, dev, src, mode, y0, x0, h, w, hp, wp, top, left, bgr, outputs="both", src_dev=None):
    """One call against the model: both outputs bit for bit; nothing outside them is written (guard bands keep their sentinel)."""
    s = torch.from_numpy(src).to(dev) if src_dev is None else src_dev
    guard = 64
    fbuf = torch.full((3 * hp * wp + 2 * guard,), SENTINEL_F, dtype=torch.float32, device=dev)
    ubuf = torch.full((3 * h * w + 2 * guard,), SENTINEL_U, dtype=torch.uint8, device=dev)
    dst = fbuf[guard:guard + 3 * hp * wp].view(3, hp, wp) if outputs in ("both", "f32") else None
    u8 = ubuf[guard:guard + 3 * h * w].view(h, w, 3) if outputs in ("both", "u8") else None
    ops.frame_u8_window(s, mode, y0, x0, h, w, dst=dst, dst_u8=u8, pad_top=top, pad_left=left, bgr=bgr)
    torch.cuda.synchronize()
    what = (mode, y0, x0, h, w, hp, wp, top, left, bgr, outputs)
    if dst is not None:
        assert torch.equal(dst.cpu(), torch.from_numpy(CF.window_f32(src, mode, y0, x0, h, w, hp, wp, top, left, bgr))), what
    else:
        assert bool((fbuf == SENTINEL_F).all()), what
    if u8 is not None:
        assert torch.equal(u8.cpu(), torch.from_numpy(CF.window_u8(src, mode, y0, x0, h, w, bgr))), what
    else:
        assert bool((ubuf == SENTINEL_U).all()), what
    for buf, val in ((fbuf, SENTINEL_F), (ubuf, SENTINEL_U)):
        assert bool((buf[:guard] == val).all()) and bool((buf[-guard:] == val).all()), what


# (H, W, y0, x0, h, w, Hp, Wp, pad_top, pad_left) with the mode-0 window; mode 1 reads 2h x 2w from the same corner
ALIGNED = [
    (64, 96, 0, 0, 32, 48, 32, 48, 0, 0),             # no padding
    (64, 96, 8, 12, 28, 40, 32, 64, 2, 12),           # both paddings, pad_left a multiple of 4
    (72, 128, 4, 16, 30, 44, 36, 52, 1, 4),           # asymmetric: 1 above / 5 below, 4 left / 4 right
    (216, 384, 54, 96, 108, 192, 128, 192, 10, 0),    # the end-to-end tree's geometry (InputPadder(32) of 108 x 192)
]
GENERAL = [
    (64, 96, 3, 5, 27, 41, 32, 48, 2, 3),             # odd x0, w % 4 != 0, odd pad_left
    (64, 96, 0, 1, 32, 44, 32, 44, 0, 0),             # only x0 is off
    (64, 98, 0, 0, 32, 48, 32, 48, 0, 0),             # W % 4 != 0: the row pitch is not a multiple of 4
    (64, 96, 2, 4, 30, 44, 37, 51, 3, 2),             # Wp % 4 != 0, asymmetric padding 3 / 4 and 2 / 5
    (40, 60, 7, 9, 13, 11, 13, 11, 0, 0),             # small window, no padding
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("geom", ALIGNED + GENERAL)
def test_kernel_equals_model(geom, bgr, mode, ops, dev):
    H, W, y0, x0, h, w, hp, wp, top, left = geom
    if mode == 1:
        h, w = min(h, (H - y0) // 2), min(w, (W - x0) // 2)
        if geom in ALIGNED:
            w -= w % 4
    src = _frame(H, W, 11 + mode)
    for outputs in ("both", "f32", "u8"):
        _check(ops, dev, src, mode, y0, x0, h, w, max(hp, h + top), max(wp, w + left), top, left, bgr, outputs)


@pytest.mark.parametrize("mode", [0, 1])
def test_misaligned_pointers_take_the_general_path_and_agree(mode, ops, dev):
    """A source view one byte into a larger buffer, and outputs at odd offsets: same results as from aligned memory."""
    H, W = 64, 96
    src = _frame(H, W, 21)
    big = torch.zeros(H * W * 3 + 16, dtype=torch.uint8, device=dev)
    view = big[1:1 + H * W * 3].view(H, W, 3)
    view.copy_(torch.from_numpy(src).to(dev))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    h, w = (32, 48) if mode == 0 else (30, 44)
    _check(ops, dev, src, mode, 2, 4, h, w, 36, 52, 3, 4, True, "both", src_dev=view)
    # aligned source, outputs one element into their buffers (the fp32 planes 4-byte, the uint8 output 1-byte aligned)
    s = torch.from_numpy(src).to(dev)
    fbuf = torch.zeros(3 * 36 * 52 + 1, dtype=torch.float32, device=dev)
    ubuf = torch.zeros(3 * h * w + 1, dtype=torch.uint8, device=dev)
    dst, u8 = fbuf[1:].view(3, 36, 52), ubuf[1:].view(h, w, 3)
    ops.frame_u8_window(s, mode, 2, 4, h, w, dst=dst, dst_u8=u8, pad_top=3, pad_left=4)
    assert torch.equal(dst.cpu(), torch.from_numpy(CF.window_f32(src, mode, 2, 4, h, w, 36, 52, 3, 4)))
    assert torch.equal(u8.cpu(), torch.from_numpy(CF.window_u8(src, mode, 2, 4, h, w)))
    assert float(fbuf[0]) == 0.0 and int(ubuf[0]) == 0


@pytest.mark.parametrize("category", evaluate.XIPH_CATEGORIES)
def test_full_size_frame(category, ops, dev):
    """2160 x 4096 -> 1080 x 2048 padded to 1088 x 2048 (InputPadder(32): 4 rows above and below), as both Xiph categories need it."""
    src = _frame(2160, 4096, 31)
    mode, y0, x0, h, w = evaluate.xiph_geometry(2160, 4096, category)
    assert (mode, y0, x0, h, w) == CF.xiph_geometry(2160, 4096, category)
    _check(ops, dev, src, mode, y0, x0, h, w, 1088, 2048, 4, 0, False, "both")


@pytest.mark.parametrize("bgr", [False, True])
def test_mode0_full_frame_equals_frame_u8_to_f32(bgr, ops, dev):
    src = torch.from_numpy(_frame(270, 480, 41)).to(dev)
    want = torch.empty(3, 320, 512, dtype=torch.float32, device=dev)
    ops.frame_u8_to_f32(src, want, 25, 16, bgr)
    got = torch.empty_like(want)
    ops.frame_u8_window(src, 0, 0, 0, 270, 480, dst=got, pad_top=25, pad_left=16, bgr=bgr)
    assert torch.equal(got, want)


def test_binding_rejects_bad_tensors(ops, dev):
    src = torch.zeros(16, 16, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="dst, dst_u8 or both"):
        ops.frame_u8_window(src, 0, 0, 0, 8, 8)
    with pytest.raises(ValueError, match=r"\[8,8,3\]"):
        ops.frame_u8_window(src, 0, 0, 0, 8, 8, dst_u8=torch.zeros(8, 9, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="fp32"):
        ops.frame_u8_window(src, 0, 0, 0, 8, 8, dst=torch.zeros(3, 8, 8, dtype=torch.float16, device=dev))
    with pytest.raises(RuntimeError, match="window outside the frame"):
        ops.frame_u8_window(src, 1, 0, 0, 9, 8, dst=torch.zeros(3, 9, 8, device=dev))


# ---------------------------------------------------------------------------------------- evaluation
CLIPS = ("ClipA", "ClipB")
FRAMES = range(2, 7, 2)          # frames 001-007: middle frames 2, 4, 6


def _write_tree(root, h=216, w=384):
    """Two clips, frames 001-007: a smooth scene drifting a little from frame to frame, plus per-pixel noise so that the 2x2 rule sees ties."""
    import pairs
    from PIL import Image
    for ci, clip in enumerate(CLIPS):
        a, b = pairs.smooth_pair(1, h, w, 70 + ci)
        rng = np.random.default_rng(80 + ci)
        os.makedirs(os.path.join(root, clip))
        for k in range(1, 8):
            t = (k - 1) / 6.0
            fr = ((1 - t) * a + t * b)[0].permute(1, 2, 0).numpy() * 255 + rng.integers(-3, 4, size=(h, w, 3))
            Image.fromarray(np.clip(np.round(fr), 0, 255).astype(np.uint8)).save(os.path.join(root, clip, f"{k:03d}.png"))
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _write_tree(str(tmp_path_factory.mktemp("xiph")))


@pytest.fixture(scope="module")
def lite(dev):
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    return net.to(dev).eval()


def _model_inputs(sample, category):
    """(im0, im1 fp32 [1,3,128,192], gt uint8 [108,192,3]) of one triplet from the numpy model alone."""
    f0, gt, f2 = (evaluate.read_rgb(q) for q in sample.frames)
    mode, y0, x0, h, w = CF.xiph_geometry(*f0.shape[:2], category)
    left, right, top, bottom = host_io.InputPadder((h, w), divisor=32)._pad
    ims = [torch.from_numpy(CF.window_f32(f, mode, y0, x0, h, w, h + top + bottom, w + left + right, top, left))[None] for f in (f0, f2)]
    return ims[0], ims[1], CF.window_u8(gt, mode, y0, x0, h, w), (top, left, h, w)


def _expected(net, samples, dev, tta=False):
    net.global_motion = True
    preds, vals, names = [], [], []
    for cat in evaluate.XIPH_CATEGORIES:
        for s in samples:
            im0, im1, gt, (top, left, h, w) = _model_inputs(s, cat)
            assert im0.shape == (1, 3, 128, 192) and gt.shape == (108, 192, 3)
            im0, im1 = im0.to(dev), im1.to(dev)
            out = net.forward(im0, im1)["I_t"]
            if tta:
                flip = net.forward(im0.flip(2).flip(3).contiguous(), im1.flip(2).flip(3).contiguous())["I_t"]
                out = (out + flip.flip(2).flip(3)) / 2
            out = out[..., top:top + h, left:left + w]
            preds.append(out[0].clone())
            vals.append(CF.xiph_metrics(gt, out.cpu()))
            names.append((cat, s.name))
    return preds, vals, names


def test_evaluate_xiph_end_to_end(tree, lite, dev):
    samples = evaluate.xiph(tree, CLIPS, FRAMES)
    assert len(samples) == 6
    res = evaluate.evaluate_xiph(lite, tree, clips=CLIPS, frames=FRAMES, keep_predictions=True)
    assert lite.global_motion is True
    preds, vals, names = _expected(lite, samples, dev)
    # category-major, then clip, then frame
    assert [(r["level"], r["name"]) for r in res.records] == names
    assert names[0] == ("resized-2k", "ClipA/002") and names[3] == ("resized-2k", "ClipB/002") and names[6] == ("cropped-4k", "ClipA/002")
    assert len(res.predictions) == 12
    for got, want, nm in zip(res.predictions, preds, names):
        assert got.shape == (3, 108, 192) and torch.equal(got, want), nm
    for rec, (p, s) in zip(res.records, vals):
        print(rec["level"], rec["name"], f"psnr {rec['psnr']:.6f} (restatement {p:.6f}, |d| {abs(rec['psnr'] - p):.2e})",
              f"ssim {rec['ssim']:.7f} (|d| {abs(rec['ssim'] - s):.2e})")
        assert abs(rec["psnr"] - p) <= TOL_PSNR and abs(rec["ssim"] - s) <= TOL_CPU, (rec, p, s)
    assert list(res.levels) == list(evaluate.XIPH_CATEGORIES)
    for ci, cat in enumerate(evaluate.XIPH_CATEGORIES):
        lv = res.levels[cat]
        assert lv["n"] == 6
        assert lv["psnr"] == float(np.mean([r["psnr"] for r in res.records[6 * ci:6 * ci + 6]]))      # the true mean over all samples
        assert lv["ssim"] == float(np.mean([r["ssim"] for r in res.records[6 * ci:6 * ci + 6]]))
    key = lambda r: [(x["level"], x["name"], x["psnr"], x["ssim"]) for x in r.records]        # noqa: E731
    # K forwards in flight: identical records
    assert key(evaluate.evaluate_xiph(lite, tree, clips=CLIPS, frames=FRAMES, streams=2)) == key(res)
    # limit counts triplets per category; one category alone
    lim = evaluate.evaluate_xiph(lite, tree, clips=CLIPS, frames=FRAMES, limit=4)
    assert key(lim) == key(res)[:4] + key(res)[6:10]
    one = evaluate.evaluate_xiph(lite, tree, clips=CLIPS, frames=FRAMES, categories=("cropped-4k",))
    assert key(one) == key(res)[6:] and list(one.levels) == ["cropped-4k"]
    text = evaluate.format_levels(res)
    assert all(cat in line and "Avg PSNR: " in line and "SSIM: " in line for cat, line in zip(evaluate.XIPH_CATEGORIES, text.splitlines()))


def test_evaluate_xiph_tta_is_the_flip_average(tree, lite, dev):
    samples = evaluate.xiph(tree, CLIPS[:1], FRAMES)
    res = evaluate.evaluate_xiph(lite, tree, clips=CLIPS[:1], frames=FRAMES, tta=True, keep_predictions=True)
    preds, vals, names = _expected(lite, samples, dev, tta=True)
    assert [(r["level"], r["name"]) for r in res.records] == names
    for got, want, nm in zip(res.predictions, preds, names):
        assert torch.equal(got, want), nm
    for rec, (p, s) in zip(res.records, vals):
        assert abs(rec["psnr"] - p) <= TOL_PSNR and abs(rec["ssim"] - s) <= TOL_CPU, (rec, p, s)


def test_every_png_is_decoded_once(tree, lite, monkeypatch):
    calls = []
    real = evaluate.read_rgb

    def counted(path):
        calls.append(path)
        return real(path)
    monkeypatch.setattr(evaluate, "read_rgb", counted)
    res = evaluate.evaluate_xiph(lite, tree, clips=CLIPS, frames=FRAMES)
    assert len(res.records) == 12
    assert len(calls) == 14 and len(set(calls)) == 14          # 2 clips x 7 frames, both categories, 6 triplets that share frames


def test_evaluate_xiph_rejects_other_sizes(tmp_path, lite):
    _write_tree(str(tmp_path / "t"), h=214, w=384)
    with pytest.raises(ValueError, match="% 4"):
        evaluate.evaluate_xiph(lite, str(tmp_path / "t"), clips=CLIPS[:1], frames=FRAMES)


def test_cli_on_xiph_tree(tree, tmp_path, dev, capsys):
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    ck = str(tmp_path / "ck.pt")
    host_io.save_checkpoint(net, ck)
    cli = importlib.import_module("benchmark.evaluate")
    out_json = str(tmp_path / "r.json")
    res = cli.main(["--dataset", "xiph", "--path", tree, "--clips", ",".join(CLIPS), "--frames", "2:7:2", "--ckpt", ck, "--model", "lite", "--limit", "3",
                    "--json", out_json, "--timings"])
    out = capsys.readouterr().out
    for cat in evaluate.XIPH_CATEGORIES:
        assert any(cat in line and "Avg PSNR: " in line and "SSIM: " in line for line in out.splitlines()), out
    assert "decode_wait" in out and "forward" in out
    rec = json.load(open(out_json))
    assert [r["level"] for r in rec["records"]] == ["resized-2k"] * 3 + ["cropped-4k"] * 3 and len(res.records) == 6
    assert set(rec["levels"]) == set(evaluate.XIPH_CATEGORIES) and rec["global_motion"] is True
