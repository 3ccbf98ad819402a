"""CPU: the numpy model of the frame-preparation kernel (tests/cpu_frames.py) against PIL's independent 2x reduction and the Xiph
script's literal geometry, the Xiph lister and protocol, the host-side argument checks of atmvfi_frame_u8_window, the CLI and the
drop-in ``read``, and the Xiph metric arithmetic against the reference's own outputs (tests/golden/xiph_ref.npz)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import cpu_frames as CF
import metric_inputs as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
metrics = importlib.import_module("atm-vfi_amd.metrics")
evaluate = importlib.import_module("atm-vfi_amd.evaluate")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")

TOL_GOLD = 3e-6        # as tests/test_metrics_cpu.py: the reference's fp32 conv3d against the fp64 restatement
TOL_PSNR = 1e-5


@pytest.mark.parametrize("seed,h,w", [(0, 64, 96), (1, 38, 50), (2, 216, 384)])
def test_area_rule_equals_pil_reduce(seed, h, w):
    """PIL's Image.reduce(2) is an independent implementation of the same rule (box average, halves rounded up).  cv2 itself is not
    available where this suite runs; INTER_AREA on uint8 at an exact scale of 2 is this rule by its definition."""
    from PIL import Image
    src = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    s = src.astype(np.int32)
    ties = ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]) % 4 == 2).mean()
    assert ties >= 0.20, f"only {ties:.3f} of the outputs are ties: the rounding rule would go untested"
    want = np.asarray(Image.fromarray(src).reduce(2))
    assert np.array_equal(CF.area2(src), want)
    assert np.array_equal(CF.window_u8(src, 1, 0, 0, h // 2, w // 2), want)
    # a window of the reduction = the reduction of the window
    assert np.array_equal(CF.window_u8(src, 1, 6, 10, 9, 13), np.asarray(Image.fromarray(src[6:24, 10:36]).reduce(2)))
    # explicit ties: (0, 0, 1, 1) -> 2/4 rounds up to 1; (255, 255, 254, 254) -> 255
    t = np.array([[[0], [0]], [[1], [1]]], dtype=np.uint8).repeat(3, axis=2)
    assert CF.area2(t).tolist() == [[[1, 1, 1]]] and CF.area2(255 - t).tolist() == [[[255, 255, 255]]]


def test_model_window_swap_division_and_padding():
    src = np.random.default_rng(3).integers(0, 256, size=(20, 28, 3), dtype=np.uint8)
    u8 = CF.window_u8(src, 0, 3, 5, 10, 17, bgr=True)
    assert np.array_equal(u8, src[3:13, 5:22, ::-1])
    f = CF.window_f32(src, 0, 3, 5, 10, 17, 16, 24, pad_top=2, pad_left=3, bgr=True)
    assert f.dtype == np.float32 and f.shape == (3, 16, 24)
    want = torch.nn.functional.pad(torch.from_numpy(u8.transpose(2, 0, 1).copy()).float()[None] / 255.0, (3, 4, 2, 4), mode="replicate")[0]
    assert torch.equal(torch.from_numpy(f), want)          # img2tensor's / 255. + InputPadder.pad


def test_xiph_geometry_is_the_scripts_literal_numbers():
    frame = np.zeros((2160, 4096, 3), dtype=np.uint8)
    for geom in (CF.xiph_geometry, evaluate.xiph_geometry):
        assert geom(2160, 4096, "resized-2k") == (1, 0, 0, 1080, 2048)          # cv2.resize(dsize=(2048, 1080))
        mode, y0, x0, h, w = geom(2160, 4096, "cropped-4k")
        assert (mode, y0, x0) == (0, 540, 1024)
        assert frame[540:-540, 1024:-1024].shape[:2] == (h, w) == (1080, 2048)
    padder = host_io.InputPadder((1, 3, 1080, 2048), divisor=metrics.XIPH.divisor)
    assert padder._pad == [0, 0, 4, 4]
    for bad in ((2162, 4096), (2160, 4098), (0, 4096)):
        with pytest.raises(ValueError, match="% 4"):
            evaluate.xiph_geometry(*bad, "resized-2k")
    with pytest.raises(ValueError, match="category"):
        evaluate.xiph_geometry(2160, 4096, "resized-4k")


def _touch_clip(root, clip, last):
    d = root / clip
    d.mkdir(parents=True)
    for k in range(1, last + 1):
        (d / f"{k:03d}.png").write_bytes(b"")


def test_xiph_lister(tmp_path):
    assert evaluate.XIPH_CLIPS == ("BoxingPractice", "Crosswalk", "DrivingPOV", "FoodMarket", "FoodMarket2", "RitualDance",
                                   "SquareAndTimelapse", "Tango")
    assert evaluate.XIPH_CATEGORIES == ("resized-2k", "cropped-4k")
    for clip in evaluate.XIPH_CLIPS:
        _touch_clip(tmp_path, clip, 99)
    got = evaluate.xiph(str(tmp_path))
    assert len(got) == 8 * 49
    assert [s.name for s in got[:2]] == ["BoxingPractice/002", "BoxingPractice/004"] and got[49].name == "Crosswalk/002"
    assert got[-1].name == "Tango/098"
    d = os.path.join(str(tmp_path), "Crosswalk")
    assert got[50].frames == (os.path.join(d, "003.png"), os.path.join(d, "004.png"), os.path.join(d, "005.png"))      # (first, gt, last)
    sub = evaluate.xiph(str(tmp_path), clips=("Tango", "Crosswalk"), frames=range(2, 7, 2))
    assert [s.name for s in sub] == ["Tango/002", "Tango/004", "Tango/006", "Crosswalk/002", "Crosswalk/004", "Crosswalk/006"]
    os.remove(os.path.join(d, "051.png"))
    with pytest.raises(FileNotFoundError, match="051.png"):
        evaluate.xiph(str(tmp_path))


def test_xiph_protocol():
    p = metrics.XIPH
    assert (p.name, p.divisor, p.global_motion, p.ensemble_global_motion, p.round_pred, p.mse_f32) == ("xiph", 32, True, None, False, True)
    assert "xiph" not in metrics.PROTOCOLS and "xiph" not in evaluate.LISTERS


def test_frame_u8_window_abi_rejects_bad_arguments_on_the_host():
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    ok = dict(src=P, H=64, W=96, bgr=0, mode=0, y0=0, x0=0, h=32, w=48, dst=P, Hp=32, Wp=48, pt=0, pl=0, u8=P)

    def call(**kw):
        a = {**ok, **kw}
        return lib.atmvfi_frame_u8_window(a["src"], a["H"], a["W"], a["bgr"], a["mode"], a["y0"], a["x0"], a["h"], a["w"], a["dst"], a["Hp"],
                                          a["Wp"], a["pt"], a["pl"], a["u8"], None)

    def err():
        return lib.atmvfi_last_error()
    assert call(src=None) == -1 and b"null source" in err()
    assert call(dst=None, u8=None) == -1 and b"both outputs are null" in err()
    assert call(mode=2) == -1 and b"unknown mode 2" in err()
    assert call(mode=-1) == -1 and b"unknown mode" in err()
    assert call(y0=33) == -1 and b"window outside the frame" in err()            # 33 + 32 > 64
    assert call(x0=49) == -1 and b"window outside the frame" in err()
    assert call(mode=1, h=33, Hp=33) == -1 and b"window outside the frame" in err()      # mode 1 reads 2h x 2w: 66 > 64
    assert call(mode=1, w=49, Wp=49) == -1 and b"window outside the frame" in err()
    assert call(y0=-1) == -1 and b"negative" in err()
    assert call(pt=1) == -1 and b"Hp 32 < h 32 + pad_top 1" in err()
    assert call(pl=2) == -1 and b"Wp 48 < w 48 + pad_left 2" in err()
    for k in ("H", "W", "h", "w", "Hp", "Wp", "pt", "pl"):
        assert call(**{k: -4}) == -1 and b"negative" in err(), k
    assert call(h=0) == -1 and b"negative or zero" in err()
    assert lib.atmvfi_plan_fn_id(b"atmvfi_frame_u8_window") >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 11


def test_cli_accepts_xiph_and_errors_cleanly_on_an_empty_root(tmp_path, capsys):
    cli = importlib.import_module("benchmark.evaluate")
    with pytest.raises(SystemExit) as e:
        cli.main(["--dataset", "xiph", "--path", str(tmp_path), "--ckpt", "x.pt"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "001.png is missing" in err and "invalid choice" not in err
    with pytest.raises(SystemExit):
        cli.main(["--dataset", "xiph", "--path", str(tmp_path), "--ckpt", "x.pt", "--categories", "resized-8k"])
    assert "unknown category" in capsys.readouterr().err


def test_benchmark_utils_read(tmp_path):
    from PIL import Image
    utils = importlib.import_module("benchmark.utils")
    img = np.random.default_rng(4).integers(0, 256, size=(12, 20, 3), dtype=np.uint8)
    Image.fromarray(img).save(str(tmp_path / "a.png"))
    Image.fromarray(img).save(str(tmp_path / "a.ppm"))
    Image.fromarray(img[:, :, 0]).save(str(tmp_path / "g.pgm"))
    got = utils.read(str(tmp_path / "a.png"))
    assert got.dtype == np.uint8 and np.array_equal(got, img) and np.array_equal(utils.read(str(tmp_path / "a.ppm")), img)
    assert np.array_equal(utils.read(str(tmp_path / "g.pgm")), np.repeat(img[:, :, :1], 3, axis=2))
    for name in ("x.flo", "x.float3", "x.pfm"):
        with pytest.raises(NotImplementedError, match=os.path.splitext(name)[1]):
            utils.read(str(tmp_path / name))


@pytest.mark.parametrize("name", list(CF.XIPH_CASES))
def test_xiph_metric_restatement_vs_reference_golden(name):
    """The reference's calculate_psnr / calculate_ssim called as test_xiph.py calls them (tools/gen_xiph_golden.py) against the
    restatement with Xiph's arithmetic: fp32 difference and square, fp64 sum; ssim_matlab with L = 1."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "xiph_ref.npz"))
    gt, pred = CF.xiph_case(name)
    np.testing.assert_allclose(MI.in_sums(gt, pred), gold[f"{name}/in_sums"], rtol=1e-12)
    psnr, ssim = CF.xiph_metrics(gt, pred)
    dp, ds = abs(psnr - float(gold[f"{name}/psnr"])), abs(ssim - float(gold[f"{name}/ssim"]))
    print(f"{name}: |dPSNR| = {dp:.3e} dB, |dSSIM| = {ds:.3e}")
    assert dp <= TOL_PSNR
    assert ds <= TOL_GOLD
