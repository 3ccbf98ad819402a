"""GPU: the fused metric kernel (atm-vfi_amd/csrc/metrics.hip) against the reference's own outputs and the CPU restatement, its
determinism, the reference-compatible return types, and the evaluation loop end to end on synthetic dataset trees."""
import importlib
import os

import numpy as np
import pytest
import torch

import cpu_metrics as C
import metric_inputs as MI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
metrics = importlib.import_module("atm-vfi_amd.metrics")
evaluate = importlib.import_module("atm-vfi_amd.evaluate")
host_io = importlib.import_module("atm-vfi_amd.host_io")
pkg = importlib.import_module("atm-vfi_amd")

TOL_GOLD = 3e-6        # kernel (fp32 filters, fp64 sums) vs the reference's fp32 conv3d, whose own rounding reaches 2e-6 (test_metrics_cpu)
TOL_CPU = 2e-6         # kernel vs the fp64 restatement
TOL_PSNR = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "metrics_ref.npz"))


@pytest.mark.parametrize("name", list(MI.CASES))
def test_kernel_vs_reference_golden(name, gold, dev):
    kind, x, y, kw = MI.case_inputs(name)
    if kind == "ssim":
        res = metrics.ssim_matlab(x.to(dev), y.to(dev), size_average=kw.get("size_average", True), full=kw.get("full", False))
        ret, cs = res if kw.get("full") else (res, None)
        ref = gold[f"{name}/ssim"]
        if ref.ndim == 2:
            ref = ref.mean(1)        # the reference's [B,W] column means (see test_metrics_cpu)
        np.testing.assert_allclose(ret.cpu().double().numpy(), ref, rtol=0, atol=TOL_GOLD)
        if cs is not None:
            assert abs(float(cs) - float(gold[f"{name}/cs"])) <= TOL_GOLD
    elif kind.startswith("u8:"):
        psnr, ssim, _ = metrics.quality(y.to(dev), torch.from_numpy(x).to(dev), protocol=kind[3:])
        assert abs(float(psnr[0]) - float(gold[f"{name}/psnr"])) <= TOL_PSNR
        assert abs(float(ssim[0]) - float(gold[f"{name}/ssim"])) <= TOL_GOLD
    else:
        assert abs(float(metrics.calculate_psnr(x.to(dev), y.to(dev))) - float(gold[f"{name}/psnr"])) <= TOL_PSNR
        assert abs(float(metrics.calculate_ssim(x.to(dev), y.to(dev))) - float(gold[f"{name}/ssim"])) <= TOL_GOLD


def _pad_view(t, dev, top, left, extra_b=0):
    """t [B,3,H,W] placed inside a larger buffer -> a strided view (the InputPadder.unpad form) holding the same values."""
    b, c, h, w = t.shape
    buf = torch.rand(b + extra_b, c + 1, h + top + 7, w + left + 9, device=dev)
    buf[:b, :c, top:top + h, left:left + w] = t.to(dev)
    return buf[:b, :c, top:top + h, left:left + w]


@pytest.mark.parametrize("seed,h,w,b", [(0, 37, 53, 1), (1, 70, 130, 3), (2, 11, 11, 2), (3, 256, 448, 1)])
def test_kernel_vs_restatement_random_shapes(seed, h, w, b, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, 3, h, w, generator=g)
    y = (x + 0.1 * torch.randn(b, 3, h, w, generator=g)).clamp(0, 1)
    want_s, want_cs = C.ssim_per_sample(x, y)
    dx = (x.double() - y.double())
    want_mse = (dx * dx).mean((1, 2, 3)).numpy()
    # strided un-pad views of both, explicit L and autodetected L
    xv, yv = _pad_view(x, dev, 3, 5), _pad_view(y, dev, 2, 7, extra_b=1)
    assert not yv.is_contiguous()
    for vr in (None, 1.0):
        raw = metrics.ssim_psnr_raw(yv, xv, val_range=vr).cpu().numpy()
        np.testing.assert_allclose(raw[:, 0], want_s, rtol=0, atol=TOL_CPU)
        np.testing.assert_allclose(raw[:, 1], want_cs, rtol=0, atol=TOL_CPU)
        np.testing.assert_allclose(raw[:, 2], want_mse, rtol=1e-12, atol=0)
    # the autodetect rule on a 0..255 range, by the value (L = 255) and explicitly
    raw255 = metrics.ssim_psnr_raw((y * 255).to(dev), (x * 255).to(dev)).cpu().numpy()
    want255 = C.ssim_per_sample(x * 255, y * 255)[0]
    np.testing.assert_allclose(raw255[:, 0], want255, rtol=0, atol=TOL_CPU)
    np.testing.assert_array_equal(raw255[:, 0], metrics.ssim_psnr_raw((y * 255).to(dev), (x * 255).to(dev), val_range=255).cpu().numpy()[:, 0])


@pytest.mark.parametrize("protocol", ["vimeo90k", "ucf101", "snufilm"])
@pytest.mark.parametrize("bgr", [False, True])
def test_uint8_ground_truth_protocols(protocol, bgr, dev):
    g = torch.Generator().manual_seed(5)
    h, w = 45, 77
    gt = (torch.rand(h, w, 3, generator=g) * 255).round().to(torch.uint8).numpy()
    pred = (torch.from_numpy(gt).permute(2, 0, 1)[None].float() / 255 + 0.03 * torch.randn(1, 3, h, w, generator=g)).clamp(0, 1)
    want_p, want_s = C.protocol_metrics(protocol, gt, pred)
    gt_dev = torch.from_numpy(np.ascontiguousarray(gt[:, :, ::-1]) if bgr else gt).to(dev)
    psnr, ssim, _ = metrics.quality(_pad_view(pred, dev, 4, 4), gt_dev, protocol=protocol, gt_bgr=bgr)
    assert abs(float(psnr[0]) - want_p) <= TOL_PSNR
    assert abs(float(ssim[0]) - want_s) <= TOL_CPU
    # rounding alone, outside a protocol
    yr = torch.round(pred * 255) / 255
    raw = metrics.ssim_psnr_raw(pred.to(dev), torch.from_numpy(gt).to(dev), round_pred=True).cpu().numpy()
    assert abs(raw[0, 0] - C.ssim_per_sample(torch.from_numpy(gt).permute(2, 0, 1)[None].float() / 255, yr)[0][0]) <= TOL_CPU


def test_two_runs_bit_identical_and_accumulate(dev):
    _, x, y, _ = MI.case_inputs("hd_1088x1920")
    x, y = x.to(dev), y.to(dev)
    a = metrics.ssim_psnr_raw(y, x).cpu()
    b = metrics.ssim_psnr_raw(y, x).cpu()
    assert torch.equal(a, b)
    acc = torch.zeros(1, 3, dtype=torch.float64, device=dev)
    metrics.ssim_psnr_raw(y, x, out=acc, accumulate=True)
    metrics.ssim_psnr_raw(y, x, out=acc, accumulate=True)
    assert torch.equal(acc.cpu(), a + a)


def test_ssim_matlab_return_types(dev):
    _, x, y, _ = MI.case_inputs("b3_256x448")
    x, y = x.to(dev), y.to(dev)
    for size_average in (True, False):
        for full in (False, True):
            r = metrics.ssim_matlab(x, y, size_average=size_average, full=full)
            ret, cs = r if full else (r, None)
            assert isinstance(ret, torch.Tensor) and ret.dtype == torch.float32 and ret.is_cuda
            assert ret.shape == (() if size_average else (3,))
            if full:
                assert isinstance(r, tuple) and len(r) == 2 and cs.shape == () and cs.dtype == torch.float32
    p = metrics.calculate_psnr(x, y)
    s = metrics.calculate_ssim(x, y)
    assert isinstance(p, np.ndarray) and p.shape == () and p.dtype == np.float32
    assert isinstance(s, np.ndarray) and s.shape == () and s.dtype == np.float32
    with pytest.raises(ValueError):
        metrics.ssim_matlab(x[..., :10], y[..., :10])


def _write_png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _frames(h, w, seed):
    import pairs
    a, b = pairs.smooth_pair(1, h, w, seed)
    mid = (a + b) / 2
    return [np.round(t[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8) for t in (a, mid, b)]


@pytest.fixture(scope="module")
def lite(dev):
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    return net.to(dev).eval()


def _expected(net, protocol, samples, dev, gm):
    """net.forward on the same inputs (the reference scripts' tensors), and the restatement's metrics of those predictions."""
    P = metrics.PROTOCOLS[protocol]
    net.global_motion = gm
    preds, vals = [], []
    for s in samples:
        f0, gt, f2 = (evaluate.read_rgb(q) for q in s.frames)
        i0, i2 = ((torch.from_numpy(f.transpose(2, 0, 1).copy()).float() / 255.0).unsqueeze(0) for f in (f0, f2))
        padder = host_io.InputPadder(i0.shape, divisor=P.divisor) if P.divisor else None
        if padder:
            i0, i2 = padder.pad(i0, i2)
        out = net.forward(i0.to(dev).contiguous(), i2.to(dev).contiguous())["I_t"]
        if padder:
            out = padder.unpad(out)
        preds.append(out[0].clone())
        vals.append(C.protocol_metrics(protocol, gt, out.cpu()))
    return preds, vals


def test_evaluate_end_to_end_vimeo_and_snufilm(tmp_path, lite, dev):
    # a Vimeo-layout tree of 4 triplets at 256x448
    vdir = tmp_path / "vimeo"
    names = [f"0000{i}/0001" for i in range(1, 5)]
    for i, n in enumerate(names):
        for fn, arr in zip(("im1.png", "im2.png", "im3.png"), _frames(256, 448, 40 + i)):
            _write_png(str(vdir / "sequences" / n / fn), arr)
    (vdir / "tri_testlist.txt").write_text("\n".join(names) + "\n")
    # a SNU-FILM tree with one 270x480 triplet (padded to 320x512 and un-padded)
    sdir = tmp_path / "snu"
    for fn, arr in zip(("0.png", "1.png", "2.png"), _frames(270, 480, 50)):
        _write_png(str(sdir / "imgs" / "clip" / fn), arr)
    (sdir / "lists").mkdir()
    for lv in evaluate.SNU_LEVELS:
        (sdir / "lists" / f"{lv}.txt").write_text("" if lv != "test-hard" else
                                                  "data/SNU-FILM/test/clip/0.png data/SNU-FILM/test/clip/1.png data/SNU-FILM/test/clip/2.png\n")
    cases = [("vimeo90k", evaluate.vimeo90k(str(vdir)), False), ("snufilm", evaluate.snufilm(str(sdir / "lists"), str(sdir / "imgs") + "/"), True),
             ("ucf101", evaluate.vimeo90k(str(vdir))[:2], False)]
    for protocol, samples, gm in cases:
        res = evaluate.evaluate(lite, samples, protocol, keep_predictions=True)
        preds, vals = _expected(lite, protocol, samples, dev, gm)
        assert len(res.records) == len(samples)
        for got, want in zip(res.predictions, preds):
            assert got.shape == want.shape and torch.equal(got, want), protocol
        for rec, (p, s) in zip(res.records, vals):
            assert abs(rec["psnr"] - p) <= TOL_PSNR and abs(rec["ssim"] - s) <= TOL_CPU, (protocol, rec, p, s)
        lv = res.levels
        assert sum(v["n"] for v in lv.values()) == len(samples)
        if protocol == "snufilm":
            assert list(lv) == ["test-hard"]
        res2 = evaluate.evaluate(lite, samples, protocol, streams=2)
        assert [(r["psnr"], r["ssim"]) for r in res2.records] == [(r["psnr"], r["ssim"]) for r in res.records], protocol
    text = evaluate.format_levels(res)
    assert text.startswith("Avg PSNR: ")


def test_cli_on_synthetic_tree(tmp_path, dev, capsys):
    vdir = tmp_path / "vimeo"
    for fn, arr in zip(("im1.png", "im2.png", "im3.png"), _frames(128, 192, 60)):
        _write_png(str(vdir / "sequences" / "a/b" / fn), arr)
    (vdir / "tri_testlist.txt").write_text("a/b\n")
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    ck = str(tmp_path / "ck.pt")
    host_io.save_checkpoint(net, ck)
    cli = importlib.import_module("benchmark.evaluate")
    out_json = str(tmp_path / "r.json")
    res = cli.main(["--dataset", "vimeo90k", "--path", str(vdir), "--ckpt", ck, "--model", "lite", "--limit", "4", "--json", out_json])
    assert "Avg PSNR: " in capsys.readouterr().out
    import json
    assert json.load(open(out_json))["records"][0]["name"] == "a/b" and len(res.records) == 1
