"""Deterministic inputs of the metric fixtures (tests/golden/metrics_ref.npz, tools/gen_metric_golden.py), regenerated from seeds by
the tests; the fixture keeps only the reference's outputs and input checksums."""
from __future__ import annotations

import numpy as np
import torch

import pairs


def _noisy(x: torch.Tensor, sigma, seed: int) -> torch.Tensor:
    """x plus Gaussian noise of ``sigma`` (one value, or one per sample), clamped to [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    s = torch.as_tensor(sigma, dtype=torch.float32).reshape(-1, 1, 1, 1)
    return (x + s * torch.randn(x.shape, generator=g)).clamp(0, 1)


def _gt_u8(h: int, w: int, seed: int) -> np.ndarray:
    """A smooth uint8 RGB ground truth [H,W,3]."""
    x, _ = pairs.smooth_pair(1, h, w, seed)
    return np.round(x[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)


# name -> (kind, builder, ssim_matlab keyword arguments)
#   kind "ssim": fp32 (img1, img2) for ssim_matlab;  "u8:<protocol>": (gt uint8 [H,W,3], pred fp32 [1,3,H,W]);
#   "calc": (img1, img2) for calculate_psnr / calculate_ssim
def _smooth(h, w, seed, sigma, b=1):
    x, _ = pairs.smooth_pair(b, h, w, seed)
    return x, _noisy(x, sigma, seed + 100)


def _random(h, w, seed):
    return pairs.random_pair(1, h, w, seed)


def _scaled(h, w, seed, scale, shift):
    x, y = _smooth(h, w, seed, 0.05)
    return x * scale + shift, y * scale + shift


def _u8(h, w, seed, sigma):
    gt = _gt_u8(h, w, seed)
    x = torch.from_numpy(gt).permute(2, 0, 1).unsqueeze(0).float() / 255.0
    return gt, _noisy(x, sigma, seed + 200)


CASES = {
    "smooth_64x96": ("ssim", lambda: _smooth(64, 96, 1, 0.05), {"full": True}),
    "random_64x96": ("ssim", lambda: _random(64, 96, 2), {}),
    "odd_37x53": ("ssim", lambda: _smooth(37, 53, 3, 0.08), {}),
    # noise from faint to heavy: SSIM spans roughly 0.3 .. 0.999
    "b3_256x448": ("ssim", lambda: _smooth(256, 448, 4, [0.003, 0.05, 0.4], b=3), {"size_average": False, "full": True}),
    "hd_1088x1920": ("ssim", lambda: _smooth(1088, 1920, 5, 0.03), {}),
    "range255_64x96": ("ssim", lambda: _scaled(64, 96, 6, 255.0, 0.0), {}),
    "range_pm1_64x96": ("ssim", lambda: _scaled(64, 96, 7, 2.0, -1.0), {"full": True}),
    "vimeo90k_u8_96x128": ("u8:vimeo90k", lambda: _u8(96, 128, 8, 0.02), {}),
    "ucf101_u8_96x128": ("u8:ucf101", lambda: _u8(96, 128, 9, 0.02), {}),
    "snufilm_u8_96x128": ("u8:snufilm", lambda: _u8(96, 128, 10, 0.02), {}),
    "calc_64x96": ("calc", lambda: _smooth(64, 96, 11, 0.04), {}),
}


def case_inputs(name: str):
    kind, build, kw = CASES[name]
    a, b = build()
    return kind, a, b, dict(kw)


def in_sums(a, b) -> np.ndarray:
    """fp64 sums of both inputs (and of their squares): a regenerated input that differs from the fixture's is caught."""
    a = np.asarray(a, dtype=np.float64) if isinstance(a, np.ndarray) else a.double().numpy()
    b = np.asarray(b, dtype=np.float64) if isinstance(b, np.ndarray) else b.double().numpy()
    return np.array([a.sum(), (a * a).sum(), b.sum(), (b * b).sum()])


def protocol_reference(protocol: str, gt: np.ndarray, pred: torch.Tensor, ssim_matlab):
    """The metric lines of the reference's dataset scripts on (uint8 RGB gt [H,W,3], fp32 pred [1,3,H,W]) -> (psnr, ssim), with the
    given ``ssim_matlab`` (the reference's, or a restatement):
      vimeo90k (test_vimeo90k.py): ssim_matlab(tensor(gt) / 255., pred); psnr of gt / 255. (fp64) - pred (fp32 -> fp64);
      ucf101 (test_ucf101.py): gt = tensor(gt / 255.).float(); ssim_matlab(gt, round(pred * 255) / 255.); psnr of the fp32 arrays;
      snufilm (test_snufilm.py): gt = tensor(gt).float() / 255.0; ssim_matlab(gt, pred); psnr as vimeo90k."""
    chw = gt.transpose(2, 0, 1)
    mid = pred[0]
    if protocol == "vimeo90k":
        ssim = float(ssim_matlab(torch.tensor(chw).unsqueeze(0) / 255., mid.unsqueeze(0)))
        d = gt / 255. - mid.numpy().transpose(1, 2, 0)
    elif protocol == "ucf101":
        g = torch.tensor(chw / 255.).float().unsqueeze(0)
        ssim = float(ssim_matlab(g, torch.round(mid * 255).unsqueeze(0) / 255.))
        out = np.round(mid.numpy().transpose(1, 2, 0) * 255) / 255.
        d = g[0].numpy().transpose(1, 2, 0) - out
    elif protocol == "snufilm":
        ssim = float(ssim_matlab((torch.tensor(chw).float() / 255.0).unsqueeze(0), mid.unsqueeze(0)))
        d = gt / 255. - mid.numpy().transpose(1, 2, 0)
    else:
        raise KeyError(protocol)
    return -10 * np.log10(float((d * d).mean())), ssim
