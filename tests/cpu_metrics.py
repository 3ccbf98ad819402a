"""CPU restatement of the fused metric kernel (atm-vfi_amd/csrc/metrics.hip), the yardstick of its tests: ssim_matlab of the reference
(benchmark/pytorch_msssim.py:82-135) restated separably -- 11-tap filters along H and W with replicate borders, then the fixed 3x3
channel mix -- in fp64 (the fp32 weights of the reference, widened), and the squared-error mean of the three dataset protocols."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F


def gaussian() -> torch.Tensor:
    g = torch.tensor([math.exp(-(k - 5) ** 2 / 4.5) for k in range(11)], dtype=torch.float32)
    return g / g.sum()


def channel_mix(g: torch.Tensor) -> torch.Tensor:
    """M[o][c] = sum of g[k] over the taps k with clamp(o + k - 5, 0, 2) == c: the replicate-padded channel axis of conv3d."""
    m = torch.zeros(3, 3, dtype=torch.float32)
    for o in range(3):
        for k in range(11):
            m[o, min(max(o + k - 5, 0), 2)] += g[k]
    return m


def _filter_hw(v: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """[N,H,W] -> the 11x11 separable Gaussian with replicate borders (vertical pass first)."""
    h, w = v.shape[-2:]
    p = F.pad(v.unsqueeze(1), (5, 5, 5, 5), mode="replicate")[:, 0]
    t = sum(g[k] * p[:, k:k + h, :] for k in range(11))
    return sum(g[k] * t[:, :, k:k + w] for k in range(11))


def ssim_per_sample(x: torch.Tensor, y: torch.Tensor, val_range=None):
    """(ssim, cs) per sample, fp64 numpy [B], of ssim_matlab(x, y) for fp32 [B,3,H,W] x, y (the arithmetic in fp64)."""
    x, y = x.double(), y.double()
    if val_range is None:
        L = (255 if float(x.max()) > 128 else 1) - (-1 if float(x.min()) < -0.5 else 0)
    else:
        L = val_range
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    g = gaussian().double()
    m = channel_mix(gaussian()).double()
    b, c, h, w = x.shape
    q = torch.stack([x, y, x * x, y * y, x * y], 1).reshape(b * 5 * 3, h, w)
    f = _filter_hw(q, g).reshape(b, 5, 3, h, w)
    f = torch.einsum("oc,bqchw->bqohw", m, f)
    mu1, mu2 = f[:, 0], f[:, 1]
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = f[:, 2] - mu1_sq, f[:, 3] - mu2_sq, f[:, 4] - mu1_mu2
    v1 = 2.0 * s12 + C2
    v2 = s1 + s2 + C2
    ssim_map = ((2 * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2)
    cs_map = v1 / v2
    return ssim_map.double().mean((1, 2, 3)).numpy(), cs_map.double().mean((1, 2, 3)).numpy()


def protocol_metrics(protocol: str, gt_u8: np.ndarray, pred: torch.Tensor):
    """(psnr, ssim) of one prediction (fp32 [1,3,H,W] or [3,H,W]) against a uint8 RGB ground truth [H,W,3] under a protocol of
    atm-vfi_amd/metrics.py PROTOCOLS, computed as the kernel defines it (fp64 sums)."""
    pred = pred.float().reshape(1, 3, *pred.shape[-2:]).cpu()
    x = torch.from_numpy(np.ascontiguousarray(gt_u8.transpose(2, 0, 1))).unsqueeze(0).float() / 255.0
    if protocol == "ucf101":
        y = torch.round(pred * 255.0) / 255.0
        mse = float(((x - y) * (x - y)).double().mean())
    elif protocol in ("vimeo90k", "snufilm"):
        y = pred
        d = gt_u8.transpose(2, 0, 1)[None].astype(np.float64) / 255.0 - y.double().numpy()
        mse = float((d * d).mean())
    else:
        raise KeyError(protocol)
    ssim, _ = ssim_per_sample(x, y)
    return (float("inf") if mse == 0 else -10 * math.log10(mse)), float(ssim[0])
