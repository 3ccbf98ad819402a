"""numpy model of the frame-preparation kernel (atm-vfi_amd/csrc/frames.hip, atmvfi_frame_u8_window), the yardstick of its tests:
the window, the 2x2 area rule in integer arithmetic, the channel swap, / 255 in fp32 and the replicate padding -- plus the CPU
restatement of the Xiph script's metric arithmetic (benchmark/test_xiph.py: calculate_psnr / calculate_ssim on frames in [0, 1])."""
from __future__ import annotations

import math

import numpy as np
import torch

import cpu_metrics as C


def area2(src: np.ndarray) -> np.ndarray:
    """uint8 [2h,2w,C] -> uint8 [h,w,C]: (a + b + c + d + 2) >> 2 over each 2x2 block (cv2.INTER_AREA at scale 2; ties round up)."""
    s = src.astype(np.int32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def window_u8(src: np.ndarray, mode: int, y0: int, x0: int, h: int, w: int, bgr: bool = False) -> np.ndarray:
    """The kernel's integer pixels: uint8 RGB [h,w,3] (its ``dst_u8``)."""
    if mode == 0:
        q = src[y0:y0 + h, x0:x0 + w]
    elif mode == 1:
        q = area2(src[y0:y0 + 2 * h, x0:x0 + 2 * w])
    else:
        raise ValueError(mode)
    assert q.shape == (h, w, 3), "window outside the frame"
    return np.ascontiguousarray(q[:, :, ::-1] if bgr else q)


def window_f32(src: np.ndarray, mode: int, y0: int, x0: int, h: int, w: int, hp: int, wp: int, pad_top: int = 0, pad_left: int = 0,
               bgr: bool = False) -> np.ndarray:
    """The kernel's ``dst``: fp32 planar [3,hp,wp] = q / 255 (fp32 division), the window at (pad_top, pad_left), replicate padding."""
    q = window_u8(src, mode, y0, x0, h, w, bgr)
    ys = np.clip(np.arange(hp) - pad_top, 0, h - 1)
    xs = np.clip(np.arange(wp) - pad_left, 0, w - 1)
    q = q[ys][:, xs]
    return np.ascontiguousarray((q.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def xiph_geometry(height: int, width: int, category: str):
    """(mode, y0, x0, h, w) per category, written from the script: cv2.resize(dsize=(W/2, H/2)) and [H/4:-H/4, W/4:-W/4]."""
    assert height % 4 == 0 and width % 4 == 0
    if category == "resized-2k":
        return 1, 0, 0, height // 2, width // 2
    return 0, height // 4, width // 4, height // 2, width // 2


def xiph_metrics(gt_u8: np.ndarray, pred: torch.Tensor):
    """(psnr, ssim) of a prediction (fp32 [1,3,H,W] or [3,H,W] in [0,1]) against a uint8 RGB ground truth [H,W,3] as test_xiph.py
    scores them: the ground truth is u8 / 255 in fp32 (img2tensor); calculate_psnr forms the difference and its square in fp32 (the
    sum is taken in fp64 here, as the kernel does); calculate_ssim is ssim_matlab with L = 1 (both images lie in [0, 1])."""
    pred = pred.float().reshape(1, 3, *pred.shape[-2:]).cpu()
    x = torch.from_numpy(np.ascontiguousarray(gt_u8.transpose(2, 0, 1))).unsqueeze(0).float() / 255.0
    d = pred - x
    mse = float((d * d).double().mean())
    ssim, _ = C.ssim_per_sample(x, pred, val_range=1)
    return (float("inf") if mse == 0 else -10 * math.log10(mse)), float(ssim[0])


# Seeded (prediction, uint8 ground truth) pairs of tests/golden/xiph_ref.npz (tools/gen_xiph_golden.py): name -> (h, w, seed, sigma)
XIPH_CASES = {
    "small_108x192": (108, 192, 21, 0.02),
    "mid_270x512": (270, 512, 22, 0.05),
    "full_1080x2048_s0.002": (1080, 2048, 23, 0.002),
    "full_1080x2048_s0.02": (1080, 2048, 23, 0.02),
    "full_1080x2048_s0.2": (1080, 2048, 23, 0.2),
}


def xiph_case(name: str):
    """-> (gt uint8 [H,W,3], pred fp32 [1,3,H,W]): a smooth ground truth and the same frame plus clamped Gaussian noise."""
    import metric_inputs as MI
    h, w, seed, sigma = XIPH_CASES[name]
    return MI._u8(h, w, seed, sigma)
