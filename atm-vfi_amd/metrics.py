"""Quality metrics of the evaluation scripts on the GPU: the reference's ``ssim_matlab`` (benchmark/pytorch_msssim.py:82-135) and
PSNR, both from ONE fused HIP kernel (``csrc/metrics.hip``, ``include/atmvfi.h`` atmvfi_ssim_psnr), plus the per-dataset metric
protocols of the reference's scripts (benchmark/test_vimeo90k.py, test_ucf101.py, test_snufilm.py, test_xiph.py) written down as data.

There is no CPU path: every entry point takes CUDA (= HIP) tensors and raises on anything else."""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import hip_ops


@dataclass(frozen=True)
class Protocol:
    """How one dataset script of the reference scores a prediction.
    ``divisor``: InputPadder divisor of the frames (0: none; the prediction is un-padded before the metric);
    ``global_motion`` / ``ensemble_global_motion``: the model switches the script sets (None: left alone);
    ``round_pred``: SSIM and PSNR see rint(pred * 255) / 255;
    ``mse_f32``: PSNR's difference and square in fp32 (else fp64, the ground truth as u8 / 255.0 in double)."""
    name: str
    divisor: int
    global_motion: bool
    ensemble_global_motion: Optional[bool]
    round_pred: bool
    mse_f32: bool


PROTOCOLS: Dict[str, Protocol] = {
    # test_vimeo90k.py: ssim_matlab(gt_u8 / 255. (fp32), pred); psnr on (u8 / 255. (fp64) - pred)
    "vimeo90k": Protocol("vimeo90k", divisor=0, global_motion=False, ensemble_global_motion=None, round_pred=False, mse_f32=False),
    # test_ucf101.py: ssim_matlab(gt, round(pred * 255) / 255); psnr on fp32 gt - fp32 rounded pred
    "ucf101": Protocol("ucf101", divisor=0, global_motion=False, ensemble_global_motion=None, round_pred=True, mse_f32=True),
    # test_snufilm.py: InputPadder(divisor=64), unpad, ssim_matlab(gt, pred); psnr as vimeo90k
    "snufilm": Protocol("snufilm", divisor=64, global_motion=True, ensemble_global_motion=False, round_pred=False, mse_f32=False),
}


# test_xiph.py: InputPadder(divisor=32), unpad, calculate_psnr(pred, gt) (difference, square and mean in fp32) and calculate_ssim(pred, gt)
# on frames in [0, 1].  The script detects SSIM's value range on the prediction (its img1), the kernel on the ground truth; both lie in
# [0, 1], so L = 1 either way.  Kept OUT of ``PROTOCOLS``: Xiph is not one list of samples but two categories cut from the same frames
# (evaluate.evaluate_xiph), and ``evaluate()`` takes this object where it is wanted.
XIPH = Protocol("xiph", divisor=32, global_motion=True, ensemble_global_motion=None, round_pred=False, mse_f32=True)


_ops_lock = threading.Lock()
_ops: Dict[int, hip_ops.HipOps] = {}
_scratch: Dict[tuple, torch.Tensor] = {}


def _ops_for(device: torch.device) -> hip_ops.HipOps:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _ops_lock:
        ops = _ops.get(idx)
        if ops is None:
            ops = _ops[idx] = hip_ops.HipOps(torch.device("cuda", idx))
        return ops


def _workspace(ops: hip_ops.HipOps, device: torch.device, b: int, h: int, w: int) -> torch.Tensor:
    """Scratch kept per (device, stream): a temporary would go back to torch's allocator while the kernels may still be queued."""
    need = ops.ssim_psnr_workspace_floats(b, h, w)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _ops_lock:
        ws = _scratch.get(key)
        if ws is None or ws.numel() < need:
            ws = _scratch[key] = torch.empty(max(need, 1 << 16), dtype=torch.float32, device=device)
        return ws


def _require_cuda(t, what: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the metric kernels run on the GPU only; got a {t.device} tensor (move it with .cuda())")


def _as_batch(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError(f"{what}: expected [B,3,H,W] or [3,H,W], got {tuple(t.shape)}")
    return t


def ssim_psnr_raw(pred, gt, *, val_range=None, round_pred: bool = False, mse_f32: bool = False, gt_bgr: bool = False,
                  out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """One launch of the fused kernel -> fp64 [B,3] device tensor (ssim, cs, mse) per sample.
    ``pred``: fp32 [B,3,H,W] (or [3,H,W]) view, any strides (an un-padded slice is read in place).  ``gt``: the reference's img1 --
    an fp32 view of pred's shape, or uint8 [B,H,W,3] / [H,W,3] (RGB, BGR with ``gt_bgr``).  ``out``: fp64 [B,3] to write into (with
    ``accumulate``: to add to, a running sum that needs no host sync)."""
    _require_cuda(pred, "pred")
    _require_cuda(gt, "gt")
    if pred.dtype != torch.float32:
        raise TypeError(f"pred: float32 expected, got {pred.dtype}")
    y = _as_batch(pred, "pred")
    if y.shape[1] != 3:
        raise ValueError(f"the metric kernel takes 3-channel images, got {tuple(y.shape)}")
    b, _, h, w = y.shape
    flags = 0
    if gt.dtype == torch.uint8:
        x = gt.unsqueeze(0) if gt.dim() == 3 else gt
        if tuple(x.shape) != (b, h, w, 3):
            raise ValueError(f"a uint8 ground truth must be [B,H,W,3] of pred's size {tuple(y.shape)}, got {tuple(gt.shape)}")
        flags |= hip_ops.SSIM_X_U8 | (hip_ops.SSIM_X_BGR if gt_bgr else 0)
    elif gt.dtype == torch.float32:
        x = _as_batch(gt, "gt")
        if x.shape != y.shape:
            raise ValueError(f"gt {tuple(gt.shape)} and pred {tuple(pred.shape)} differ in shape")
    else:
        raise TypeError(f"gt: float32 or uint8 expected, got {gt.dtype}")
    if h < 11 or w < 11:
        raise ValueError(f"ssim_matlab on images smaller than 11x11 ({h}x{w}) shrinks the reference's window; not supported")
    if round_pred:
        flags |= hip_ops.SSIM_ROUND_Y
    if mse_f32:
        flags |= hip_ops.SSIM_MSE_F32
    dev = y.device
    if out is None:
        out = torch.zeros(b, 3, dtype=torch.float64, device=dev) if accumulate else torch.empty(b, 3, dtype=torch.float64, device=dev)
    if accumulate:
        flags |= hip_ops.SSIM_ACCUMULATE
    if torch.is_tensor(val_range):
        val_range = val_range.item()
    ops = _ops_for(dev)
    with torch.cuda.device(dev):
        ops.ssim_psnr(x, y, out, _workspace(ops, dev, b, h, w), float(val_range) if val_range is not None else 0.0, flags)
    return out


def psnr_from_mse(mse):
    """-10 log10(mse) (the scripts' math.log10 on the fp64 mean); works on fp64 tensors and Python floats."""
    if torch.is_tensor(mse):
        return -10.0 * torch.log10(mse)
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def quality(pred, gt, *, protocol=None, val_range=None, round_pred: bool = False, gt_bgr: bool = False, out=None):
    """Per-sample (psnr, ssim, cs), fp64 [B] device tensors, of ``pred`` against ``gt`` (see ``ssim_psnr_raw`` for the forms).
    ``protocol``: a ``PROTOCOLS`` name or ``Protocol``: its rounding and PSNR arithmetic (the padding is the caller's business: pass
    the un-padded prediction).  ``out``: fp64 [B,3] buffer that receives (ssim, cs, mse)."""
    mse_f32 = False
    if protocol is not None:
        p = PROTOCOLS[protocol] if isinstance(protocol, str) else protocol
        round_pred, mse_f32 = round_pred or p.round_pred, p.mse_f32
    raw = ssim_psnr_raw(pred, gt, val_range=val_range, round_pred=round_pred, mse_f32=mse_f32, gt_bgr=gt_bgr, out=out)
    return psnr_from_mse(raw[:, 2]), raw[:, 0], raw[:, 1]


def _check_window(window_size, window):
    if window_size != 11 or window is not None:
        raise NotImplementedError("ssim_matlab: only the reference's default window (window_size=11, window=None) is implemented")


def ssim_matlab(img1, img2, window_size=11, window=None, size_average=True, full=False, val_range=None):
    """The reference's ``ssim_matlab`` (benchmark/pytorch_msssim.py:82-135) with its signature and return types: a 0-d fp32 tensor,
    [B] with ``size_average=False``, ``(ret, cs)`` with ``full``.  img1 / img2: CUDA fp32 [B,3,H,W], H and W >= 11."""
    _check_window(window_size, window)
    _require_cuda(img1, "img1")
    if img1.dtype != torch.float32:
        raise TypeError(f"img1: float32 expected, got {img1.dtype}")
    raw = ssim_psnr_raw(img2, img1, val_range=val_range)
    ret = raw[:, 0].mean() if size_average else raw[:, 0]
    cs = raw[:, 1].mean()
    ret, cs = ret.to(torch.float32), cs.to(torch.float32)
    if full:
        return ret, cs
    return ret


def calculate_ssim(img1, img2, window_size=11, window=None, size_average=True, full=False, val_range=None):
    """benchmark/psnr_ssim.py's ``calculate_ssim``: ``ssim_matlab``, the value returned as a numpy fp32 scalar unless ``full``."""
    res = ssim_matlab(img1, img2, window_size=window_size, window=window, size_average=size_average, full=full, val_range=val_range)
    if full:
        return res
    return res.detach().cpu().numpy()


def calculate_psnr(img1, img2):
    """benchmark/psnr_ssim.py's ``calculate_psnr``: -10 log10(mean((img1 - img2)^2)) in fp32, a numpy fp32 scalar.  The squared
    differences are formed in fp32 as torch does and summed in fp64 by the kernel; the mean is rounded to fp32 before the log."""
    _require_cuda(img1, "img1")
    raw = ssim_psnr_raw(img2, img1, val_range=1.0, mse_f32=True)
    mse = raw[:, 2].mean().to(torch.float32)
    return (-10 * torch.log10(mse)).detach().cpu().numpy()
