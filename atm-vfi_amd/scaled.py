"""Half-resolution motion (``motion_scale=2``): motion is estimated on 2x reduced frames, the frame is synthesised at full size.  An
addition of this project (the reference has nothing like it), opt-in, off by default.  This module is the DEFINITION and holds the host
twins of the two kernels (include/atmvfi.h: atmvfi_frame_half, atmvfi_synth_up2; csrc/warp.hip).

Definition, for fp32 [B,3,H,W] canvases im0, im1 with H, W even (``compose_torch``; F = torch.nn.functional, flow_warp the
reference's: zeros padding, align_corners=True grid)::

    h0, h1 = F.avg_pool2d(im0, 2), F.avg_pool2d(im1, 2)
    o      = forward(h0, h1)
    up     = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
    f0, f1 = 2 * up(o.opt_flow_0), 2 * up(o.opt_flow_1)
    m      = up(o.occ_mask1)
    r      = up(o.im_t_list[0] - (o.occ_mask1 * o.I_t_0 + (1 - o.occ_mask1) * o.I_t_1))
    I_t    = clamp(m * flow_warp(im0, f0) + (1 - m) * flow_warp(im1, f1) + r, 0, 1)

The reduction is a box average and the up-sampling the half-pixel-centre bilinear: the two maps are exact inverses (half pixel j sits at
full position 2 j + 0.5), so the flow scale is exactly 2.  Every up-sampling weight is 0.25 or 0.75 (``up2_taps``).

The twins fix the arithmetic, one fp32 rounding per operation:
  frame_half   out = ((a + b) + (c + d)) * 0.25, a b the top-row pair and c d the bottom-row pair of the 2 x 2 block;
  residual     s - (m1 * a + (1 - m1) * c) at the half-size pixel (warp_blend's expression);
  up-sampling  wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
  warp         the taps of warp.hip's make_taps (the reference's coordinate round trip), sample_plane's order of the four products;
               a non-finite coordinate samples 0.0 exactly;
  synthesis    clamp((m * a + (1 - m) * c) + r, 0, 1);  uint8: rint(x * 255) half to even, clamped (frame_f32_to_u8's pixel).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
HALF_KEYS = ("im_t_list", "I_t_0", "I_t_1", "opt_flow_0", "opt_flow_1", "occ_mask1")
WANT_KEYS = ("opt_flow_0", "opt_flow_1", "occ_mask1")


def check_scale(scale, who: str = "motion_scale") -> int:
    if scale not in (1, 2) or isinstance(scale, bool):
        raise ValueError(f"{who} must be 1 or 2, got {scale!r}")
    return int(scale)


# ------------------------------------------------------------------------------------------------------------------- the definition (torch)
def flow_warp_torch(img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """The reference's flow_warp: bilinear grid_sample of ``img`` at pixel + flow, zeros padding, align_corners=True."""
    _, _, h, w = img.shape
    xs = torch.arange(w, dtype=img.dtype, device=img.device).view(1, 1, w) + flow[:, 0]
    ys = torch.arange(h, dtype=img.dtype, device=img.device).view(1, h, 1) + flow[:, 1]
    grid = torch.stack((2.0 * xs / (w - 1) - 1.0, 2.0 * ys / (h - 1) - 1.0), dim=-1)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def synth_torch(im0: torch.Tensor, im1: torch.Tensor, o: dict) -> dict:
    """The last five lines of the definition -> {"I_t", "opt_flow_0", "opt_flow_1", "occ_mask1"} at full size."""
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
    f0, f1 = 2 * up(o["opt_flow_0"]), 2 * up(o["opt_flow_1"])
    m1 = o["occ_mask1"]
    m = up(m1)
    r = up(o["im_t_list"][0] - (m1 * o["I_t_0"] + (1 - m1) * o["I_t_1"]))
    it = (m * flow_warp_torch(im0, f0) + (1 - m) * flow_warp_torch(im1, f1) + r).clamp(0, 1)
    return {"I_t": it, "opt_flow_0": f0, "opt_flow_1": f1, "occ_mask1": m}


def compose_torch(forward, im0: torch.Tensor, im1: torch.Tensor) -> dict:
    """The definition, on any ``forward(im0, im1) -> dict`` -> ``synth_torch``'s dict plus "half", forward's dict."""
    o = forward(F.avg_pool2d(im0, 2), F.avg_pool2d(im1, 2))
    return dict(synth_torch(im0, im1, o), half=o)


# ------------------------------------------------------------------------------------------------------------------------ the numpy twins
def _f32(t) -> np.ndarray:
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=F32)


def frame_half_numpy(src) -> np.ndarray:
    """atmvfi_frame_half on [...,H,W] fp32 -> [...,H/2,W/2], bit for bit."""
    s = _f32(src)
    if s.ndim < 2 or s.shape[-2] % 2 or s.shape[-1] % 2 or s.shape[-2] < 2 or s.shape[-1] < 2:
        raise ValueError(f"frame_half: H and W must be even and at least 2, got {s.shape}")
    return (((s[..., 0::2, 0::2] + s[..., 0::2, 1::2]) + (s[..., 1::2, 0::2] + s[..., 1::2, 1::2])) * F32(0.25)).astype(F32)


def up2_taps(n: int):
    """Output index 0 .. 2n-1 of the x2 up-sampling -> (i0, i1, w0, w1): even x reads max(x/2 - 1, 0) and x/2 with weights 0.25 and
    0.75, odd x reads (x - 1)/2 and min((x + 1)/2, n - 1) with weights 0.75 and 0.25."""
    x = np.arange(2 * n)
    odd = (x & 1) == 1
    i0 = np.where(odd, (x - 1) // 2, np.maximum(x // 2 - 1, 0))
    i1 = np.where(odd, np.minimum((x + 1) // 2, n - 1), x // 2)
    w0 = np.where(odd, F32(0.75), F32(0.25)).astype(F32)
    return i0, i1, w0, (F32(1.0) - w0).astype(F32)


def up2_numpy(t) -> np.ndarray:
    """[...,h,w] fp32 -> [...,2h,2w]: the kernel's up-sampling, bit for bit.  The taps and weights are those of F.interpolate(scale 2,
    bilinear, align_corners=False): equal to it exactly wherever the products and sums are exact (integer-valued maps), and within its
    roundings otherwise -- ATen's CPU kernel fuses some multiply-adds and does so differently from one tensor size to another (measured
    on torch 2.10: a 400 x 300 map equals "first product of each pair fused" bit for bit, a 16 x 24 map differs from that form and from
    this one in 40-46 % of the elements by one ulp), so no single fp32 expression reproduces it everywhere."""
    t = _f32(t)
    r0, r1, wy0, wy1 = up2_taps(t.shape[-2])
    c0, c1, wx0, wx1 = up2_taps(t.shape[-1])
    wy0, wy1 = wy0[:, None], wy1[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        top = (wx0 * t[..., r0, :][..., c0] + wx1 * t[..., r0, :][..., c1]).astype(F32)
        bot = (wx0 * t[..., r1, :][..., c0] + wx1 * t[..., r1, :][..., c1]).astype(F32)
        return (wy0 * top + wy1 * bot).astype(F32)


def up2_torch(t: torch.Tensor) -> torch.Tensor:
    """``up2_numpy`` on a torch tensor of any device (the same expression)."""
    def taps(n):
        i0, i1, w0, w1 = up2_taps(n)
        as_t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=t.device)
        return as_t(i0, torch.long), as_t(i1, torch.long), as_t(w0, t.dtype), as_t(w1, t.dtype)
    r0, r1, wy0, wy1 = taps(t.shape[-2])
    c0, c1, wx0, wx1 = taps(t.shape[-1])
    top = wx0 * t[..., r0, :][..., c0] + wx1 * t[..., r0, :][..., c1]
    bot = wx0 * t[..., r1, :][..., c0] + wx1 * t[..., r1, :][..., c1]
    return wy0[:, None] * top + wy1[:, None] * bot


def _ref_coord(p: np.ndarray, size: int) -> np.ndarray:
    hi = F32(size - 1)
    return (((F32(2.0) * p) / hi - F32(1.0) + F32(1.0)) / F32(2.0)) * hi


def warp_numpy(src, flow) -> np.ndarray:
    """atmvfi_flow_warp's arithmetic (make_taps + sample_plane of warp.hip) on src [B,C,H,W], flow [B,2,H,W], fp32; the same bits as
    tests/warp_ref.py's emulation."""
    src, flow = _f32(src), _f32(flow)
    b, c, h, w = src.shape
    one = F32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        ix = _ref_coord(np.arange(w, dtype=F32)[None, None, :] + flow[:, 0], w)
        iy = _ref_coord(np.arange(h, dtype=F32)[None, :, None] + flow[:, 1], h)
        fx0, fy0 = np.floor(ix), np.floor(iy)
        cx = np.fmin(np.fmax(fx0, F32(-2.0)), F32(w) + one)
        cy = np.fmin(np.fmax(fy0, F32(-2.0)), F32(h) + one)
        far = (cx != fx0) | (cy != fy0) | np.isnan(ix) | np.isnan(iy)
        x0, y0 = cx.astype(np.int64), cy.astype(np.int64)
        ax, ay = (ix - fx0).astype(F32), (iy - fy0).astype(F32)
        wts = ((one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay)
        v = np.zeros((b, c, h, w), F32)
        bi = np.arange(b)[:, None, None]
        for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts):
            yy, xx = y0 + dy, x0 + dx
            live = ~far & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            tap = np.moveaxis(src[bi, :, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], -1, 1)
            v = np.where(live[:, None], v + tap * wt[:, None], v).astype(F32)
    return v


def residual_numpy(it_sum, it0, it1, m1) -> np.ndarray:
    """s - (m1 a + (1 - m1) c) at the half-size pixels, fp32."""
    s, a, c, m1 = _f32(it_sum), _f32(it0), _f32(it1), _f32(m1)
    return (s - (m1 * a + (F32(1.0) - m1) * c)).astype(F32)


def to_u8_numpy(x, window=None, bgr: bool = False) -> np.ndarray:
    """fp32 [B,3,H,W] -> uint8 [B,hh,ww,3]: ``frame_f32_to_u8`` of the window (pad_top, pad_left, hh, ww)."""
    x = _f32(x)
    pt, pl, hh, ww = (0, 0) + x.shape[2:] if window is None else window
    q = np.clip(np.rint((x[:, :, pt:pt + hh, pl:pl + ww] * F32(255.0)).astype(F32)), 0, 255).astype(np.uint8)
    q = np.moveaxis(q, 1, -1)
    return np.ascontiguousarray(q[..., ::-1] if bgr else q)


def synth_up2_numpy(half: dict, store0, store1=None, slots0: Optional[Sequence[int]] = None, slots1: Optional[Sequence[int]] = None) -> dict:
    """atmvfi_synth_up2's arithmetic on numpy arrays or CPU tensors, one fp32 rounding per operation: ``half`` holds forward's half-size outputs (HALF_KEYS), the stores are
    [S,3,2h,2w], pair b reads store0[slots0[b]] and store1[slots1[b]] (default b).  -> {"I_t", "opt_flow_0", "opt_flow_1", "occ_mask1"},
    fp32 numpy arrays at full size."""
    s = _f32(half["im_t_list"][0])
    b = s.shape[0]
    m1 = _f32(half["occ_mask1"])
    store0 = _f32(store0)
    store1 = store0 if store1 is None else _f32(store1)
    l = store0[list(range(b)) if slots0 is None else [int(i) for i in slots0]]
    r = store1[list(range(b)) if slots1 is None else [int(i) for i in slots1]]
    with np.errstate(invalid="ignore", over="ignore"):
        f0 = (up2_numpy(half["opt_flow_0"]) * F32(2.0)).astype(F32)
        f1 = (up2_numpy(half["opt_flow_1"]) * F32(2.0)).astype(F32)
    m = up2_numpy(m1)
    res = up2_numpy(residual_numpy(s, half["I_t_0"], half["I_t_1"], m1))
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((m * warp_numpy(l, f0) + (F32(1.0) - m) * warp_numpy(r, f1)) + res).astype(F32)
        it = np.fmin(np.fmax(v, F32(0.0)), F32(1.0)).astype(F32)
    return {"I_t": it, "opt_flow_0": f0, "opt_flow_1": f1, "occ_mask1": m}


def forward_scaled_host(forward, im0: torch.Tensor, im1: torch.Tensor, want=()) -> dict:
    """``Network.forward_scaled`` for a model without the HIP backend: ``forward`` on the twins' half-size frames, then the synthesis
    twin.  CPU tensors in, CPU tensors out: {"I_t", "half", and what ``want`` names}."""
    if im0.shape != im1.shape or im0.dim() != 4 or im0.shape[1] != 3 or im0.shape[2] % 2 or im0.shape[3] % 2:
        raise ValueError(f"forward_scaled: two [B,3,H,W] frames with even H and W expected, got {tuple(im0.shape)} and {tuple(im1.shape)}")
    if set(want) - set(WANT_KEYS):
        raise ValueError(f"forward_scaled: want takes {sorted(WANT_KEYS)}, got {sorted(set(want) - set(WANT_KEYS))}")
    o = forward(torch.from_numpy(frame_half_numpy(im0)), torch.from_numpy(frame_half_numpy(im1)))
    full = synth_up2_numpy(o, _f32(im0), _f32(im1))
    out = {"I_t": torch.from_numpy(full["I_t"]), "half": o}
    out.update({k: torch.from_numpy(full[k]) for k in want})
    return out
