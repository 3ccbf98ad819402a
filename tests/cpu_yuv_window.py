"""Per-pixel model of ``atmvfi_yuv_decode`` (``mode``) (include/atmvfi.h; atm-vfi_amd/csrc/yuv_window.hip), the yardstick of
``yuv.window_numpy`` and of the kernel: the definition says "no new arithmetic", so the model is the two existing ones put together --
``cpu_yuv.decode``'s explicit loops over the WHOLE frame (chroma neighbours clamp at the frame's edges), then ``cpu_frames.window_u8``
/ ``window_f32`` (the window, the 2x2 area rule on the 8-bit pixels, / 255 in fp32, replicate padding).  Shares no code with the
package."""
from functools import lru_cache

import numpy as np

import cpu_frames as CF
import cpu_yuv as CY

# (name, depth, matrix, full_range, siting): every format the call accepts
FORMATS = [(f"{d}bit-{m}-{'full' if f else 'limited'}-{s}", d, m, f, s)
           for d, m, f, s in [(8, m, f, s) for m in ("bt601", "bt709") for f in (0, 1) for s in ("centre", "left")] +
           [(10, m, 0, s) for m in ("bt601", "bt709") for s in ("centre", "left")]]

# frame (H, W) -> {mode: (y0, x0, h, w)}: the smallest geometries at which the kernel can still go wrong
WHOLE_16 = ((16, 16), {0: (0, 0, 16, 16), 1: (0, 0, 8, 8)})                  # the whole frame: every edge clamps
INNER_40x56 = ((40, 56), {0: (4, 8, 16, 24), 1: (4, 8, 16, 24)})            # chroma neighbours lie outside the window
ODD_37x53 = ((37, 53), {0: (2, 4, 35, 49), 1: (0, 0, 18, 26)})              # the last odd row / column: the frame-edge clamp
CROP_24x72 = ((24, 72), {0: (6, 18, 12, 36), 1: (2, 18, 8, 24)})               # x0 % 4 == 2 on an aligned frame (W = 8 * odd: the centre crop)
WIDE_16x4200 = ((16, 4200), {0: (0, 0, 16, 4200), 1: (0, 0, 8, 2100)})      # several column tiles, more than one workgroup per row


@lru_cache(maxsize=None)
def _frame(H, W, depth, seed):
    f = CY.random_frame(H, W, depth, seed)
    f.setflags(write=False)
    return f


def frame(H, W, depth, seed=5):
    """A seeded uniform-random packed I420 frame (read-only, shared)."""
    return _frame(H, W, depth, seed)


@lru_cache(maxsize=None)
def decoded(H, W, depth, matrix, full_range, siting, seed=5):
    """``cpu_yuv.decode`` of ``frame(...)``: uint8 [H,W,3], computed once per format."""
    out = CY.decode(frame(H, W, depth, seed), H, W, matrix, full_range, siting, depth)
    out.setflags(write=False)
    return out


def window_u8(rgb, mode, y0, x0, h, w):
    return np.array(CF.window_u8(np.asarray(rgb), mode, y0, x0, h, w))          # (a writable copy: the decoded frame is shared)


def window_f32(rgb, mode, y0, x0, h, w, hp, wp, pad_top=0, pad_left=0):
    return CF.window_f32(np.asarray(rgb), mode, y0, x0, h, w, hp, wp, pad_top, pad_left)
