"""Deep RGB frames (10 / 12 / 16 bit, ``pixfmt.DeepRGB``) on the host: the vectorised numpy twins of ``atmvfi_rgb16_decode`` /
``atmvfi_rgb16_encode`` (csrc/rgb16.hip), bit for bit what the kernels compute -- what a model without the HIP backend runs on
(``segments.HostBackend``) and what the tests hold the loops to.  Nothing of the reference, whose scripts read 8-bit images.

The definition is the project's own (include/atmvfi.h spells it out; tests/cpu_rgb16.py is its per-sample model).  A frame is
``3 H W`` little-endian uint16 samples, LSB-aligned, ``top = 2**depth - 1``, in one of three layouts: "rgb48" (interleaved R G B),
"bgr48" (interleaved B G R) or "gbrp" (planes G, B, R).  Decoding takes ``q' = min(q, top)`` -- bits above the depth are never
trusted -- and hands the network fp32 ``q' / top`` with the bits of the fp32 division, as ``frame_u8_to_f32`` defines ``q / 255``; the
8-bit probe picture, on which scene signatures and frame differences run unchanged, is ``q' >> (depth - 8)``.  Encoding is
``clip(rint(fl32(x * top)), 0, top)``, half to even: ``frame_f32_to_u8``'s pixel with ``top`` in place of 255.
``rint(fl32(fl32(q / top) * top)) == q`` for every code of the three depths, and at depth 16 ``q = 257 b`` decodes to
``fl32(b / 255)``: ``frame_u8_to_f32``'s value for ``b``."""
from __future__ import annotations

import numpy as np

from .pixfmt import DeepRGB


def _rgb_view(buf, fmt: DeepRGB, who: str) -> np.ndarray:
    """the frame's samples as an [H,W,3] view in R, G, B order"""
    if not isinstance(fmt, DeepRGB):
        raise ValueError(f"{who}: a yuv.DeepRGB expected (got {type(fmt).__name__})")
    a, H, W = fmt.check(buf, who), fmt.height, fmt.width
    if fmt.layout == "gbrp":
        return a.reshape(3, H, W)[[2, 0, 1]].transpose(1, 2, 0)
    a = a.reshape(H, W, 3)
    return a[:, :, ::-1] if fmt.layout == "bgr48" else a


def _window(who: str, fmt: DeepRGB, window):
    y0, x0, h, w = (0, 0, fmt.height, fmt.width) if window is None else (int(v) for v in window)
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > fmt.height or x0 + w > fmt.width:
        raise ValueError(f"{who}: window {h} x {w} at ({y0}, {x0}) outside the {fmt.height} x {fmt.width} frame")
    return y0, x0, h, w


def _layout_of(rgb: np.ndarray, fmt: DeepRGB) -> np.ndarray:
    """[h,w,3] R, G, B samples -> the 1-D frame in the layout's order"""
    if fmt.layout == "gbrp":
        return np.ascontiguousarray(rgb[:, :, [1, 2, 0]].transpose(2, 0, 1)).reshape(-1)
    return np.ascontiguousarray(rgb[:, :, ::-1] if fmt.layout == "bgr48" else rgb).reshape(-1)


def decode_numpy_f32(buf, fmt: DeepRGB, window=None) -> np.ndarray:
    """One frame of ``fmt`` -> fp32 [h,w,3] RGB = min(q, top) / top of ``window=(y0, x0, h, w)`` (default: the frame; any origin): the
    bits of ``atmvfi_rgb16_decode``'s canvas (without padding)."""
    y0, x0, h, w = _window("rgb16.decode_numpy_f32", fmt, window)
    q = np.minimum(_rgb_view(buf, fmt, "rgb16.decode_numpy_f32")[y0:y0 + h, x0:x0 + w], np.uint16(fmt.top))
    return np.ascontiguousarray(q.astype(np.float32) / np.float32(fmt.top))


def probe_numpy(buf, fmt: DeepRGB, window=None) -> np.ndarray:
    """One frame of ``fmt`` -> its 8-bit probe picture uint8 [h,w,3] RGB = min(q, top) >> (depth - 8): the bits of
    ``atmvfi_rgb16_decode``'s ``dst_u8``."""
    y0, x0, h, w = _window("rgb16.probe_numpy", fmt, window)
    q = np.minimum(_rgb_view(buf, fmt, "rgb16.probe_numpy")[y0:y0 + h, x0:x0 + w], np.uint16(fmt.top))
    return np.ascontiguousarray((q >> (fmt.depth - 8)).astype(np.uint8))


def encode_numpy(rgb_f32, fmt: DeepRGB) -> np.ndarray:
    """fp32 [H,W,3] RGB in units of 1 (finite; values outside [0, 1] clamp) -> one frame of ``fmt`` (1-D uint16), the sample
    ``clip(rint(fl32(x * top)), 0, top)``: the bits of ``atmvfi_rgb16_encode``."""
    if not isinstance(fmt, DeepRGB):
        raise ValueError(f"rgb16.encode_numpy: a yuv.DeepRGB expected (got {type(fmt).__name__})")
    x = np.asarray(rgb_f32)
    if x.dtype != np.float32 or x.shape != (fmt.height, fmt.width, 3):
        raise ValueError(f"rgb16.encode_numpy: a float32 [{fmt.height},{fmt.width},3] frame expected, got {x.dtype} {tuple(x.shape)}")
    p = np.clip(np.rint(x * np.float32(fmt.top)), 0, fmt.top).astype(np.uint16)
    return _layout_of(p, fmt)


def crop(buf, fmt: DeepRGB, y0: int, x0: int, h: int, w: int) -> np.ndarray:
    """The h x w window at (y0, x0), any origin, as a frame of ``fmt.cropped(h, w)`` (1-D uint16): the samples untouched."""
    y0, x0, h, w = _window("rgb16.crop", fmt, (y0, x0, h, w))
    return _layout_of(_rgb_view(buf, fmt, "rgb16.crop")[y0:y0 + h, x0:x0 + w], fmt)
