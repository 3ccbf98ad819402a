"""Planar YUV 4:2:0 (I420) frames and Y4M files for the video loops: the format, the host twins of the HIP colour conversion
(``atmvfi_yuv_decode`` / ``atmvfi_yuv_encode``, csrc/yuv.hip / yuv_encode.hip), a YUV4MPEG2 reader and writer, and ``interpolate_y4m``.

Nothing of the reference: its scripts read PNGs and hand video to OpenCV.  Decoders, ``ffmpeg -f yuv4mpegpipe`` pipes and the Xiph
clips deliver planar 4:2:0; with ``pixfmt=Format(...)`` the loops (``interpolate_video_2x`` / ``FramePipeline`` /
``interpolate_video_nx``) take and yield packed I420 arrays -- 1.5 bytes per pixel each way instead of 3 -- and convert on the device.

The definition is the project's own, in int32 (``>>`` floors), so the device, ``decode_numpy`` / ``encode_numpy`` and the per-pixel
model of the tests agree bit for bit; include/atmvfi.h spells it out.  In short: a frame is Y [H,W], U [ch,cw], V [ch,cw] back to
back (ch = (H + 1) // 2, cw = (W + 1) // 2; uint8, or uint16 0..1023 for depth 10, decode only); decoding upsamples chroma with
(3, 1) taps (left siting: (4, 0) / (2, 2) horizontally) and applies ``COEFFS[matrix, full_range][0]`` at 14 bits; encoding takes the
uint8 RGB pixel (from fp32: ``frame_f32_to_u8``'s pixel), box-filters chroma over 2 x 2 (left siting: 1-2-1 x 2) un-rounded sums and
applies ``COEFFS[..][1]``.  Not reproduced: ffmpeg's swscale (other filters, other rounding) -- it is not available to compare with.
By default 10-bit input is decoded to 8-bit RGB and what the loops produce is 8-bit.

``keep_depth=True`` (the loops, ``interpolate_y4m``) keeps a 10-bit format's depth end to end (``atmvfi_yuv_decode`` (``keep_depth``) /
``atmvfi_yuv_encode`` (depth 10), the same two files; twins ``decode_numpy_f32`` and ``encode_numpy`` of an fp32 source): the same chroma
filters on the 10-bit samples, ``COEFFS10[matrix]`` at 14 bits (luma scaled by 876 / 1023, chroma by 896 / 1023), offsets 64 / 512,
RGB clipped to 0..1023 and handed to the network as ``q / 1023`` (the fp32 division); encoding takes
``clip(rint(fl32(x * 1023)), 0, 1023)`` and writes uint16 samples.  Produced frames are 10-bit, originals the caller's arrays.

``Surface`` (``atmvfi_yuv_decode`` / ``atmvfi_yuv_encode``): what a hardware decoder or an ``ffmpeg -f rawvideo``
pipe delivers -- NV12 / NV21 / P010 (interleaved chroma, 10-bit samples in the upper bits) and frames with a row pitch and a chroma
offset.  It is accepted wherever a ``Format`` is (``pixfmt=``, the twins, ``crop``, ``to_8bit``); the arithmetic is the ``Format``'s,
applied to the samples the surface describes.  ``repack`` moves frames between layouts, ``RawReader`` / ``RawWriter`` /
``interpolate_raw`` are the headerless counterparts of the Y4M classes.

``Format(..., subsampling="422" | "444")`` (``atmvfi_yuv_decode`` / ``atmvfi_yuv_encode``): planar 4:2:2 and 4:4:4 frames, 8
and 10 bit, with chroma planes [H, cw] and [H, W].  Decoding 4:2:2 filters along the row only (the columns and weights of 4:2:0,
``(wx0 c0 + wx1 c1 + 2) >> 2``), 4:4:4 takes the pixel's own samples; encoding takes the same horizontal taps over one row (sh = 1
centre, 2 left) or the pixel itself (sh = 0).  Coefficients, offsets, clips and depth rules are the 4:2:0 ones.  A window's or crop's
origin is a multiple of the subsampling step per axis.  ``Y4MReader(..., accept=("420", "422", "444"))`` reads C422, C444, C422p10
and C444p10 (C422* as left-sited: Y4M's 4:2:2 is co-sited), ``Y4MWriter`` writes them, ``surface_of`` knows yuv422p, yuv444p,
yuv422p10le and yuv444p10le, and every loop takes such a format or planar surface as ``pixfmt``.

``Packed(fmt, layout, pitch)`` (``atmvfi_yuv_unpack`` / ``atmvfi_yuv_pack``, csrc/yuv_packed.hip): packed 4:2:2 as capture cards deliver
it -- UYVY, YUY2, Y210 and v210.  ``unpack_numpy`` / ``pack_numpy`` move the sample values between such a frame and the planar 4:2:2
frame of ``packed.planar``, with no arithmetic; bytes and component slots that hold no sample are never interpreted and are written
as zero.  ``interpolate_video_nx``, ``interpolate_video_retimed`` and ``interpolate_raw`` take a ``Packed`` as ``pixfmt``: inside, the
stream is the planar one; ``surface_of`` knows uyvy422, yuyv422, y210le and v210.

``DeepRGB(height, width, depth, layout)`` (``atmvfi_rgb16_decode`` / ``atmvfi_rgb16_encode``, csrc/rgb16.hip; twins in rgb16.py): RGB
frames above 8 bits -- rgb48, bgr48 and gbrp at 10, 12 or 16 bit -- as ``pixfmt`` of every loop, always with the depth kept
(``keep_depth=True``; there is no 8-bit down-conversion rule).  ``decode_numpy`` (the 8-bit probe picture), ``decode_numpy_f32``,
``encode_numpy`` and ``crop`` hand such a format to rgb16.py; ``surface_of`` knows rgb48le, bgr48le, gbrp10le, gbrp12le and gbrp16le.

``Format``, ``Surface``, ``Packed``, ``DeepRGB`` and ``as_surface`` are defined in the leaf module ``pixfmt.py`` (hip_ops.py validates against them) and
re-exported here; ``interpolate_y4m`` and ``interpolate_raw`` are front ends of one stream driver."""
from __future__ import annotations

import io
import os
from fractions import Fraction
from typing import Iterator, Optional

import numpy as np

from .pixfmt import (CHROMAS, MATRICES, PACKED_LAYOUTS, RGB_DEPTHS, RGB_LAYOUTS, SITINGS, SUBSAMPLINGS, DeepRGB, Format, Packed,  # noqa: F401
                     Surface, _layout_name, _only_420, _origin_error, _tight_surface, as_surface, deep_rgb_refusals)
from . import rgb16

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SHIFT = 14


def derive_coeffs(matrix: str, full_range: bool = False, depth: int = 8):
    """([kY, kRV, kGU, kGV, kBU], 3 x 3 encode rows Y / U / V over (R, G, B)) = rint(c * 2^14) of the float64 matrices of (Kr, Kb);
    limited range scales luma by 219 / 255 and chroma by 224 / 255.  ``depth=10`` (limited range only; 10-bit RGB on the other side,
    ``COEFFS10``): luma by 876 / 1023, chroma by 896 / 1023."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    if depth == 10:
        if full_range:
            raise ValueError("derive_coeffs: 10-bit full range is not supported")
        sy, sc = 876.0 / 1023.0, 896.0 / 1023.0
    elif depth == 8:
        sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    else:
        raise ValueError(f"derive_coeffs: depth must be 8 or 10 (got {depth!r})")
    dec = [1.0 / sy, 2 * (1 - kr) / sc, -2 * (1 - kb) * kb / kg / sc, -2 * (1 - kr) * kr / kg / sc, 2 * (1 - kb) / sc]
    enc = [[kr * sy, kg * sy, kb * sy],
           [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc],
           [0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]]
    q = lambda v: int(np.rint(v * (1 << SHIFT)))
    return [q(v) for v in dec], [[q(v) for v in row] for row in enc]


# (matrix, full_range) -> (decode [kY, kRV, kGU, kGV, kBU], encode rows Y / U / V over (R, G, B)); kCoeffs of csrc/yuv_common.h
COEFFS = {
    ("bt601", False): ((19077, 26149, -6419, -13320, 33050), ((4207, 8260, 1604), (-2428, -4768, 7196), (7196, -6026, -1170))),
    ("bt601", True): ((16384, 22970, -5638, -11700, 29032), ((4899, 9617, 1868), (-2765, -5427, 8192), (8192, -6860, -1332))),
    ("bt709", False): ((19077, 29372, -3494, -8731, 34610), ((2991, 10064, 1016), (-1649, -5547, 7196), (7196, -6536, -660))),
    ("bt709", True): ((16384, 25802, -3069, -7670, 30402), ((3483, 11718, 1183), (-1877, -6315, 8192), (8192, -7441, -751))),
}

# matrix -> the same pair with the depth kept (10-bit limited-range samples <-> 10-bit RGB); kCoeffs10 of csrc/yuv_common.h
COEFFS10 = {
    "bt601": ((19133, 26226, -6438, -13359, 33148), ((4195, 8235, 1599), (-2421, -4754, 7175), (7175, -6008, -1167))),
    "bt709": ((19133, 29459, -3504, -8757, 34711), ((2983, 10034, 1013), (-1644, -5531, 7175), (7175, -6517, -658))),
}


def planes(buf, fmt):
    return fmt.planes(buf)


def out_format(pixfmt, deep: bool):
    """What the loops produce for input of ``pixfmt``: the format itself with the depth kept, its 8-bit form otherwise; a ``Surface``
    without its padding (P010 in: P010 out with ``deep``, NV12 out without)."""
    if isinstance(pixfmt, DeepRGB):         # (always with the depth kept: the loops refuse anything else)
        return pixfmt
    if isinstance(pixfmt, (Surface, Packed)):
        return pixfmt.tight() if deep else pixfmt.as_8bit()
    return pixfmt if deep else pixfmt.as_8bit()


def passes_through(pixfmt) -> bool:
    """An uncropped original of ``pixfmt`` leaves the loops as the caller's own array: every ``Format``, a ``Surface`` without padding,
    a ``Packed`` at its default pitch."""
    return not isinstance(pixfmt, (Surface, Packed)) or pixfmt.is_tight


# ------------------------------------------------------------------------------------------------ packed 4:2:2
_PAIR_SLOTS = {"uyvy": (1, 0, 3, 2), "yuy2": (0, 1, 2, 3), "y210": (0, 1, 2, 3)}        # (Y0, U, Y1, V) among a pair's four samples
# v210's twelve component slots of a group, three per word from bit 0 up: (Cb0, Y0, Cr0) (Y1, Cb1, Y2) (Cr1, Y3, Cb2) (Y4, Cr2, Y5)
_V210_Y, _V210_CB, _V210_CR = (1, 3, 5, 7, 9, 11), (0, 4, 8), (2, 6, 10)


def unpack_numpy(buf, packed: Packed) -> np.ndarray:
    """One frame of ``packed`` -> the planar 4:2:2 frame of ``packed.planar`` (1-D, uint8 or uint16): the sample values, moved (y210:
    ``s >> 6``; v210: the ten bits of a slot).  Row padding, v210's slots beyond the width and bits 30-31 and y210's low six bits are
    not interpreted.  The bits of ``atmvfi_yuv_unpack``."""
    a = packed.check(buf, "yuv.unpack_numpy")
    H, W = packed.height, packed.width
    rows = a.view(np.uint8).reshape(H, packed.pitch)[:, :packed.row_bytes]
    if packed.layout == "v210":
        g = (W + 5) // 6
        w = np.ascontiguousarray(rows).view("<u4").reshape(H, g, 4, 1).astype(np.uint32)
        slots = ((w >> np.array([0, 10, 20], np.uint32)) & 1023).reshape(H, g, 12)
        Y, U, V = (slots[:, :, list(k)].reshape(H, -1)[:, :n] for k, n in ((_V210_Y, W), (_V210_CB, W // 2), (_V210_CR, W // 2)))
    else:
        s = np.ascontiguousarray(rows).view("<u2" if packed.layout == "y210" else np.uint8).reshape(H, W // 2, 4)
        if packed.layout == "y210":
            s = s >> 6
        y0, u, y1, v = _PAIR_SLOTS[packed.layout]
        Y, U, V = s[:, :, [y0, y1]].reshape(H, W), s[:, :, u], s[:, :, v]
    return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(packed.planar.dtype)


def pack_numpy(planar_buf, packed: Packed) -> np.ndarray:
    """A planar 4:2:2 frame of ``packed.planar`` -> one frame of ``packed.tight()`` (1-D): the sample values, moved (y210: ``v << 6``;
    v210: ``v & 1023``); everything that holds no sample is zero.  ``unpack_numpy(pack_numpy(p, k), k) == p``.  The bits of
    ``atmvfi_yuv_pack``."""
    t = packed.tight()
    H, W = t.height, t.width
    Y, U, V = (p.astype(np.uint32) for p in t.planar.planes(t.planar.check(planar_buf, "yuv.pack_numpy")))
    if t.layout == "v210":
        g = (W + 5) // 6
        slots = np.zeros((H, g, 12), np.uint32)
        for plane, k in ((Y, _V210_Y), (U, _V210_CB), (V, _V210_CR)):
            full = np.zeros((H, g * len(k)), np.uint32)
            full[:, :plane.shape[1]] = plane & 1023
            slots[:, :, list(k)] = full.reshape(H, g, len(k))
        words = slots[:, :, 0::3] | slots[:, :, 1::3] << 10 | slots[:, :, 2::3] << 20
        out = np.zeros((H, t.pitch), np.uint8)
        out[:, :16 * g] = words.astype("<u4").view(np.uint8).reshape(H, 16 * g)
        return out.reshape(-1)
    s = np.empty((H, W // 2, 4), np.uint32)
    y0, u, y1, v = _PAIR_SLOTS[t.layout]
    s[:, :, y0], s[:, :, y1], s[:, :, u], s[:, :, v] = Y[:, 0::2], Y[:, 1::2], U, V
    if t.layout == "y210":
        s = (s << 6) & 0xffff
    return s.astype(t.dtype).reshape(-1)


def _samples(buf, fmt):
    """The frame's sample VALUES as int32 (Y, U, V): a ``Format``'s planes, or a ``Surface``'s with the ``msb`` shift undone."""
    Y, U, V = (p.astype(np.int32) for p in fmt.planes(buf))
    if isinstance(fmt, Surface) and fmt.msb:
        Y, U, V = Y >> 6, U >> 6, V >> 6
    return Y, U, V


def _pack(Y, U, V, s: Surface) -> np.ndarray:
    """Sample values (``msb``: shifted here) -> one frame of ``s``; padding samples are zero."""
    out = np.zeros(s.frame_samples, s.dtype)
    sh = 6 if s.msb else 0
    for dst, src in zip(s.planes(out), (Y, U, V)):
        dst[...] = np.asarray(src).astype(np.int64) << sh
    return out


def repack(buf, src, dst) -> np.ndarray:
    """One frame of ``src`` as a frame of ``dst`` (each a ``Surface`` or a ``Format``; the same size and depth): the sample values
    untouched, moved between layouts; ``msb`` shifts by 6 (into an ``msb`` surface the low bits are zero).  Padding of ``dst`` is zero."""
    a, b = as_surface(src), as_surface(dst)
    if a.subsampling != b.subsampling:
        raise ValueError(f"yuv.repack: subsampling {a.subsampling} and {b.subsampling} differ (repack moves samples, it does not resample)")
    if (a.height, a.width, a.depth) != (b.height, b.width, b.depth):
        raise ValueError(f"yuv.repack: {a.height} x {a.width} depth {a.depth} and {b.height} x {b.width} depth {b.depth} differ in size or depth")
    Y, U, V = a.planes(buf)
    sh = 6 if a.msb else 0
    return _pack(Y >> sh, U >> sh, V >> sh, b)


def _chroma_taps(ys, xs, ch: int, cw: int, siting: str, subsampling: str = "420"):
    """The chroma taps of luma rows ``ys`` and columns ``xs`` of the frame: rows ``r0, r1`` (weights 3, 1), columns ``q0, q1`` with
    weights ``wx0, wx1``; neighbours clamp at the frame's edges.  4:2:2 has no vertical filter (r0 = r1 = y: (4 a + 8) >> 4 is
    (a + 2) >> 2), 4:4:4 none at all (q0 = q1 = x with weights (4, 0): (16 c + 8) >> 4 is c)."""
    if subsampling == "420":
        r0 = ys >> 1
        r1 = np.clip(r0 + np.where(ys & 1, 1, -1), 0, ch - 1)
    else:
        r0 = r1 = ys
    if subsampling == "444":
        return r0, r1, xs, xs, np.full(len(xs), 4, np.int32), np.zeros(len(xs), np.int32)
    q0 = xs >> 1
    if siting == "left":
        q1 = np.minimum(q0 + 1, cw - 1)
        wx0 = np.where(xs & 1, 2, 4).astype(np.int32)
    else:
        q1 = np.clip(q0 + np.where(xs & 1, 1, -1), 0, cw - 1)
        wx0 = np.full(len(xs), 3, np.int32)
    return r0, r1, q0, q1, wx0, 4 - wx0


def _to_rgb(Y, U, V, taps, coeffs, yo: int, mid: int, T: int, top: int) -> np.ndarray:
    """Chroma filter, matrix and clip: the luma window ``Y`` (int32 [h,w]) and the frame's chroma planes with the window's ``taps``
    -> int32 [h,w,3] RGB in 0..top."""
    r0, r1, q0, q1, wx0, wx1 = taps
    lo, hi = min(r0.min(), r1.min()), max(r0.max(), r1.max()) + 1           # the chroma rows the window touches

    def up(c):
        a = wx0 * c[lo:hi, q0] + wx1 * c[lo:hi, q1]
        return (3 * a[r0 - lo] + a[r1 - lo] + 8) >> 4

    kY, kRV, kGU, kGV, kBU = coeffs
    y, u, v = kY * (Y - yo), up(U) - mid, up(V) - mid
    half = 1 << (T - 1)
    return np.clip(np.stack([(y + kRV * v + half) >> T, (y + kGU * u + kGV * v + half) >> T, (y + kBU * u + half) >> T], axis=-1), 0, top)


def _decode_window(buf, fmt: Format, y0: int, x0: int, h: int, w: int, keep: bool = False) -> np.ndarray:
    """The checked window of the whole frame's decode as int32 [h,w,3] RGB: 0..255, or 0..1023 with the 10-bit depth kept."""
    Y, U, V = _samples(buf, fmt)
    taps = _chroma_taps(np.arange(y0, y0 + h), np.arange(x0, x0 + w), *fmt.chroma_shape, fmt.siting, fmt.subsampling)
    if keep:
        pixel = COEFFS10[fmt.matrix][0], 64, 512, 14, 1023
    elif fmt.depth == 10:
        pixel = COEFFS[fmt.matrix, fmt.full_range][0], 64, 512, 16, 255
    else:
        pixel = COEFFS[fmt.matrix, fmt.full_range][0], (0 if fmt.full_range else 16), 128, 14, 255
    return _to_rgb(Y[y0:y0 + h, x0:x0 + w], U, V, taps, *pixel)


def decode_numpy(buf, fmt: Format, bgr: bool = False) -> np.ndarray:
    """Packed I420 frame -> uint8 [H,W,3] RGB (BGR if ``bgr``): the bits of ``atmvfi_yuv_decode``'s ``dst_u8``.  A ``DeepRGB``
    frame: its 8-bit probe picture (``rgb16.probe_numpy``)."""
    if isinstance(fmt, DeepRGB):
        q = rgb16.probe_numpy(buf, fmt)
        return np.ascontiguousarray(q[:, :, ::-1]) if bgr else q
    q = _decode_window(buf, fmt, 0, 0, fmt.height, fmt.width)
    return np.ascontiguousarray(q[:, :, ::-1] if bgr else q).astype(np.uint8)


def window_numpy(buf, fmt: Format, mode: int, y0: int, x0: int, h: int, w: int) -> np.ndarray:
    """Packed I420 frame -> uint8 [h,w,3] RGB: the bits of ``atmvfi_yuv_decode`` (``mode``)'s ``dst_u8`` -- ``mode`` 0: the h x w window at
    (y0, x0) of ``decode_numpy``'s frame; ``mode`` 1: the 2x area reduction ``(a + b + c + d + 2) >> 2`` of its 2h x 2w window there
    (each pixel clipped to 8 bits first).  The window is a window of the whole frame's decode: chroma neighbours are the frame's.
    Even origin, as ``crop``.  Only the window is decoded."""
    mode, y0, x0, h, w = int(mode), int(y0), int(x0), int(h), int(w)
    _only_420("window_numpy", fmt)
    if mode not in (0, 1):
        raise ValueError(f"window_numpy: unknown mode {mode} (0: crop, 1: area 2x)")
    if y0 % 2 or x0 % 2:
        raise ValueError(f"window_numpy: the window origin ({y0}, {x0}) must be even for 4:2:0 frames")
    s = 2 if mode == 1 else 1
    H, W = fmt.height, fmt.width
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + s * h > H or x0 + s * w > W:
        raise ValueError(f"window_numpy: window outside the frame (mode {mode} reads {s * h} x {s * w} source pixels at ({y0}, {x0}) of a "
                         f"{H} x {W} frame)")
    q = _decode_window(buf, fmt, y0, x0, s * h, s * w)
    if mode == 1:
        q = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
    return np.ascontiguousarray(q.astype(np.uint8))


def decode_numpy_f32(buf, fmt: Format, window=None) -> np.ndarray:
    """Packed 10-bit I420 frame -> fp32 [h,w,3] RGB = q / 1023, the depth kept: the bits of ``atmvfi_yuv_decode`` (``keep_depth``) (without
    padding).  ``window=(y0, x0, h, w)`` (even origin, as ``crop``): that window of the whole frame's decode -- chroma neighbours
    are the frame's, not the window's.  A ``DeepRGB`` frame: ``rgb16.decode_numpy_f32`` (q / top; any origin)."""
    if isinstance(fmt, DeepRGB):
        return rgb16.decode_numpy_f32(buf, fmt, window=window)
    if fmt.depth != 10:
        raise ValueError("decode_numpy_f32: a 10-bit format expected (8-bit frames decode with decode_numpy)")
    fmt.planes(buf)                                 # the frame is checked before the window
    H, W = fmt.height, fmt.width
    y0, x0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
    err = _origin_error("decode_numpy_f32", fmt, y0, x0)
    if err is not None:
        raise err
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError(f"decode_numpy_f32: window {h} x {w} at ({y0}, {x0}) outside the {H} x {W} frame")
    return _decode_window(buf, fmt, y0, x0, h, w, keep=True).astype(np.float32) / np.float32(1023)


def encode_numpy(rgb, fmt: Format, bgr: bool = False) -> np.ndarray:
    """uint8 [H,W,3] RGB (BGR if ``bgr``) -> packed 8-bit I420 frame (1-D uint8): the bits of ``atmvfi_yuv_encode``.  For a 10-bit
    ``fmt``: fp32 [H,W,3] RGB in units of 1 (finite; values outside [0, 1] clamp) -> packed 10-bit frame (1-D uint16), the pixel
    ``clip(rint(fl32(x * 1023)), 0, 1023)``: the bits of ``atmvfi_yuv_encode`` (depth 10); a uint8 source is refused.  A ``DeepRGB``
    format: ``rgb16.encode_numpy`` of an fp32 source."""
    if isinstance(fmt, DeepRGB):
        return rgb16.encode_numpy(rgb, fmt)
    rgb = np.asarray(rgb)
    deep = fmt.depth == 10 and rgb.dtype == np.float32
    if fmt.depth != 8 and not deep:
        raise ValueError("encode_numpy: encoding a uint8 source is 8-bit only (a 10-bit format takes an fp32 [H,W,3] source)")
    if (not deep and rgb.dtype != np.uint8) or rgb.shape != (fmt.height, fmt.width, 3):
        raise ValueError(f"encode_numpy: a {'float32' if deep else 'uint8'} [{fmt.height},{fmt.width},3] frame expected, got {rgb.dtype} "
                         f"{tuple(rgb.shape)}")
    if deep:
        p = np.clip(np.rint(rgb * np.float32(1023.0)), 0, 1023).astype(np.int32)
    else:
        p = rgb.astype(np.int32)
    if bgr:
        p = p[:, :, ::-1]
    H, W = fmt.height, fmt.width
    ch, cw = fmt.chroma_shape
    _, (eY, eU, eV) = COEFFS10[fmt.matrix] if deep else COEFFS[fmt.matrix, fmt.full_range]
    dot = lambda e, s: e[0] * s[..., 0] + e[1] * s[..., 1] + e[2] * s[..., 2]
    yo, mid, top = (64, 512, 1023) if deep else (0 if fmt.full_range else 16, 128, 255)
    Y = np.clip(((dot(eY, p) + (1 << 13)) >> 14) + yo, 0, top)
    if fmt.subsampling == "420":
        ra = 2 * np.arange(ch)
        rows, sh = p[ra] + p[np.minimum(ra + 1, H - 1)], 1
    else:                                           # 4:2:2, 4:4:4: a chroma row per luma row
        rows, sh = p, 0
    ca = 2 * np.arange(cw)
    if fmt.subsampling == "444":
        s = rows
    elif fmt.siting == "left":
        s, sh = rows[:, np.maximum(ca - 1, 0)] + 2 * rows[:, ca] + rows[:, np.minimum(ca + 1, W - 1)], sh + 2
    else:
        s, sh = rows[:, ca] + rows[:, np.minimum(ca + 1, W - 1)], sh + 1
    U = np.clip(((dot(eU, s) + (1 << (13 + sh))) >> (14 + sh)) + mid, 0, top)
    V = np.clip(((dot(eV, s) + (1 << (13 + sh))) >> (14 + sh)) + mid, 0, top)
    if isinstance(fmt, Surface):
        if not fmt.is_tight:
            raise ValueError("encode_numpy: encodes write tight surfaces only (surface.tight())")
        return _pack(Y, U, V, fmt)
    return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(np.uint16 if deep else np.uint8)


def crop(buf, fmt: Format, y0: int, x0: int, h: int, w: int) -> np.ndarray:
    """The h x w window at (y0, x0) of a packed frame as a packed frame of ``fmt.cropped(h, w)``: plane crops, the samples untouched.
    The origin must be even (a chroma sample covers two luma rows and columns)."""
    if isinstance(fmt, DeepRGB):            # (any origin)
        return rgb16.crop(buf, fmt, y0, x0, h, w)
    y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    err = _origin_error("yuv.crop", fmt, y0, x0, "crop")
    if err is not None:
        raise err
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > fmt.height or x0 + w > fmt.width:
        raise ValueError(f"yuv.crop: window {h} x {w} at ({y0}, {x0}) outside the {fmt.height} x {fmt.width} frame")
    if isinstance(fmt, Packed):             # unpack, the planar crop, pack: the tight frame of the window
        return pack_numpy(crop(unpack_numpy(buf, fmt), fmt.planar, y0, x0, h, w), fmt.cropped(h, w))
    Y, U, V = fmt.planes(buf)
    (sy, sx), (ch, cw) = fmt.steps, fmt.cropped(h, w).chroma_shape
    cy, cx = y0 // sy, x0 // sx
    if isinstance(fmt, Surface):            # the tight surface of the window, the stored samples as they are
        out = np.empty(fmt.cropped(h, w).frame_samples, fmt.dtype)
        oy, ou, ov = fmt.cropped(h, w).planes(out)
        oy[...], ou[...], ov[...] = Y[y0:y0 + h, x0:x0 + w], U[cy:cy + ch, cx:cx + cw], V[cy:cy + ch, cx:cx + cw]
        return out
    return np.concatenate([Y[y0:y0 + h, x0:x0 + w].reshape(-1), U[cy:cy + ch, cx:cx + cw].reshape(-1), V[cy:cy + ch, cx:cx + cw].reshape(-1)])


# ------------------------------------------------------------------------------------------------ YUV4MPEG2
Y4M_MAGIC = b"YUV4MPEG2"
# C tag -> (siting, depth); "420" is the format's default and means what "420jpeg" means
Y4M_TAGS = {"420": ("centre", 8), "420jpeg": ("centre", 8), "420mpeg2": ("left", 8), "420p10": ("centre", 10)}
# the 4:2:2 and 4:4:4 tags (read only when the reader is told to accept them) -> (siting, depth, subsampling).  C422 is taken as
# left-sited: the Y4M convention for 4:2:2 is co-sited chroma
Y4M_SUB_TAGS = {"422": ("left", 8, "422"), "444": ("centre", 8, "444"), "422p10": ("left", 10, "422"), "444p10": ("centre", 10, "444")}


class Y4MReader:
    """A YUV4MPEG2 stream (a path or a binary file object): ``fmt`` (a ``Format``; matrix "auto" by height, range from
    ``XCOLORRANGE``, siting and depth from the ``C`` tag), ``fps`` (a ``fractions.Fraction``), ``ctag`` / ``aspect`` as read; iterating
    yields the frames as 1-D uint8 (uint16 for 10-bit) arrays; ``len()`` when the file is seekable.  Accepted: C420, C420jpeg,
    C420mpeg2, C420p10, progressive.  Refused, naming the tag: C420paldv, 4:2:2, 4:4:4, mono and interlaced streams.  ``matrix``: the format's matrix when "auto" (by height) is not wanted.
    ``accept``: the subsamplings to read; with "422" / "444" in it C422, C422p10 (left-sited: the Y4M convention for 4:2:2 is
    co-sited chroma) and C444, C444p10 are read as well.  A tag outside ``accept`` is refused by name.
    ``interlaced`` (default False: interlaced streams are refused as above): tags It / Ib are read into ``interlace`` ("t" / "b") and
    the frames delivered woven, for ``fields.deinterlace_video``; Im (mixed) stays refused."""

    def __init__(self, path_or_file, matrix: str = "auto", accept=("420",), interlaced: bool = False):
        accept = tuple(str(a) for a in accept)
        for a in accept:
            if a not in SUBSAMPLINGS:
                raise ValueError(f"Y4MReader: unknown subsampling {a!r} in accept (420, 422, 444)")
        self._own = isinstance(path_or_file, (str, os.PathLike))
        self.f = open(path_or_file, "rb") if self._own else path_or_file
        line = self._line()
        tok = line.split(b" ")
        if not tok or tok[0] != Y4M_MAGIC:
            raise ValueError("Y4MReader: not a YUV4MPEG2 stream (no signature)")
        w = h = None
        self.fps, self.ctag, self.aspect, self.interlace, full = Fraction(0), "420", None, None, False
        for t in tok[1:]:
            t = t.decode("ascii", "replace")
            if not t:
                continue
            k, v = t[0], t[1:]
            if k == "W":
                w = int(v)
            elif k == "H":
                h = int(v)
            elif k == "F":
                n, d = v.split(":")
                self.fps = Fraction(int(n), int(d)) if int(d) else Fraction(0)
            elif k == "A":
                self.aspect = v
            elif k == "I":
                self.interlace = v
                if v not in ("p", "?") and not (interlaced and v in ("t", "b")):
                    if interlaced and v == "m":
                        raise ValueError("Y4MReader: mixed-mode interlacing is not supported (tag Im; It and Ib are read)")
                    raise ValueError(f"Y4MReader: interlaced streams are not supported (tag I{v})")
            elif k == "C":
                self.ctag = v
            elif k == "X" and v.upper() == "COLORRANGE=FULL":
                full = True
        if w is None or h is None:
            raise ValueError("Y4MReader: the header gives no W / H")
        known = {t: v + ("420",) for t, v in Y4M_TAGS.items()}
        known.update(Y4M_SUB_TAGS)
        if self.ctag not in known or known[self.ctag][2] not in accept:
            read = (["C420, C420jpeg, C420mpeg2", "C420p10"] if "420" in accept else []) + \
                [f"C{t}" for t, v in Y4M_SUB_TAGS.items() if v[2] in accept]
            if self._own:
                self.f.close()
            raise ValueError(f"Y4MReader: unsupported chroma format (tag C{self.ctag}); {', '.join(read[:-1])} and {read[-1]} are read")
        siting, depth, sub = known[self.ctag]
        self.fmt = Format(h, w, matrix, full, siting, depth, sub)   # the header cannot name the matrix: the caller may
        self._data0 = self._tell()

    def _tell(self):
        try:
            return self.f.tell() if self.f.seekable() else None
        except (AttributeError, OSError, io.UnsupportedOperation):
            return None

    def _line(self) -> bytes:
        out = bytearray()
        while True:
            c = self.f.read(1)
            if not c:
                if out:
                    raise ValueError("Y4MReader: the stream ends inside a header line")
                return b""
            if c == b"\n":
                return bytes(out)
            out += c
            if len(out) > 4096:
                raise ValueError("Y4MReader: header line too long")

    def __len__(self):
        if self._data0 is None:
            raise TypeError("Y4MReader: the stream is not seekable: no length")
        pos = self.f.tell()
        end = self.f.seek(0, os.SEEK_END)
        self.f.seek(pos)
        return (end - self._data0) // (len(b"FRAME\n") + self.fmt.frame_bytes)       # plain FRAME markers, as every writer emits

    def __iter__(self) -> Iterator[np.ndarray]:
        n = self.fmt.frame_bytes
        while True:
            line = self._line()
            if not line:
                return
            if not line.startswith(b"FRAME"):
                raise ValueError(f"Y4MReader: FRAME marker expected, got {line[:16]!r}")
            data = self.f.read(n)
            while 0 < len(data) < n:            # pipes deliver short reads
                more = self.f.read(n - len(data))
                if not more:
                    break
                data += more
            if len(data) != n:
                raise ValueError(f"Y4MReader: truncated frame ({len(data)} of {n} bytes)")
            yield np.frombuffer(data, dtype="<u2" if self.fmt.depth == 10 else np.uint8).astype(self.fmt.dtype, copy=True)

    def skip(self, count: int) -> int:
        """Pass over the next ``count`` frames without delivering them: a seek per frame when the stream is seekable, read and dropped
        otherwise.  Returns how many were there to skip (fewer than ``count`` at the end of the stream)."""
        n, done = self.fmt.frame_bytes, 0
        end = None
        if self._data0 is not None:
            pos = self.f.tell()
            end = self.f.seek(0, os.SEEK_END)
            self.f.seek(pos)
        while done < count:
            line = self._line()
            if not line:
                break
            if not line.startswith(b"FRAME"):
                raise ValueError(f"Y4MReader: FRAME marker expected, got {line[:16]!r}")
            if end is not None:
                if self.f.tell() + n > end:
                    raise ValueError(f"Y4MReader: truncated frame ({end - self.f.tell()} of {n} bytes)")
                self.f.seek(n, os.SEEK_CUR)
            else:
                left = n
                while left:
                    got = len(self.f.read(min(left, 1 << 22)))
                    if not got:
                        raise ValueError(f"Y4MReader: truncated frame ({n - left} of {n} bytes)")
                    left -= got
            done += 1
        return done

    def close(self):
        if self._own:
            self.f.close()

    release = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Y4MWriter:
    """Writes packed I420 frames of ``fmt`` as YUV4MPEG2 at ``fps`` (anything ``Fraction`` accepts: the rate is written as an exact
    ratio).  ``ctag``: the C tag to write when it should differ from the format's canonical one (420jpeg / 420mpeg2 / 420p10; 422,
    422p10 for left-sited 4:2:2 and 444, 444p10 are the only tags of their formats)."""

    def __init__(self, path_or_file, fmt: Format, fps, ctag: Optional[str] = None, aspect: Optional[str] = None):
        self._own = isinstance(path_or_file, (str, os.PathLike))
        self.f = open(path_or_file, "wb") if self._own else path_or_file
        self.fmt, self.fps = fmt, Fraction(fps)
        if fmt.subsampling == "420":
            canon = "420p10" if fmt.depth == 10 else ("420mpeg2" if fmt.siting == "left" else "420jpeg")
            described = Y4M_TAGS.get(ctag) == (fmt.siting, fmt.depth)
        else:
            canon = fmt.subsampling + ("p10" if fmt.depth == 10 else "")
            if Y4M_SUB_TAGS[canon] != (fmt.siting, fmt.depth, fmt.subsampling):
                raise ValueError(f"Y4MWriter: no Y4M tag describes {fmt} (C{canon} is {Y4M_SUB_TAGS[canon][0]}-sited)")
            described = ctag == canon
        if ctag is not None and not described:
            raise ValueError(f"Y4MWriter: tag C{ctag} does not describe {fmt}")
        self.ctag = ctag or canon
        head = f"YUV4MPEG2 W{fmt.width} H{fmt.height} F{self.fps.numerator}:{self.fps.denominator} Ip A{aspect or '0:0'} C{self.ctag}"
        head += " XCOLORRANGE=FULL" if fmt.full_range else " XCOLORRANGE=LIMITED"
        self.f.write(head.encode("ascii") + b"\n")
        self.frames = 0

    def write(self, frame):
        a = self.fmt.check(frame, "Y4MWriter.write")
        self.f.write(b"FRAME\n")
        self.f.write(a.astype("<u2", copy=False).tobytes() if self.fmt.depth == 10 else a.tobytes())
        self.frames += 1

    def close(self):
        if self._own:
            self.f.close()
        else:
            self.f.flush()

    release = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class RawReader:
    """A headerless stream of frames of ``surface`` (a ``Surface`` or a ``Format``) at ``fps`` -- what ``ffmpeg -f rawvideo -pix_fmt
    nv12|p010le|yuv420p...`` pipes -- from a path or a binary file object.  As ``Y4MReader``: iterating yields 1-D arrays of
    ``surface.dtype`` (little-endian on the wire), short reads of a pipe are completed, a frame cut off by the end of the stream is a
    ``ValueError``, ``skip(count)``, ``len()`` when seekable, a context manager."""

    def __init__(self, path_or_file, surface, fps):
        self._own = isinstance(path_or_file, (str, os.PathLike))
        self.f = open(path_or_file, "rb") if self._own else path_or_file
        self.surface = self.fmt = surface
        self.fps = Fraction(fps)
        self._n = int(surface.frame_bytes)
        try:
            self._data0 = self.f.tell() if self.f.seekable() else None
        except (AttributeError, OSError, io.UnsupportedOperation):
            self._data0 = None

    def _end(self):
        pos = self.f.tell()
        end = self.f.seek(0, os.SEEK_END)
        self.f.seek(pos)
        return end

    def __len__(self):
        if self._data0 is None:
            raise TypeError("RawReader: the stream is not seekable: no length")
        return (self._end() - self._data0) // self._n

    def __iter__(self) -> Iterator[np.ndarray]:
        n = self._n
        while True:
            data = self.f.read(n)
            if not data:
                return
            while len(data) < n:                # pipes deliver short reads
                more = self.f.read(n - len(data))
                if not more:
                    break
                data += more
            if len(data) != n:
                raise ValueError(f"RawReader: truncated frame ({len(data)} of {n} bytes)")
            # (by the sample type: a v210 frame is a 10-bit BYTE stream)
            yield np.frombuffer(data, dtype="<u2" if np.dtype(self.surface.dtype).itemsize == 2 else np.uint8).astype(self.surface.dtype, copy=True)

    def skip(self, count: int) -> int:
        """Pass over the next ``count`` frames without delivering them (a seek per frame when seekable, read and dropped otherwise).
        Returns how many were there to skip."""
        n, done = self._n, 0
        end = self._end() if self._data0 is not None else None
        while done < count:
            if end is not None:
                left = end - self.f.tell()
                if left <= 0:
                    break
                if left < n:
                    raise ValueError(f"RawReader: truncated frame ({left} of {n} bytes)")
                self.f.seek(n, os.SEEK_CUR)
            else:
                left = n
                while left:
                    got = len(self.f.read(min(left, 1 << 22)))
                    if not got:
                        break
                    left -= got
                if left == n:
                    break
                if left:
                    raise ValueError(f"RawReader: truncated frame ({n - left} of {n} bytes)")
            done += 1
        return done

    def close(self):
        if self._own:
            self.f.close()

    release = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class RawWriter:
    """Writes frames of ``surface`` (a ``Surface`` or a ``Format``) back to back, headerless, little-endian."""

    def __init__(self, path_or_file, surface):
        self._own = isinstance(path_or_file, (str, os.PathLike))
        self.f = open(path_or_file, "wb") if self._own else path_or_file
        self.surface = self.fmt = surface
        self.frames = 0

    def write(self, frame):
        a = self.surface.check(frame, "RawWriter.write")
        self.f.write(a.astype("<u2", copy=False).tobytes() if a.dtype.itemsize == 2 else a.tobytes())
        self.frames += 1

    def close(self):
        if self._own:
            self.f.close()
        else:
            self.f.flush()

    release = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def to_8bit(frame, fmt) -> np.ndarray:
    """A frame of ``fmt`` as a frame of ``fmt.as_8bit()``: itself for 8-bit input; 10-bit input goes through RGB on the host
    (``encode_numpy(decode_numpy(frame))``: the 8-bit picture the loops saw)."""
    if fmt.depth == 8:
        return frame
    if isinstance(fmt, Packed):             # (v210 -> uyvy, y210 -> yuy2)
        return pack_numpy(to_8bit(unpack_numpy(frame, fmt), fmt.planar), fmt.as_8bit())
    return encode_numpy(decode_numpy(frame, fmt), fmt.as_8bit())


def _interpolate_stream(who, open_reader, open_writer, model, kw, *, factor, scene, tta, interpolator, keep_depth, fps_out, levels, dedup,
                        shutter, interlaced=None, deint="mc", deint_only=False):
    """The one driver of ``interpolate_y4m`` and ``interpolate_raw`` (``who``, for the messages): the frames of ``rd = open_reader()``
    (``rd.fmt`` is the loops' ``pixfmt``, ``rd.fps`` the rate) through the loops into ``open_writer(rd, out_format, rate)``.  What the
    arguments alone decide is refused before anything is opened; after that both ends are closed on every path, a refusal before
    the writer exists included.  ``interlaced`` ("tff" / "bff"; "auto": the reader's ``interlace`` tag, a progressive one: None): the
    loop runs on ``fields.deinterlace_video(reader, ...)`` at twice the reader's rate -- two chained generators, the frames passing
    through host memory between them; ``deint_only``: the field-rate stream is written and no further loop runs.  None: the code
    path of before, nothing new is touched."""
    from .host_io import _hip_ops_of, interpolate_video_2x
    from .multiframe import centre_window, interpolate_video_nx, nx_levels
    from .retime import _check_rates, interpolate_video_retimed
    from .scaled import check_scale
    if check_scale(kw.pop("motion_scale", 1), f"{who}: motion_scale") == 2:       # (1: the loops as they are called without it)
        if shutter is not None:
            raise ValueError(f"{who}: shutter does not go with motion_scale=2")
        kw["motion_scale"] = 2
    if fps_out is None:
        if shutter is not None:
            raise ValueError(f"{who}: shutter needs fps_out (the synthetic shutter belongs to the rate conversion)")
        nx_levels(factor)
    elif "time_interval" in kw:
        raise ValueError(f"{who}: fps_out and time_interval do not go together")
    if interlaced is None and deint_only:
        raise ValueError(f"{who}: deint_only needs interlaced (tff, bff{', auto' if who == 'interpolate_y4m' else ''})")
    rd = open_reader()
    pixfmt, wr, n_in, report = rd.fmt, None, [0], {}
    fps_in = rd.fps
    try:
        if interlaced == "auto":
            interlaced = {"t": "tff", "b": "bff"}.get(getattr(rd, "interlace", None))
        if interlaced is not None:
            from . import fields
            fields.check_stream(who, pixfmt, keep_depth, interlaced, deint)
            fps_in = rd.fps * 2
        deep_rgb_refusals(who, pixfmt, keep_depth, active=kw.get("active"), shutter=shutter)
    except ValueError:
        rd.close()
        raise

    def counted():
        for f in rd:
            n_in[0] += 1
            yield f
    source = counted
    if interlaced is not None:
        # the deinterlacer's own cut record: the caller's ``scene`` belongs to the loop that follows (with ``deint_only``: to this one)
        d_scene = scene if deint_only or scene is None else type(scene)(scene.hist, scene.grid)
        source = lambda woven=counted, fmt=pixfmt: fields.deinterlace_video(woven(), model, order=interlaced, mode=deint, pixfmt=fmt,
                                                                            keep_depth=keep_depth, scene=d_scene)
        pixfmt = out_format(pixfmt, bool(keep_depth) and pixfmt.depth > 8)        # what the loop behind it reads
    counted = source
    try:
        if deint_only:
            rate = fps_in
        elif fps_out is None:
            rate = fps_in * factor / int(kw.get("time_interval", 1))
        else:
            _, rate, levels = _check_rates(fps_in, fps_out, levels)
        _, _, oh, ow = centre_window(pixfmt.height, pixfmt.width, kw.get("crop"))
        deep = bool(keep_depth) and pixfmt.depth > 8
        src_out = pixfmt.cropped(oh, ow)            # (a Surface's is tight)
        wr = open_writer(rd, src_out if deep else src_out.as_8bit(), rate)
        if deint_only:
            frames = counted()
        elif fps_out is not None:
            if shutter is not None:
                kw["shutter"] = shutter
            frames = (interpolator or interpolate_video_retimed)(counted(), model, fps_in, rate, levels=levels, dedup=dedup, scene=scene, tta=tta,
                                                                 pixfmt=pixfmt, keep_depth=deep, report=report, **kw)
        else:
            if deep:
                kw["keep_depth"] = True
            if interpolator is None:
                nx_only = tta or factor != 2 or any(k in kw for k in ("crop", "time_interval", "max_batch", "pool", "active", "motion_scale")) \
                    or isinstance(pixfmt, Packed)        # (the 2x loop does not take packed 4:2:2: factor=2 of the N-x loop does)
                if not nx_only and _hip_ops_of(model)[0] is not None:
                    interpolator = interpolate_video_2x
                else:
                    interpolator = lambda frames, model, **k: interpolate_video_nx(frames, model, factor=factor, tta=tta, **k)
            frames = interpolator(counted(), model, pixfmt=pixfmt, scene=scene, **kw)
        if isinstance(pixfmt, Packed) and pixfmt.depth == 10 and not deep:
            # (an original is a frame of the 10-bit layout: y210 by its dtype, v210 by its size -- a v210 row is longer than a uyvy one)
            is_original = lambda f: f.dtype == src_out.dtype and f.size == src_out.frame_samples
        else:
            is_original = lambda f: f.dtype == np.uint16 and not deep
        for f in frames:
            wr.write(to_8bit(f, src_out) if is_original(f) else f)
    finally:
        rd.close()
        if wr is not None:
            wr.close()
    info = {"fps_in": rd.fps, "fps_out": rate, "size": (ow, oh), "frames_in": n_in[0], "frames_out": wr.frames}
    if fps_out is not None and not deint_only:
        info["forwards"] = report.get("forwards", 0)
        if shutter is not None:
            info["blended"] = report.get("blended", 0)
        if dedup is not None:
            info["dropped"] = list(dedup.dropped)
    if scene is not None:
        info["cuts"] = list(scene.cuts)
    return info


def interpolate_y4m(src, dst, model, factor: int = 2, scene=None, tta: bool = False, interpolator=None, matrix: str = "auto",
                    keep_depth: bool = False, fps_out=None, levels: int = 3, dedup=None, shutter=None, interlaced=None, deint: str = "mc",
                    deint_only: bool = False, **kw):
    """Y4M file (or binary file object) ``src`` -> Y4M ``dst`` at ``fps * factor`` (``/ time_interval`` when given): an exact
    rational, 30000/1001 in gives 60000/1001 out.  Frames travel as I420 both ways (``pixfmt``); originals are written as read,
    predicted frames are encoded on the device.  The same format tags are written; 10-bit input is decoded on the device and written
    back as 8-bit (C420jpeg), its originals converted on the host.  ``factor=2`` on a GPU ``Network`` without ``tta`` / ``crop`` /
    ``time_interval`` runs ``interpolate_video_2x``, everything else ``interpolate_video_nx``; ``interpolator(frames, model, pixfmt=,
    ...)`` overrides.  ``matrix``: as for ``Y4MReader`` (a Y4M header cannot name it).  ``keep_depth`` (changes nothing for 8-bit
    input): a C420p10 stream is written back as C420p10 -- originals byte for byte as read, predictions encoded on the device from
    the fp32 prediction at 10 bits; nothing is re-quantised to 8 bit.  Returns ``{"fps_in", "fps_out", "size", "frames_in", "frames_out"}`` and, with ``scene``, ``"cuts"``.

    ``fps_out`` (an int, a ``Fraction`` or a string such as ``"60000/1001"``; default None: everything above, unchanged): a rate
    conversion instead -- ``retime.interpolate_video_retimed`` from the stream's own rate to exactly ``fps_out``, which the written
    header carries, with ``levels`` and ``dedup`` (a ``retime.Duplicates``) handed on; ``factor`` is ignored and there is no
    ``time_interval``.  The dict gains ``"forwards"`` and, with ``dedup``, ``"dropped"``.  ``shutter`` (a ``shutter.Shutter`` or an
    angle; only with ``fps_out``, else ``ValueError``; 8-bit output only): the conversion's synthetic shutter; the dict gains
    ``"blended"``.  ``active`` (an ``active.ActiveArea`` or a fixed window, among ``kw``; not with ``crop`` or ``shutter``): the
    network runs on the active picture of letterboxed video, in either loop (``factor=2`` goes to ``interpolate_video_nx`` then); a
    10-bit stream needs ``keep_depth`` for it.  ``motion_scale`` (1 or 2, among ``kw``; 2 not with ``shutter``): half-resolution
    motion, handed on to either loop (``factor=2`` goes to ``interpolate_video_nx`` then).

    ``interlaced`` (None, the default: everything above, and It / Ib streams refused as before; "tff", "bff" or "auto": the header's
    It / Ib tag, a progressive header: None): the stream is woven interlaced video.  It is deinterlaced to field rate first
    (``fields.deinterlace_video``, ``deint`` = "mc" or "bob"; 4:2:2 and 4:4:4 only, 10-bit with ``keep_depth``) and the chosen loop
    runs on that progressive stream at ``2 fps``; the written header says Ip and the resulting rate.  ``deint_only=True``: the
    field-rate stream itself is written and no further loop runs (``scene`` then belongs to the deinterlacer)."""
    if interlaced not in (None, "tff", "bff", "auto"):
        raise ValueError(f"interpolate_y4m: unknown interlaced {interlaced!r} (tff, bff, auto)")
    # (the same tag as read where the depth is the stream's; 10-bit input written as 8 bit takes the format's canonical tag)
    open_writer = lambda rd, out, rate: Y4MWriter(dst, out, rate, ctag=rd.ctag if out.depth == rd.fmt.depth else None, aspect=rd.aspect)
    return _interpolate_stream("interpolate_y4m", lambda: Y4MReader(src, matrix=matrix, accept=SUBSAMPLINGS, interlaced=interlaced is not None),
                               open_writer, model, kw, factor=factor, scene=scene, tta=tta, interpolator=interpolator, keep_depth=keep_depth,
                               fps_out=fps_out, levels=levels, dedup=dedup, shutter=shutter, interlaced=interlaced, deint=deint, deint_only=deint_only)


PIX_FMTS = {"nv12": ("uv", 8, False), "nv21": ("vu", 8, False), "p010le": ("uv", 10, True), "yuv420p": ("planar", 8, False),
            "yuv420p10le": ("planar", 10, False)}
# the planar 4:2:2 / 4:4:4 names -> (depth, subsampling)
PIX_FMTS_SUB = {"yuv422p": (8, "422"), "yuv444p": (8, "444"), "yuv422p10le": (10, "422"), "yuv444p10le": (10, "444")}
# the packed 4:2:2 names -> (layout, depth).  (v210 is a codec to ffmpeg, ``-c:v v210 -f rawvideo``, not a ``-pix_fmt``)
PIX_FMTS_PACKED = {"uyvy422": ("uyvy", 8), "yuyv422": ("yuy2", 8), "y210le": ("y210", 10), "v210": ("v210", 10)}
# the deep RGB names -> (layout, depth)
PIX_FMTS_RGB = {"rgb48le": ("rgb48", 16), "bgr48le": ("bgr48", 16), "gbrp10le": ("gbrp", 10), "gbrp12le": ("gbrp", 12), "gbrp16le": ("gbrp", 16)}


def surface_of(pix_fmt: str, h: int, w: int, pitch=None, **format_kw) -> Surface:
    """ffmpeg's ``-pix_fmt`` name (nv12, nv21, p010le, yuv420p, yuv420p10le, yuv422p, yuv444p, yuv422p10le, yuv444p10le) -> the
    ``Surface``; ``pitch`` (bytes): the luma rows' and the interleaved chroma rows', planar chroma rows half of it (4:4:4: all of it).
    uyvy422, yuyv422, y210le and v210 -> the ``Packed`` (``pitch``: its rows').  rgb48le, bgr48le, gbrp10le, gbrp12le and gbrp16le ->
    the ``DeepRGB`` (tight frames only: a ``pitch`` or a format keyword is refused)."""
    if pix_fmt in PIX_FMTS_RGB:
        if pitch is not None or format_kw:
            raise ValueError(f"yuv.surface_of: {pix_fmt} frames are tight RGB: no pitch, matrix, range or siting goes with them")
        layout, depth = PIX_FMTS_RGB[pix_fmt]
        return DeepRGB(h, w, depth=depth, layout=layout)
    if pix_fmt in PIX_FMTS_PACKED:
        layout, depth = PIX_FMTS_PACKED[pix_fmt]
        return Packed(Format(h, w, depth=depth, subsampling="422", **format_kw), layout, pitch)
    if pix_fmt in PIX_FMTS_SUB:            # planar: 4:2:2 chroma rows have half the pitch, 4:4:4 rows all of it
        depth, sub = PIX_FMTS_SUB[pix_fmt]
        cp = None if pitch is None else (int(pitch) if sub == "444" else int(pitch) // 2)
        return Surface(Format(h, w, depth=depth, subsampling=sub, **format_kw), "planar", False, pitch, cp)
    if pix_fmt not in PIX_FMTS:
        raise ValueError(f"yuv.surface_of: unknown pixel format {pix_fmt!r} ({', '.join(list(PIX_FMTS) + list(PIX_FMTS_SUB) + list(PIX_FMTS_PACKED) + list(PIX_FMTS_RGB))})")
    chroma, depth, msb = PIX_FMTS[pix_fmt]
    cp = None if pitch is None else (int(pitch) // 2 if chroma == "planar" else int(pitch))
    return Surface(Format(h, w, depth=depth, **format_kw), chroma, msb, pitch, cp)


def interpolate_raw(src, dst, model, surface, fps, factor: int = 2, scene=None, tta: bool = False, interpolator=None,
                    keep_depth: bool = False, fps_out=None, levels: int = 3, dedup=None, shutter=None, interlaced=None, deint: str = "mc",
                    deint_only: bool = False, **kw):
    """``interpolate_y4m`` for headerless streams (``RawReader`` / ``RawWriter``): frames of ``surface`` at ``fps`` in ``src`` ->
    frames of ``surface.tight().cropped(h, w)`` in ``dst`` (the 8-bit counterpart for 10-bit input without ``keep_depth``, originals
    converted on the host), at ``fps * factor`` or at ``fps_out``.  Every keyword is ``interpolate_y4m``'s (there is no ``matrix``: the
    surface's format names it, and ``interlaced`` is "tff" or "bff": there is no header to take it from); the same dict is returned."""
    if interlaced not in (None, "tff", "bff"):
        raise ValueError(f"interpolate_raw: unknown interlaced {interlaced!r} (tff, bff; a headerless stream has no tag for auto)")
    surface = surface if isinstance(surface, (Packed, DeepRGB)) else as_surface(surface)
    return _interpolate_stream("interpolate_raw", lambda: RawReader(src, surface, fps), lambda rd, out, rate: RawWriter(dst, out), model, kw,
                               factor=factor, scene=scene, tta=tta, interpolator=interpolator, keep_depth=keep_depth, fps_out=fps_out,
                               levels=levels, dedup=dedup, shutter=shutter, interlaced=interlaced, deint=deint, deint_only=deint_only)


# what a user of this module needs from the loops
from .host_io import FramePipeline, interpolate_video_2x, load_model_checkpoint  # noqa: E402,F401
from .multiframe import interpolate_video_nx  # noqa: E402,F401
from .scene import SceneCuts  # noqa: E402,F401
from .active import ActiveArea  # noqa: E402,F401
from .retime import Duplicates, interpolate_video_retimed  # noqa: E402,F401
from .shutter import Shutter, blend_numpy, shutter_slots  # noqa: E402,F401
# interlaced input (``interlaced=`` above; not in the reference): atm-vfi_amd/fields.py
from .fields import bob_numpy, deinterlace_video, field_parity, rows_numpy, weave_numpy  # noqa: E402,F401
