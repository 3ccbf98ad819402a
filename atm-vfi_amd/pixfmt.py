"""The frame descriptors of the YUV code: ``Format`` (a packed planar frame), ``Surface`` (a decoder's layout of one), ``Packed`` (a
capture card's packed 4:2:2 frame), ``DeepRGB`` (an RGB frame above 8 bits) and the rules they share.  A leaf module (numpy only):
hip_ops.py validates against these classes and yuv.py, which re-exports every name here, builds the twins, the readers and the
loops' front ends on them."""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np


MATRICES = ("bt601", "bt709")
SITINGS = ("centre", "left")
SUBSAMPLINGS = ("420", "422", "444")        # ids 0 / 1 / 2 (include/atmvfi.h)


class YuvDesc(ctypes.Structure):
    """``atmvfi_yuv_desc`` (include/atmvfi.h): what one frame is, without pointers.  Zero means default / off."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("H", "W", "depth", "matrix", "full_range", "siting", "subsampling", "chroma", "msb")]
                + [(n, ctypes.c_int64) for n in ("pitch", "chroma_pitch", "chroma_offset")])


@functools.lru_cache(maxsize=1024)
def _desc_block(desc) -> YuvDesc:
    """``desc_block`` of a ``Format`` (the packed planar frame: no strides) or a ``Surface`` (its own).  One block per descriptor VALUE:
    equal descriptors share it, so a launch plan records one address for them; each keeps it as a ``cached_property`` (which writes the
    frozen object's ``__dict__``, not through ``__setattr__``): the device calls pass it by address on every launch."""
    f = desc.fmt if isinstance(desc, Surface) else desc
    blk = YuvDesc(H=f.height, W=f.width, depth=f.depth, matrix=f.matrix_id, full_range=int(f.full_range), siting=f.siting_id,
                  subsampling=f.subsampling_id)
    if f is not desc:
        blk.chroma, blk.msb = desc.chroma_id, int(desc.msb)
        blk.pitch, blk.chroma_pitch, blk.chroma_offset = desc.pitch, desc.chroma_pitch, desc.chroma_offset
    return blk


@dataclass(frozen=True)
class Format:
    """A packed planar frame format: Y, U, V back to back.  ``matrix="auto"``: bt709 for ``height >= 720``, bt601 below.
    ``subsampling``: "420" (I420: chroma ``((H + 1) // 2, (W + 1) // 2)``), "422" (``(H, (W + 1) // 2)``) or "444" (``(H, W)``, where a
    siting has no meaning: only "centre" is accepted, so that equal formats compare equal)."""
    height: int
    width: int
    matrix: str = "auto"
    full_range: bool = False
    siting: str = "centre"
    depth: int = 8
    subsampling: str = "420"

    def __post_init__(self):
        if int(self.height) < 1 or int(self.width) < 1:
            raise ValueError(f"yuv.Format: height and width must be at least 1 (got {self.height} x {self.width})")
        m = self.matrix
        if m == "auto":
            m = "bt709" if self.height >= 720 else "bt601"
        if m not in MATRICES:
            raise ValueError(f"yuv.Format: unknown matrix {self.matrix!r} (auto, bt601, bt709)")
        if self.siting not in SITINGS:
            raise ValueError(f"yuv.Format: unknown siting {self.siting!r} (centre, left)")
        if self.depth not in (8, 10):
            raise ValueError(f"yuv.Format: depth must be 8 or 10 (got {self.depth!r})")
        if self.depth == 10 and self.full_range:
            raise ValueError("yuv.Format: 10-bit full range is not supported")
        if self.subsampling not in SUBSAMPLINGS:
            raise ValueError(f"yuv.Format: unknown subsampling {self.subsampling!r} (420, 422, 444)")
        if self.subsampling == "444" and self.siting != "centre":
            raise ValueError(f"yuv.Format: siting {self.siting!r} has no meaning for subsampling 444 (leave it at centre)")
        object.__setattr__(self, "height", int(self.height))
        object.__setattr__(self, "width", int(self.width))
        object.__setattr__(self, "matrix", m)
        object.__setattr__(self, "full_range", bool(self.full_range))

    @property
    def chroma_shape(self) -> Tuple[int, int]:
        sy, sx = self.steps
        return (self.height + sy - 1) // sy, (self.width + sx - 1) // sx

    @property
    def steps(self) -> Tuple[int, int]:
        """Luma rows and columns per chroma sample: what a window's or a crop's origin must be a multiple of."""
        return {"420": (2, 2), "422": (1, 2), "444": (1, 1)}[self.subsampling]

    @property
    def subsampling_id(self) -> int:
        return SUBSAMPLINGS.index(self.subsampling)

    @property
    def frame_samples(self) -> int:
        ch, cw = self.chroma_shape
        return self.height * self.width + 2 * ch * cw

    @property
    def frame_bytes(self) -> int:
        return self.frame_samples * (2 if self.depth == 10 else 1)

    @property
    def dtype(self):
        return np.uint16 if self.depth == 10 else np.uint8

    @property
    def matrix_id(self) -> int:
        return MATRICES.index(self.matrix)

    @property
    def siting_id(self) -> int:
        return SITINGS.index(self.siting)

    def check(self, buf, what: str = "yuv") -> np.ndarray:
        """``buf`` as the 1-D sample array of one frame of this format (a view), or ``ValueError``."""
        a = np.asarray(buf)
        if a.dtype != self.dtype or a.size != self.frame_samples or not a.flags.c_contiguous:
            raise ValueError(f"{what}: a contiguous {np.dtype(self.dtype).name} {_layout_name(self)} frame of {self.frame_samples} samples "
                             f"({self.height} x {self.width}) expected, got {a.dtype} {tuple(a.shape)}")
        return a.reshape(-1)

    def planes(self, buf):
        """(Y [H,W], U [ch,cw], V [ch,cw]) views of a packed frame."""
        a = self.check(buf, "yuv.Format.planes")
        ch, cw = self.chroma_shape
        n, c = self.height * self.width, ch * cw
        return a[:n].reshape(self.height, self.width), a[n:n + c].reshape(ch, cw), a[n + c:].reshape(ch, cw)

    desc_block = functools.cached_property(_desc_block)

    def as_8bit(self) -> "Format":
        return self if self.depth == 8 else replace(self, depth=8)

    def cropped(self, h: int, w: int) -> "Format":
        return replace(self, height=int(h), width=int(w))


CHROMAS = ("planar", "uv", "vu")


def _layout_name(fmt) -> str:
    return {"420": "I420", "422": "planar 4:2:2", "444": "planar 4:4:4"}[fmt.subsampling]


def _origin_error(who: str, fmt, y0: int, x0: int, noun: str = "window"):
    """The origin rule of a window or crop of ``fmt``: a multiple of the subsampling step per axis.  None, or the ``ValueError``."""
    sy, sx = fmt.steps
    if y0 % sy == 0 and x0 % sx == 0:
        return None
    if fmt.subsampling == "420":
        return ValueError(f"{who}: the {noun} origin ({y0}, {x0}) must be even for 4:2:0 frames")
    return ValueError(f"{who}: the {noun} origin ({y0}, {x0}) must have an even x0 for 4:2:2 frames")


def _not_420(who: str, fmt):
    """The refusal of a 4:2:2 / 4:4:4 frame where only 4:2:0 is read or written: the ``ValueError`` (per-frame callers test and raise)."""
    return ValueError(f"{who}: 4:2:0 frames only (got subsampling {fmt.subsampling}; yuv_sub_decode / yuv_sub_encode take 4:2:2 and 4:4:4)")


def _only_420(who: str, fmt):
    if fmt.subsampling != "420":
        raise _not_420(who, fmt)


@dataclass(frozen=True)
class Surface:
    """One frame as a decoder hands it over: one contiguous buffer of ``fmt.dtype`` samples with a layout.  ``fmt`` (a ``Format``)
    supplies size, matrix, range, siting and depth; the pixel arithmetic is the ``Format``'s, applied to the samples found here.

    ``chroma``: "planar" (the U plane, then the V plane), "uv" (one plane of interleaved pairs, U first: NV12 / P010) or "vu" (V
    first: NV21).  ``msb`` (depth 10 only): a stored sample is ``value << 6``; decoding takes ``s >> 6``, encoding writes ``v << 6``.
    ``pitch`` / ``chroma_pitch``: row strides in bytes, multiples of the sample size and at least the row's own bytes; default tight
    (``W b``; ``cw b`` planar, ``2 cw b`` interleaved).  ``chroma_offset``: the byte offset of the first chroma row, a multiple of the
    sample size and at least ``pitch * H`` (the default); planar V follows U at ``chroma_offset + chroma_pitch * ch``.  ``nbytes``:
    the whole buffer through the last chroma row's own bytes; frames are 1-D arrays of ``nbytes // itemsize`` samples.  Padding is
    never read; encodes write tight surfaces only.  ``Surface.i420(h, w)`` is byte for byte a ``Format`` frame."""
    fmt: Format
    chroma: str = "planar"
    msb: bool = False
    pitch: Optional[int] = None
    chroma_pitch: Optional[int] = None
    chroma_offset: Optional[int] = None

    def __post_init__(self):
        if not isinstance(self.fmt, Format):
            raise ValueError(f"yuv.Surface: fmt must be a yuv.Format (got {type(self.fmt).__name__})")
        if self.chroma not in CHROMAS:
            raise ValueError(f"yuv.Surface: unknown chroma layout {self.chroma!r} (planar, uv, vu)")
        if self.msb and self.fmt.depth != 10:
            raise ValueError("yuv.Surface: msb needs depth 10 (8-bit samples fill their byte)")
        if self.fmt.subsampling != "420" and self.chroma != "planar":
            raise ValueError(f"yuv.Surface: interleaved chroma ({self.chroma}) is 4:2:0 only (got subsampling {self.fmt.subsampling}; "
                             "4:2:2 and 4:4:4 surfaces are planar)")
        b, (H, W), (ch, cw) = self.itemsize, (self.fmt.height, self.fmt.width), self.fmt.chroma_shape
        crow = (cw if self.chroma == "planar" else 2 * cw) * b
        pitch = W * b if self.pitch is None else int(self.pitch)
        cpitch = crow if self.chroma_pitch is None else int(self.chroma_pitch)
        if pitch % b or pitch < W * b:
            raise ValueError(f"yuv.Surface: pitch {pitch} must be a multiple of the sample size {b} and at least a luma row's {W * b} bytes")
        if cpitch % b or cpitch < crow:
            raise ValueError(f"yuv.Surface: chroma_pitch {cpitch} must be a multiple of the sample size {b} and at least a chroma row's "
                             f"{crow} bytes")
        off = pitch * H if self.chroma_offset is None else int(self.chroma_offset)
        if off % b or off < pitch * H:
            raise ValueError(f"yuv.Surface: chroma_offset {off} must be a multiple of the sample size {b} and at least pitch * H = {pitch * H}")
        object.__setattr__(self, "msb", bool(self.msb))
        object.__setattr__(self, "pitch", pitch)
        object.__setattr__(self, "chroma_pitch", cpitch)
        object.__setattr__(self, "chroma_offset", off)
        # derived once (the device calls ask for both on every launch); not fields: equality and hash are the layout's
        rows = 2 * ch - 1 if self.chroma == "planar" else ch - 1
        object.__setattr__(self, "_nbytes", off + cpitch * rows + crow)
        object.__setattr__(self, "_tight", (pitch, cpitch, off) == (W * b, crow, W * b * H))

    @classmethod
    def nv12(cls, h: int, w: int, pitch=None, chroma_offset=None, **format_kw) -> "Surface":
        """NV12: 8-bit, interleaved UV; the chroma rows share the luma pitch."""
        return cls(Format(h, w, depth=8, **format_kw), "uv", False, pitch, pitch, chroma_offset)

    @classmethod
    def p010(cls, h: int, w: int, pitch=None, chroma_offset=None, **format_kw) -> "Surface":
        """P010: 10-bit samples in the upper bits of 16-bit words, interleaved UV; the chroma rows share the luma pitch."""
        return cls(Format(h, w, depth=10, **format_kw), "uv", True, pitch, pitch, chroma_offset)

    @classmethod
    def i420(cls, h: int, w: int, pitch=None, chroma_offset=None, **format_kw) -> "Surface":
        """Planar I420 (``depth=10``: LSB-aligned uint16); with a ``pitch`` the chroma rows have half of it."""
        return cls(Format(h, w, **format_kw), "planar", False, pitch, None if pitch is None else int(pitch) // 2, chroma_offset)

    # what the loops and helpers read of a Format
    height = property(lambda self: self.fmt.height)
    width = property(lambda self: self.fmt.width)
    matrix = property(lambda self: self.fmt.matrix)
    full_range = property(lambda self: self.fmt.full_range)
    siting = property(lambda self: self.fmt.siting)
    depth = property(lambda self: self.fmt.depth)
    dtype = property(lambda self: self.fmt.dtype)
    chroma_shape = property(lambda self: self.fmt.chroma_shape)
    matrix_id = property(lambda self: self.fmt.matrix_id)
    siting_id = property(lambda self: self.fmt.siting_id)
    subsampling = property(lambda self: self.fmt.subsampling)
    subsampling_id = property(lambda self: self.fmt.subsampling_id)
    steps = property(lambda self: self.fmt.steps)
    chroma_id = property(lambda self: CHROMAS.index(self.chroma))
    desc_block = functools.cached_property(_desc_block)

    @property
    def itemsize(self) -> int:
        return 2 if self.fmt.depth == 10 else 1

    @property
    def nbytes(self) -> int:
        return self._nbytes

    frame_bytes = nbytes

    @property
    def frame_samples(self) -> int:
        return self.nbytes // self.itemsize

    @property
    def is_tight(self) -> bool:
        return self._tight

    def tight(self) -> "Surface":
        return Surface(self.fmt, self.chroma, self.msb)

    def cropped(self, h: int, w: int) -> "Surface":
        return Surface(self.fmt.cropped(h, w), self.chroma, self.msb)

    def as_8bit(self) -> "Surface":
        """The tight 8-bit counterpart (P010 -> NV12), itself for a tight 8-bit surface."""
        return self.tight() if self.fmt.depth == 8 else Surface(self.fmt.as_8bit(), self.chroma, False)

    def check(self, buf, what: str = "yuv") -> np.ndarray:
        """``buf`` as the 1-D sample array of one frame of this surface (a view), or ``ValueError``."""
        a = np.asarray(buf)
        if a.dtype != self.dtype or a.size != self.frame_samples or not a.flags.c_contiguous:
            raise ValueError(f"{what}: a contiguous {np.dtype(self.dtype).name} {self.chroma} surface of {self.frame_samples} samples "
                             f"({self.height} x {self.width}, pitch {self.pitch}) expected, got {a.dtype} {tuple(a.shape)}")
        return a.reshape(-1)

    def planes(self, buf):
        """(Y [H,W], U [ch,cw], V [ch,cw]) strided views of the STORED samples (``msb``: still shifted); padding is not part of them."""
        a = self.check(buf, "yuv.Surface.planes")
        b, (ch, cw) = self.itemsize, self.fmt.chroma_shape
        view = lambda off, rows, cols, rs, cs: np.lib.stride_tricks.as_strided(a[off // b:], (rows, cols), (rs, cs), writeable=a.flags.writeable)
        Y = view(0, self.height, self.width, self.pitch, b)
        if self.chroma == "planar":
            return Y, view(self.chroma_offset, ch, cw, self.chroma_pitch, b), \
                view(self.chroma_offset + self.chroma_pitch * ch, ch, cw, self.chroma_pitch, b)
        first, second = (view(self.chroma_offset + k * b, ch, cw, self.chroma_pitch, 2 * b) for k in (0, 1))
        return (Y, first, second) if self.chroma == "uv" else (Y, second, first)


PACKED_LAYOUTS = ("uyvy", "yuy2", "y210", "v210")      # ids 0..3 (include/atmvfi.h, atmvfi_yuv_unpack)
_PACKED_DEPTH = {"uyvy": 8, "yuy2": 8, "y210": 10, "v210": 10}
_PACKED_8BIT = {"v210": "uyvy", "y210": "yuy2"}


@dataclass(frozen=True)
class Packed:
    """One frame as a capture card hands it over: packed 4:2:2, luma and chroma interleaved in one plane.  ``fmt`` (a ``Format`` with
    ``subsampling="422"``) supplies size, matrix, range, siting and depth; the pixel arithmetic is the ``Format``'s, applied to the
    samples found here (``planar``: the tight planar frame they unpack to -- ``yuv.unpack_numpy`` / ``pack_numpy``, ``HipOps.yuv_unpack``
    / ``yuv_pack`` move the sample values, nothing else).

    ``layout``: "uyvy" (8 bit, uint8, U0 Y0 V0 Y1 per pixel pair), "yuy2" (8 bit, uint8, Y0 U0 Y1 V0), "y210" (10 bit, uint16, Y0 U0 Y1
    V0, a stored sample is ``value << 6``) or "v210" (10 bit, a uint8 byte stream: groups of four little-endian 32-bit words for 6
    pixels, three components per word in bits 0-9, 10-19, 20-29: (Cb0, Y0, Cr0), (Y1, Cb1, Y2), (Cr1, Y3, Cb2), (Y4, Cr2, Y5)).  The
    width is even.  ``pitch``: the row stride in bytes, at least the row's own bytes (``2 W``, ``2 W``, ``4 W``, ``ceil(W / 6) * 16``)
    and a multiple of 4 (v210: 16); default ``2 W``, ``2 W``, ``4 W`` and v210's ``ceil(W / 48) * 128``.  ``nbytes = pitch * H``;
    frames are 1-D arrays of ``nbytes // itemsize`` samples.  Bytes and component slots that hold no sample (row padding, v210's
    slots beyond W and bits 30-31, y210's low six bits) are never interpreted on unpack and written as zero on pack."""
    fmt: Format
    layout: str
    pitch: Optional[int] = None

    def __post_init__(self):
        if not isinstance(self.fmt, Format):
            raise ValueError(f"yuv.Packed: fmt must be a yuv.Format (got {type(self.fmt).__name__})")
        if self.layout not in PACKED_LAYOUTS:
            raise ValueError(f"yuv.Packed: unknown layout {self.layout!r} ({', '.join(PACKED_LAYOUTS)})")
        if self.fmt.subsampling != "422":
            raise ValueError(f"yuv.Packed: {self.layout} is a 4:2:2 layout (got subsampling {self.fmt.subsampling})")
        if self.fmt.depth != _PACKED_DEPTH[self.layout]:
            raise ValueError(f"yuv.Packed: {self.layout} holds {_PACKED_DEPTH[self.layout]}-bit samples (got depth {self.fmt.depth})")
        W = self.fmt.width
        if W % 2:
            raise ValueError(f"yuv.Packed: {self.layout} carries chroma per pixel pair: the width must be even (got {W})")
        row, unit = self.row_bytes, 16 if self.layout == "v210" else 4
        pitch = self.default_pitch if self.pitch is None else int(self.pitch)
        if pitch % unit or pitch < row:
            raise ValueError(f"yuv.Packed: pitch {pitch} must be a multiple of {unit} and at least a {self.layout} row's {row} bytes")
        object.__setattr__(self, "pitch", pitch)

    height = property(lambda self: self.fmt.height)
    width = property(lambda self: self.fmt.width)
    matrix = property(lambda self: self.fmt.matrix)
    full_range = property(lambda self: self.fmt.full_range)
    siting = property(lambda self: self.fmt.siting)
    depth = property(lambda self: self.fmt.depth)
    subsampling = property(lambda self: self.fmt.subsampling)
    steps = property(lambda self: self.fmt.steps)
    layout_id = property(lambda self: PACKED_LAYOUTS.index(self.layout))

    @property
    def row_bytes(self) -> int:
        """the bytes of a row that hold samples"""
        W = self.fmt.width
        return {"uyvy": 2 * W, "yuy2": 2 * W, "y210": 4 * W, "v210": (W + 5) // 6 * 16}[self.layout]

    @property
    def default_pitch(self) -> int:
        return (self.fmt.width + 47) // 48 * 128 if self.layout == "v210" else self.row_bytes

    @property
    def dtype(self):
        return np.uint16 if self.layout == "y210" else np.uint8

    @property
    def itemsize(self) -> int:
        return 2 if self.layout == "y210" else 1

    @property
    def nbytes(self) -> int:
        return self.pitch * self.fmt.height

    frame_bytes = nbytes

    @property
    def frame_samples(self) -> int:
        return self.nbytes // self.itemsize

    @property
    def is_tight(self) -> bool:
        return self.pitch == self.default_pitch

    @property
    def planar(self) -> Format:
        """The tight planar 4:2:2 ``Format`` the samples unpack to."""
        return self.fmt

    def tight(self) -> "Packed":
        return self if self.is_tight else Packed(self.fmt, self.layout)

    def cropped(self, h: int, w: int) -> "Packed":
        return Packed(self.fmt.cropped(h, w), self.layout)

    def as_8bit(self) -> "Packed":
        """The tight 8-bit counterpart (v210 -> uyvy, y210 -> yuy2), ``tight()`` for an 8-bit layout."""
        return self.tight() if self.fmt.depth == 8 else Packed(self.fmt.as_8bit(), _PACKED_8BIT[self.layout])

    def check(self, buf, what: str = "yuv") -> np.ndarray:
        """``buf`` as the 1-D sample array of one frame of this layout (a view), or ``ValueError``."""
        a = np.asarray(buf)
        if a.dtype != self.dtype or a.size != self.frame_samples or not a.flags.c_contiguous:
            raise ValueError(f"{what}: a contiguous {np.dtype(self.dtype).name} {self.layout} frame of {self.frame_samples} samples "
                             f"({self.height} x {self.width}, pitch {self.pitch}) expected, got {a.dtype} {tuple(a.shape)}")
        return a.reshape(-1)


RGB_LAYOUTS = ("rgb48", "bgr48", "gbrp")      # ids 0..2 (include/atmvfi.h, atmvfi_rgb16_decode)
RGB_DEPTHS = (10, 12, 16)


@dataclass(frozen=True)
class DeepRGB:
    """One RGB frame above 8 bits (film scans, RGB mezzanine codecs, ffmpeg's ``rgb48le`` / ``bgr48le`` / ``gbrp10le`` / ``gbrp12le`` /
    ``gbrp16le``): ``3 H W`` little-endian uint16 samples, LSB-aligned, ``top = 2**depth - 1``, tight (there is no pitch).  ``layout``:
    "rgb48" (interleaved R G B: the bytes of a uint16 ``[H,W,3]`` array), "bgr48" (B first: what OpenCV returns for a 16-bit image) or
    "gbrp" (three planes ``[H,W]`` in the order G, B, R).  The arithmetic is rgb16.py's (``atmvfi_rgb16_decode`` / ``_encode``): the
    network sees ``min(q, top) / top`` and produced samples are ``clip(rint(x * top))``.  Frames travel as the caller's arrays: any
    contiguous uint16 array of ``3 H W`` samples (``[H,W,3]``, ``[3,H,W]``, 1-D).  The loops keep the depth always (``keep_depth=True``)."""
    height: int
    width: int
    depth: int = 16
    layout: str = "rgb48"

    def __post_init__(self):
        if int(self.height) < 1 or int(self.width) < 1:
            raise ValueError(f"yuv.DeepRGB: height and width must be at least 1 (got {self.height} x {self.width})")
        if self.depth not in RGB_DEPTHS:
            raise ValueError(f"yuv.DeepRGB: depth must be 10, 12 or 16 (got {self.depth!r})")
        if self.layout not in RGB_LAYOUTS:
            raise ValueError(f"yuv.DeepRGB: unknown layout {self.layout!r} ({', '.join(RGB_LAYOUTS)})")
        object.__setattr__(self, "height", int(self.height))
        object.__setattr__(self, "width", int(self.width))
        object.__setattr__(self, "depth", int(self.depth))

    steps = (1, 1)              # a window or crop begins anywhere
    dtype = np.uint16
    itemsize = 2
    is_tight = True
    layout_id = property(lambda self: RGB_LAYOUTS.index(self.layout))
    top = property(lambda self: (1 << self.depth) - 1)

    @property
    def frame_samples(self) -> int:
        return 3 * self.height * self.width

    @property
    def frame_bytes(self) -> int:
        return 2 * self.frame_samples

    nbytes = frame_bytes

    def tight(self) -> "DeepRGB":
        return self

    def cropped(self, h: int, w: int) -> "DeepRGB":
        return replace(self, height=int(h), width=int(w))

    def check(self, buf, what: str = "rgb16") -> np.ndarray:
        """``buf`` as the 1-D sample array of one frame of this format (a view), or ``ValueError``."""
        a = np.asarray(buf)
        if a.dtype != np.uint16 or a.size != self.frame_samples or not a.flags.c_contiguous:
            raise ValueError(f"{what}: a contiguous uint16 {self.layout} frame of {self.frame_samples} samples "
                             f"({self.height} x {self.width}, depth {self.depth}) expected, got {a.dtype} {tuple(a.shape)}")
        return a.reshape(-1)


def deep_rgb_refusals(caller: str, pixfmt, keep_depth, active=None, shutter=None):
    """What a ``DeepRGB`` stream does not go with (``ValueError``); any other ``pixfmt``, or none, passes."""
    if not isinstance(pixfmt, DeepRGB):
        return
    if not keep_depth:
        raise ValueError(f"{caller}: a DeepRGB pixfmt runs with the depth kept only: pass keep_depth=True (no 8-bit down-conversion of "
                         "RGB is defined; dithering is the caller's business)")
    if active is not None:
        raise ValueError(f"{caller}: active does not go with a DeepRGB pixfmt (composing deep frames needs a 16-bit frame_compose: a follow-up)")
    if shutter is not None:
        raise ValueError(f"{caller}: shutter does not go with a DeepRGB pixfmt (a deep blend needs a 16-bit resolve: a follow-up)")


@functools.lru_cache(maxsize=64)
def _tight_surface(fmt: Format) -> Surface:
    return Surface(fmt)


def as_surface(fmt) -> Surface:
    """A ``Surface`` as it is; a ``Format`` as its tight planar surface (the same bytes; surfaces are immutable, so one per format is
    kept: the device calls ask on every launch)."""
    return fmt if isinstance(fmt, Surface) else _tight_surface(fmt)
