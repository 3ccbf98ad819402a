"""The active picture of letterboxed video for ``multiframe.interpolate_video_nx(..., active=)``.

The reference's scripts only ever see full-picture clips: nothing here is ported.  Cinema content in a 16:9 container is about a
quarter black bars, and the loop runs the network on them like on anything else.  With ``active=ActiveArea()`` the loop finds the bars
on the first frames of the stream, runs the network on the picture's window alone (as it does for a ``crop``), and puts every produced
window back into a full-size frame whose bars are the bytes of the nearer original (ties to the earlier one, the cut rule's
convention): frame count, frame size and the originals are those of the plain loop.  Content that enters the bars later (subtitles, a
change of aspect ratio) sends the loop back to the whole frame for the rest of the stream.  Off by default (``active=None``: the code
path and the frames of before).

Line maxima of a frame (``borders_numpy`` here, ``atmvfi_frame_borders`` / ``HipOps.frame_borders`` on the device, the same bits):
int32[H + W] --
  luma         Y = (77 R + 150 G + 29 B + 128) >> 8 (the signature's, scene.py);
  out[y]       the maximum of Y over row y;        out[H + x]  the maximum of Y over column x.
Policy, all integer (``rect_of`` / ``lock`` / ``violates``): a line is a BAR LINE iff its maximum is <= ``peak``; a frame's rect is what
the runs of bar lines from the four edges leave, snapped outward to even; the window of a run is the union of the rects of the first
``probe`` decided frames, used only if its padded area is smaller than the whole frame's; a later frame with a non-bar line outside
the window is a violation.

YUV streams (``pixfmt=``; ``yuv_borders_numpy`` / ``yuv_compose_numpy`` here, ``atmvfi_yuv_borders`` / ``atmvfi_yuv_compose`` on the device,
the same bits).  The line maxima are those of the LUMA plane's sample values, as stored (``msb``: ``>> 6``): a maximum commutes with
every monotone map, so nothing is converted per sample and the threshold is mapped once per stream instead -- ``bar_code(fmt, peak)``
is the sample code of the 8-bit full-range level ``peak``, and ``rect_of`` / ``violates`` / ``probe_stream`` / ``check`` take it as their
threshold.  Chroma is not examined: dark saturated content in a bar counts as bar, which is harmless because the bars of every
produced frame are the nearer original's own samples, moved plane by plane and never converted."""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

# The default, placed from the statistics of tests/golden/active_ref.npz (README "Active picture"; tests/test_active_cpu.py asserts
# the margins): the largest maximum of a bar line at least 8 lines from the picture is 16 (lifted black, every JPEG quality), the
# smallest content-edge maximum of the five pictures 46.  peak must lie in [1.5 x 16, 46 / 1.5] = [24, 30.6]; 24, the lower end (1.50x
# to the bars, 1.92x to the content), is also the default limit of ffmpeg's cropdetect.  No labelled footage was available: the default is unvalidated on real video.
DEFAULT_PEAK = 24

Rect = Tuple[int, int, int, int]          # (y0, x0, y1, x1): rows y0 .. y1 - 1, columns x0 .. x1 - 1
Window = Tuple[int, int, int, int]        # (y0, x0, h, w)


# ------------------------------------------------------------------------------------------------ host twins
def _u8_frame(frame, who: str) -> np.ndarray:
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"{who}: a uint8 [H,W,3] frame expected, got {frame.dtype} {tuple(frame.shape)}")
    return frame


def borders_numpy(frame: np.ndarray, bgr: bool = True) -> np.ndarray:
    """int32[H + W] line maxima of a uint8 [H,W,3] frame on the host: what ``atmvfi_frame_borders`` computes on the device, bit for
    bit."""
    frame = _u8_frame(frame, "borders_numpy")
    H, W = frame.shape[:2]
    if H < 16 or W < 16:
        raise ValueError(f"borders_numpy: the frame must be at least 16 x 16 (got {H} x {W})")
    px = frame.astype(np.int32)
    r, b = (px[:, :, 2], px[:, :, 0]) if bgr else (px[:, :, 0], px[:, :, 2])
    y = (77 * r + 150 * px[:, :, 1] + 29 * b + 128) >> 8
    return np.concatenate([y.max(axis=1), y.max(axis=0)]).astype(np.int32)


def _window(window, H: int, W: int, who: str) -> Window:
    try:
        y0, x0, h, w = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: a window (y0, x0, h, w) expected, got {window!r}") from None
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError(f"{who}: window {h} x {w} at ({y0}, {x0}) outside the {H} x {W} frame")
    return y0, x0, h, w


def compose_numpy(border: np.ndarray, window, src: Optional[np.ndarray] = None, win_u8: Optional[np.ndarray] = None, pad_top: int = 0,
                  pad_left: int = 0, bgr: bool = False) -> np.ndarray:
    """uint8 [H,W,3]: the bytes of ``border`` outside ``window`` = (y0, x0, h, w) and, inside, ``frame_f32_to_u8``'s pixel of ``src``
    (fp32 [3,Hp,Wp], the window at (pad_top, pad_left): x * 255 in fp32, round half to even, clamp, RGB -> BGR if ``bgr``) or the bytes
    of ``win_u8`` (uint8 [h,w,3], already in output order) -- exactly one: what ``atmvfi_frame_compose`` writes, bit for bit."""
    border = _u8_frame(border, "compose_numpy")
    H, W = border.shape[:2]
    y0, x0, h, w = _window(window, H, W, "compose_numpy")
    if (src is None) == (win_u8 is None):
        raise ValueError("compose_numpy: give exactly one of src and win_u8")
    out = border.copy()
    if win_u8 is not None:
        win_u8 = _u8_frame(win_u8, "compose_numpy")
        if win_u8.shape[:2] != (h, w):
            raise ValueError(f"compose_numpy: win_u8 is {win_u8.shape[0]} x {win_u8.shape[1]}, the window {h} x {w}")
        out[y0:y0 + h, x0:x0 + w] = win_u8
        return out
    src = np.asarray(src)
    if src.dtype != np.float32 or src.ndim != 3 or src.shape[0] != 3 or pad_top < 0 or pad_left < 0 or pad_top + h > src.shape[1] or \
            pad_left + w > src.shape[2]:
        raise ValueError(f"compose_numpy: src must be fp32 [3,Hp,Wp] holding the {h} x {w} window at ({pad_top}, {pad_left}), got "
                         f"{src.dtype} {tuple(src.shape)}")
    q = np.rint(src[:, pad_top:pad_top + h, pad_left:pad_left + w] * np.float32(255.0))
    q = np.clip(np.nan_to_num(q, nan=0.0), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    out[y0:y0 + h, x0:x0 + w] = q[:, :, ::-1] if bgr else q
    return out


# ------------------------------------------------------------------------------------------------ YUV twins
def bar_code(fmt, peak: int) -> int:
    """The luma sample code of ``fmt`` (a ``yuv.Format`` or ``Surface``) that the 8-bit full-range level ``peak`` maps to: ``peak``
    itself for full range (8-bit only); limited range at depth d ``(16 << (d - 8)) + (peak * (219 << (d - 8))) // 255`` -- 36 at 8 and
    146 at 10 bits for the default 24.  A line is a bar line iff its largest luma sample is <= this."""
    peak = int(peak)
    if fmt.full_range:
        return peak
    up = fmt.depth - 8
    return (16 << up) + (peak * (219 << up)) // 255


def yuv_borders_numpy(buf, fmt) -> np.ndarray:
    """int32[H + W] line maxima of the luma plane of one frame of ``fmt`` (a ``yuv.Format`` or ``Surface``) on the host: the largest
    sample value (``msb``: ``>> 6``) of every row, then of every column -- what ``atmvfi_yuv_borders`` computes, bit for bit."""
    H, W = fmt.height, fmt.width
    if H < 16 or W < 16:
        raise ValueError(f"yuv_borders_numpy: the frame must be at least 16 x 16 (got {H} x {W})")
    Y = fmt.planes(buf)[0]
    if getattr(fmt, "msb", False):
        Y = Y >> 6
    return np.concatenate([Y.max(axis=1), Y.max(axis=0)]).astype(np.int32)


def yuv_window_error(who: str, fmt, window):
    """The window rule of ``yuv_compose``: origin on multiples of the subsampling step per axis, end on a multiple or at the frame's
    edge (an odd frame's last chroma row or column covers one luma line) -- every chroma sample is the window's or the bars'.  None,
    or the ``ValueError``."""
    y0, x0, h, w = window
    (sy, sx), H, W = fmt.steps, fmt.height, fmt.width
    if y0 % sy or x0 % sx or ((y0 + h) % sy and y0 + h != H) or ((x0 + w) % sx and x0 + w != W):
        return ValueError(f"{who}: the window {h} x {w} at ({y0}, {x0}) must begin and end on multiples of the subsampling step {(sy, sx)} "
                          f"or at the frame's edge")
    return None


def yuv_compose_numpy(border, fmt, window, win_frame) -> np.ndarray:
    """One TIGHT frame of ``fmt`` (1-D; a ``Surface``'s without its padding): the sample values of ``border`` (a frame of ``fmt``)
    outside ``window`` = (y0, x0, h, w) and those of ``win_frame``, a frame of the tight ``fmt.cropped(h, w)``, inside -- what
    ``atmvfi_yuv_compose`` writes when ``win_frame`` is the window's encode, bit for bit."""
    from . import yuv
    H, W = fmt.height, fmt.width
    y0, x0, h, w = _window(window, H, W, "yuv_compose_numpy")
    err = yuv_window_error("yuv_compose_numpy", fmt, (y0, x0, h, w))
    if err is not None:
        raise err
    tight = yuv.as_surface(fmt).tight()
    out = yuv.repack(border, fmt, tight)
    (sy, sx), sub = fmt.steps, tight.cropped(h, w)
    cy, cx = y0 // sy, x0 // sx
    for dst, src, (oy, ox) in zip(tight.planes(out), sub.planes(np.asarray(win_frame)), ((y0, x0), (cy, cx), (cy, cx))):
        dst[oy:oy + src.shape[0], ox:ox + src.shape[1]] = src
    return out


# ------------------------------------------------------------------------------------------------ policy (pure functions)
def _runs(line: np.ndarray, peak: int) -> Tuple[int, int]:
    """(leading, trailing): the lengths of the runs of bar lines (maximum <= peak) from both ends; n, n when every line is one."""
    lit = np.flatnonzero(np.asarray(line, dtype=np.int64) > int(peak))
    n = len(line)
    return (n, n) if lit.size == 0 else (int(lit[0]), n - 1 - int(lit[-1]))


def rect_of(profile, H: int, W: int, peak: int) -> Rect:
    """(y0, x0, y1, x1) of a frame from its line maxima (int[H + W]): what the runs of bar lines from the four edges leave, snapped
    outward to even (``y0 = top & ~1``, ``y1 = H - (bottom & ~1)``, likewise in x).  A dark line inside the picture never matters.  An
    all-bar frame gives an empty rect (y1 <= y0)."""
    profile = np.asarray(profile)
    if profile.shape != (H + W,):
        raise ValueError(f"rect_of: a profile of H + W = {H + W} words expected, got {tuple(profile.shape)}")
    top, bottom = _runs(profile[:H], peak)
    left, right = _runs(profile[H:], peak)
    return top & ~1, left & ~1, H - (bottom & ~1), W - (right & ~1)


def decided(rect: Rect, H: int, W: int) -> bool:
    """False for a rect that is empty or has fewer than H / 4 rows or W / 4 columns: a black frame, a fade-in."""
    rows, cols = rect[2] - rect[0], rect[3] - rect[1]
    return rows > 0 and cols > 0 and 4 * rows >= H and 4 * cols >= W


def padded_area(h: int, w: int, divisor: Optional[int]) -> int:
    if not divisor:
        return h * w
    return (-(-h // divisor) * divisor) * (-(-w // divisor) * divisor)


def lock(rects: Sequence[Rect], H: int, W: int, divisor: Optional[int], need: int = 1) -> Window:
    """The window (y0, x0, h, w) of a run from the rects of its decided frames: their union, if its padded area under ``divisor`` is
    smaller than the whole frame's; else -- and with no rect at all -- the whole frame.  ``divisor=None`` (no padding): the window's
    sides must also be multiples of ``need`` (what the network asks of an unpadded frame), else the whole frame."""
    whole = (0, 0, H, W)
    rects = [r for r in rects if decided(r, H, W)]
    if not rects:
        return whole
    y0, x0 = min(r[0] for r in rects), min(r[1] for r in rects)
    y1, x1 = max(r[2] for r in rects), max(r[3] for r in rects)
    h, w = y1 - y0, x1 - x0
    if not divisor and (h % max(1, int(need)) or w % max(1, int(need))):
        return whole
    return (y0, x0, h, w) if padded_area(h, w, divisor) < padded_area(H, W, divisor) else whole


def violates(profile, window: Window, H: int, W: int, peak: int) -> bool:
    """True when a line outside ``window`` is no bar line (its maximum exceeds ``peak``)."""
    profile = np.asarray(profile)
    if profile.shape != (H + W,):
        raise ValueError(f"violates: a profile of H + W = {H + W} words expected, got {tuple(profile.shape)}")
    y0, x0, h, w = window
    rows, cols = profile[:H], profile[H:]
    outside = np.concatenate([rows[:y0], rows[y0 + h:], cols[:x0], cols[x0 + w:]])
    return bool(outside.size and int(outside.max()) > int(peak))


def fixed_window(window, H: int, W: int) -> Window:
    """``active=(y0, x0, h, w)``: even values inside the frame, or ``ValueError``."""
    y0, x0, h, w = _window(window, H, W, "interpolate_video_nx: active")
    if (y0 | x0 | h | w) & 1:
        raise ValueError(f"interpolate_video_nx: active window {(y0, x0, h, w)} must have even values")
    return y0, x0, h, w


class ActiveArea:
    """The active-picture policy and the record of one run.  Hand one to ``interpolate_video_nx`` as ``active=``.

    ``peak``: a line is a bar line iff its luma maximum is <= peak.  ``probe`` / ``patience``: before its first output the loop reads
    frames until ``probe`` decided ones were seen, ``patience`` frames were read or the stream ended, and locks the union of their rects.
    After the run ``.window`` is the locked (y0, x0, h, w) -- the whole frame when nothing was gained --, ``.probed`` the number of
    frames read for it, ``.fallback_at`` the index of the segment from which the loop went back to the whole frame (None: never) and
    ``.stats`` one rect (y0, x0, y1, x1) per frame examined, probing first.  All are reset at the start of each run."""

    def __init__(self, peak: int = DEFAULT_PEAK, probe: int = 8, patience: int = 48):
        self.peak, self.probe, self.patience = int(peak), int(probe), int(patience)
        if not 0 <= self.peak <= 255 or self.probe < 1 or self.patience < 1:
            raise ValueError(f"ActiveArea: peak in 0..255, probe and patience >= 1 expected (got {peak!r}, {probe!r}, {patience!r})")
        self.begin()

    def begin(self):
        """Start of a run: forget the previous one."""
        self.code = self.peak                        # the run's threshold: ``peak``, or its sample code on a YUV stream (``bar_code``)
        self.window: Optional[Window] = None
        self.probed = 0
        self.fallback_at: Optional[int] = None
        self.stats: List[Rect] = []

    def probe_stream(self, frames: Iterable, H: int, W: int, divisor: Optional[int], need: int, step: int,
                     profile_of: Callable[[np.ndarray], np.ndarray], code: Optional[int] = None, accept: Optional[Callable] = None) -> list:
        """Read frames from ``frames`` and lock ``.window``; returns the frames read, for the loop to replay.  Only every ``step``-th
        frame (the ones the loop uploads) is examined; all count towards ``patience``.  ``code``: the run's threshold in the units of
        the profiles (default ``peak``; a YUV stream: ``bar_code``), which ``check`` keeps using; ``accept(frame)``: raises for a frame
        that is not the stream's (default: uint8 [H,W,3])."""
        self.code = self.peak if code is None else int(code)
        held, rects = [], []
        for f in frames:
            if len(held) % step == 0:
                if accept is not None:
                    accept(f)
                elif getattr(f, "shape", None) != (H, W, 3) or f.dtype != np.uint8:
                    raise ValueError(f"interpolate_video_nx: expected uint8 [{H},{W},3] frames, got {getattr(f, 'dtype', None)} "
                                     f"{tuple(getattr(f, 'shape', ()))}")
                r = rect_of(profile_of(f), H, W, self.code)
                self.stats.append(r)
                if decided(r, H, W):
                    rects.append(r)
            held.append(f)
            if len(rects) >= self.probe or len(held) >= self.patience:
                break
        self.probed = len(held)
        self.window = lock(rects, H, W, divisor, need)
        return held

    def check(self, profile, H: int, W: int) -> bool:
        """Record a frame of the main loop; True when it violates the locked window."""
        self.stats.append(rect_of(profile, H, W, self.code))
        return violates(profile, self.window, H, W, self.code)

    def __repr__(self):
        return f"ActiveArea(peak={self.peak}, probe={self.probe}, patience={self.patience})"
