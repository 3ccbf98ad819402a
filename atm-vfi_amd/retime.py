"""Frame-rate conversion to any output rate (24 -> 60, 25 -> 50 / 60, 30000/1001 -> 60, 24 -> 120, also downwards), with optional
dropping of repeated frames.  Nothing here exists in the reference: its scripts multiply the rate by 2, 4 or 8.

The network predicts the midpoint of two frames only, so every produced frame sits on a DYADIC position of a segment of the source:

* source frame ``i`` is at time ``i / fps_in``; ``kept = [0 = k_0 < k_1 < ...]`` are the frames that survive duplicate dropping (all of
  them without ``dedup``); segment ``j`` spans ``kept[j] ... kept[j + 1]``, ``g_j = kept[j + 1] - kept[j]`` source periods;
* output ``m`` is at ``T_m = m / fps_out`` for every ``m >= 0`` with ``T_m <= kept[-1] / fps_in``; with ``u = T_m fps_in`` it lies in the
  segment with ``kept[j] <= u < kept[j + 1]`` (the one output with ``u == kept[-1]`` is position N of the last segment) at
  ``tau = (u - kept[j]) / g_j``, and is shown as position ``p = floor(tau N + 1/2)`` of ``N = 2**levels`` (half up): ``p == 0`` and
  ``p == N`` are the originals themselves, any other ``p`` the interpolated frame at ``p / N``.  The timing error is at most
  ``g_j / (2 N)`` source periods.  All of this is ``fractions.Fraction`` / integer arithmetic: no float decides a position
  (``retime_slots``);
* only the nodes of the recursion tree that those positions need are evaluated (``sparse_levels``: the ancestor closure): 2.0 forwards
  per interpolated frame at 24 -> 60 with 3 levels, against 7 per segment for the full 8x recursion.

Duplicates (``Duplicates``, ``dedup=``): animation on twos or threes, 24p carried in 30p.  Interpolating between two copies of a picture
and then jumping is the judder a rate conversion is meant to remove; dropping the copy only widens a segment.  A histogram-and-cell-sum
signature (scene.py) cannot see a repeated frame; the per-pixel comparison of two resident frames is ``atmvfi_frame_difference``
(csrc/framediff.hip; ``difference_numpy`` here gives the same bits): int32[258] = the 16 x 16 cell sums of ``|Ya - Yb|``, the peak, the
number of differing pixels, of the signature's luma and cells.  ``d_cell`` = the largest per-pixel cell SAD, ``d_peak`` = the peak; frame
``i`` is a duplicate of source frame ``i - 1`` iff ``d_cell <= cell`` and ``d_peak <= peak``.

``interpolate_video_retimed`` / ``video_retimed``: the loop and its adapter (re-exported from ``host_io`` and ``yuv``)."""
from __future__ import annotations

import itertools
import math
from fractions import Fraction
from typing import Iterable, Iterator, List, Optional, Tuple

import numpy as np

from .multiframe import centre_window
from .scene import _bounds
from .segments import DeviceBackend, HostBackend, chain, open_stream, planar_of

DIFF_WORDS = 258
MAX_LEVELS = 6
# The defaults, placed from the statistics of tests/golden/dedup_ref.npz (README "Frame-rate conversion"; tests/test_retime_cpu.py asserts
# the margins): the duplicate set (every picture against its JPEG q95 / q90 re-encodes and against itself plus uniform noise of +-1, +-2,
# +-3) reaches d_cell 2.99 and d_peak 16; the motion set (128-pixel windows panned by ONE pixel) starts at d_cell 29.27 and d_peak 110.
# Each threshold keeps 1.5 x to both sides: cell in [4.5, 19.5], peak in [24, 73].  No labelled footage was available: the defaults are
# unvalidated on real video.
DEFAULT_CELL = 9.0
DEFAULT_PEAK = 40


# ------------------------------------------------------------------------------------------------ timeline (no device)
def as_rate(value, name: str = "rate") -> Fraction:
    """A frame rate as an exact ``Fraction``: an int, a ``Fraction``, a string such as ``"60000/1001"`` or ``"59.94"`` (read as the
    decimal it spells), or a float that is a whole number.  Other floats are refused: no float decides a position."""
    if isinstance(value, bool):
        raise ValueError(f"{name}: a frame rate expected, got {value!r}")
    if isinstance(value, float):
        if not value.is_integer():
            raise ValueError(f"{name}: {value!r} is not exact; pass a Fraction or a string such as '60000/1001'")
        value = int(value)
    try:
        rate = Fraction(value)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"{name}: a frame rate expected, got {value!r}") from None
    if rate <= 0:
        raise ValueError(f"{name} must be positive, got {value!r}")
    return rate


def _check_rates(fps_in, fps_out, levels) -> Tuple[Fraction, Fraction, int]:
    fi, fo = as_rate(fps_in, "fps_in"), as_rate(fps_out, "fps_out")
    if not isinstance(levels, int) or isinstance(levels, bool) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be in 1..{MAX_LEVELS}, got {levels!r}")
    if (1 << levels) * fi < fo:
        raise ValueError(f"{levels} levels place {1 << levels} positions per source period: too few for {fi} -> {fo} fps "
                         "(a span-1 segment would repeat a position)")
    return fi, fo, levels


def _retime_segments(kept: Iterable[int], fi: Fraction, fo: Fraction, levels: int) -> Iterator[Tuple[int, List[int]]]:
    """``(j, [p, ...])`` for EVERY segment j, in order, as soon as ``kept[j + 1]`` is known (a segment without outputs: an empty
    list); after the last segment the one output at ``kept[-1]`` as ``(j_last, [N])`` -- ``(0, [0])`` for a one-frame stream."""
    n = 1 << levels
    step = fi / fo                                   # source periods per output
    it = iter(kept)
    lo = next(it, None)
    if lo is None:
        return
    if lo != 0:
        raise ValueError(f"kept must start with frame 0, got {lo!r}")
    m, j = 0, -1
    for hi in it:
        if not isinstance(hi, (int, np.integer)) or hi <= lo:
            raise ValueError(f"kept must be strictly increasing integers, got {hi!r} after {lo!r}")
        j += 1
        ps = []
        while m * step < hi:                         # kept[j] <= u < kept[j + 1]
            ps.append(math.floor((m * step - lo) / (hi - lo) * n + Fraction(1, 2)))
            m += 1
        yield j, ps
        lo = int(hi)
    if m * step == lo:                               # u == kept[-1]
        yield (j, [n]) if j >= 0 else (0, [0])


def retime_slots(kept: Iterable[int], fps_in, fps_out, levels: int) -> Iterator[Tuple[int, int]]:
    """The outputs of a rate conversion in time order, as ``(j, p)`` = (segment, position 0..N of it), N = ``2**levels`` (the module's
    docstring has the definition).  ``kept``: any iterable of the kept source frame indices, ``0 = k_0 < k_1 < ...``; an output is yielded
    as soon as ``kept[j + 1]`` has been read, so a loop over it streams.  ``ValueError`` for a rate <= 0, ``levels`` outside 1..6, or
    ``2**levels fps_in < fps_out``.  ``fps_out < fps_in`` is allowed: segments without an output simply yield nothing."""
    fi, fo, levels = _check_rates(fps_in, fps_out, levels)
    return ((j, p) for j, ps in _retime_segments(kept, fi, fo, levels) for p in ps)


def sparse_levels(positions: Iterable[int], levels: int) -> List[List[Tuple[int, int, int]]]:
    """The part of the N-x recursion (N = ``2**levels``) that ``positions`` (each in 0..N; 0 and N are the source frames and need
    nothing) depend on -- their ancestor closure -- in ``multiframe.nx_levels``' form: ``levels`` lists of (left, right, out), sorted by
    ``out``, some possibly empty.  Node ``p = odd * 2**s`` has the parents ``p - 2**s`` and ``p + 2**s`` and belongs to level
    ``levels - s``.  ``sparse_levels(range(1, N), L) == nx_levels(N)``."""
    if not isinstance(levels, int) or isinstance(levels, bool) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be in 1..{MAX_LEVELS}, got {levels!r}")
    n = 1 << levels
    need, todo = set(), []
    for p in positions:
        if not isinstance(p, (int, np.integer)) or isinstance(p, bool) or not 0 <= p <= n:
            raise ValueError(f"positions must be integers in 0..{n}, got {p!r}")
        todo.append(int(p))
    while todo:
        p = todo.pop()
        if p in need or p == 0 or p == n:
            continue
        need.add(p)
        half = p & -p                                # 2**s
        todo += [p - half, p + half]
    out: List[List[Tuple[int, int, int]]] = [[] for _ in range(levels)]
    for p in sorted(need):
        half = p & -p
        out[levels - half.bit_length()].append((p - half, p + half, p))
    return out


# ------------------------------------------------------------------------------------------------ duplicates
def difference_numpy(a: np.ndarray, b: np.ndarray, window: Optional[Tuple[int, int, int, int]] = None, bgr: bool = True) -> np.ndarray:
    """int32[258] difference of the ``window`` = (y0, x0, h, w) (default: the whole frame) of two uint8 [H,W,3] frames on the host: what
    ``atmvfi_frame_difference`` computes on the device, bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    for f in (a, b):
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f"difference_numpy: uint8 [H,W,3] frames expected, got {f.dtype} {tuple(f.shape)}")
    if a.shape != b.shape:
        raise ValueError(f"difference_numpy: two frames of one size expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    H, W = a.shape[:2]
    y0, x0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
    if h < 16 or w < 16:
        raise ValueError(f"difference_numpy: the window must be at least 16 x 16 (got {h} x {w})")
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"difference_numpy: window {h} x {w} at ({y0}, {x0}) outside the {H} x {W} frame")

    def luma(f):
        px = f[y0:y0 + h, x0:x0 + w].astype(np.int32)
        r, bl = (px[:, :, 2], px[:, :, 0]) if bgr else (px[:, :, 0], px[:, :, 2])
        return (77 * r + 150 * px[:, :, 1] + 29 * bl + 128) >> 8
    d = np.abs(luma(a) - luma(b))
    rows = np.add.reduceat(d.astype(np.int64), _bounds(h)[:16], axis=0)
    cells = np.add.reduceat(rows, _bounds(w)[:16], axis=1)
    if cells.max() > np.iinfo(np.int32).max or h * w > np.iinfo(np.int32).max:
        raise ValueError(f"difference_numpy: a {h} x {w} window is too large (cell sums and the pixel count must fit int32)")
    out = np.empty(DIFF_WORDS, np.int32)
    out[:256] = cells.reshape(-1)
    out[256] = d.max()
    out[257] = np.count_nonzero(d)
    return out


def duplicate_statistics(diff, h: int, w: int) -> Tuple[float, int]:
    """(d_cell, d_peak) of a difference of h x w windows: ``d_cell`` = the maximum over the 256 cells of SAD / pixels of the cell, in
    float64 from the integers; ``d_peak`` = word 256."""
    d = np.asarray(diff, dtype=np.int64)
    if d.shape != (DIFF_WORDS,):
        raise ValueError("duplicate_statistics: a difference of 258 words expected")
    n = np.outer(np.diff(_bounds(h)), np.diff(_bounds(w))).reshape(-1).astype(np.float64)
    return float(np.max(d[:256] / n)), int(d[256])


class Duplicates:
    """The duplicate policy and the record of one run.  Frame ``i >= 1`` is compared with source frame ``i - 1`` (kept or not) over the
    crop window; it is a duplicate iff ``d_cell <= cell`` and ``d_peak <= peak``, and it is DROPPED iff it is a duplicate, fewer than
    ``max_run`` frames were dropped immediately before it, and it is not the last frame of the stream (the last frame is always kept: a
    frame held back as a duplicate becomes kept when the stream ends behind it).  Hand one to ``interpolate_video_retimed`` as
    ``dedup=``; after the run ``.dropped`` holds the indices of the dropped frames and ``.stats`` one ``(d_cell, d_peak)`` per compared
    frame (``stats[i - 1]`` is frame i's).  Both are reset at the start of each run.

    The limit of the policy: a small low-contrast change -- an 8 x 8 patch moving by 40 levels -- passes both tests and is dropped, and a
    heavily re-compressed repeat (JPEG q75 reaches 6.2 / 41, q50 9.0 / 52) is not seen as one."""

    def __init__(self, cell: float = DEFAULT_CELL, peak: int = DEFAULT_PEAK, max_run: int = 3):
        if int(max_run) < 0:
            raise ValueError(f"max_run must be >= 0, got {max_run!r}")
        self.cell, self.peak, self.max_run = float(cell), int(peak), int(max_run)
        self.begin()

    def begin(self):
        """Start of a run: forget the previous one."""
        self.dropped: List[int] = []
        self.stats: List[Tuple[float, int]] = []
        self._run = 0

    def is_duplicate(self, d_cell: float, d_peak: int) -> bool:
        return d_cell <= self.cell and d_peak <= self.peak

    def judge(self, diff, h: int, w: int) -> bool:
        """Record the next frame (its difference against the source frame before it, of h x w windows); True when it is dropped --
        provisionally: ``finish`` takes the stream's last frame back."""
        st = duplicate_statistics(diff, h, w)
        index = len(self.stats) + 1
        self.stats.append(st)
        drop = self.is_duplicate(*st) and self._run < self.max_run
        self._run = self._run + 1 if drop else 0
        if drop:
            self.dropped.append(index)
        return drop

    def finish(self) -> bool:
        """End of the stream: the last frame is kept.  True when it had been held back as a duplicate."""
        if self.dropped and self.dropped[-1] == len(self.stats):
            self.dropped.pop()
            self._run = 0
            return True
        return False

    def __repr__(self):
        return f"Duplicates(cell={self.cell}, peak={self.peak}, max_run={self.max_run})"


# ------------------------------------------------------------------------------------------------ the loop
def interpolate_video_retimed(frames, model, fps_in, fps_out, levels: int = 3, dedup: Optional[Duplicates] = None,
                              crop: Optional[Tuple[int, int]] = None, isBGR: bool = True, divisor: Optional[int] = 64, tta: bool = False,
                              max_batch: int = 4, pool: bool = True, scene=None, pixfmt=None, keep_depth: bool = False, report=None,
                              motion_scale: int = 1, active=None, shutter=None):
    """Frame-rate conversion ``fps_in -> fps_out`` (ints, ``Fraction``s or strings such as ``"30000/1001"``) over any iterable of uint8
    [H,W,3] frames: yields, in time order, output ``m`` at ``m / fps_out`` for every m up to the last kept frame's time, as the module's
    docstring defines -- the nearest of ``N = 2**levels`` positions of its segment.  Positions 0 and N are the originals and pass through
    as the caller's own arrays (their centre ``crop=(h, w)`` window when given), position N of a segment and position 0 of the next
    being the same frame; every output is yielded exactly once.  Only the recursion nodes that a segment's positions need are evaluated
    (``sparse_levels``), level by level in batches of at most ``max_batch`` pairs on ``segments._SegmentRunner``; a segment without an
    interpolated output (``fps_out < fps_in`` has many) runs no forward.  When a widened segment maps two outputs to one position, the
    second is a copy of the same produced frame.

    ``dedup`` (a ``Duplicates``; default None): every frame is compared with the source frame before it (``atmvfi_frame_difference`` on
    the copy stream behind its upload, against the previous upload's resident frame; one 1 032-byte read per frame), duplicates are
    dropped from the timeline and their segment widens: the outputs in it are interpolated between the kept frames around them.
    ``dedup.dropped`` / ``dedup.stats`` hold the run's record.

    ``scene`` (a ``scene.SceneCuts``): the signatures of a segment's two ends are compared; a cut segment runs no forward, its outputs
    at ``p <= N/2`` are copies of the first original and the rest copies of the second.

    ``divisor``, ``tta``, ``pool``, ``pixfmt`` and ``keep_depth`` as in ``multiframe.interpolate_video_nx`` (with a 10-bit ``pixfmt``
    and ``keep_depth`` the resident uint8 RGB frame is made only when ``dedup`` or ``scene`` needs it; a ``yuv.Packed`` is taken as
    there: unpacked behind the upload, packed in front of the download; a ``yuv.DeepRGB`` as there too: ``keep_depth=True`` only, the
    8-bit probe picture made when ``dedup`` or ``scene`` needs it, not with ``active`` or ``shutter``).  There is no ``time_interval``.
    A model without the HIP backend gets the same frames through torch and the numpy twins.  ``report`` (a dict): filled with
    ``"outputs"``, ``"interpolated"`` and ``"forwards"`` (the recursion nodes evaluated: pairs through the network, the second pass of
    flip-TTA not counted) of the run.

    ``shutter`` (a ``shutter.Shutter``, or an angle in degrees; default None: the loop as above, nothing new allocated or launched): a
    synthetic shutter.  The outputs stay the same in number and time; each integrates the samples -- the dyadic positions of the
    stream -- inside its exposure ``angle / 360 / fps_out``, in linear light or in code values, as atm-vfi_amd/shutter.py defines
    (``shutter_slots`` is the timeline, ``blend_numpy`` the arithmetic).  A segment's sparse schedule is the union of its interior
    samples; a sample is accumulated on the device where it would have been converted for the output ring
    (``atmvfi_shutter_accumulate``) and an output that closes is resolved there (``atmvfi_shutter_resolve``) and leaves by the
    existing device -> host copy.  An output of a single sample is exactly what ``shutter=None`` yields for that position (an
    original: the caller's own array), so a small angle reproduces the unblurred conversion bit for bit; no output mixes two shots
    of a ``scene`` cut; with a ``pixfmt`` the originals of a blurred output take part as their decoded RGB.  8-bit only:
    ``keep_depth`` on a 10-bit format is refused (``ValueError``), as are an angle outside (0, 360] and an exposure whose total
    weight exceeds 32767.  ``report`` also gets ``"blended"`` (outputs of more than one sample) and ``"samples"``.

    ``active`` (an ``active.ActiveArea`` or a fixed even window; default None: the loop as above, nothing new allocated or launched;
    not with ``crop`` or ``shutter``: ``ValueError``): the active picture of letterboxed video, as in
    ``multiframe.interpolate_video_nx`` -- the same probe-and-replay in front of the loop, RGB frames and ``pixfmt`` alike (a 10-bit
    one with ``keep_depth``).  Every uploaded frame is examined, a dropped duplicate too; a frame with a non-bar line outside the
    window sends the loop back to the whole frame from the segment that ends at it (a dropped one: at the next kept frame).  A
    produced position p carries the bars of the nearer end of its segment (p <= N/2: the first), also across a widened segment; a
    cut segment or one without an interpolated output runs no forward.

    ``motion_scale`` (1, the default: the loop as above, nothing new allocated or launched; or 2): half-resolution motion, as in
    ``multiframe.interpolate_video_nx``; not with ``shutter`` (``ValueError``).

    The rates and ``levels`` are checked at the call; ``ValueError`` as ``retime_slots`` raises it."""
    fi, fo, levels = _check_rates(fps_in, fps_out, levels)
    from .pixfmt import deep_rgb_refusals
    from .scaled import check_scale
    motion_scale = check_scale(motion_scale, "interpolate_video_retimed: motion_scale")
    if motion_scale == 2 and shutter is not None:
        raise ValueError("interpolate_video_retimed: shutter does not go with motion_scale=2")
    deep_rgb_refusals("interpolate_video_retimed", pixfmt, keep_depth, active=active, shutter=shutter)
    if active is not None and shutter is not None:
        raise ValueError("interpolate_video_retimed: active does not go with shutter (a blurred output mixes whole frames)")
    if shutter is not None:
        from .shutter import as_shutter
        shutter = as_shutter(shutter)
        shutter.check(fi, fo, levels)
        if pixfmt is not None and keep_depth and pixfmt.depth == 10:
            raise ValueError("interpolate_video_retimed: shutter blends 8-bit pixels; a 10-bit blend (keep_depth=True) is out of scope")
    return _retimed(frames, model, fi, fo, levels, dedup, crop, isBGR, divisor, tta, max_batch, pool, scene, pixfmt, keep_depth, report,
                    shutter, active, motion_scale)


def _retimed(frames, model, fi, fo, levels, dedup, crop, isBGR, divisor, tta, max_batch, pool, scene, pixfmt, keep_depth, report,
             shutter=None, active=None, motion_scale=1):
    from .host_io import _hip_ops_of
    from .multiframe import _active_refusals, _active_window
    if active is not None and crop is not None:
        _active_refusals("interpolate_video_retimed", active, crop, pixfmt, keep_depth, None)
    area = active if hasattr(active, "probe_stream") else None
    if area is not None:
        area.begin()
    n = 1 << levels
    if scene is not None:
        scene.begin()
    if dedup is not None:
        dedup.begin()
    count = report if report is not None else {}
    count.update(outputs=0, interpolated=0, forwards=0)
    it = iter(frames)
    first = next(it, None)
    if first is None:
        return
    if active is not None:
        _active_refusals("interpolate_video_retimed", active, crop, pixfmt, keep_depth, first)
    st = open_stream(first, crop, pixfmt, keep_depth, isBGR, "interpolate_video_retimed")
    packed, pixfmt = planar_of(pixfmt)               # (a packed 4:2:2 stream is its planar stream from here on)
    if pixfmt is None and (first.ndim != 3 or first.shape[2] != 3 or first.dtype != np.uint8):
        raise ValueError(f"interpolate_video_retimed: expected uint8 [H,W,3] frames, got {first.dtype} {tuple(first.shape)}")
    (h, w), original = st.window[2:], st.original
    ops, dev = _hip_ops_of(model)
    common = dict(n=n, divisor=divisor, tta=tta, pixfmt=pixfmt, caller="interpolate_video_retimed")
    if packed is not None:
        common["packed"] = packed
    if motion_scale != 1:
        common["motion_scale"] = motion_scale
    generic = ops is None or not hasattr(ops, "pool_blocks")
    if active is not None:
        win, source = _active_window(active, first, it, st, model, None if generic else (ops, dev), divisor, 1, pixfmt,
                                     "interpolate_video_retimed", packed=packed, scale=motion_scale)
        first, it = next(source), source             # (the probed frames replayed)
        common.update(window=win, watch=area is not None)
    if generic:
        be = HostBackend(model, st, max_batch=max(1, int(max_batch)), dedup=dedup, light=None if shutter is None else shutter.light, **common)
    else:
        # distinct interpolated positions of one segment: its outputs, at most ceil(g fps_out / fps_in) of them, g <= max_run + 1
        span = 1 if dedup is None else dedup.max_run + 1
        per_segment = -((-span * fo.numerator * fi.denominator) // (fo.denominator * fi.numerator))
        be = DeviceBackend(model, ops, dev, st, crop=crop, max_batch=max_batch, pool=pool, scene=scene is not None, dedup=dedup is not None,
                           sparse=True, out_slots=min(n - 1, per_segment),
                           blend=None if shutter is None else (shutter.light, per_segment + 1), **common)   # the outputs a segment can close
    ends, number = {}, itertools.count()             # kept frames by their number on the timeline, until their segments are done
    sig = {}                                         # signatures of segment ends that a later segment starts with
    violated = []                                    # an examined frame left the active picture: the next segment runs on the whole frame

    def judged(e):
        """a frame whose upload has landed: its borders against the locked window (kept or dropped: it was uploaded)"""
        if be.watching and not violated and area.check(be.borders(e), st.H, st.W):
            violated.append(e["i"])

    def kept():
        """The indices of the kept frames.  Frame k is judged when frame k + 1 has been read (and its upload started: one frame ahead
        of the forwards); a duplicate that turns out to be the last frame is kept."""
        pending = None
        for i, f in enumerate(chain(first, it)):
            e = {"i": i, "f": f}
            be.admit(e)
            if i == 0:
                be.first(e)
                if scene is not None:
                    sig[0] = be.signature(e)
            if pending is not None:
                judged(pending)
            if pending is not None and not (dedup is not None and pending["i"] > 0 and dedup.judge(be.difference(pending), h, w)):
                ends[next(number)] = pending
                yield pending["i"]
            pending = e
        judged(pending)
        if dedup is not None and pending["i"] > 0:
            dedup.judge(be.difference(pending), h, w)
            dedup.finish()
        ends[next(number)] = pending
        yield pending["i"]

    def blended():
        """The loop under a shutter: ``shutter._plan``'s records, one per segment and one for the end of the stream."""
        from .shutter import _plan
        count.update(blended=0, samples=0)

        def cut_of(j):
            if scene is None:
                return False
            sig_a = sig.pop(j)
            sig[j + 1] = be.signature(ends[j + 1])
            return scene.judge(sig_a, sig[j + 1], h, w)
        first_original = {}                          # output -> [samples gathered, its first sample if that is an original: (frame, copy?)]
        for rec in _plan(kept(), fi, fo, levels, shutter, cut_of):
            j, cut, tail = rec["j"], rec["cut"], rec["tail"]
            a, b = ends.get(j), ends.get(j + 1)
            ops, outs = [], []
            singles = {op[1] for op in rec["ops"] if op[0] == "close" and len(op[3]) == 1}       # they close here with one sample
            unsent = set()
            for op in rec["ops"]:
                if op[0] == "add":
                    p = op[2]
                    got = first_original.setdefault(op[1], [0, None])
                    if got[0] == 0 and (p == 0 or p == n or cut):
                        got[1] = ((a if (p == 0 or (p < n and p <= n // 2)) else b)["f"], 0 < p < n)
                        if op[1] in singles:         # an original that passes through: the backend never hears of it
                            unsent.add(op[1])
                    got[0] += 1
                    if op[1] not in unsent:
                        ops.append(op)
                elif op[0] == "reset":
                    first_original.pop(op[1], None)
                    unsent.discard(op[1])
                    ops.append(op)
                else:
                    m, pos, samples = op[1:]
                    got = first_original.pop(m)
                    count["outputs"] += 1
                    count["interpolated"] += 0 < pos[1] < n
                    count["samples"] += len(samples)
                    count["blended"] += len(samples) > 1
                    single = got[1] if len(samples) == 1 else None       # what shutter=None yields for that position
                    outs.append(single)
                    if m not in unsent:
                        ops.append(("close" if single is None else "drop", m))
            if rec["need"] and not cut:
                count["forwards"] += sum(len(lv) for lv in sparse_levels(rec["need"], levels))
            made = iter(be.blended(a, b, ops, rec["need"], cut, tail))
            for single in outs:
                if single is None:
                    yield next(made)
                else:
                    yield np.array(original(single[0]), copy=True) if single[1] else original(single[0])
            if not tail:
                del ends[j]
    try:
        if shutter is not None:
            yield from blended()
            return
        ran = -1
        for j, ps in _retime_segments(kept(), fi, fo, levels):
            if j == ran or j + 1 not in ends:        # the output at the last kept frame (a one-frame stream: at its only frame)
                count["outputs"] += len(ps)
                for _ in ps:
                    yield original(ends[j + 1 if j == ran else j]["f"])
                continue
            a, b = ends[j], ends[j + 1]
            ran = j
            if violated and be.watching:             # (every frame up to b has been examined)
                area.fallback_at = j
                be.whole_frame()
            interior = sorted({p for p in ps if 0 < p < n})
            cut = False
            if scene is not None:
                sig_a = sig.pop(j)
                sig[j + 1] = be.signature(b)
                cut = scene.judge(sig_a, sig[j + 1], h, w)
            made = be.segment(a, b, interior, cut)
            if made:
                count["forwards"] += sum(len(lv) for lv in sparse_levels(interior, levels))
            count["outputs"] += len(ps)
            count["interpolated"] += sum(0 < p < n for p in ps)
            seen = set()
            for p in ps:
                if p == 0 or p == n:
                    yield original((a if p == 0 else b)["f"])
                elif cut:
                    yield np.array(original((a if p <= n // 2 else b)["f"]), copy=True)
                elif p in seen:
                    yield made[p].copy()
                else:
                    seen.add(p)
                    yield made[p]
            del ends[j]
    finally:
        be.close()


def video_retimed(cap, make_writer, model, fps_out, interpolator=None, crop: Optional[Tuple[int, int]] = None, **kw):
    """``multiframe.video_nx``'s contract for a rate conversion: reads FPS, W, H from ``cap`` (a whole-number FPS, or pass ``fps_in=``
    among ``kw`` for an exact one such as ``"30000/1001"``), opens the sink with ``make_writer(fps_out, (W, H))`` -- the crop's size
    when cropping; ``fps_out`` as an int when it is whole, else as a float -- writes what ``interpolator(frames, model, fps_in,
    fps_out, crop=, **kw)`` yields (default ``interpolate_video_retimed``) and releases both ends, also when a frame fails.  Returns
    ``{"fps_in", "fps_out", "size", "frames_in", "frames_out", "forwards"}``, with ``dedup=`` among ``kw`` also ``"dropped"`` and with
    ``scene=`` also ``"cuts"``."""
    from .host_io import CAP_PROP_FPS, CAP_PROP_FRAME_HEIGHT, CAP_PROP_FRAME_WIDTH, capture_frames
    fi = as_rate(kw.pop("fps_in"), "fps_in") if "fps_in" in kw else as_rate(int(cap.get(CAP_PROP_FPS)), "fps_in")
    fo = as_rate(fps_out, "fps_out")
    _check_rates(fi, fo, kw.get("levels", 3))
    w, h = int(cap.get(CAP_PROP_FRAME_WIDTH)), int(cap.get(CAP_PROP_FRAME_HEIGHT))
    _, _, oh, ow = centre_window(h, w, crop)
    plain = lambda r: int(r) if r.denominator == 1 else float(r)
    out = make_writer(plain(fo), (ow, oh))
    n_in, report = [0], kw.pop("report", None)
    report = {} if report is None else report

    def counted():
        for f in capture_frames(cap):
            if f.shape[:2] != (h, w):
                raise ValueError(f"video_retimed: the capture announced {w}x{h} frames and delivered {f.shape[1]}x{f.shape[0]}")
            n_in[0] += 1
            yield f
    n_out = 0
    try:
        for frame in (interpolator or interpolate_video_retimed)(counted(), model, fi, fo, crop=crop, report=report, **kw):
            out.write(frame)
            n_out += 1
    finally:
        cap.release()
        out.release()
    info = {"fps_in": plain(fi), "fps_out": plain(fo), "size": (ow, oh), "frames_in": n_in[0], "frames_out": n_out,
            "forwards": report.get("forwards", 0)}
    if kw.get("dedup") is not None:
        info["dropped"] = list(kw["dedup"].dropped)
    if kw.get("scene") is not None:
        info["cuts"] = list(kw["scene"].cuts)
    return info
