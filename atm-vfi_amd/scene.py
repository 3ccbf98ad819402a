"""Scene-cut detection for the video loops (``host_io.interpolate_video_2x`` / ``FramePipeline``, ``multiframe.interpolate_video_nx``).

The reference's scripts only ever see single-shot clips and have no such guard: nothing here is ported.  At a shot change the network
is asked for the "motion" between two unrelated pictures and returns a morph of both; with ``scene=SceneCuts()`` the loops compare a
small integer signature of the two ends of every segment, run NO forward for a segment they class a cut, and emit copies of the nearer
original instead (ties to the earlier one).  Off by default (``scene=None``: the code path and the frames of before).

Signature of a frame window (``signature_numpy`` here, ``atmvfi_frame_signature`` / ``HipOps.frame_signature`` on the device, the same
bits): int32[288] --
  luma           Y = (77 R + 150 G + 29 B + 128) >> 8;
  sig[16 i + j]  the sum of Y over rows [i h // 16, (i + 1) h // 16) x columns [j w // 16, (j + 1) w // 16): a 16 x 16 grid;
  sig[256 + b]   the number of pixels with Y >> 3 == b: 32 bins.
Statistics of two signatures (``cut_statistics``): ``d_hist`` = sum |Ha - Hb| / (2 h w) in [0, 1] -- blind to motion, separates shots --
and ``d_grid`` = the mean over the cells of |mean luma a - mean luma b| -- exposure flicker moves bins but hardly moves mean luma.  A
segment is a cut iff ``d_hist >= hist`` AND ``d_grid >= grid``."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

SIG_WORDS = 288
# The defaults, placed from the statistics of tests/golden/scene_ref.npz (README "Scene cuts"; tests/test_scene_cpu.py asserts the
# margins): the largest d_hist of the continuous set (the consecutive pair; 128-pixel windows of every picture panned by up to 1/4 of
# their side) is 0.2007, the smallest d_hist of the nine unrelated pairs 0.4893 and their smallest d_grid 39.35.  hist must lie in
# [1.5 x 0.2007, 0.4893 / 1.5] = [0.301, 0.326]; grid below 39.35 / 1.5 = 26.2.  No labelled footage was available: the defaults are
# unvalidated on real video.
DEFAULT_HIST = 0.31
DEFAULT_GRID = 24.0


def _bounds(n: int) -> np.ndarray:
    return np.arange(17, dtype=np.int64) * n // 16


def signature_numpy(frame: np.ndarray, window: Optional[Tuple[int, int, int, int]] = None, bgr: bool = True) -> np.ndarray:
    """int32[288] signature of the ``window`` = (y0, x0, h, w) (default: the whole frame) of a uint8 [H,W,3] frame on the host: what
    ``atmvfi_frame_signature`` computes on the device, bit for bit."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"signature_numpy: a uint8 [H,W,3] frame expected, got {frame.dtype} {tuple(frame.shape)}")
    H, W = frame.shape[:2]
    y0, x0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
    if h < 16 or w < 16:
        raise ValueError(f"signature_numpy: the window must be at least 16 x 16 (got {h} x {w})")
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"signature_numpy: window {h} x {w} at ({y0}, {x0}) outside the {H} x {W} frame")
    px = frame[y0:y0 + h, x0:x0 + w].astype(np.int32)
    r, b = (px[:, :, 2], px[:, :, 0]) if bgr else (px[:, :, 0], px[:, :, 2])
    y = (77 * r + 150 * px[:, :, 1] + 29 * b + 128) >> 8
    rows = np.add.reduceat(y.astype(np.int64), _bounds(h)[:16], axis=0)
    cells = np.add.reduceat(rows, _bounds(w)[:16], axis=1)
    if cells.max() > np.iinfo(np.int32).max:
        raise ValueError(f"signature_numpy: a {h} x {w} window is too large (cell sums must fit int32)")
    sig = np.empty(SIG_WORDS, np.int32)
    sig[:256] = cells.reshape(-1)
    sig[256:] = np.bincount((y >> 3).reshape(-1), minlength=32)
    return sig


def cut_statistics(sig_a, sig_b, h: int, w: int) -> Tuple[float, float]:
    """(d_hist, d_grid) of two signatures of h x w windows, in float64 from the integers: ``d_hist`` = sum_b |Ha - Hb| / (2 h w), in
    [0, 1]; ``d_grid`` = the mean over the 256 cells of |Sa / n - Sb / n| in luma levels, n the cell's pixel count."""
    a, b = np.asarray(sig_a, dtype=np.int64), np.asarray(sig_b, dtype=np.int64)
    if a.shape != (SIG_WORDS,) or b.shape != (SIG_WORDS,):
        raise ValueError("cut_statistics: two signatures of 288 words expected")
    d_hist = float(np.abs(a[256:] - b[256:]).sum()) / (2.0 * h * w)
    n = np.outer(np.diff(_bounds(h)), np.diff(_bounds(w))).reshape(-1).astype(np.float64)
    d_grid = float(np.mean(np.abs(a[:256] / n - b[:256] / n)))
    return d_hist, d_grid


class SceneCuts:
    """The cut policy and the record of one run: a segment is a cut iff ``d_hist >= hist`` and ``d_grid >= grid``.  Hand one to
    ``interpolate_video_2x`` / ``FramePipeline`` / ``interpolate_video_nx`` as ``scene=``; after the run ``.cuts`` holds the 0-based
    indices of the cut segments and ``.stats`` one ``(d_hist, d_grid)`` per segment.  Both are reset at the start of each run."""

    def __init__(self, hist: float = DEFAULT_HIST, grid: float = DEFAULT_GRID):
        self.hist, self.grid = float(hist), float(grid)
        self.cuts: List[int] = []
        self.stats: List[Tuple[float, float]] = []

    def begin(self):
        """Start of a run: forget the previous one."""
        self.cuts, self.stats = [], []

    def is_cut(self, d_hist: float, d_grid: float) -> bool:
        return d_hist >= self.hist and d_grid >= self.grid

    def judge(self, sig_a, sig_b, h: int, w: int) -> bool:
        """Record the next segment (its two ends' signatures, of h x w windows); True when it is a cut."""
        st = cut_statistics(sig_a, sig_b, h, w)
        cut = self.is_cut(*st)
        if cut:
            self.cuts.append(len(self.stats))
        self.stats.append(st)
        return cut

    def __repr__(self):
        return f"SceneCuts(hist={self.hist}, grid={self.grid})"


def cut_fill(first, second, factor: int) -> list:
    """The ``factor - 1`` frames of a cut segment: position k <= N / 2 is a copy of ``first``, k > N / 2 a copy of ``second`` (the
    nearer original, ties to the earlier one).  ``first`` / ``second``: the two originals as they are emitted (already cropped)."""
    return [np.array(first if k <= factor // 2 else second, copy=True) for k in range(1, factor)]
