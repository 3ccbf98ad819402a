"""A synthetic shutter (motion blur) for the frame-rate conversion of ``retime.py``: every output integrates the sub-frames of the N-x
recursion that fall inside its exposure, instead of showing the one dyadic position nearest to its time.  Nothing here exists in the
reference, and nothing here touches a device: the definition, the two light tables and the host twin of the two kernels of
csrc/shutter.hip (``atmvfi_shutter_accumulate`` / ``atmvfi_shutter_resolve``).  ``fractions.Fraction`` and integers only: no float
decides the membership of a window.

* ``N = 2**levels``; ``kept``, segments ``j`` and spans ``g_j`` as in ``retime.py``, ``J`` segments.  The SAMPLES of the stream are the
  positions ``(j, p)``, ``p = 0 ... N - 1``, of every segment plus the terminal ``(J - 1, N)``; sample ``(j, p)`` is at
  ``t = (kept[j] + g_j p / N) / fps_in`` and weighs ``g_j`` (a widened segment's sparser samples count for the time they stand for).
  ``(j, N)`` of a non-last segment IS sample ``(j + 1, 0)`` and is counted there.
* ``Shutter(angle, light)``: the exposure is ``E = angle / 360 / fps_out``, ``0 < angle <= 360``.  The outputs are ``retime_slots``'
  outputs, unchanged in number and time (``T_m = m / fps_out``, position ``(j_m, p_m)``); output m's window is the half-open
  ``[T_m - E/2, T_m + E/2)`` and ``S_m`` the samples inside it whose SHOT is that of ``(j_m, p_m)`` -- ``{(j_m, p_m)}`` if there is
  none.  The shot of a sample: the number of cut segments completely before it, plus one inside a cut segment at ``p > N/2`` (a cut
  segment's samples are copies of its first frame up to ``N/2`` and of its second beyond, as everywhere): no output mixes two shots.
  Windows of distinct outputs are disjoint (``angle <= 360``): a sample belongs to at most one output.
* ``|S_m| == 1``: the output is what ``shutter=None`` yields for that position (a small angle reproduces the unblurred conversion bit
  for bit).  Otherwise it is, per channel, ``acc = sum w_k LUT[q_k]``, ``v = (acc + (Wt >> 1)) // Wt``, ``Wt = sum w_k <= 32767``
  (``65535 Wt`` stays inside int32), and the code k whose ``LUT[k]`` is nearest to v: the number of ``k`` in 1..255 with
  ``v >= thr[k]``, ``thr[k] = (LUT[k - 1] + LUT[k] + 1) >> 1``.  ``q_k`` is the uint8 RGB pixel the loop would have emitted for the
  sample.  ``light="code"``: ``LUT[q] = 257 q`` (the plain average of code values); ``light="linear"``: ``LUT[q] = rint(65535
  eotf(q / 255))`` with the sRGB curve, derived in float64 (tests/test_shutter_cpu.py holds the literals below to the derivation).
* The stated limit: the half-open window puts an output's mean sample time up to half a sample (``g / (2 N)`` source periods) early
  -- the size of the retiming's own timing error.  A trapezoid rule is out of scope.

``shutter_slots`` is the timeline, ``blend_numpy`` the arithmetic, ``_plan`` the streaming form both ``shutter_slots`` and the loop
(``retime.interpolate_video_retimed(shutter=)``) read."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Iterable, Iterator, List, Sequence, Tuple

import numpy as np

from .retime import _check_rates, as_rate

MAX_WEIGHT = 32767

SHUTTER_TABLES = {
    "code": (
            0,   257,   514,   771,  1028,  1285,  1542,  1799,  2056,  2313,  2570,  2827,  3084,  3341,  3598,  3855,
         4112,  4369,  4626,  4883,  5140,  5397,  5654,  5911,  6168,  6425,  6682,  6939,  7196,  7453,  7710,  7967,
         8224,  8481,  8738,  8995,  9252,  9509,  9766, 10023, 10280, 10537, 10794, 11051, 11308, 11565, 11822, 12079,
        12336, 12593, 12850, 13107, 13364, 13621, 13878, 14135, 14392, 14649, 14906, 15163, 15420, 15677, 15934, 16191,
        16448, 16705, 16962, 17219, 17476, 17733, 17990, 18247, 18504, 18761, 19018, 19275, 19532, 19789, 20046, 20303,
        20560, 20817, 21074, 21331, 21588, 21845, 22102, 22359, 22616, 22873, 23130, 23387, 23644, 23901, 24158, 24415,
        24672, 24929, 25186, 25443, 25700, 25957, 26214, 26471, 26728, 26985, 27242, 27499, 27756, 28013, 28270, 28527,
        28784, 29041, 29298, 29555, 29812, 30069, 30326, 30583, 30840, 31097, 31354, 31611, 31868, 32125, 32382, 32639,
        32896, 33153, 33410, 33667, 33924, 34181, 34438, 34695, 34952, 35209, 35466, 35723, 35980, 36237, 36494, 36751,
        37008, 37265, 37522, 37779, 38036, 38293, 38550, 38807, 39064, 39321, 39578, 39835, 40092, 40349, 40606, 40863,
        41120, 41377, 41634, 41891, 42148, 42405, 42662, 42919, 43176, 43433, 43690, 43947, 44204, 44461, 44718, 44975,
        45232, 45489, 45746, 46003, 46260, 46517, 46774, 47031, 47288, 47545, 47802, 48059, 48316, 48573, 48830, 49087,
        49344, 49601, 49858, 50115, 50372, 50629, 50886, 51143, 51400, 51657, 51914, 52171, 52428, 52685, 52942, 53199,
        53456, 53713, 53970, 54227, 54484, 54741, 54998, 55255, 55512, 55769, 56026, 56283, 56540, 56797, 57054, 57311,
        57568, 57825, 58082, 58339, 58596, 58853, 59110, 59367, 59624, 59881, 60138, 60395, 60652, 60909, 61166, 61423,
        61680, 61937, 62194, 62451, 62708, 62965, 63222, 63479, 63736, 63993, 64250, 64507, 64764, 65021, 65278, 65535),
    "linear": (
            0,    20,    40,    60,    80,    99,   119,   139,   159,   179,   199,   219,   241,   264,   288,   313,
          340,   367,   396,   427,   458,   491,   526,   562,   599,   637,   677,   718,   761,   805,   851,   898,
          947,   997,  1048,  1101,  1156,  1212,  1270,  1330,  1391,  1453,  1517,  1583,  1651,  1720,  1790,  1863,
         1937,  2013,  2090,  2170,  2250,  2333,  2418,  2504,  2592,  2681,  2773,  2866,  2961,  3058,  3157,  3258,
         3360,  3464,  3570,  3678,  3788,  3900,  4014,  4129,  4247,  4366,  4488,  4611,  4736,  4864,  4993,  5124,
         5257,  5392,  5530,  5669,  5810,  5953,  6099,  6246,  6395,  6547,  6700,  6856,  7014,  7174,  7335,  7500,
         7666,  7834,  8004,  8177,  8352,  8528,  8708,  8889,  9072,  9258,  9445,  9635,  9828, 10022, 10219, 10417,
        10619, 10822, 11028, 11235, 11446, 11658, 11873, 12090, 12309, 12530, 12754, 12980, 13209, 13440, 13673, 13909,
        14146, 14387, 14629, 14874, 15122, 15371, 15623, 15878, 16135, 16394, 16656, 16920, 17187, 17456, 17727, 18001,
        18277, 18556, 18837, 19121, 19407, 19696, 19987, 20281, 20577, 20876, 21177, 21481, 21787, 22096, 22407, 22721,
        23038, 23357, 23678, 24002, 24329, 24658, 24990, 25325, 25662, 26001, 26344, 26688, 27036, 27386, 27739, 28094,
        28452, 28813, 29176, 29542, 29911, 30282, 30656, 31033, 31412, 31794, 32179, 32567, 32957, 33350, 33745, 34143,
        34544, 34948, 35355, 35764, 36176, 36591, 37008, 37429, 37852, 38278, 38706, 39138, 39572, 40009, 40449, 40891,
        41337, 41785, 42236, 42690, 43147, 43606, 44069, 44534, 45002, 45473, 45947, 46423, 46903, 47385, 47871, 48359,
        48850, 49344, 49841, 50341, 50844, 51349, 51858, 52369, 52884, 53401, 53921, 54445, 54971, 55500, 56032, 56567,
        57105, 57646, 58190, 58737, 59287, 59840, 60396, 60955, 61517, 62082, 62650, 63221, 63795, 64372, 64952, 65535),
}
LIGHTS = ("code", "linear")          # the kernels' `light` argument: the index


class Shutter:
    """``angle`` degrees of a rotary shutter at the OUTPUT rate (180: half the output period is exposed; an int, a ``Fraction`` or a
    string read by ``retime.as_rate``'s rules; ``0 < angle <= 360``) and the domain the samples are averaged in (``light``: "linear"
    or "code")."""

    def __init__(self, angle=180, light: str = "linear"):
        try:
            self.angle = as_rate(angle, "angle")
        except ValueError:
            raise ValueError(f"angle must satisfy 0 < angle <= 360, got {angle!r}") from None
        if self.angle > 360:
            raise ValueError(f"angle must satisfy 0 < angle <= 360, got {angle!r}")
        if light not in SHUTTER_TABLES:
            raise ValueError(f"light must be one of {LIGHTS}, got {light!r}")
        self.light = light

    def check(self, fi: Fraction, fo: Fraction, levels: int):
        """``ValueError`` when a window of this conversion can weigh more than ``MAX_WEIGHT`` (without dropped frames a window of
        ``E fps_in`` source periods holds at most ``ceil(E fps_in N)`` samples of weight 1)."""
        worst = math.ceil(self.angle / 360 * fi / fo * (1 << levels))
        if worst > MAX_WEIGHT:
            raise ValueError(f"shutter: {fi} -> {fo} fps with {levels} levels at {self.angle} degrees puts up to {worst} samples into "
                             f"one exposure; the total weight must stay within {MAX_WEIGHT}")

    def __repr__(self):
        return f"Shutter(angle={self.angle}, light={self.light!r})"


def as_shutter(value) -> Shutter:
    """A ``Shutter``, or an angle (then ``light="linear"``)."""
    return value if isinstance(value, Shutter) else Shutter(value)


def _plan(kept: Iterable[int], fi: Fraction, fo: Fraction, levels: int, shutter: Shutter, cut_of=None) -> Iterator[dict]:
    """The exposure of every output, streamed segment by segment: one record ``{"j", "cut", "tail", "ops", "need"}`` per segment as soon
    as ``kept[j + 1]`` is known, and a last one with ``tail`` set for what the end of the stream decides (the terminal sample and the
    outputs still open).  ``cut_of(j)`` is asked once per segment, when it is reached.  ``ops`` in time order:

    * ``("add", m, p, w)``: position p of this segment (0..N - 1; N only in the tail record, or as the sole sample of an output that no
      sample reaches) joins output m with weight w;
    * ``("reset", m)``: what output m has gathered so far belongs to another shot and is forgotten;
    * ``("close", m, (j_m, p_m), [(j, p, w), ...])``: output m is complete -- ``S_m`` -- and leaves, in the order of m.

    ``need``: the interior positions among this record's adds -- the sparse schedule of the segment.  An output whose own position lies
    in a later segment gathers samples before its shot is known: a sample of another shot than the ones gathered resets it (the
    output's shot cannot be the earlier one), and so does its own position when that turns out to lie beyond a cut."""
    n = 1 << levels
    step = fi / fo                                   # source periods per output
    half = shutter.angle / 720 * step                # half an exposure, in source periods
    it = iter(kept)
    lo = next(it, None)
    if lo is None:
        return
    if lo != 0:
        raise ValueError(f"kept must start with frame 0, got {lo!r}")
    open_ = {}                                       # m -> [position or None, shot or None, shot of the samples, samples, weight]
    state = {"m": 0, "base": 0}                      # the next output to place; cut segments completely before the current one
    POS, SHOT, RUN, S, WT = range(5)

    def add(ops, need, m, j, p, w, shot):
        rec = open_.setdefault(m, [None, None, None, [], 0])
        if rec[SHOT] is not None:
            if shot != rec[SHOT]:
                return
        elif rec[S] and rec[RUN] != shot:
            rec[S], rec[WT] = [], 0
            ops.append(("reset", m))
        rec[RUN] = shot
        rec[S].append((j, p, w))
        rec[WT] += w
        ops.append(("add", m, p, w))
        if 0 < p < n:
            need.add(p)

    def place(ops, m, pos, shot):
        rec = open_.setdefault(m, [None, None, None, [], 0])
        rec[POS], rec[SHOT] = pos, shot
        if rec[S] and rec[RUN] != shot:
            rec[S], rec[WT] = [], 0
            ops.append(("reset", m))

    def close(ops, m):
        rec = open_.pop(m)
        if rec[WT] > MAX_WEIGHT:
            raise ValueError(f"shutter: {fi} -> {fo} fps with {levels} levels at {shutter.angle} degrees: output {m} gathers a total "
                             f"weight of {rec[WT]}, the limit is {MAX_WEIGHT}")
        ops.append(("close", m, rec[POS], list(rec[S])))

    j, g = -1, 1
    for hi in it:
        if not isinstance(hi, (int, np.integer)) or hi <= lo:
            raise ValueError(f"kept must be strictly increasing integers, got {hi!r} after {lo!r}")
        j, g = j + 1, int(hi - lo)
        cut = bool(cut_of(j)) if cut_of is not None else False
        ops, need, base = [], set(), state["base"]
        shot_at = lambda p: base + (1 if cut and 2 * p > n else 0)
        while state["m"] * step < hi:                # kept[j] <= u < kept[j + 1]: retime_slots' position
            p = math.floor((state["m"] * step - lo) / g * n + Fraction(1, 2))
            place(ops, state["m"], (j, p), shot_at(p))
            state["m"] += 1
        for p in range(n):
            u = lo + Fraction(g * p, n)
            m = max(0, math.floor((u - half) / step) + 1)          # the one output with u < T_m + E/2 <= u + a period of the output
            if m * step - half <= u:
                add(ops, need, m, j, p, g, shot_at(p))
        for m in sorted(open_):
            pos = open_[m][POS]
            if pos is None:
                continue
            t = lo + Fraction(g * pos[1], n)
            if pos[0] == j and not open_[m][S] and not (m * step - half <= t < m * step + half):
                # no sample reaches this output and none will (its own position is the nearest): it shows its position
                add(ops, need, m, j, pos[1], g, open_[m][SHOT])
            if m * step + half <= hi:                # every later sample lies behind the window
                close(ops, m)
        yield {"j": j, "cut": cut, "tail": False, "ops": ops, "need": sorted(need)}
        state["base"] += cut
        lo = int(hi)
    ops = []
    if j < 0:                                        # a one-frame stream: its frame
        ops += [("add", 0, 0, 1), ("close", 0, (0, 0), [(0, 0, 1)])]
        yield {"j": 0, "cut": False, "tail": True, "ops": ops, "need": []}
        return
    if state["m"] * step == lo:                      # the output at the last kept frame
        place(ops, state["m"], (j, n), state["base"])
        state["m"] += 1
    m = max(0, math.floor((lo - half) / step) + 1)
    if m * step - half <= lo:                        # the terminal sample
        add(ops, set(), m, j, n, g, state["base"])
    for m in sorted(open_):
        if open_[m][POS] is not None:                # (an output placed behind the last frame does not exist)
            close(ops, m)
    yield {"j": j, "cut": False, "tail": True, "ops": ops, "need": []}


class Exposures:
    """The open outputs of a blended stream on the device (``segments._SegmentRunner`` executes ``_plan``'s operations on it): an
    int32 accumulator [3,h,w] per output that is open.  They are allocated on demand, one per output that is open at the same time --
    the level-ordered schedule visits a segment's samples out of time order, so every output a segment touches is open until the
    segment ends -- returned to a free list when their output closes, and kept until the runner goes.  An fp32 sample is the padded
    canvas (``pad_top`` / ``pad_left``), a uint8 sample the window itself."""

    def __init__(self, ops, dev, h: int, w: int, light: str, pad_top: int = 0, pad_left: int = 0):
        self.ops, self.dev, self.h, self.w, self.light, self.pad = ops, dev, h, w, light, (pad_top, pad_left)
        self.accs, self.free = [], []                # the accumulators; the indices of those no output holds
        self.open = {}                               # output -> [accumulator, samples and weight since the last reset]

    def add(self, m: int, weight: int, src=None, src_u8=None):
        a = self.open.get(m)
        if a is None:
            if not self.free:
                import torch
                self.accs.append(torch.empty(3, self.h, self.w, dtype=torch.int32, device=self.dev))
                self.free.append(len(self.accs) - 1)
            a = self.open[m] = [self.free.pop(), 0, 0]
        pad = self.pad if src is not None else (0, 0)
        self.ops.shutter_accumulate(self.accs[a[0]], src=src, src_u8=src_u8, weight=weight, light=self.light, first=a[1] == 0,
                                    pad_top=pad[0], pad_left=pad[1])
        a[1] += 1
        a[2] += weight

    def reset(self, m: int):
        """Forget what output ``m`` has gathered (a scene cut); it keeps its accumulator."""
        if m in self.open:
            self.open[m][1:] = [0, 0]

    def close(self, m: int):
        """Output ``m`` is done: ``(accumulator, total weight)`` for ``shutter_resolve`` -- the accumulator goes back to the free list,
        and stream order keeps it whole until the resolve has read it -- or None for an output that holds no sample."""
        a = self.open.pop(m, None)
        if a is None:
            return None
        self.free.append(a[0])
        return (self.accs[a[0]], a[2]) if a[1] else None


def shutter_slots(kept: Iterable[int], fps_in, fps_out, levels: int, shutter, cuts: Iterable[int] = ()) -> Iterator[Tuple[int, Tuple[int, int], List[Tuple[int, int, int]]]]:
    """The outputs of a rate conversion under a shutter, in time order, as ``(m, (j_m, p_m), [(j, p, weight), ...])``: the output's
    number, its ``retime_slots`` position and its sample set ``S_m`` in time order (the module's docstring has the definition).  ``cuts``:
    the indices of the segments that are scene cuts.  Streams as ``retime_slots`` does: an output is yielded as soon as the last kept
    frame its window can reach has been read.  ``ValueError`` as ``retime_slots`` raises it, for an angle outside (0, 360] and for a
    total weight beyond 32767 (naming rates, levels and angle)."""
    fi, fo, levels = _check_rates(fps_in, fps_out, levels)
    shutter = as_shutter(shutter)
    shutter.check(fi, fo, levels)
    cuts = frozenset(int(c) for c in cuts)
    return ((op[1], op[2], op[3]) for rec in _plan(kept, fi, fo, levels, shutter, cuts.__contains__) for op in rec["ops"] if op[0] == "close")


def blend_numpy(frames_u8: Sequence[np.ndarray], weights: Sequence[int], light: str = "linear") -> np.ndarray:
    """The blend of uint8 frames of one shape with positive integer weights on the host: what ``atmvfi_shutter_accumulate`` over the
    frames followed by ``atmvfi_shutter_resolve`` computes on the device, bit for bit."""
    if light not in SHUTTER_TABLES:
        raise ValueError(f"light must be one of {LIGHTS}, got {light!r}")
    frames = [np.asarray(f) for f in frames_u8]
    weights = [int(w) for w in weights]
    if not frames or len(frames) != len(weights):
        raise ValueError(f"blend_numpy: {len(frames)} frames and {len(weights)} weights")
    if any(f.dtype != np.uint8 or f.shape != frames[0].shape for f in frames):
        raise ValueError("blend_numpy: uint8 frames of one shape expected")
    total = sum(weights)
    if min(weights) < 1 or total > MAX_WEIGHT:
        raise ValueError(f"blend_numpy: weights must be >= 1 and sum to at most {MAX_WEIGHT}, got {weights}")
    lut = np.asarray(SHUTTER_TABLES[light], dtype=np.int32)
    acc = np.zeros(frames[0].shape, dtype=np.int32)                # 65535 * 32767 < 2**31
    for f, w in zip(frames, weights):
        acc += np.int32(w) * lut[f]
    v = (acc + (total >> 1)) // total
    thr = (lut[:-1] + lut[1:] + 1) >> 1                            # thr[k - 1] of the definition's thr[k], k = 1..255
    return np.searchsorted(thr, v, side="right").astype(np.uint8)
