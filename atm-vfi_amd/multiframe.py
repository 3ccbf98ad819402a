"""4x / 8x (any power of two) interpolation by recursion, the loop of the reference's ``benchmark/davis-vid.py:88-135``:
``pred = F(I0, I1)``, then ``pred025 = F(I0, pred)`` and ``pred075 = F(pred, I1)`` -- the deeper levels fed with the UNROUNDED fp32
prediction -- with a centre crop, a frame stride (``time_interval``) and optional flip-TTA.

* ``nx_levels`` / ``nx_sequence``: the schedule and the order of the loop, pure Python (tested without a GPU);
* ``FramePool``: device-resident frames and per-frame tokens, so that what ``Network.forward`` computes per frame (encoder, cross-scale
  fusions, LayerNorm'ed tokens) is computed once per DISTINCT frame (``Network.forward_pooled``) instead of once per appearance in a
  pair: N/2 frame encodes per segment instead of 2 (N - 1);
* ``interpolate_video_nx`` / ``video_nx`` / ``inference_nx``: the loop and its adapters (re-exported from ``host_io``); the loop reaches the
  model through the backends of segments.py, which it shares with ``retime.interpolate_video_retimed``.

Deviations from the script, on purpose: (1) with ``tta`` EVERY produced frame is the flip-TTA average (the script averages the middle
frame only); the next level still consumes the un-averaged prediction, as the script's order of operations has it (:102-112).  (2) with
a crop the originals are written cropped (the script hands the uncropped originals to a writer opened at the crop size, :86, 120, 135).
Opt-in, not in the script at all: ``scene=SceneCuts()`` (atm-vfi_amd/scene.py) runs no forward for a segment that straddles a shot
change and emits copies of the nearer original.
"""
from __future__ import annotations

import itertools
from collections import deque
from typing import Callable, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import segments
from .segments import DeviceBackend, HostBackend, chain, open_stream, planar_of


# ------------------------------------------------------------------------------------------------ schedule (no device)
def nx_levels(factor: int) -> List[List[Tuple[int, int, int]]]:
    """The recursion of an N-x interpolation (N = ``factor``, a power of two >= 2) in slot positions 0..N (0 and N: the two source
    frames; position k: the frame at t = k/N): level 1 ``[(0, N, N/2)]``, level 2 ``[(0, N/2, N/4), (N/2, N, 3N/4)]``, ... each entry
    (left, right, out).  The 2^(l-1) pairs of level l are independent of each other: a ready-made batch."""
    if not isinstance(factor, int) or isinstance(factor, bool) or factor < 2 or factor & (factor - 1):
        raise ValueError(f"factor must be a power of two >= 2, got {factor!r}")
    levels, span = [], factor
    while span >= 2:
        levels.append([(a, a + span, a + span // 2) for a in range(0, factor, span)])
        span //= 2
    return levels


def nx_sequence(frames: Iterable, segment: Callable, factor: int, time_interval: int = 1) -> Iterator:
    """The order of davis-vid.py:88-135 over any iterable: per segment ``(f_i, f_{i+s})``, ``s = time_interval``,
    ``i in range(0, n - s, s)``, yields ``f_i`` and then the ``factor - 1`` frames that ``segment(f_i, f_{i+s})`` returns (t = 1/N ...
    (N-1)/N, in temporal order); after the last segment its second frame once.  Frames between ``i`` and ``i + s`` are consumed and
    dropped, and so are trailing frames that form no full segment.  An empty input yields nothing; fewer than ``s + 1`` frames yield
    nothing either (the script writes an undefined frame there).  ``segment`` sees its frames one segment ahead of the yields only
    in so far as it is called before its first output is yielded."""
    nx_levels(factor)
    s = int(time_interval)
    if s < 1:
        raise ValueError(f"time_interval must be >= 1, got {time_interval!r}")
    it = iter(frames)
    a = next(it, None)
    if a is None:
        return
    last = None
    while True:
        b = None
        for _ in range(s):
            b = next(it, None)
            if b is None:
                break
        if b is None:
            break
        mids = segment(a, b)
        if len(mids) != factor - 1:
            raise ValueError(f"segment returned {len(mids)} frames, {factor - 1} expected")
        yield a
        for m in mids:
            yield m
        a = last = b
    if last is not None:
        yield last


def centre_window(height: int, width: int, crop: Optional[Tuple[int, int]]) -> Tuple[int, int, int, int]:
    """(y0, x0, h, w) of davis-vid.py:95: rows ``H//2 - h//2 ... H//2 + h//2``, columns likewise (so an odd h loses one row: h is
    rounded down to even, as the script's slice does).  ``crop=None``: the whole frame."""
    if crop is None:
        return 0, 0, height, width
    h, w = int(crop[0]), int(crop[1])
    if h < 2 or w < 2 or h > height or w > width:
        raise ValueError(f"crop {crop} does not fit a {height}x{width} frame")
    return height // 2 - h // 2, width // 2 - w // 2, 2 * (h // 2), 2 * (w // 2)


# ------------------------------------------------------------------------------------------------ pool
class FramePool:
    """``slots`` device-resident frames of one padded size with what the network computes per frame: ``frames`` [S,3,Hp,Wp] fp32,
    ``tokens_l`` [S,h*w,C] (LayerNorm'ed local tokens, h = Hp/8), ``tokens_g`` [S,h_*w_,Cg] (global tokens, h_ = Hp/16) and per slot a
    validity key of its tokens (``keys``: None = stale; else the weights' identity, ``global_motion``, precision / checked build -- the
    device and shape are the pool's own).  At 1080p (1088x1920, network_base) a slot is 25 + 50 + 22 MB: nine slots (8x) stay under
    1 GB.  ``Network.forward_pooled(pool, left, right)`` fills and reads the tokens."""

    def __init__(self, model, hp: int, wp: int, slots: int):
        import torch
        dev = next(model.parameters()).device
        if dev.type != "cuda" or not hasattr(model, "forward_pooled"):
            raise RuntimeError("FramePool needs an atm-vfi_amd Network on the GPU")
        if hp % 16 or wp % 16:
            raise ValueError(f"FramePool: Hp and Wp must be multiples of 16 (got {hp}x{wp})")
        if not 1 <= int(slots) <= 1024:
            raise ValueError(f"FramePool: 1..1024 slots, got {slots}")
        v = model._v
        self.model, self.hp, self.wp, self.slots, self.device = model, int(hp), int(wp), int(slots), dev
        self.ops = model._ops(dev)
        mk = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.frames = mk(self.slots, 3, hp, wp)
        self.tokens_l = mk(self.slots, (hp // 8) * (wp // 8), v.local_dim)
        self.tokens_g = mk(self.slots, (hp // 16) * (wp // 16), v.global_dim)
        self.keys: List[Optional[tuple]] = [None] * self.slots

    def frame(self, slot: int):
        """The [1,3,Hp,Wp] view of a slot's frame.  Whoever writes through it calls ``invalidate(slot)``."""
        return self.frames[slot:slot + 1]

    def invalidate(self, slot: int):
        self.keys[slot] = None

    def put(self, slot: int, src):
        """Write a frame ([3,Hp,Wp] or [1,3,Hp,Wp] fp32 on the pool's device) into ``slot`` (one ``atmvfi_pool_blocks`` scatter)
        and invalidate the slot's tokens."""
        if tuple(src.shape[-3:]) != (3, self.hp, self.wp) or src.numel() != 3 * self.hp * self.wp:
            raise ValueError(f"FramePool.put: expected a [3,{self.hp},{self.wp}] frame, got {tuple(src.shape)}")
        if src.device != self.device:
            raise ValueError(f"FramePool.put: the frame lives on {src.device}, the pool on {self.device}")
        self.ops.pool_blocks(self.frames, [int(slot)], src.detach().float().contiguous(), to_pool=True)
        self.keys[slot] = None

    def nbytes(self) -> int:
        return 4 * (self.frames.numel() + self.tokens_l.numel() + self.tokens_g.numel())

    def release(self):
        self.frames = self.tokens_l = self.tokens_g = None
        self.keys = []


# ------------------------------------------------------------------------------------------------ the loop
# (``_Uploader`` and ``_SegmentRunner`` live in segments.py with the rest of the plumbing; they stay reachable here, where the tests
# and the documents have always named them)
_Uploader, _SegmentRunner = segments._Uploader, segments._SegmentRunner


def _active_window(active, first, it, st, model, device, divisor, step, pixfmt=None, caller: str = "interpolate_video_nx", packed=None,
                   scale: int = 1):
    """``(window, frames)`` of ``active=`` (both loops): a fixed window as it is given; an ``ActiveArea`` after its probe, the frames
    it read replayed in front of ``it`` (the loop uploads them again); a fixed window's even values fit every subsampling.  ``device``: ``(ops, dev)`` of the HIP backend, or None.
    A window that gains nothing is None: the whole frame, the plain loop.  ``pixfmt``: the frames are that format's, the profiles
    those of their luma plane and the threshold its sample code (``active.bar_code``); a locked window that ends on an odd line of a
    subsampled frame is widened by that line (``active.yuv_window_error`` holds the rule).  ``packed`` (a ``yuv.Packed``, ``pixfmt`` its
    planar format): a probed frame is unpacked first (on the device by ``HipOps.yuv_unpack``).  ``scale`` (``motion_scale``): the canvas
    a window is judged under is that of ``divisor * scale``, in multiples the network needs after the reduction."""
    from . import active as _active
    accept = (packed or pixfmt).check if pixfmt is not None else None
    if not hasattr(active, "probe_stream"):
        win, frames = _active.fixed_window(active, st.H, st.W), chain(first, it)
    else:
        if device is None:
            if packed is not None:
                from .yuv import unpack_numpy
                profile_of = lambda f: _active.yuv_borders_numpy(unpack_numpy(f, packed), pixfmt)
            else:
                profile_of = (lambda f: _active.borders_numpy(f, bgr=st.isBGR)) if pixfmt is None else (lambda f: _active.yuv_borders_numpy(f, pixfmt))
        else:
            import torch
            ops, dev = device

            def profile_of(f):
                with torch.cuda.device(dev):
                    if pixfmt is None:
                        return ops.frame_borders(torch.from_numpy(np.ascontiguousarray(f)).to(dev), bgr=bool(st.isBGR)).cpu().numpy()
                    d = torch.from_numpy(accept(f, caller).view(np.uint8)).to(dev)
                    return ops.yuv_borders(d if packed is None else ops.yuv_unpack(d, packed), pixfmt).cpu().numpy()
        need = (16 if getattr(model, "global_motion", True) else 8) * scale
        divisor = divisor * scale if divisor else divisor
        yuv_kw = {} if pixfmt is None else dict(code=_active.bar_code(pixfmt, active.peak), accept=lambda f: accept(f, caller))
        held = active.probe_stream(chain(first, it), st.H, st.W, divisor, need, step, profile_of, **yuv_kw)
        win = active.window
        if pixfmt is not None and win != (0, 0, st.H, st.W):
            (sy, sx), (y0, x0, h, w) = pixfmt.steps, win
            win = active.window = (y0, x0, h + (y0 + h) % sy * (y0 + h != st.H), w + (x0 + w) % sx * (x0 + w != st.W))
        frames = itertools.chain(held, it)
    return (None if win == (0, 0, st.H, st.W) else win), frames


def _active_refusals(caller: str, active, crop, pixfmt, keep_depth, first):
    """What ``active=`` does not go with, and -- with a ``pixfmt`` -- a first frame that is not of the format."""
    if crop is not None:
        raise ValueError(f"{caller}: active does not go with crop (the active picture is found on whole frames)")
    if pixfmt is None:
        return
    if pixfmt.depth == 10 and not keep_depth:
        raise ValueError(f"{caller}: active with a 10-bit pixfmt needs the depth kept: pass keep_depth=True (8-bit output converts the "
                         "originals through RGB, so the bars of produced frames could not match theirs)")
    a = np.asarray(first)
    if a.dtype != pixfmt.dtype or a.size != pixfmt.frame_samples:
        raise ValueError(f"{caller}: active with pixfmt expects frames of the format, got {a.dtype} {tuple(a.shape)}")


def interpolate_video_nx(frames, model, factor: int = 4, time_interval: int = 1, crop: Optional[Tuple[int, int]] = None, isBGR: bool = True,
                         divisor: Optional[int] = 64, tta: bool = False, max_batch: int = 4, pool: bool = True, scene=None, pixfmt=None,
                         keep_depth: bool = False, active=None, motion_scale: int = 1):
    """N-x slow motion over any iterable of uint8 [H,W,3] frames (davis-vid.py:88-135; decoding / encoding stays with the caller):
    per segment ``(f_i, f_{i+s})``, ``s = time_interval``, yields ``f_i`` and the frames at t = 1/N ... (N-1)/N, after the last segment
    its second frame once -- ``segments * N + 1`` frames.  Originals pass through bit-equal (their centre ``crop=(h, w)`` window when
    given); frames between ``i`` and ``i + s`` are consumed and dropped.

    Every source frame is uploaded and converted once and lives in pool position 0 or N; position N's frame and tokens become position
    0's of the next segment by swapping slots.  Level l of the recursion runs as batches of at most ``max_batch`` pairs; its ``I_t``
    feeds the next level as returned (padded fp32, unrounded).  ``divisor=None``: no padding (what the script does).  ``tta``: every
    produced frame is the flip-TTA average; the next level consumes the un-averaged prediction.  ``pool=True``: per-frame work once per
    distinct frame (``Network.forward_pooled``); ``pool=False``: plain ``model.forward`` calls on the same level batches (same
    outputs; the A/B baseline, and what a model without ``forward_pooled`` gets).  The runner raises ``model.max_workspaces`` to the
    number of batch sizes of its schedule while it runs and restores it.  ``factor=2`` gives ``interpolate_video_2x``'s frames.

    ``scene`` (a ``scene.SceneCuts``; default None: the loop as above): scene-cut detection, not in the script.  The signatures of
    the two ends of every segment (of the crop window; computed on the device where the frame lands, one segment ahead) are compared;
    a segment classed a cut runs NO forward and its N - 1 positions are bit-equal copies of the nearer original -- position k <= N/2
    the first, k > N/2 the second, cropped when cropping.  ``scene.cuts`` / ``scene.stats`` hold the run's record.

    ``pixfmt`` (a ``yuv.Format``; default None: the loop as above): frames in and out are packed planar I420 arrays.  Every source
    frame is uploaded as I420 and decoded once on the copy stream into the resident uint8 RGB frame everything above reads; produced
    frames are encoded on the device (8-bit, also for 10-bit input) in front of the device -> host copy.  Originals -- cut copies
    included -- pass through as the caller's own bytes (``yuv.crop`` of them when cropping: the crop origin must be even, else
    ``ValueError``); ``isBGR`` is ignored.

    ``keep_depth`` (default False; changes nothing without a 10-bit ``pixfmt``): the 10-bit depth is kept end to end.  Every uploaded
    frame is decoded by ``atmvfi_yuv_decode`` (``keep_depth``) straight from its I420 bytes into the pool slot (the crop as the kernel's window;
    the network sees q / 1023, no 8-bit round trip), produced frames are ``atmvfi_yuv_encode`` (depth 10) of the fp32 prediction (with
    ``tta``: of the fp32 average) and leave as 1-D uint16 arrays of ``pixfmt.cropped(h, w)``; deeper levels consume the unrounded
    prediction as always.  The resident uint8 RGB frame is made only when ``scene`` needs its signature: signatures, and so cut
    decisions, are those of the 8-bit path.  A model without the HIP backend does the same with the numpy twins.

    ``active`` (an ``active.ActiveArea`` or a fixed even window ``(y0, x0, h, w)``; default None: the loop as above; not with
    ``crop``: ``ValueError``): the network runs on the active picture of letterboxed video.  Before its first output the loop
    reads frames from ``frames`` until the policy has seen enough (``probe`` decided frames, ``patience`` frames, the stream's end),
    keeps them on the host, locks the union of their rects as the window and replays them.  A window that gains nothing under
    ``divisor`` is the whole frame: the loop as above.  Else every uploaded frame gets its line maxima on the copy stream
    (``HipOps.frame_borders``), the network runs at the window's padded size, and a produced position k is the prediction's window
    composed (``HipOps.frame_compose``) into a full-size frame with the bars of the nearer original (k <= N/2: the first).  Originals
    pass through as the caller's own arrays; ``scene`` works on the whole frame as before.  A frame with a non-bar line outside the
    window ends it: from the segment that ends at that frame on, the loop runs on the whole frame for the rest of the stream.  With
    ``time_interval`` > 1 the frames that are not uploaded are not examined.  A tuple is never probed nor checked.
    ``active.window`` / ``.probed`` / ``.fallback_at`` / ``.stats`` hold the run's record.
    With a ``pixfmt`` the line maxima are those of the uploaded surface's luma plane (``HipOps.yuv_borders``) against the sample code
    of ``peak`` (``active.bar_code``; chroma is not examined), the two border frames are the uploaded surfaces themselves, and a
    produced position leaves through ``HipOps.yuv_compose``: the window's encode inside, the nearer original's own samples outside,
    plane by plane -- the bars never pass through RGB.  A 10-bit ``pixfmt`` needs ``keep_depth=True`` (``ValueError`` otherwise: 8-bit
    output converts the originals on the host, no sample copy reproduces that), and a first frame that is not of the ``pixfmt`` is
    refused before anything else.

    ``pixfmt=yuv.Packed(...)`` (packed 4:2:2: uyvy, yuy2, y210, v210): inside, the stream is the planar 4:2:2 stream of
    ``pixfmt.planar`` and everything above holds for it.  Every uploaded frame is unpacked on the copy stream right behind its copy
    (``HipOps.yuv_unpack``), a produced frame is encoded into a planar scratch and packed into the output ring (``HipOps.yuv_pack``):
    the same layout at its default pitch, for a 10-bit layout without ``keep_depth`` its 8-bit one (v210 -> uyvy, y210 -> yuy2).
    Originals at the default pitch are the caller's own arrays, at another pitch their tight repacks.

    ``pixfmt=yuv.DeepRGB(...)`` (RGB above 8 bits: rgb48, bgr48 or gbrp at 10, 12 or 16 bit; needs ``keep_depth=True``, not with
    ``active``: ``ValueError``): frames are contiguous uint16 arrays of ``3 H W`` samples in any shape.  The uploaded bytes stay in the
    slot, ``atmvfi_rgb16_decode`` decodes them straight into the pool slot (the crop as the kernel's window; the network sees
    min(q, top) / top) and, only when ``scene`` needs a signature, makes the 8-bit probe picture q >> (depth - 8) on the copy stream:
    cut decisions are those of the truncated 8-bit picture.  Produced frames are ``atmvfi_rgb16_encode`` of the fp32 prediction (with
    ``tta``: of the fp32 average) and leave as 1-D uint16 arrays of ``pixfmt.cropped(h, w)``; originals, and the copies of a cut
    segment, are the caller's own arrays (``rgb16.crop`` of them when cropping: any origin).

    ``motion_scale`` (1, the default: the loop as above; or 2; scaled.py holds the definition): half-resolution motion, an addition
    of this project.  Frames are padded under ``divisor * 2``; every source frame is kept at full size AND as its 2 x 2 box average
    (``HipOps.frame_half``); the network -- pool, plans, batches as above -- runs on the halves, and one launch per batch
    (``HipOps.synth_up2``) up-samples flows, mask and residual and warps and blends the full-size frames.  A deeper level reads the
    full-size prediction as returned and its half.  Everything that consumes the prediction -- ``pixfmt``, ``keep_depth``, ``crop``,
    ``scene``, ``active``, ``tta`` (rotated at full size), ``time_interval`` -- is as above.  A model without the HIP backend does the
    same with the numpy twins."""
    from .host_io import _hip_ops_of
    from .scaled import check_scale
    motion_scale = check_scale(motion_scale, "interpolate_video_nx: motion_scale")
    from .pixfmt import deep_rgb_refusals
    from .scene import cut_fill
    nx_levels(factor)
    deep_rgb_refusals("interpolate_video_nx", pixfmt, keep_depth, active=active)
    if active is not None and crop is not None:
        _active_refusals("interpolate_video_nx", active, crop, pixfmt, keep_depth, None)
    if scene is not None:
        scene.begin()
    area = active if hasattr(active, "probe_stream") else None
    if area is not None:
        area.begin()
    it = iter(frames)
    first = next(it, None)
    if first is None:
        return
    if active is not None:
        _active_refusals("interpolate_video_nx", active, crop, pixfmt, keep_depth, first)
    st = open_stream(first, crop, pixfmt, keep_depth, isBGR, "interpolate_video_nx")
    packed, pixfmt = planar_of(pixfmt)               # (a packed 4:2:2 stream is its planar stream from here on)
    step = int(time_interval)
    if step < 1:
        raise ValueError(f"time_interval must be >= 1, got {time_interval!r}")
    ops, dev = _hip_ops_of(model)
    generic = ops is None or not hasattr(ops, "pool_blocks")
    source, win = chain(first, it), None
    if active is not None:
        win, source = _active_window(active, first, it, st, model, None if generic else (ops, dev), divisor, step, pixfmt, packed=packed,
                                     scale=motion_scale)
    common = dict(n=factor, divisor=divisor, tta=tta, pixfmt=pixfmt, window=win, watch=area is not None)
    if motion_scale != 1:
        common["motion_scale"] = motion_scale
    if packed is not None:
        common["packed"] = packed
    if generic:
        be = HostBackend(model, st, max_batch=max(1, int(max_batch)), **common)
    else:
        be = DeviceBackend(model, ops, dev, st, crop=crop, max_batch=max_batch, pool=pool, scene=scene is not None, **common)
    h, w = st.window[2:]
    done, sig = 0, None                              # segments enqueued; the signature of the last one's second frame

    def ahead():
        """The source frames, those that end a segment admitted as soon as they are read (the device backend starts their upload: one
        segment ahead of the forwards) and wrapped into their entries."""
        hold = step if be.lookahead else 0           # the consumer sees frame j only after frame j + hold has been admitted
        buf = deque()
        for k, f in enumerate(source):
            if k % step == 0:
                f = {"f": f}
                be.admit(f)
            buf.append(f)
            while len(buf) > hold:
                yield buf.popleft()
        yield from buf

    def segment(a, b):
        # enqueue this segment and deliver it at once: the order generator wants its frames now
        nonlocal done, sig
        done += 1
        # (cut segments are watched too; the first segment brings two new frames, every later one its second)
        if be.watching and any([area.check(be.borders(e), st.H, st.W) for e in ((a, b) if done == 1 else (b,))]):
            area.fallback_at = done - 1
            be.whole_frame()
        cut = False
        if scene is not None:
            # on the device both signatures were enqueued with their uploads, b's one segment ago: the event has long completed
            sig_a, sig = (be.signature(a) if done == 1 else sig), be.signature(b)
            cut = scene.judge(sig_a, sig, h, w)
        made = be.segment(a, b, None, cut)           # (a cut: the frames take their places, no forward)
        return cut_fill(st.original(a["f"]), st.original(b["f"]), factor) if cut else list(made.values())
    try:
        for x in nx_sequence(ahead(), segment, factor, step):
            yield st.original(x["f"]) if type(x) is dict else x          # an original: the caller's array (its crop)
    finally:
        be.close()


def inference_nx(img0, img1, model, factor: int = 4, isBGR: bool = True, divisor: Optional[int] = 64, tta: bool = False,
                 motion_scale: int = 1) -> List[np.ndarray]:
    """Two uint8 [H,W,3] frames -> the ``factor - 1`` uint8 frames between them (t = 1/N ... (N-1)/N), by the recursion of
    davis-vid.py:102-106.  ``motion_scale``: as ``interpolate_video_nx``."""
    out = list(interpolate_video_nx([img0, img1], model, factor=factor, isBGR=isBGR, divisor=divisor, tta=tta, motion_scale=motion_scale))
    return out[1:-1]


def video_nx(cap, make_writer, model, factor: int = 4, fps_out: Optional[int] = None, interpolator=None, time_interval: int = 1,
             crop: Optional[Tuple[int, int]] = None, **kw):
    """``host_io.video_2x``'s contract for N-x: reads FPS, W, H from ``cap``, opens the sink with ``make_writer(fps_out or factor * FPS
    // time_interval, (W, H))`` -- the crop's size when cropping -- writes what ``interpolator(frames, model, factor=, time_interval=,
    crop=, **kw)`` yields (default ``interpolate_video_nx``) and releases both ends, also when a frame fails.  The script hard-codes
    10 fps (davis-vid.py:74); pass ``fps_out=10`` for that.  Returns ``{"fps_in", "fps_out", "size", "frames_in", "frames_out"}``, and
    with ``scene=SceneCuts(...)`` among ``kw`` also ``"cuts"``: the indices of the segments classed scene cuts."""
    from .host_io import CAP_PROP_FPS, CAP_PROP_FRAME_HEIGHT, CAP_PROP_FRAME_WIDTH, capture_frames
    nx_levels(factor)
    fps = int(cap.get(CAP_PROP_FPS))
    w, h = int(cap.get(CAP_PROP_FRAME_WIDTH)), int(cap.get(CAP_PROP_FRAME_HEIGHT))
    _, _, oh, ow = centre_window(h, w, crop)
    rate = int(fps_out) if fps_out else factor * fps // int(time_interval)
    out = make_writer(rate, (ow, oh))
    n_in = [0]

    def counted():
        for f in capture_frames(cap):
            if f.shape[:2] != (h, w):
                raise ValueError(f"video_nx: the capture announced {w}x{h} frames and delivered {f.shape[1]}x{f.shape[0]}")
            n_in[0] += 1
            yield f
    n_out = 0
    try:
        for frame in (interpolator or interpolate_video_nx)(counted(), model, factor=factor, time_interval=time_interval, crop=crop, **kw):
            out.write(frame)
            n_out += 1
    finally:
        cap.release()
        out.release()
    info = {"fps_in": fps, "fps_out": rate, "size": (ow, oh), "frames_in": n_in[0], "frames_out": n_out}
    if kw.get("scene") is not None:
        info["cuts"] = list(kw["scene"].cuts)
    return info
