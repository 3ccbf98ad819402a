"""What ``multiframe.interpolate_video_nx`` and ``retime.interpolate_video_retimed`` stand on; internal to the package, no API.

* ``open_stream``: the prologue of a loop -- frame size, centre window, what an original becomes when yielded, the output format;
* ``_Uploader``: every source frame goes to the device once, with its probes (signature, difference, borders) behind the copy;
* ``_SegmentRunner``: one segment of the recursion on the device -- pool positions, level schedule, output ring, the shutter's blend;
* ``HostBackend`` / ``DeviceBackend``: the one way either loop reaches a model.  A loop wraps every frame it admits into an entry
  ``{"f": frame}`` and speaks ``admit / first / difference / signature / borders / segment / blended / whole_frame / close``; the host
  backend is torch / numpy (any callable ``forward(im0, im1) -> {"I_t"}``), bit for bit what the device backend computes.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np


# ------------------------------------------------------------------------------------------------ the prologue
class Stream(NamedTuple):
    """What a loop knows once it has seen its first frame."""
    H: int
    W: int
    window: Tuple[int, int, int, int]                # (y0, x0, h, w): ``centre_window`` of the crop
    crop_rgb: Callable                               # uint8 [H,W,3] -> its window
    original: Callable                               # the caller's own array -> what is yielded for it
    out_fmt: object                                  # the ``yuv.Format`` of produced frames (None: uint8 RGB)
    deep: bool                                       # a 10-bit ``pixfmt`` with ``keep_depth``; a ``yuv.DeepRGB`` always
    isBGR: bool                                      # (a ``pixfmt`` overrides it: False)
    packed: object = None                            # a ``yuv.Packed`` stream: the tight layout produced frames are packed into


def planar_of(pixfmt):
    """``(packed, pixfmt)`` of a loop's ``pixfmt``: a ``yuv.Packed`` and the planar 4:2:2 format its stream IS inside the loop; any other
    ``pixfmt``, or none, as ``(None, pixfmt)``."""
    from .pixfmt import Packed
    return (pixfmt, pixfmt.planar) if isinstance(pixfmt, Packed) else (None, pixfmt)


def open_stream(first, crop, pixfmt, keep_depth, isBGR, caller: str) -> Stream:
    from .multiframe import centre_window
    H, W = first.shape[:2] if pixfmt is None else (pixfmt.height, pixfmt.width)
    y0, x0, h, w = window = centre_window(H, W, crop)
    whole = (h, w) == (H, W)
    crop_rgb = (lambda f: f) if whole else (lambda f: np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]))
    if pixfmt is None:
        return Stream(H, W, window, crop_rgb, crop_rgb, None, False, isBGR)
    from . import yuv
    err = None if crop is None else yuv._origin_error(caller, pixfmt, y0, x0, "crop")      # (a multiple of the subsampling step)
    if err is not None:
        raise err
    yuv.deep_rgb_refusals(caller, pixfmt, keep_depth)
    deep = bool(keep_depth) and pixfmt.depth > 8
    # (a padded yuv.Surface: originals lose the padding)
    original = (lambda f: f) if (whole and yuv.passes_through(pixfmt)) else (lambda f: yuv.crop(f, pixfmt, y0, x0, h, w))
    out = yuv.out_format(pixfmt, deep).cropped(h, w)
    if isinstance(pixfmt, yuv.Packed):      # produced frames: encoded as planar 4:2:2, then packed
        return Stream(H, W, window, crop_rgb, original, out.planar, deep, False, out)
    return Stream(H, W, window, crop_rgb, original, out, deep, False)


def chain(first, it):
    yield first
    yield from it


def _canvas(h: int, w: int, divisor, need: Optional[int] = None, pool: bool = False, scale: int = 1) -> Tuple[int, int, int, int]:
    """(pad_top, pad_left, Hp, Wp) of an h x w window under ``InputPadder(divisor)`` (no divisor: no padding).  ``need`` (the device
    path: 16 with global motion, else 8) and ``pool`` refuse a canvas the network cannot take.  ``scale`` (``motion_scale``): the
    network runs on the canvas reduced by it, so the canvas is that of ``divisor * scale`` and ``need`` / ``pool`` hold for its reduction."""
    from .host_io import InputPadder
    left = right = top = bottom = 0
    if divisor:
        left, right, top, bottom = InputPadder((1, 3, h, w), divisor=divisor * scale)._pad
    hp, wp = h + top + bottom, w + left + right
    if need is not None and (hp % (need * scale) or wp % (need * scale)):
        raise ValueError(f"interpolate_video_nx: {hp}x{wp} frames need a divisor (multiples of {need * scale})")
    if pool and (hp % (16 * scale) or wp % (16 * scale)):
        raise ValueError(f"interpolate_video_nx: pool=True needs frame sides that are multiples of {16 * scale} (got {hp}x{wp})")
    if need is None and scale > 1 and (hp % scale or wp % scale):
        raise ValueError(f"interpolate_video_nx: motion_scale={scale} needs even frame sides or a divisor (got {hp}x{wp})")
    return top, left, hp, wp


# ------------------------------------------------------------------------------------------------ uploads
class _Probe(NamedTuple):
    name: str
    words: int                                       # int32 words per frame
    workspace: object                                # one scratch: every probe runs on the copy stream, one after the other
    launch: Callable                                 # (previous upload's slot, this slot, out, workspace)
    pairs: bool = False                              # reads the previous upload too: nothing to do for the first


class _Uploader:
    """Every source frame goes to the device ONCE: a ring of pinned host slots + device staging filled on a copy stream, ahead of the
    kernel that converts it (as ``host_io.interpolate_video_2x_distributed`` does).

    ``pixfmt=(ops, fmt)`` (planar I420 input): pinned and device staging hold ``fmt.frame_bytes``; ``atmvfi_yuv_decode`` runs on the
    copy stream behind the copy and fills the slot's resident uint8 RGB frame ``d`` -- what the probes, ``take`` and everything
    downstream read, as for an RGB upload.  ``deep`` (a 10-bit ``pixfmt`` with ``keep_depth``): ``take`` hands the uploaded I420 bytes
    themselves to ``convert`` (``atmvfi_yuv_decode`` (``keep_depth``) decodes them into the pool slot: no 8-bit round trip); the uint8 RGB frame is
    made only for a signature (or a difference).  A ``yuv.DeepRGB`` ``pixfmt`` is always ``deep``: the slot's ``yuv`` bytes are the
    uploaded RGB frame, ``atmvfi_rgb16_decode`` decodes them into the pool slot and, for a signature or a difference, makes the 8-bit
    probe picture ``d`` on the copy stream.

    The probes.  Each is computed ONCE per frame, on the copy stream right behind the copy that brought the frame, into int32 words of
    the slot; the words follow into a pinned twin and an event is recorded.  The reader of that name waits for the event -- recorded
    when the upload was issued, one segment before the segment that asks -- and returns a copy of the words.  Within an upload they
    run in the order signature, difference, borders.

    ``signature=(ops, (y0, x0, h, w), bgr)`` (scene-cut detection): ``HipOps.frame_signature``, 288 words.

    ``difference=(ops, (y0, x0, h, w), bgr)`` (duplicate detection of ``retime.interpolate_video_retimed``): behind every upload but the
    first, ``HipOps.frame_difference`` of the PREVIOUS upload's resident uint8 frame and this one, 258 words.  Lifetimes: the previous
    upload's device frame is read on the copy stream, and the copy that next overwrites it is issued on that same stream later:
    stream order.  A frame that is never ``take``n (a dropped duplicate) records no ``free`` event, so with ``difference`` a slot's
    reuse also waits for its own ``ready`` event: its pinned bytes have left the host before they are overwritten.

    ``borders=(ops, bgr)`` (the active picture, ``active.ActiveArea``): the frame's line maxima (``HipOps.frame_borders``), H + W words;
    with a ``pixfmt`` those of the uploaded surface's luma plane (``HipOps.yuv_borders`` on the slot's ``yuv`` bytes: no RGB frame is
    needed for it).  ``stop_borders()`` ends it for the uploads still to come.

    ``packed`` (a ``yuv.Packed``, with ``pixfmt=(ops, packed.planar)``): the frames arrive in that layout.  The pinned slot and one more
    device staging buffer per slot (``pk``) hold ``packed.nbytes``; ``HipOps.yuv_unpack`` runs on the copy stream right behind the
    copy, into the slot's ``yuv`` bytes, before anything else: from there on the slot holds a planar frame as above.

    ``caller``: the loop's name, for the refusal of a frame of another size or type."""

    def __init__(self, dev, height: int, width: int, depth: int = 3, signature=None, pixfmt=None, deep: bool = False, difference=None,
                 borders=None, caller: str = "interpolate_video_nx", packed=None):
        import torch
        self.torch, self.dev, self.h, self.w, self.depth, self.caller = torch, dev, height, width, depth, caller
        self.pixfmt, self.deep, self.packed = pixfmt, bool(deep), packed
        self.probes: List[_Probe] = []
        if signature is not None:
            s_ops, s_win, s_bgr = signature
            self.probes.append(_Probe("signature", 288, s_ops.frame_signature_workspace(*s_win[2:]), lambda prev, s, out, ws:
                                      s_ops.frame_signature(s["d"], *s_win, bgr=s_bgr, out=out, workspace=ws)))
        if difference is not None:
            d_ops, d_win, d_bgr = difference
            self.probes.append(_Probe("difference", 258, d_ops.frame_difference_workspace(*d_win[2:]), lambda prev, s, out, ws:
                                      d_ops.frame_difference(prev["d"], s["d"], *d_win, bgr=d_bgr, out=out, workspace=ws), pairs=True))
        if borders is not None:
            b_ops, b_bgr = borders
            if pixfmt is None:
                self.probes.append(_Probe("borders", height + width, b_ops.frame_borders_workspace(height, width), lambda prev, s, out, ws:
                                          b_ops.frame_borders(s["d"], bgr=b_bgr, out=out, workspace=ws)))
            else:
                self.probes.append(_Probe("borders", height + width, b_ops.yuv_borders_workspace(height, width), lambda prev, s, out, ws:
                                          b_ops.yuv_borders(s["yuv"], pixfmt[1], out=out, workspace=ws)))
        self.pairs, self.prev = difference is not None, None          # prev: the slot of the previous upload
        yuv_shape = in_shape = (height, width, 3) if pixfmt is None else (pixfmt[1].frame_bytes,)
        if packed is not None:
            in_shape = (packed.nbytes,)
        need_rgb = not self.deep or signature is not None or difference is not None
        self.ring = [{"h": torch.empty(*in_shape, dtype=torch.uint8).pin_memory(),
                      "d": torch.empty(height, width, 3, dtype=torch.uint8, device=dev) if need_rgb else None,
                      "ready": torch.cuda.Event(), "free": torch.cuda.Event()} for _ in range(depth)]
        for s in self.ring:
            s["h_np"] = s["h"].numpy()
            if pixfmt is not None:
                s["yuv"] = torch.empty(*yuv_shape, dtype=torch.uint8, device=dev)
            if packed is not None:
                s["pk"] = torch.empty(*in_shape, dtype=torch.uint8, device=dev)
            for p in self.probes:                    # name -> (device words, pinned twin, its numpy view, event)
                pinned = torch.empty(p.words, dtype=torch.int32).pin_memory()
                s[p.name] = (torch.empty(p.words, dtype=torch.int32, device=dev), pinned, pinned.numpy(), torch.cuda.Event())
        self.copy_in = torch.cuda.Stream(dev)
        self.issued = 0

    def upload(self, frame):
        """Start the host -> device copy of ``frame``; returns the ring slot to hand to ``take``."""
        torch = self.torch
        if self.pixfmt is not None:
            frame = (self.packed or self.pixfmt[1]).check(frame, self.caller).view(np.uint8)
        elif frame.shape != (self.h, self.w, 3) or frame.dtype != np.uint8:
            raise ValueError(f"{self.caller}: expected uint8 [{self.h},{self.w},3] frames, got {frame.dtype} {tuple(frame.shape)}")
        slot = self.ring[self.issued % self.depth]
        if self.issued >= self.depth:
            slot["free"].synchronize()                # the kernel that read this slot's device copy has run
            if self.pairs:
                slot["ready"].synchronize()           # a frame that was never taken: its copy has left the pinned bytes
        np.copyto(slot["h_np"], frame)                # numpy's single-threaded memcpy (see host_io.FramePipeline._upload)
        with torch.cuda.stream(self.copy_in):
            if self.pixfmt is None:
                slot["d"].copy_(slot["h"], non_blocking=True)
            else:
                if self.packed is None:
                    slot["yuv"].copy_(slot["h"], non_blocking=True)
                else:
                    slot["pk"].copy_(slot["h"], non_blocking=True)
                    self.pixfmt[0].yuv_unpack(slot["pk"], self.packed, dst=slot["yuv"])
                if slot["d"] is not None:
                    self.pixfmt[0].yuv_decode(slot["yuv"], self.pixfmt[1], dst_u8=slot["d"])
            slot["ready"].record(self.copy_in)
            for p in self.probes:
                if p.pairs and self.prev is None:
                    continue
                words, pinned, _, ready = slot[p.name]
                p.launch(self.prev, slot, words, p.workspace)
                pinned.copy_(words, non_blocking=True)
                ready.record(self.copy_in)
            self.prev = slot
        self.issued += 1
        return slot

    def _read(self, name: str, slot) -> np.ndarray:
        """A probe's words of the frame in ``slot`` (a copy; the slot's words are rewritten by its next upload)."""
        _, _, words, ready = slot[name]
        ready.synchronize()
        return words.copy()

    def signature(self, slot) -> np.ndarray:
        """The int32[288] signature of the frame in ``slot``."""
        return self._read("signature", slot)

    def difference(self, slot) -> np.ndarray:
        """The int32[258] difference of the frame in ``slot`` against the upload before it (not defined for the first upload)."""
        return self._read("difference", slot)

    def borders(self, slot) -> np.ndarray:
        """The int32[H + W] line maxima of the frame in ``slot``."""
        return self._read("borders", slot)

    def stop_borders(self):
        self.probes = [p for p in self.probes if p.name != "borders"]

    def take(self, slot, convert):
        """Run ``convert(device uint8 frame, the uploaded surface's bytes or None)`` on the current stream once the slot's copy has
        landed (``deep``: the first is the surface's bytes too)."""
        cur = self.torch.cuda.current_stream(self.dev)
        cur.wait_event(slot["ready"])
        convert(slot["yuv"] if self.deep else slot["d"], slot.get("yuv"))
        slot["free"].record(cur)


# ------------------------------------------------------------------------------------------------ one segment on the device
class _SegmentRunner:
    """One segment of the N-x recursion on the device: source frames in pool positions 0 and N, level l as batches of at most
    ``max_batch`` pairs, every produced ``I_t`` (padded canvas, fp32, as returned: no un-pad / re-pad, no rounding) into the pool slot it
    belongs to and, through ``frame_f32_to_u8`` (or ``tta_merge``), into the output ring.

    Workspaces: batches of different size are different workspaces of the model, and its LRU of two would free and reallocate them
    per level at 8x (batch sizes 1, 2, 4).  The runner RAISES ``model.max_workspaces`` to the number of batch sizes of its schedule for
    its lifetime and restores it in ``close()``.  The launch plans of ``forward_pooled`` are recorded into those same workspaces (one per
    batch size, whatever the stale count), so the raise covers them too: no plan of the steady state is evicted and recorded again.

    ``run(..., levels=, emit=)`` (``retime.interpolate_video_retimed``): a sparse schedule (``retime.sparse_levels``) instead of the full
    recursion, and the positions that leave for the host -- the others are ancestors only and stay in the pool.  ``out_slots``: the size
    of the output ring (default N - 1: every position); ``batch_sizes``: the batch sizes a sparse schedule can bring (default: those of
    the full recursion).

    How a produced position leaves is chosen once, here (``self.leave``, one of the ``_leave_*`` functions of ``_LEAVE``):
    ``out_fmt`` (a yuv.Format of the window's size): as packed I420 (``yuv_encode``) instead of uint8 RGB; ``deep_fmt`` (the 10-bit
    input Format, with keep_depth): source frames are decoded from their I420 bytes straight into the pool slot (the crop as the
    kernel's window) and produced frames leave as 10-bit I420 (``out_fmt`` is 10-bit then); with ``tta`` the average -- its uint8
    pixels, or with the depth kept the fp32 canvas itself -- is made first.

    ``blend=(light, entries)`` and ``run(..., blend=ops)`` (``retime.interpolate_video_retimed(shutter=)``): a sample is accumulated
    (``shutter.Exposures``) where it would have been converted for the output ring -- from the fp32 prediction, with ``tta`` from
    ``tta_merge``'s uint8 pixels, positions 0 and N and the copies of a cut segment from the pool's resident canvases -- and an output
    that closes is resolved into an output ring entry (with an 8-bit ``out_fmt`` into a uint8 RGB buffer that ``yuv_encode`` encodes)
    and leaves by the same device -> host copy.  ``ops``: ``shutter._plan``'s, a close as ``("close", m)`` or, for an output the caller
    serves itself, ``("drop", m)``.  The output ring holds the outputs one ``run`` can close.

    ``window=(y0, x0, h, w)`` (the active picture, ``active=`` of both loops; no ``crop`` or blend with it): the network
    runs on that window -- pool, plans and batch sizes as for a crop -- and the runner keeps two resident BORDER frames, the originals
    in positions 0 and N, copied device to device where the source frame is converted and swapped with the positions: uint8 [H,W,3],
    or with ``out_fmt`` / ``deep_fmt`` the uploaded surfaces in the input layout ``border_fmt``.  A produced position k leaves through
    ``frame_compose`` (``yuv_compose``) into a FULL-SIZE output ring entry: the prediction's window inside -- with ``tta`` ``tta_merge``'s
    uint8 window, with the depth kept the fp32 average -- and the bars of the nearer original (k <= N/2: position 0) outside.

    ``pack`` (a tight ``yuv.Packed`` whose ``planar`` is ``out_fmt``; a packed 4:2:2 stream): the output ring holds frames of that
    layout.  A produced frame leaves as above into ONE planar scratch and ``HipOps.yuv_pack`` writes the ring entry from it.

    ``motion_scale=2`` (half-resolution motion, scaled.py; not with ``blend``): the canvas is that of ``divisor * 2`` and everything
    above -- pads, window, every ``_leave_*`` -- stays full-size.  Per set a second, FULL-SIZE frame store ``full`` exists beside the
    pool, whose frames and network geometry are halved: a source frame is converted into its full-size slot and ``frame_half``'d into
    the pool slot; ``_forward`` hands the forward's whole dict to ``synth_up2`` with the pairs' slot lists on the full-size store; a
    prediction that feeds a deeper level goes to both stores, the full-size prediction as returned and its ``frame_half``; ``tta``
    rotates at full size.  With ``motion_scale=1`` ``full`` IS ``frames`` and nothing else is allocated or launched."""

    def __init__(self, model, ops, dev, height, width, factor, crop, bgr, divisor, tta, max_batch, pool, out_fmt=None, deep_fmt=None,
                 out_slots=None, batch_sizes=None, blend=None, window=None, border_fmt=None, pack=None, motion_scale=1):
        import torch
        from .multiframe import FramePool, centre_window, nx_levels
        self.torch, self.model, self.ops, self.dev = torch, model, ops, dev
        self.n, self.bgr, self.tta, self.use_pool = factor, bool(bgr), bool(tta), bool(pool)
        self.levels = nx_levels(factor)
        self.max_batch = max(1, min(int(max_batch), 16))
        self.out_fmt, self.deep_fmt = out_fmt, deep_fmt
        u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
        self.y0, self.x0, self.h, self.w = centre_window(height, width, crop)
        self.border = self.border_fmt = None
        if window is not None:
            if crop is not None or blend is not None or (out_fmt is None) != (border_fmt is None):
                raise ValueError("_SegmentRunner: window goes with no crop or blend, and with a format only with the border's")
            self.y0, self.x0, self.h, self.w = (int(v) for v in window)
            self.border_fmt = border_fmt
            self.border = [u8(height, width, 3) if border_fmt is None else u8(border_fmt.frame_bytes) for _ in range(2)]
            self.border_of = {0: 0, factor: 1}       # position -> border frame; swapped with the positions
        self.scale = sc = int(motion_scale)
        if sc == 2 and blend is not None:
            raise ValueError("_SegmentRunner: motion_scale=2 does not go with a blend")
        self.pad_top, self.pad_left, self.hp, self.wp = _canvas(self.h, self.w, divisor, 16 if getattr(model, "global_motion", True) else 8,
                                                               self.use_pool, sc)
        self.nh, self.nw = self.hp // sc, self.wp // sc          # the network's geometry
        S, sets = factor + 1, 2 if self.tta else 1   # (with tta a second set: the 180-degree rotations)
        self.pools = [FramePool(model, self.nh, self.nw, S) for _ in range(sets)] if self.use_pool else None
        self.frames = ([p.frames for p in self.pools] if self.use_pool else
                       [torch.empty(S, 3, self.nh, self.nw, dtype=torch.float32, device=dev) for _ in range(sets)])
        self.full = self.frames if sc == 1 else [torch.empty(S, 3, self.hp, self.wp, dtype=torch.float32, device=dev) for _ in range(sets)]
        self.phys = list(range(S))                   # schedule position -> pool slot; positions 0 and N swap slots per segment
        self.have_first = self.fresh = False
        self.gather = {}                             # plain mode: the pairs of a batch are gathered into contiguous [B,3,Hp,Wp] inputs
        out_shape = (out_fmt.frame_bytes,) if out_fmt is not None else (height, width, 3) if self.border is not None else (self.h, self.w, 3)
        self.pack = self.planar = None
        if pack is not None:
            if out_fmt is None or pack.planar != out_fmt or not pack.is_tight:
                raise ValueError("_SegmentRunner: pack must be the tight packed layout of out_fmt")
            self.pack, self.planar, out_shape = pack, u8(out_fmt.frame_bytes), (pack.nbytes,)
        n_out = factor - 1 if out_slots is None else max(1, min(int(out_slots), factor - 1))
        self.blend = None
        if blend is not None:
            if deep_fmt is not None:
                raise ValueError("_SegmentRunner: a blend of 10-bit frames is not supported")
            from .shutter import Exposures
            n_out = max(1, int(blend[1]))
            self.blend = Exposures(ops, dev, self.h, self.w, blend[0], self.pad_top, self.pad_left)
            self.blend_u8 = u8(self.h, self.w, 3) if (out_fmt is not None or self.tta) else None
        self.out_d = u8(n_out, *out_shape)
        self.out_h = [torch.empty(n_out, *out_shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.merged = None
        if (out_fmt is not None or self.border is not None) and self.tta:       # the average: its uint8 pixels, or with the depth kept the fp32 canvas itself
            self.merged = (torch.empty(3, self.hp, self.wp, dtype=torch.float32, device=dev) if deep_fmt is not None else u8(self.h, self.w, 3))
        mode = "compose" if self.border is not None else "deep" if deep_fmt is not None else "yuv" if out_fmt is not None else "u8"
        self.leave = self._LEAVE[mode, self.tta]     # (the plain function, not a bound method: the runner must not hold itself alive)
        if self.pack is not None:
            self._leave_planar, self.leave = self.leave, _SegmentRunner._leave_packed
        self.out_evt = [torch.cuda.Event() for _ in range(2)]
        self.seg = 0
        self.copy_out = torch.cuda.Stream(dev)
        self.done = torch.cuda.Event()
        sizes = {min(self.max_batch, len(lv) - i) for lv in self.levels for i in range(0, len(lv), self.max_batch)}
        if batch_sizes is not None:
            sizes = set(batch_sizes)
        self._keep_max_ws = getattr(model, "max_workspaces", None)
        if self._keep_max_ws is not None and len(sizes) > self._keep_max_ws:
            model.max_workspaces = len(sizes)

    def close(self):
        if self._keep_max_ws is not None:
            self.model.max_workspaces = self._keep_max_ws
        if self.pools:
            for p in self.pools:
                p.release()

    # -- source frames
    def _convert_into(self, pos):
        slot = self.phys[pos]

        def convert(d_u8, surface=None):
            dst = self.full[0][slot]
            if self.deep_fmt is not None:             # d_u8: the frame's I420 bytes
                self.ops.yuv_decode(d_u8, self.deep_fmt, dst=dst, window=(self.y0, self.x0, self.h, self.w), pad_top=self.pad_top,
                                    pad_left=self.pad_left, keep_depth=True)
            elif (self.y0, self.x0, self.h, self.w) == (0, 0) + tuple(d_u8.shape[:2]):
                self.ops.frame_u8_to_f32(d_u8, dst, self.pad_top, self.pad_left, self.bgr)
            else:
                self.ops.frame_u8_window(d_u8, 0, self.y0, self.x0, self.h, self.w, dst=dst, pad_top=self.pad_top, pad_left=self.pad_left,
                                         bgr=self.bgr)
            if self.tta:
                self.ops.frame_rot180(dst, self.full[1][slot])
            if self.scale == 2:
                for k in range(len(self.full)):
                    self.ops.frame_half(self.full[k][slot], self.frames[k][slot])
            if self.pools:
                for p in self.pools:
                    p.invalidate(slot)
            if self.border is not None:              # (a format: the uploaded surface itself, never a converted frame)
                self.border[self.border_of[pos]].copy_(d_u8 if self.border_fmt is None else surface, non_blocking=True)
        return convert

    def first(self, up: _Uploader, slot):
        """Convert the stream's first frame into position 0 NOW, ahead of the first ``run`` (which then gets ``slot_a=None``): a loop
        that may read many frames before its first segment is known (dropped duplicates) must not leave frame 0 in the upload ring."""
        with self.torch.cuda.device(self.dev):
            up.take(slot, self.first_resident)

    def first_resident(self, d_u8, surface=None):
        """``first`` for a frame that is on the device already (what ``_Uploader.take`` hands over, for the current stream to read)."""
        with self.torch.cuda.device(self.dev):
            self._convert_into(0)(d_u8, surface)
        self.have_first = self.fresh = True

    def _forward(self, k, lefts, rights):
        """I_t [B,3,Hp,Wp] of the pairs (slots) on frame set ``k`` (0: the frames, 1: their 180-degree rotations)."""
        if self.use_pool:
            out = self.model.forward_pooled(self.pools[k], lefts, rights)
        else:
            b = len(lefts)
            g = self.gather.get(b)
            if g is None:
                g = self.gather[b] = self.torch.empty(2 * b, 3, self.nh, self.nw, dtype=self.torch.float32, device=self.dev)
            self.ops.pool_blocks(self.frames[k], lefts + rights, g)
            out = self.model.forward(g[:b], g[b:])
        if self.scale == 1:
            return out["I_t"]
        return self.ops.synth_up2(out, self.full[k], self.full[k], lefts, rights)["I_t"]      # the pairs' full-size frames by slot: no gather

    def _run_levels(self, levels, wanted, sink):
        """The schedule level by level in batches of at most ``max_batch`` pairs: ``sink(pos, pred, flip)`` for every produced position
        in ``wanted`` (None: all of them) -- ``pred`` the fp32 prediction [3,Hp,Wp], ``flip`` that of the rotated frames with ``tta``
        (else None) -- the others are ancestors only; what a later level reads goes back into the pool."""
        torch = self.torch
        last = max((li for li, lv in enumerate(levels) if lv), default=0)
        for li, level in enumerate(levels):
            for i in range(0, len(level), self.max_batch):
                chunk = level[i:i + self.max_batch]
                lefts = [self.phys[a] for a, _, _ in chunk]
                rights = [self.phys[b] for _, b, _ in chunk]
                outs = [self.phys[o] for _, _, o in chunk]
                pred = self._forward(0, lefts, rights)
                shown = [wanted is None or pos in wanted for _, _, pos in chunk]
                flip = self._forward(1, lefts, rights) if self.tta and any(shown) else None
                for j, (_, _, pos) in enumerate(chunk):
                    if shown[j]:                       # (else an ancestor only: it stays in the pool)
                        sink(pos, pred[j], None if flip is None else flip[j])
                if li < last:                          # the next level reads these frames (the un-averaged prediction)
                    self.ops.pool_blocks(self.full[0], outs, pred, to_pool=True)
                    if self.tta:
                        rot = self.gather.get(("rot", len(chunk)))
                        if rot is None:
                            rot = self.gather[("rot", len(chunk))] = torch.empty_like(pred)
                        self.ops.frame_rot180(pred, rot)
                        self.ops.pool_blocks(self.full[1], outs, rot, to_pool=True)
                    if self.scale == 2:                # ... and their halves, which the network reads
                        half = self.gather.get(("half", len(chunk)))
                        if half is None:
                            half = self.gather[("half", len(chunk))] = torch.empty(len(chunk), 3, self.nh, self.nw, dtype=torch.float32, device=self.dev)
                        for k, src in enumerate((pred, rot) if self.tta else (pred,)):
                            self.ops.frame_half(src, half)
                            self.ops.pool_blocks(self.frames[k], outs, half, to_pool=True)
                    if self.pools:
                        for p in self.pools:
                            for s in outs:
                                p.invalidate(s)

    # -- how a produced position leaves: (position, fp32 prediction, that of the rotated frames or None, the output ring entry)
    def _leave_u8(self, pos, pred, flip, u8):
        self.ops.frame_f32_to_u8(pred, u8, self.pad_top, self.pad_left, self.bgr)

    def _leave_u8_tta(self, pos, pred, flip, u8):
        self.ops.tta_merge(pred, flip, out_u8=u8, pad_top=self.pad_top, pad_left=self.pad_left, bgr=self.bgr)

    def _leave_yuv(self, pos, pred, flip, u8):
        self.ops.yuv_encode(u8, self.out_fmt, src=pred, pad_top=self.pad_top, pad_left=self.pad_left)

    def _leave_yuv_tta(self, pos, pred, flip, u8):   # the average's uint8 pixels, then their encoding
        self.ops.tta_merge(pred, flip, out_u8=self.merged, pad_top=self.pad_top, pad_left=self.pad_left, bgr=False)
        self.ops.yuv_encode(u8, self.out_fmt, src_u8=self.merged)

    def _leave_deep_tta(self, pos, pred, flip, u8):  # the fp32 average, then its encoding
        self.ops.tta_merge(pred, flip, out=self.merged)
        self.ops.yuv_encode(u8, self.out_fmt, src=self.merged, pad_top=self.pad_top, pad_left=self.pad_left)

    def _bars(self, pos):
        """the border frame of the nearer original, and the window"""
        return self.border[self.border_of[0 if pos <= self.n // 2 else self.n]], (self.y0, self.x0, self.h, self.w)

    def _compose(self, u8, pos, src=None, win=None):
        """the window -- the fp32 canvas ``src`` or the uint8 pixels ``win`` -- back into a full frame"""
        border, window = self._bars(pos)
        if self.out_fmt is None:
            self.ops.frame_compose(u8, border, window, src=src, win_u8=win, pad_top=self.pad_top, pad_left=self.pad_left, bgr=self.bgr)
        else:
            self.ops.yuv_compose(u8, self.out_fmt, border, self.border_fmt, window, src=src, src_u8=win, pad_top=self.pad_top,
                                 pad_left=self.pad_left)

    def _leave_compose(self, pos, pred, flip, u8):
        self._compose(u8, pos, src=pred)

    def _leave_compose_tta(self, pos, pred, flip, u8):
        if self.deep_fmt is not None:                # the fp32 average
            self.ops.tta_merge(pred, flip, out=self.merged)
            return self._compose(u8, pos, src=self.merged)
        self.ops.tta_merge(pred, flip, out_u8=self.merged, pad_top=self.pad_top, pad_left=self.pad_left, bgr=self.bgr and self.out_fmt is None)
        self._compose(u8, pos, win=self.merged)

    def _leave_packed(self, pos, pred, flip, u8):    # the planar frame as without ``pack``, then its packed form
        self._leave_planar(self, pos, pred, flip, self.planar)
        self.ops.yuv_pack(self.planar, self.pack, dst=u8)

    _LEAVE = {("u8", False): _leave_u8, ("u8", True): _leave_u8_tta, ("yuv", False): _leave_yuv, ("yuv", True): _leave_yuv_tta,
              ("deep", False): _leave_yuv, ("deep", True): _leave_deep_tta,      # (out_fmt is the 10-bit format then)
              ("compose", False): _leave_compose, ("compose", True): _leave_compose_tta}

    def _send(self, ring, count):
        """The first ``count`` output ring entries to the host, behind everything enqueued so far; ``out_d`` is rewritten by the next
        segment, so its kernels wait for this copy."""
        torch = self.torch
        cur = torch.cuda.current_stream(self.dev)
        self.done.record(cur)
        self.copy_out.wait_event(self.done)
        with torch.cuda.stream(self.copy_out):
            self.out_h[ring][:count].copy_(self.out_d[:count], non_blocking=True)
            self.out_evt[ring].record(self.copy_out)
        cur.wait_event(self.out_evt[ring])

    def run(self, up: _Uploader, slot_a, slot_b, cut: bool = False, levels=None, emit=None, blend=None):
        """Enqueue one segment: ``slot_a`` (None when the previous segment's second frame is this one's first) and ``slot_b`` are
        upload slots.  Returns a handle for ``result``.  ``cut`` (a scene cut: the caller emits copies of the originals): the source
        frames still take their places -- position N's frame, with tokens marked stale, is the next segment's position 0 whatever this
        segment was -- but no forward runs, nothing is written to the middle slots or the output ring, and None is returned.
        ``levels`` (default: the full recursion) / ``emit`` (default: every position): the schedule to run and the positions, in the
        order of ``result``, that are written to the output ring; ``emit`` holds at most ``out_slots`` positions, all in ``levels``.
        ``blend`` (default None: all of the above; else without ``emit``): the segment's samples are accumulated and the outputs that
        close here resolved, see the class comment; a handle is returned also for a cut, ``result(handle, closes)`` gives the frames."""
        n = self.n
        levels = self.levels if levels is None else levels
        index = None if emit is None else {pos: k for k, pos in enumerate(emit)}       # position -> output ring entry
        if index is not None and (len(index) > self.out_d.shape[0] or not index.keys() <= {o for lv in levels for _, _, o in lv}):
            raise ValueError(f"_SegmentRunner.run: emit {list(emit)} does not fit the schedule or the {self.out_d.shape[0]} output slots")
        with self.torch.cuda.device(self.dev):
            if self.fresh:                           # position 0 holds the stream's first frame already (``first``)
                self.fresh = False
            elif self.have_first:
                self.phys[0], self.phys[n] = self.phys[n], self.phys[0]      # frame AND tokens of slot N become slot 0's: no copy
                if self.border is not None:
                    self.border_of[0], self.border_of[n] = self.border_of[n], self.border_of[0]
            else:
                up.take(slot_a, self._convert_into(0))
                self.have_first = True
            up.take(slot_b, self._convert_into(n))
            if blend is not None:
                return self._run_blended([] if cut else levels, blend, cut)
            if cut:
                return None
            ring = self.seg & 1
            self.seg += 1
            if index is None:
                self._run_levels(levels, None, lambda pos, pred, flip: self.leave(self, pos, pred, flip, self.out_d[pos - 1]))
            else:
                self._run_levels(levels, index, lambda pos, pred, flip: self.leave(self, pos, pred, flip, self.out_d[index[pos]]))
            self._send(ring, self.out_d.shape[0] if index is None else len(index))
            return ring

    # -- synthetic shutter
    def _blend_end(self, op, k):
        """a reset, close or drop; -> the number of output ring entries in use"""
        if op[0] == "reset":
            self.blend.reset(op[1])
            return k
        closed = self.blend.close(op[1])             # (accumulator, total weight), or None for an output without samples
        if op[0] == "drop":
            return k
        if closed is None or k >= self.out_d.shape[0]:
            raise RuntimeError(f"_SegmentRunner: output {op[1]} closes without samples or beyond the {self.out_d.shape[0]} output slots")
        if self.out_fmt is None:
            self.ops.shutter_resolve(*closed, self.out_d[k], light=self.blend.light, bgr=self.bgr)
        else:                                        # the blend's uint8 pixels, then their encoding
            self.ops.shutter_resolve(*closed, self.blend_u8, light=self.blend.light)
            if self.pack is None:
                self.ops.yuv_encode(self.out_d[k], self.out_fmt, src_u8=self.blend_u8)
            else:
                self.ops.yuv_encode(self.planar, self.out_fmt, src_u8=self.blend_u8)
                self.ops.yuv_pack(self.planar, self.pack, dst=self.out_d[k])
        return k + 1

    def _run_blended(self, levels, ops, cut):
        n, acc = self.n, self.blend
        if acc is None:
            raise ValueError("_SegmentRunner.run: blend needs a runner made with blend=")
        ring = self.seg & 1
        self.seg += 1
        closes = 0
        if not any(levels):                          # every sample is a resident canvas: in time order
            for op in ops:
                if op[0] == "add":
                    pos = op[2] if not (cut and 0 < op[2] < n) else (0 if op[2] <= n // 2 else n)
                    acc.add(op[1], op[3], src=self.frames[0][self.phys[pos]])
                else:
                    closes = self._blend_end(op, closes)
        else:                                        # (resets precede the adds of a segment that is no cut)
            # position -> [(output, weight)]: where a widened segment's positions lie further apart than the outputs, two outputs show
            # one position -- one through its window and one, or both, as the position nearest to a window that holds no sample
            adds = {}
            for op in ops:
                if op[0] == "add":
                    adds.setdefault(op[2], []).append((op[1], op[3]))
            if not adds.keys() - {0, n} <= {o for lv in levels for _, _, o in lv}:
                raise ValueError(f"_SegmentRunner.run: samples {sorted(adds)} do not fit the schedule")
            for op in ops:
                if op[0] == "reset":
                    acc.reset(op[1])
            for pos in (0, n):
                for m, w in adds.get(pos, ()):
                    acc.add(m, w, src=self.frames[0][self.phys[pos]])

            def gather(pos, pred, flip):
                if self.tta:                           # the average's uint8 pixels are the sample
                    self.ops.tta_merge(pred, flip, out_u8=self.blend_u8, pad_top=self.pad_top, pad_left=self.pad_left, bgr=False)
                for m, w in adds[pos]:
                    acc.add(m, w, **({"src_u8": self.blend_u8} if self.tta else {"src": pred}))
            self._run_levels(levels, adds, gather)
            for op in ops:
                if op[0] in ("close", "drop"):
                    closes = self._blend_end(op, closes)
        if closes:
            self._send(ring, closes)
        return ring

    def tail(self, ops):
        """The end of a blended stream: the terminal sample (position N of the last ``run``) and the outputs still open."""
        with self.torch.cuda.device(self.dev):
            return self._run_blended([], ops, False)

    def result(self, ring, count: Optional[int] = None) -> List[np.ndarray]:
        """The frames of a ``run``: all N - 1, or the first ``count`` output ring entries (a run with ``emit``)."""
        self.out_evt[ring].synchronize()
        arr = self.out_h[ring].numpy()
        count = self.n - 1 if count is None else count
        if (self.deep_fmt is not None) if self.pack is None else self.pack.itemsize == 2:
            return [arr[k].copy().view(np.uint16) for k in range(count)]
        return [arr[k].copy() for k in range(count)]


def _generic_segment(model, factor, crop_of, isBGR, divisor, tta, max_batch, load=None, store=None, motion_scale=1):
    """``segment`` for a model without the HIP backend (any callable ``forward(im0, im1) -> {"I_t"}``): torch ops, same schedule, the
    canvas of ``_canvas`` as on the device.  ``load(frame) -> fp32 [h,w,3]`` / ``store(fp32 [h,w,3]) -> frame`` replace the uint8 RGB
    conversions at both ends (the 10-bit I420 twins, with ``keep_depth``).  ``motion_scale=2``: the canvas of ``divisor * 2`` and
    ``scaled.forward_scaled_host`` (the twins of ``frame_half`` and ``synth_up2`` around the model's forward) in ``forward``'s place."""
    import torch
    import torch.nn.functional as F
    from .multiframe import nx_levels
    dev = next(model.parameters()).device
    levels = nx_levels(factor)
    if motion_scale == 2:
        from .scaled import forward_scaled_host
        forward = lambda l, r: {"I_t": forward_scaled_host(model.forward, l.cpu(), r.cpu())["I_t"].to(dev)}
    else:
        forward = model.forward

    def to_t(img):
        if load is not None:
            return torch.tensor(np.ascontiguousarray(load(img).transpose(2, 0, 1))).to(dev).unsqueeze(0)
        img = crop_of(img)
        if isBGR:
            img = img[:, :, ::-1]
        return (torch.tensor(np.ascontiguousarray(img.transpose(2, 0, 1))).to(dev) / 255.).unsqueeze(0)

    def segment(fa, fb, levels=levels, emit=None):
        """``levels`` / ``emit`` (``retime.interpolate_video_retimed``): a sparse schedule and the positions to return, in order."""
        a, b = to_t(fa), to_t(fb)
        h, w = a.shape[-2:]
        top, left, hp, wp = _canvas(h, w, divisor, scale=motion_scale)
        if divisor:
            a, b = (F.pad(x, [left, wp - w - left, top, hp - h - top], mode="replicate") for x in (a, b))
        fr = {0: a, factor: b}
        shown = {}
        for level in levels:
            for i in range(0, len(level), max_batch):
                chunk = level[i:i + max_batch]
                l = torch.cat([fr[x] for x, _, _ in chunk], 0)
                r = torch.cat([fr[y] for _, y, _ in chunk], 0)
                pred = forward(l, r)["I_t"]
                out = pred
                if tta:
                    pf = forward(l.flip(2).flip(3).contiguous(), r.flip(2).flip(3).contiguous())["I_t"]
                    out = (pred + pf.flip(2).flip(3)) / 2
                for j, (_, _, pos) in enumerate(chunk):
                    fr[pos] = pred[j:j + 1]
                    shown[pos] = out[j:j + 1]
        res = []
        for pos in (range(1, factor) if emit is None else emit):
            p = shown[pos][..., top:top + h, left:left + w]
            if store is not None:
                res.append(store(np.ascontiguousarray(p[0].detach().float().cpu().numpy().transpose(1, 2, 0))))
                continue
            p = np.round(p[0].detach().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
            res.append(p[:, :, ::-1].copy() if isBGR else p)
        return res
    return segment


# ------------------------------------------------------------------------------------------------ the backends
class HostBackend:
    """A model without the HIP backend: torch / numpy (``_generic_segment``, ``retime.difference_numpy``, ``scene.signature_numpy``,
    ``active.borders_numpy`` / ``compose_numpy`` and their ``yuv_`` forms, ``shutter.blend_numpy``).  An I420 frame is decoded once
    (``_rgb``: kept in its entry, so the frame that ends a segment is not decoded again when it starts the next).  ``window`` (the
    active picture): the forwards run on that window of the frames and every produced window is composed into a full frame with the
    bars of the nearer original -- with a ``pixfmt`` the window's encode into the original's own samples -- until ``whole_frame()``;
    ``watching``: the loop examines ``borders`` of the frames it admits.  ``packed`` (a ``yuv.Packed``, ``pixfmt`` its planar format):
    an admitted frame is unpacked once (``yuv.unpack_numpy``; ``_frame``), everything above works on the planar frame, and what is
    produced is packed into ``st.packed`` (``yuv.pack_numpy``).  ``motion_scale=2``: see ``_generic_segment``."""
    lookahead = False                                # (nothing is gained by reading a segment ahead)

    def __init__(self, model, st: Stream, n, divisor, tta, max_batch, pixfmt=None, dedup=None, light=None, window=None, watch=False,
                 caller: str = "interpolate_video_nx", packed=None, motion_scale=1):
        self.n, self.levels, self.st, self.pixfmt, self.caller, self.packed = n, n.bit_length() - 1, st, pixfmt, caller, packed
        self.dedup, self.prev_rgb = dedup, None
        self.light, self.gathered = light, {}        # (the synthetic shutter: ``blended``)
        self.watching = window is not None and watch
        self._generic = lambda crop_of, **kw: _generic_segment(model, n, crop_of, st.isBGR, divisor, tta, max_batch, motion_scale=motion_scale, **kw)
        self._build(window)

    def _build(self, window):
        """``seg`` on ``window`` of the frames (None: the stream's own crop window); ``win_fmt``: the format its frames are encoded to"""
        st, self.window = self.st, window
        y0, x0, h, w = st.window if window is None else window
        self.win_fmt = st.out_fmt if window is None or st.out_fmt is None else st.out_fmt.cropped(h, w)
        if st.deep:
            from . import yuv
            self.seg = self._generic(None, load=lambda f: yuv.decode_numpy_f32(f, self.pixfmt, window=(y0, x0, h, w)),
                                     store=lambda p: yuv.encode_numpy(p, self.win_fmt))
        elif window is not None:
            self.seg = self._generic(lambda f: np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]))
        else:
            self.seg = self._generic(st.crop_rgb)

    def _frame(self, e):
        """the frame of ``pixfmt`` (a packed 4:2:2 frame: unpacked once)"""
        if self.packed is None:
            return e["f"]
        if "planar" not in e:
            from . import yuv
            e["planar"] = yuv.unpack_numpy(e["f"], self.packed)
        return e["planar"]

    def _packed_out(self, frames):
        if self.packed is None:
            return frames
        from . import yuv
        return [yuv.pack_numpy(f, self.st.packed) for f in frames]

    def _rgb(self, e):
        """the uint8 [H,W,3] picture of a frame (an I420 frame: decoded once)"""
        if self.pixfmt is None:
            return e["f"]
        if "rgb" not in e:
            from . import yuv
            e["rgb"] = yuv.decode_numpy(self._frame(e), self.pixfmt)
        return e["rgb"]

    def admit(self, e):
        if self.pixfmt is not None:
            (self.packed or self.pixfmt).check(e["f"], self.caller)
        if self.dedup is not None:
            from .retime import difference_numpy
            rgb = self._rgb(e)
            if self.prev_rgb is not None:
                e["diff"] = difference_numpy(self.prev_rgb, rgb, self.st.window, bgr=self.st.isBGR)
            self.prev_rgb = rgb

    def first(self, e):
        pass

    def difference(self, e):
        return e["diff"]

    def signature(self, e):
        from .scene import signature_numpy
        return signature_numpy(self._rgb(e), self.st.window, bgr=self.st.isBGR)

    def borders(self, e):
        from .active import borders_numpy, yuv_borders_numpy
        return borders_numpy(e["f"], bgr=self.st.isBGR) if self.pixfmt is None else yuv_borders_numpy(self._frame(e), self.pixfmt)

    def whole_frame(self):
        """The active picture has ended: the whole frame from the next ``segment`` on."""
        self.watching = False
        self._build(None)

    def segment(self, a, b, interior, cut):
        """The frames between two admitted frames as ``{position: frame}``: ``interior`` (sorted positions in 1..N-1; None: all of
        them, the full recursion) on their sparse schedule.  A ``cut`` runs nothing."""
        if cut or (interior is not None and not interior):
            return {}
        from .retime import sparse_levels
        fa, fb = (self._frame(a), self._frame(b)) if (self.pixfmt is None or self.st.deep) else (self._rgb(a), self._rgb(b))
        if interior is None:
            interior, made = range(1, self.n), self.seg(fa, fb)
        else:
            made = self.seg(fa, fb, levels=sparse_levels(interior, self.levels), emit=interior)
        if self.pixfmt is not None and not self.st.deep:
            from . import yuv
            made = [yuv.encode_numpy(m, self.win_fmt) for m in made]
        if self.window is not None:
            from .active import compose_numpy, yuv_compose_numpy
            bars = lambda k: self._frame(a if k <= self.n // 2 else b)
            if self.pixfmt is None:
                made = [compose_numpy(bars(k), self.window, win_u8=m) for k, m in zip(interior, made)]
            else:
                made = [yuv_compose_numpy(bars(k), self.pixfmt, self.window, m) for k, m in zip(interior, made)]
        return dict(zip(interior, self._packed_out(made)))

    def blended(self, a, b, ops, need, cut, tail):
        """One record of ``shutter._plan`` (closes as ``("close", m)`` / ``("drop", m)``): the frames of its closes, in order --
        ``shutter.blend_numpy`` of the uint8 RGB frames the loop would have emitted for the samples."""
        n, made, out = self.n, {}, []
        if need and not cut:
            from .retime import sparse_levels
            fa, fb = (a["f"], b["f"]) if self.pixfmt is None else (self._rgb(a), self._rgb(b))
            made = dict(zip(need, self.seg(fa, fb, levels=sparse_levels(need, self.levels), emit=need)))
        for op in ops:
            if op[0] == "add":
                p = op[2]
                if 0 < p < n and not cut:
                    frame = made[p]
                else:
                    frame = self.st.crop_rgb(self._rgb(a if (p == 0 or (p < n and p <= n // 2)) else b))
                self.gathered.setdefault(op[1], []).append((frame, op[3]))
            elif op[0] == "close":
                from .shutter import blend_numpy
                frames, weights = zip(*self.gathered.pop(op[1]))
                frame = blend_numpy(frames, weights, self.light)
                if self.pixfmt is not None:
                    from . import yuv
                    frame = self._packed_out([yuv.encode_numpy(frame, self.st.out_fmt)])[0]
                out.append(frame)
            else:                                    # a reset, or an output the loop serves itself
                self.gathered.pop(op[1], None)
        return out

    def close(self):
        pass


class DeviceBackend:
    """The HIP path: ``_Uploader`` (the probes on the copy stream behind each upload) and ``_SegmentRunner``.  Every frame that ends a
    segment is converted into the pool once, when its segment runs; a frame that ends none (a dropped duplicate) is uploaded and
    compared and never converted.

    The upload ring and its lifetimes.  The N-x loop starts the upload of a segment's second frame one segment ahead (``lookahead``):
    three slots.  The retimed loop issues frame k's upload when it is read; frame k - 1 is judged -- and, if kept, its segment
    enqueued, which ``take``s its slot -- before frame k + 1 is read.  So when upload k + 1 is issued the slots still in use are k (the
    next difference reads its device frame; its ``take`` is yet to come) and k - 1 (its ``take`` may be in flight: the ``free`` event).
    Three slots would do; with ``dedup`` the ring has four.  A held-back duplicate at the end of the stream is ``take``n after the last
    upload: nothing can overwrite it.  With dropped duplicates the stream's FIRST frame is the one frame whose segment may be many
    uploads away: the retimed loop has it converted into pool position 0 when it is admitted (``first``); else the first ``segment``
    converts both its frames.

    ``sparse`` (the retimed loop): ``out_slots`` output ring entries and the batch sizes any sparse schedule can bring.  ``window`` /
    ``watch`` (the active picture): the windowed runner and the ``borders`` probe; ``whole_frame()`` replaces the runner.  ``packed`` (a
    ``yuv.Packed``, ``pixfmt`` its planar format): the uploader unpacks behind the copy and the runner packs in front of the output
    ring (``st.packed``); everything between is the planar stream's."""
    lookahead = True

    def __init__(self, model, ops, dev, st: Stream, n, crop, divisor, tta, max_batch, pool, pixfmt=None, scene=False, dedup=False,
                 sparse=False, out_slots=None, blend=None, window=None, watch=False, caller: str = "interpolate_video_nx", packed=None,
                 motion_scale=1):
        self.n, self.levels, self.started = n, n.bit_length() - 1, False
        batch_sizes = range(1, min(max(1, min(int(max_batch), 16)), max(1, n // 2)) + 1) if sparse else None
        self._runner = lambda window: _SegmentRunner(model, ops, dev, st.H, st.W, n, crop, st.isBGR, divisor, tta, max_batch,
                                                     pool and hasattr(model, "forward_pooled"), out_fmt=st.out_fmt,
                                                     deep_fmt=pixfmt if st.deep else None, out_slots=out_slots, batch_sizes=batch_sizes,
                                                     blend=blend, window=window,
                                                     border_fmt=pixfmt if window is not None else None, pack=st.packed,
                                                     motion_scale=motion_scale)
        self.pixfmt, self.ops, self.dev, self.hw = pixfmt, ops, dev, (st.H, st.W)
        self.runner = self._runner(window)
        self.watching = window is not None and watch
        sig = (ops, st.window, bool(st.isBGR))
        self.up = _Uploader(dev, st.H, st.W, depth=4 if dedup else 3, signature=sig if scene else None,
                            pixfmt=None if pixfmt is None else (ops, pixfmt), deep=st.deep, difference=sig if dedup else None,
                            borders=(ops, bool(st.isBGR)) if self.watching else None, caller=caller, packed=packed)

    def admit(self, e):
        e["slot"] = self.up.upload(e["f"])

    def first(self, e):
        self.runner.first(self.up, e["slot"])
        self.started = True

    def difference(self, e):
        return self.up.difference(e["slot"])

    def signature(self, e):
        return self.up.signature(e["slot"])

    def borders(self, e):
        return self.up.borders(e["slot"])

    def whole_frame(self):
        """The active picture has ended: a runner on the whole frame for the rest of the stream.  The next segment's first frame is
        position N of the windowed runner's last segment (position 0 when ``first`` alone has run): its border frame is the resident
        copy the new runner converts again -- the uint8 frame, or with a ``pixfmt`` the uploaded surface, which without ``keep_depth``
        is decoded to the uint8 RGB frame first."""
        self.up.stop_borders()
        old = self.runner
        resident = old.border[old.border_of[0 if old.fresh else self.n]] if self.started else None
        old.close()
        self.runner, self.watching = self._runner(None), False
        if resident is None:
            return
        if self.pixfmt is None or self.runner.deep_fmt is not None:
            return self.runner.first_resident(resident, resident)
        import torch
        with torch.cuda.device(self.dev):
            rgb = torch.empty(*self.hw, 3, dtype=torch.uint8, device=self.dev)
            self.ops.yuv_decode(resident, self.pixfmt, dst_u8=rgb)
        self.runner.first_resident(rgb)

    def _ends(self, a, b):
        """the upload slots a ``run`` takes: the first frame's only when nothing has converted it yet"""
        sa, self.started = (None if self.started else a["slot"]), True
        return self.up, sa, b["slot"]

    def segment(self, a, b, interior, cut):
        """``HostBackend.segment`` on the device; a ``cut`` or a segment without interior runs no forward, but its frames take
        their places."""
        if cut or (interior is not None and not interior):
            self.runner.run(*self._ends(a, b), cut=True)
            return {}
        if interior is None:
            return dict(zip(range(1, self.n), self.runner.result(self.runner.run(*self._ends(a, b)))))
        from .retime import sparse_levels
        ring = self.runner.run(*self._ends(a, b), levels=sparse_levels(interior, self.levels), emit=interior)
        return dict(zip(interior, self.runner.result(ring, len(interior))))

    def blended(self, a, b, ops, need, cut, tail):
        """``HostBackend.blended`` on the device: the segment's sparse schedule is the union of its interior samples, every sample is
        accumulated where it would have been converted, and what closes is resolved into the output ring (``_SegmentRunner``)."""
        from .retime import sparse_levels
        closes = sum(op[0] == "close" for op in ops)
        if tail:
            ring = self.runner.tail(ops)
        else:
            ring = self.runner.run(*self._ends(a, b), cut=cut, levels=sparse_levels(need, self.levels), blend=ops)
        return self.runner.result(ring, closes) if closes else []

    def close(self):
        self.runner.close()
