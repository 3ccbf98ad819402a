"""4x / 8x (any power of two) interpolation by recursion, the loop of the reference's ``benchmark/davis-vid.py:88-135``:
``pred = F(I0, I1)``, then ``pred025 = F(I0, pred)`` and ``pred075 = F(pred, I1)`` -- the deeper levels fed with the UNROUNDED fp32
prediction -- with a centre crop, a frame stride (``time_interval``) and optional flip-TTA.

* ``nx_levels`` / ``nx_sequence``: the schedule and the order of the loop, pure Python (tested without a GPU);
* ``FramePool``: device-resident frames and per-frame tokens, so that what ``Network.forward`` computes per frame (encoder, cross-scale
  fusions, LayerNorm'ed tokens) is computed once per DISTINCT frame (``Network.forward_pooled``) instead of once per appearance in a
  pair: N/2 frame encodes per segment instead of 2 (N - 1);
* ``interpolate_video_nx`` / ``video_nx`` / ``inference_nx``: the runner and its adapters (re-exported from ``host_io``).

Deviations from the script, on purpose: (1) with ``tta`` EVERY produced frame is the flip-TTA average (the script averages the middle
frame only); the next level still consumes the un-averaged prediction, as the script's order of operations has it (:102-112).  (2) with
a crop the originals are written cropped (the script hands the uncropped originals to a writer opened at the crop size, :86, 120, 135).
Opt-in, not in the script at all: ``scene=SceneCuts()`` (atm-vfi_amd/scene.py) runs no forward for a segment that straddles a shot
change and emits copies of the nearer original.
"""
from __future__ import annotations

from collections import deque
from typing import Callable, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np


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


# ------------------------------------------------------------------------------------------------ runner
class _Uploader:
    """Every source frame goes to the device ONCE: a ring of pinned host slots + device staging filled on a copy stream, ahead of the
    kernel that converts it (as ``host_io.interpolate_video_2x_distributed`` does).

    ``signature=(ops, (y0, x0, h, w), bgr)`` (scene-cut detection): the frame's signature (``HipOps.frame_signature``) is computed ONCE,
    on the copy stream right behind the copy that brought the frame, and its 1 152 bytes follow it back into a pinned word array of the
    slot; ``signature(slot)`` waits for that event -- recorded when the upload was issued, one segment before the segment that asks --
    and returns the words.

    ``pixfmt=(ops, fmt)`` (planar I420 input): pinned and device staging hold ``fmt.frame_bytes``; ``atmvfi_yuv420_to_rgb`` runs on the
    copy stream behind the copy and fills the slot's resident uint8 RGB frame ``d`` -- what the signature, ``take`` and everything
    downstream read, as for an RGB upload.  ``deep`` (a 10-bit ``pixfmt`` with ``keep_depth``): ``take`` hands the uploaded I420 bytes
    themselves to ``convert`` (``atmvfi_yuv420p10_to_f32`` decodes them into the pool slot: no 8-bit round trip); the uint8 RGB frame is
    made only for a signature (or a difference).

    ``difference=(ops, (y0, x0, h, w), bgr)`` (duplicate detection of ``retime.interpolate_video_retimed``): behind every upload but the
    first, ``HipOps.frame_difference`` of the PREVIOUS upload's resident uint8 frame and this one runs on the copy stream and its 1 032
    bytes follow into a pinned word array of the slot (``difference(slot)``).  Lifetimes: the previous upload's device frame is read on
    the copy stream, and the copy that next overwrites it is issued on that same stream later: stream order.  A frame that is never
    ``take``n (a dropped duplicate) records no ``free`` event, so with ``difference`` a slot's reuse also waits for its own ``ready``
    event: its pinned bytes have left the host before they are overwritten.

    ``borders=(ops, bgr)`` (the active picture, ``active.ActiveArea``): the frame's line maxima (``HipOps.frame_borders``) are computed
    on the copy stream behind the copy, and their (H + W) * 4 bytes follow into a pinned word array of the slot, exactly as a
    signature does; ``borders(slot)`` waits for that event.  ``stop_borders()`` ends it for the uploads still to come."""

    def __init__(self, dev, height: int, width: int, depth: int = 3, signature=None, pixfmt=None, deep: bool = False, difference=None,
                 borders=None):
        import torch
        self.torch, self.dev, self.h, self.w, self.depth = torch, dev, height, width, depth
        self.sig, self.pixfmt, self.deep, self.dif, self.bor = signature, pixfmt, bool(deep), difference, borders
        in_shape = (height, width, 3) if pixfmt is None else (pixfmt[1].frame_bytes,)
        need_rgb = not self.deep or signature is not None or difference is not None
        self.ring = [{"h": torch.empty(*in_shape, dtype=torch.uint8).pin_memory(),
                      "d": torch.empty(height, width, 3, dtype=torch.uint8, device=dev) if need_rgb else None,
                      "ready": torch.cuda.Event(), "free": torch.cuda.Event()} for _ in range(depth)]
        for s in self.ring:
            s["h_np"] = s["h"].numpy()
            if pixfmt is not None:
                s["yuv"] = torch.empty(*in_shape, dtype=torch.uint8, device=dev)
            if signature is not None:
                s["sig_d"] = torch.empty(288, dtype=torch.int32, device=dev)
                s["sig_h"] = torch.empty(288, dtype=torch.int32).pin_memory()
                s["sig_h_np"], s["sig_ready"] = s["sig_h"].numpy(), torch.cuda.Event()
        if signature is not None:                     # one scratch: every signature runs on the copy stream, one after the other
            self.sig_ws = signature[0].frame_signature_workspace(*signature[1][2:])
        if difference is not None:
            for s in self.ring:
                s["dif_d"] = torch.empty(258, dtype=torch.int32, device=dev)
                s["dif_h"] = torch.empty(258, dtype=torch.int32).pin_memory()
                s["dif_h_np"], s["dif_ready"] = s["dif_h"].numpy(), torch.cuda.Event()
            self.dif_ws = difference[0].frame_difference_workspace(*difference[1][2:])
            self.prev = None                          # the slot of the previous upload
        if borders is not None:
            for s in self.ring:
                s["bor_d"] = torch.empty(height + width, dtype=torch.int32, device=dev)
                s["bor_h"] = torch.empty(height + width, dtype=torch.int32).pin_memory()
                s["bor_h_np"], s["bor_ready"] = s["bor_h"].numpy(), torch.cuda.Event()
            self.bor_ws = borders[0].frame_borders_workspace(height, width)
        self.copy_in = torch.cuda.Stream(dev)
        self.issued = 0

    def upload(self, frame):
        """Start the host -> device copy of ``frame``; returns the ring slot to hand to ``take``."""
        torch = self.torch
        if self.pixfmt is not None:
            frame = self.pixfmt[1].check(frame, "interpolate_video_nx").view(np.uint8)
        elif frame.shape != (self.h, self.w, 3) or frame.dtype != np.uint8:
            raise ValueError(f"interpolate_video_nx: expected uint8 [{self.h},{self.w},3] frames, got {frame.dtype} {tuple(frame.shape)}")
        slot = self.ring[self.issued % self.depth]
        if self.issued >= self.depth:
            slot["free"].synchronize()                # the kernel that read this slot's device copy has run
            if self.dif is not None:
                slot["ready"].synchronize()           # a frame that was never taken: its copy has left the pinned bytes
        np.copyto(slot["h_np"], frame)                # numpy's single-threaded memcpy (see host_io.FramePipeline._upload)
        with torch.cuda.stream(self.copy_in):
            if self.pixfmt is None:
                slot["d"].copy_(slot["h"], non_blocking=True)
            else:
                slot["yuv"].copy_(slot["h"], non_blocking=True)
                if slot["d"] is not None:
                    self.pixfmt[0].yuv_decode(slot["yuv"], self.pixfmt[1], dst_u8=slot["d"])
            slot["ready"].record(self.copy_in)
            if self.sig is not None:
                ops, (y0, x0, h, w), bgr = self.sig
                ops.frame_signature(slot["d"], y0, x0, h, w, bgr=bgr, out=slot["sig_d"], workspace=self.sig_ws)
                slot["sig_h"].copy_(slot["sig_d"], non_blocking=True)
                slot["sig_ready"].record(self.copy_in)
            if self.dif is not None:
                if self.prev is not None:
                    ops, (y0, x0, h, w), bgr = self.dif
                    ops.frame_difference(self.prev["d"], slot["d"], y0, x0, h, w, bgr=bgr, out=slot["dif_d"], workspace=self.dif_ws)
                    slot["dif_h"].copy_(slot["dif_d"], non_blocking=True)
                    slot["dif_ready"].record(self.copy_in)
                self.prev = slot
            if self.bor is not None:
                self.bor[0].frame_borders(slot["d"], bgr=self.bor[1], out=slot["bor_d"], workspace=self.bor_ws)
                slot["bor_h"].copy_(slot["bor_d"], non_blocking=True)
                slot["bor_ready"].record(self.copy_in)
        self.issued += 1
        return slot

    def signature(self, slot) -> np.ndarray:
        """The int32[288] signature of the frame in ``slot`` (a copy; the slot's words are rewritten by its next upload)."""
        slot["sig_ready"].synchronize()
        return slot["sig_h_np"].copy()

    def difference(self, slot) -> np.ndarray:
        """The int32[258] difference of the frame in ``slot`` against the upload before it (a copy; not defined for the first upload)."""
        slot["dif_ready"].synchronize()
        return slot["dif_h_np"].copy()

    def borders(self, slot) -> np.ndarray:
        """The int32[H + W] line maxima of the frame in ``slot`` (a copy; the slot's words are rewritten by its next upload)."""
        slot["bor_ready"].synchronize()
        return slot["bor_h_np"].copy()

    def stop_borders(self):
        self.bor = None

    def take(self, slot, convert):
        """Run ``convert(device uint8 frame)`` on the current stream once the slot's copy has landed (``deep``: the device I420 bytes)."""
        cur = self.torch.cuda.current_stream(self.dev)
        cur.wait_event(slot["ready"])
        convert(slot["yuv"] if self.deep else slot["d"])
        slot["free"].record(cur)


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

    ``blend=(light, entries)`` and ``run(..., blend=ops)`` (``retime.interpolate_video_retimed(shutter=)``): a sample is accumulated
    (``atmvfi_shutter_accumulate``) where it would have been converted for the output ring -- from the fp32 prediction, with ``tta`` from
    ``tta_merge``'s uint8 pixels, positions 0 and N and the copies of a cut segment from the pool's resident canvases -- and an output
    that closes is resolved (``atmvfi_shutter_resolve``) into an output ring entry (with an 8-bit ``out_fmt`` into a uint8 RGB buffer
    that ``rgb_to_yuv420`` encodes) and leaves by the same device -> host copy.  ``ops``: ``shutter._plan``'s, a close as
    ``("close", m)`` or, for an output the caller serves itself, ``("drop", m)``.

    ``window=(y0, x0, h, w)`` (the active picture, ``interpolate_video_nx(active=)``; no ``crop``, formats or blend with it): the network
    runs on that window -- pool, plans and batch sizes as for a crop -- and the runner keeps two resident uint8 [H,W,3] BORDER frames,
    the originals in positions 0 and N, copied where the source frame is converted and swapped with the positions.  A produced
    position k leaves through ``frame_compose`` into a FULL-SIZE output ring entry: the prediction's window (with ``tta``:
    ``tta_merge``'s uint8 window) inside, the bars of the nearer original (k <= N/2: position 0) outside."""

    def __init__(self, model, ops, dev, height, width, factor, crop, bgr, divisor, tta, max_batch, pool, out_fmt=None, deep_fmt=None,
                 out_slots=None, batch_sizes=None, blend=None, window=None):
        import torch
        from .host_io import InputPadder
        self.torch, self.model, self.ops, self.dev = torch, model, ops, dev
        self.n, self.bgr, self.tta, self.use_pool = factor, bool(bgr), bool(tta), bool(pool)
        self.levels = nx_levels(factor)
        self.max_batch = max(1, min(int(max_batch), 16))
        self.y0, self.x0, self.h, self.w = centre_window(height, width, crop)
        self.border = None
        if window is not None:
            if crop is not None or out_fmt is not None or deep_fmt is not None or blend is not None:
                raise ValueError("_SegmentRunner: window goes with no crop, format or blend")
            self.y0, self.x0, self.h, self.w = (int(v) for v in window)
            self.border = [torch.empty(height, width, 3, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.border_of = {0: 0, factor: 1}       # position -> border frame; swapped with the positions
            self.win_u8 = torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=dev) if self.tta else None
        if divisor is None:
            self.pad_left = self.pad_top = 0
            self.hp, self.wp = self.h, self.w
        else:
            pad = InputPadder((1, 3, self.h, self.w), divisor=divisor)
            self.pad_left, _, self.pad_top, _ = pad._pad
            self.hp, self.wp = self.h + pad._pad[2] + pad._pad[3], self.w + pad._pad[0] + pad._pad[1]
        need = 16 if getattr(model, "global_motion", True) else 8
        if self.hp % need or self.wp % need:
            raise ValueError(f"interpolate_video_nx: {self.hp}x{self.wp} frames need a divisor (multiples of {need})")
        if self.use_pool and (self.hp % 16 or self.wp % 16):
            raise ValueError(f"interpolate_video_nx: pool=True needs frame sides that are multiples of 16 (got {self.hp}x{self.wp})")
        S = factor + 1
        if self.use_pool:
            self.pools = [FramePool(model, self.hp, self.wp, S) for _ in range(2 if self.tta else 1)]
            self.frames = [p.frames for p in self.pools]
        else:
            self.pools = None
            self.frames = [torch.empty(S, 3, self.hp, self.wp, dtype=torch.float32, device=dev) for _ in range(2 if self.tta else 1)]
        self.phys = list(range(S))                   # schedule position -> pool slot; positions 0 and N swap slots per segment
        self.have_first = self.fresh = False
        # plain mode: the pairs of a batch are gathered into contiguous [B,3,Hp,Wp] inputs
        self.gather = {}
        # out_fmt (a yuv.Format of the window's size): the produced frames leave as packed I420 (rgb_to_yuv420) instead of uint8 RGB
        # deep_fmt (the 10-bit input Format, with keep_depth): source frames are decoded from their I420 bytes straight into the pool
        # slot (yuv420p10_to_f32, the crop as the kernel's window) and produced frames leave as 10-bit I420 (f32_to_yuv420p10; out_fmt
        # is 10-bit then)
        self.out_fmt, self.deep_fmt = out_fmt, deep_fmt
        out_shape = (self.h, self.w, 3) if out_fmt is None else (out_fmt.frame_bytes,)
        if self.border is not None:
            out_shape = (height, width, 3)
        n_out = factor - 1 if out_slots is None else max(1, min(int(out_slots), factor - 1))
        # blend = (light, entries) (``retime.interpolate_video_retimed(shutter=)``): the output ring holds the outputs one ``run`` can
        # close, and samples are gathered in int32 accumulators of the window's size.  They are allocated on demand, one per output that
        # is open at the same time -- the level-ordered schedule visits a segment's samples out of time order, so every output a segment
        # touches is open until the segment ends -- returned to a free list when their output closes, and kept until the runner goes
        self.blend = None
        if blend is not None:
            if deep_fmt is not None:
                raise ValueError("_SegmentRunner: a blend of 10-bit frames is not supported")
            n_out = max(1, int(blend[1]))
            self.blend = {"light": blend[0], "accs": [], "free": [], "of": {},
                          "u8": torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=dev) if (out_fmt is not None or self.tta) else None}
        self.out_d = torch.empty(n_out, *out_shape, dtype=torch.uint8, device=dev)
        self.out_h = [torch.empty(n_out, *out_shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.merged = None
        if out_fmt is not None and self.tta:         # the average: its uint8 pixels, or with the depth kept the fp32 canvas itself
            self.merged = (torch.empty(3, self.hp, self.wp, dtype=torch.float32, device=dev) if deep_fmt is not None else
                           torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=dev))
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

        def convert(d_u8):
            dst = self.frames[0][slot]
            if self.deep_fmt is not None:             # d_u8: the frame's I420 bytes
                self.ops.yuv_decode(d_u8, self.deep_fmt, dst=dst, window=(self.y0, self.x0, self.h, self.w), pad_top=self.pad_top,
                                    pad_left=self.pad_left, keep_depth=True)
            elif (self.y0, self.x0, self.h, self.w) == (0, 0) + tuple(d_u8.shape[:2]):
                self.ops.frame_u8_to_f32(d_u8, dst, self.pad_top, self.pad_left, self.bgr)
            else:
                self.ops.frame_u8_window(d_u8, 0, self.y0, self.x0, self.h, self.w, dst=dst, pad_top=self.pad_top, pad_left=self.pad_left,
                                         bgr=self.bgr)
            if self.tta:
                self.ops.frame_rot180(dst, self.frames[1][slot])
            if self.pools:
                for p in self.pools:
                    p.invalidate(slot)
            if self.border is not None:
                self.border[self.border_of[pos]].copy_(d_u8, non_blocking=True)
        return convert

    def first(self, up: _Uploader, slot):
        """Convert the stream's first frame into position 0 NOW, ahead of the first ``run`` (which then gets ``slot_a=None``): a loop
        that may read many frames before its first segment is known (dropped duplicates) must not leave frame 0 in the upload ring."""
        with self.torch.cuda.device(self.dev):
            up.take(slot, self._convert_into(0))
        self.have_first = self.fresh = True

    def first_resident(self, d_u8):
        """``first`` for a frame that is on the device already (a uint8 [H,W,3] tensor the current stream may read)."""
        with self.torch.cuda.device(self.dev):
            self._convert_into(0)(d_u8)
        self.have_first = self.fresh = True

    def _forward(self, k, lefts, rights):
        """I_t [B,3,Hp,Wp] of the pairs (slots) on frame set ``k`` (0: the frames, 1: their 180-degree rotations)."""
        if self.use_pool:
            return self.model.forward_pooled(self.pools[k], lefts, rights)["I_t"]
        b = len(lefts)
        g = self.gather.get(b)
        if g is None:
            g = self.gather[b] = self.torch.empty(2 * b, 3, self.hp, self.wp, dtype=self.torch.float32, device=self.dev)
        self.ops.pool_blocks(self.frames[k], lefts + rights, g)
        return self.model.forward(g[:b], g[b:])["I_t"]

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
                    self.ops.pool_blocks(self.frames[0], outs, pred, to_pool=True)
                    if self.tta:
                        rot = self.gather.get(("rot", len(chunk)))
                        if rot is None:
                            rot = self.gather[("rot", len(chunk))] = torch.empty_like(pred)
                        self.ops.frame_rot180(pred, rot)
                        self.ops.pool_blocks(self.frames[1], outs, rot, to_pool=True)
                    if self.pools:
                        for p in self.pools:
                            for s in outs:
                                p.invalidate(s)

    def run(self, up: _Uploader, slot_a, slot_b, cut: bool = False, levels=None, emit=None, blend=None):
        """Enqueue one segment: ``slot_a`` (None when the previous segment's second frame is this one's first) and ``slot_b`` are
        upload slots.  Returns a handle for ``result``.  ``cut`` (a scene cut: the caller emits copies of the originals): the source
        frames still take their places -- position N's frame, with tokens marked stale, is the next segment's position 0 whatever this
        segment was -- but no forward runs, nothing is written to the middle slots or the output ring, and None is returned.
        ``levels`` (default: the full recursion) / ``emit`` (default: every position): the schedule to run and the positions, in the
        order of ``result``, that are written to the output ring; ``emit`` holds at most ``out_slots`` positions, all in ``levels``.
        ``blend`` (default None: all of the above; else without ``emit``): the segment's samples are accumulated and the outputs that
        close here resolved, see the class comment; a handle is returned also for a cut, ``result(handle, closes)`` gives the frames."""
        torch, n = self.torch, self.n
        levels = self.levels if levels is None else levels
        index = None if emit is None else {pos: k for k, pos in enumerate(emit)}       # position -> output ring entry
        if index is not None and (len(index) > self.out_d.shape[0] or not index.keys() <= {o for lv in levels for _, _, o in lv}):
            raise ValueError(f"_SegmentRunner.run: emit {list(emit)} does not fit the schedule or the {self.out_d.shape[0]} output slots")
        with torch.cuda.device(self.dev):
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

            def to_ring(pos, pred, flip):
                u8 = self.out_d[pos - 1 if index is None else index[pos]]
                if self.border is not None:            # the window back into a full frame, the bars of the nearer original
                    bars, win = self.border[self.border_of[0 if pos <= n // 2 else n]], (self.y0, self.x0, self.h, self.w)
                    if self.tta:
                        self.ops.tta_merge(pred, flip, out_u8=self.win_u8, pad_top=self.pad_top, pad_left=self.pad_left, bgr=self.bgr)
                        self.ops.frame_compose(u8, bars, win, win_u8=self.win_u8)
                    else:
                        self.ops.frame_compose(u8, bars, win, src=pred, pad_top=self.pad_top, pad_left=self.pad_left, bgr=self.bgr)
                elif self.deep_fmt is not None:
                    src = pred
                    if self.tta:                       # the fp32 average, then its encoding
                        self.ops.tta_merge(pred, flip, out=self.merged)
                        src = self.merged
                    self.ops.yuv_encode(u8, self.out_fmt, src=src, pad_top=self.pad_top, pad_left=self.pad_left)
                elif self.out_fmt is not None:
                    if self.tta:                       # the average's uint8 pixels, then their encoding
                        self.ops.tta_merge(pred, flip, out_u8=self.merged, pad_top=self.pad_top, pad_left=self.pad_left, bgr=False)
                        self.ops.yuv_encode(u8, self.out_fmt, src_u8=self.merged)
                    else:
                        self.ops.yuv_encode(u8, self.out_fmt, src=pred, pad_top=self.pad_top, pad_left=self.pad_left)
                elif self.tta:
                    self.ops.tta_merge(pred, flip, out_u8=u8, pad_top=self.pad_top, pad_left=self.pad_left, bgr=self.bgr)
                else:
                    self.ops.frame_f32_to_u8(pred, u8, self.pad_top, self.pad_left, self.bgr)
            self._run_levels(levels, index, to_ring)
            cur = torch.cuda.current_stream(self.dev)
            self.done.record(cur)
            self.copy_out.wait_event(self.done)
            with torch.cuda.stream(self.copy_out):
                if index is None:
                    self.out_h[ring].copy_(self.out_d, non_blocking=True)
                else:
                    self.out_h[ring][:len(index)].copy_(self.out_d[:len(index)], non_blocking=True)
                self.out_evt[ring].record(self.copy_out)
            # out_d is rewritten by the next segment: its kernels wait for this copy
            cur.wait_event(self.out_evt[ring])
            return ring

    # -- synthetic shutter
    def _accumulate(self, m, w, src=None, src_u8=None):
        st = self.blend
        a = st["of"].get(m)
        if a is None:
            if not st["free"]:
                st["accs"].append(self.torch.empty(3, self.h, self.w, dtype=self.torch.int32, device=self.dev))
                st["free"].append(len(st["accs"]) - 1)
            a = st["of"][m] = [st["free"].pop(), 0, 0]               # accumulator, samples and weight since the last reset
        pad = (self.pad_top, self.pad_left) if src is not None else (0, 0)
        self.ops.shutter_accumulate(st["accs"][a[0]], src=src, src_u8=src_u8, weight=w, light=st["light"], first=a[1] == 0,
                                    pad_top=pad[0], pad_left=pad[1])
        a[1] += 1
        a[2] += w

    def _blend_end(self, op, k):
        """a reset, close or drop; -> the number of output ring entries in use"""
        st = self.blend
        if op[0] == "reset":
            if op[1] in st["of"]:
                st["of"][op[1]][1:] = [0, 0]
            return k
        a = st["of"].pop(op[1], None)
        if a is not None:
            st["free"].append(a[0])
        if op[0] == "drop":
            return k
        if a is None or a[1] == 0 or k >= self.out_d.shape[0]:
            raise RuntimeError(f"_SegmentRunner: output {op[1]} closes without samples or beyond the {self.out_d.shape[0]} output slots")
        if self.out_fmt is None:
            self.ops.shutter_resolve(st["accs"][a[0]], a[2], self.out_d[k], light=st["light"], bgr=self.bgr)
        else:                                                          # the blend's uint8 pixels, then their encoding
            self.ops.shutter_resolve(st["accs"][a[0]], a[2], st["u8"], light=st["light"])
            self.ops.yuv_encode(self.out_d[k], self.out_fmt, src_u8=st["u8"])
        return k + 1

    def _run_blended(self, levels, ops, cut):
        torch, n, st = self.torch, self.n, self.blend
        if st is None:
            raise ValueError("_SegmentRunner.run: blend needs a runner made with blend=")
        ring = self.seg & 1
        self.seg += 1
        closes = 0
        if not any(levels):                          # every sample is a resident canvas: in time order
            for op in ops:
                if op[0] == "add":
                    pos = op[2] if not (cut and 0 < op[2] < n) else (0 if op[2] <= n // 2 else n)
                    self._accumulate(op[1], op[3], src=self.frames[0][self.phys[pos]])
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
                    self._blend_end(op, 0)
            for pos in (0, n):
                for m, w in adds.get(pos, ()):
                    self._accumulate(m, w, src=self.frames[0][self.phys[pos]])

            def gather(pos, pred, flip):
                if self.tta:                           # the average's uint8 pixels are the sample
                    self.ops.tta_merge(pred, flip, out_u8=st["u8"], pad_top=self.pad_top, pad_left=self.pad_left, bgr=False)
                for m, w in adds[pos]:
                    self._accumulate(m, w, **({"src_u8": st["u8"]} if self.tta else {"src": pred}))
            self._run_levels(levels, adds, gather)
            for op in ops:
                if op[0] in ("close", "drop"):
                    closes = self._blend_end(op, closes)
        if closes:
            cur = torch.cuda.current_stream(self.dev)
            self.done.record(cur)
            self.copy_out.wait_event(self.done)
            with torch.cuda.stream(self.copy_out):
                self.out_h[ring][:closes].copy_(self.out_d[:closes], non_blocking=True)
                self.out_evt[ring].record(self.copy_out)
            cur.wait_event(self.out_evt[ring])       # out_d is rewritten by the next segment: its kernels wait for this copy
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
        if self.deep_fmt is not None:
            return [arr[k].copy().view(np.uint16) for k in range(count)]
        return [arr[k].copy() for k in range(count)]


def _generic_segment(model, factor, crop_of, isBGR, divisor, tta, max_batch, load=None, store=None):
    """``segment`` for a model without the HIP backend (any callable ``forward(im0, im1) -> {"I_t"}``): torch ops, same schedule.
    ``load(frame) -> fp32 [h,w,3]`` / ``store(fp32 [h,w,3]) -> frame`` replace the uint8 RGB conversions at both ends (the 10-bit
    I420 twins, with ``keep_depth``)."""
    import torch
    from .host_io import InputPadder
    dev = next(model.parameters()).device
    levels = nx_levels(factor)

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
        padder = InputPadder(a.shape, divisor=divisor) if divisor else None
        if padder:
            a, b = padder.pad(a, b)
        fr = {0: a, factor: b}
        shown = {}
        for level in levels:
            for i in range(0, len(level), max_batch):
                chunk = level[i:i + max_batch]
                l = torch.cat([fr[x] for x, _, _ in chunk], 0)
                r = torch.cat([fr[y] for _, y, _ in chunk], 0)
                pred = model.forward(l, r)["I_t"]
                out = pred
                if tta:
                    pf = model.forward(l.flip(2).flip(3).contiguous(), r.flip(2).flip(3).contiguous())["I_t"]
                    out = (pred + pf.flip(2).flip(3)) / 2
                for j, (_, _, pos) in enumerate(chunk):
                    fr[pos] = pred[j:j + 1]
                    shown[pos] = out[j:j + 1]
        res = []
        for pos in (range(1, factor) if emit is None else emit):
            p = shown[pos]
            if padder:
                p = padder.unpad(p)
            if store is not None:
                res.append(store(np.ascontiguousarray(p[0].detach().float().cpu().numpy().transpose(1, 2, 0))))
                continue
            p = np.round(p[0].detach().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
            res.append(p[:, :, ::-1].copy() if isBGR else p)
        return res
    return segment


def interpolate_video_nx(frames, model, factor: int = 4, time_interval: int = 1, crop: Optional[Tuple[int, int]] = None, isBGR: bool = True,
                         divisor: Optional[int] = 64, tta: bool = False, max_batch: int = 4, pool: bool = True, scene=None, pixfmt=None,
                         keep_depth: bool = False, active=None):
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
    frame is decoded by ``atmvfi_yuv420p10_to_f32`` straight from its I420 bytes into the pool slot (the crop as the kernel's window;
    the network sees q / 1023, no 8-bit round trip), produced frames are ``atmvfi_f32_to_yuv420p10`` of the fp32 prediction (with
    ``tta``: of the fp32 average) and leave as 1-D uint16 arrays of ``pixfmt.cropped(h, w)``; deeper levels consume the unrounded
    prediction as always.  The resident uint8 RGB frame is made only when ``scene`` needs its signature: signatures, and so cut
    decisions, are those of the 8-bit path.  A model without the HIP backend does the same with the numpy twins.

    ``active`` (an ``active.ActiveArea`` or a fixed even window ``(y0, x0, h, w)``; default None: the loop as above; not with ``crop``
    or ``pixfmt``: ``ValueError``): the network runs on the active picture of letterboxed video.  Before its first output the loop
    reads frames from ``frames`` until the policy has seen enough (``probe`` decided frames, ``patience`` frames, the stream's end),
    keeps them on the host, locks the union of their rects as the window and replays them.  A window that gains nothing under
    ``divisor`` is the whole frame: the loop as above.  Else every uploaded frame gets its line maxima on the copy stream
    (``HipOps.frame_borders``), the network runs at the window's padded size, and a produced position k is the prediction's window
    composed (``HipOps.frame_compose``) into a full-size frame with the bars of the nearer original (k <= N/2: the first).  Originals
    pass through as the caller's own arrays; ``scene`` works on the whole frame as before.  A frame with a non-bar line outside the
    window ends it: from the segment that ends at that frame on, the loop runs on the whole frame for the rest of the stream.  With
    ``time_interval`` > 1 the frames that are not uploaded are not examined.  A tuple is never probed nor checked.
    ``active.window`` / ``.probed`` / ``.fallback_at`` / ``.stats`` hold the run's record."""
    from .host_io import _hip_ops_of
    from .scene import cut_fill, signature_numpy
    nx_levels(factor)
    if active is not None and (crop is not None or pixfmt is not None):
        raise ValueError("interpolate_video_nx: active does not go with " + ("crop" if crop is not None else "pixfmt") +
                         " (the active picture is found on whole uint8 frames)")
    if scene is not None:
        scene.begin()
    area = active if hasattr(active, "probe_stream") else None
    if area is not None:
        area.begin()
    it = iter(frames)
    first = next(it, None)
    if first is None:
        return
    H, W = first.shape[:2] if pixfmt is None else (pixfmt.height, pixfmt.width)
    y0, x0, h, w = centre_window(H, W, crop)
    crop_of = (lambda f: f) if crop is None else (lambda f: np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]))
    out_fmt = None
    if pixfmt is not None:
        from . import yuv
        err = None if crop is None else yuv._origin_error("interpolate_video_nx", pixfmt, y0, x0, "crop")      # (a multiple of the subsampling step)
        if err is not None:
            raise err
        deep = bool(keep_depth) and pixfmt.depth == 10
        isBGR, out_fmt = False, yuv.out_format(pixfmt, deep).cropped(h, w)
        crop_rgb, whole = crop_of, (h, w) == (H, W) and yuv.passes_through(pixfmt)     # (a padded yuv.Surface: originals lose the padding)
        crop_of = (lambda f: f) if whole else (lambda f: yuv.crop(f, pixfmt, y0, x0, h, w))          # of the caller's I420 frames
    ops, dev = _hip_ops_of(model)
    generic = ops is None or not hasattr(ops, "pool_blocks")
    win = None                                       # the active window, when the loop runs on one
    if active is not None:
        from . import active as _active
        if generic:
            profile_of = lambda f: _active.borders_numpy(f, bgr=isBGR)
        else:
            def profile_of(f):
                import torch
                with torch.cuda.device(dev):
                    return ops.frame_borders(torch.from_numpy(np.ascontiguousarray(f)).to(dev), bgr=bool(isBGR)).cpu().numpy()
        if area is None:
            win = _active.fixed_window(active, H, W)
        else:
            if int(time_interval) < 1:
                raise ValueError(f"time_interval must be >= 1, got {time_interval!r}")
            need = 16 if getattr(model, "global_motion", True) else 8
            held = area.probe_stream(_chain(first, it), H, W, divisor, need, int(time_interval), profile_of)
            it = _chain_all(held[1:], it)            # the probed frames are replayed: the loop uploads them again
            win = area.window
        if win == (0, 0, H, W):                      # nothing gained: the plain path
            win = area = None
    if generic:
        watch = None
        if win is not None:
            seg, watch = _active_generic_segment(model, factor, win, isBGR, divisor, tta, max(1, int(max_batch)), area, profile_of, (H, W))
        elif pixfmt is not None and deep:
            seg = _generic_segment(model, factor, None, False, divisor, tta, max(1, int(max_batch)),
                                   load=lambda f: yuv.decode_numpy_f32(f, pixfmt, window=(y0, x0, h, w)),
                                   store=lambda p: yuv.encode_numpy(p, out_fmt))
        else:
            seg = _generic_segment(model, factor, crop_of if pixfmt is None else crop_rgb, isBGR, divisor, tta, max(1, int(max_batch)))
        if pixfmt is not None and not deep:
            rgb_segment, decoded = seg, {"of": None, "rgb": None}

            def rgb_of(f):
                """the decoded frame, kept for the frame that is the next segment's first"""
                if decoded["of"] is not f:
                    decoded.update(of=f, rgb=yuv.decode_numpy(f, pixfmt))
                return decoded["rgb"]

            def seg(a, b):
                ra = rgb_of(a)
                return [yuv.encode_numpy(m, out_fmt) for m in rgb_segment(ra, rgb_of(b))]
        if scene is not None:
            forward_segment, known = seg, {"of": None, "sig": None}
            sig_of = signature_numpy if pixfmt is None else (lambda f, win, bgr: signature_numpy(yuv.decode_numpy(f, pixfmt), win, bgr=False))

            def seg(a, b):
                sig_a = known["sig"] if known["of"] is a else sig_of(a, (y0, x0, h, w), bgr=isBGR)
                sig_b = sig_of(b, (y0, x0, h, w), bgr=isBGR)
                known.update(of=b, sig=sig_b)                # b is the next segment's first frame
                if scene.judge(sig_a, sig_b, h, w):
                    return cut_fill(crop_of(a), crop_of(b), factor)
                return forward_segment(a, b)
        each = (lambda a, b: seg(a, b)) if watch is None else (lambda a, b: (watch(a, b), seg(a, b))[1])      # (cut segments are watched too)
        for f in nx_sequence(_chain(first, it), each, factor, time_interval):
            if pixfmt is not None:
                yield crop_of(f) if (not whole and f.size == pixfmt.frame_samples) else f       # originals are cropped here
            else:
                yield f if f.shape[:2] == (h, w) else crop_of(f)
        return
    make_runner = lambda window: _SegmentRunner(model, ops, dev, H, W, factor, crop, isBGR, divisor, tta, max_batch,
                                                pool and hasattr(model, "forward_pooled"), out_fmt=out_fmt,
                                                deep_fmt=pixfmt if (pixfmt is not None and deep) else None, window=window)
    runner = make_runner(win)
    up = _Uploader(dev, H, W, signature=None if scene is None else (ops, (y0, x0, h, w), bool(isBGR)),
                   pixfmt=None if pixfmt is None else (ops, pixfmt), deep=pixfmt is not None and deep,
                   borders=None if (win is None or area is None) else (ops, bool(isBGR)))
    state = {"first": True, "sig": None, "seg": 0, "watch": win is not None and area is not None}

    def segment(fa, fb):
        # enqueue this segment; deliver it at once (the order generator wants its frames now).  The upload of fb was started when it was
        # read from the source, one segment ahead, by `ahead()` below.
        nonlocal runner
        sa = uploads.popleft() if state["first"] else None
        state["first"] = False
        sb = uploads.popleft()
        state["seg"] += 1
        if state["watch"]:
            # the line maxima were enqueued with the uploads, as the signatures are
            bad = [area.check(up.borders(s), H, W) for s in (sa, sb) if s is not None]
            if any(bad):
                # back to the whole frame for the rest of the stream.  This segment's first frame is position N of the windowed
                # runner's last segment: its border frame is the resident uint8 copy the new runner converts again
                area.fallback_at, state["watch"] = state["seg"] - 1, False
                up.stop_borders()
                resident = None if sa is not None else runner.border[runner.border_of[factor]]
                runner.close()
                runner = make_runner(None)
                if resident is not None:
                    runner.first_resident(resident)
        if scene is not None:
            # both signatures were enqueued with their uploads, fb's one segment ago: in steady state the event has long completed
            if sa is not None:
                state["sig"] = up.signature(sa)
            sig_a, state["sig"] = state["sig"], up.signature(sb)
            if scene.judge(sig_a, state["sig"], h, w):
                runner.run(up, sa, sb, cut=True)
                return cut_fill(crop_of(fa), crop_of(fb), factor)
        return runner.result(runner.run(up, sa, sb))

    uploads = deque()

    def ahead():
        """The source frames with the uploads of segment ends started as soon as they are read: one segment ahead of the forwards."""
        s = int(time_interval)
        if s < 1:
            raise ValueError(f"time_interval must be >= 1, got {time_interval!r}")
        buf = deque()
        k = 0
        for f in _chain(first, it):
            if k % s == 0:
                uploads.append(up.upload(f))
            k += 1
            buf.append(f)
            # hold back one segment: the generator consuming this sees frame j only after frame j + s has begun to upload
            while len(buf) > s:
                yield buf.popleft()
        while buf:
            yield buf.popleft()
    try:
        for f in nx_sequence(ahead(), segment, factor, time_interval):
            if pixfmt is not None:      # an original (the caller's array, the input format's size) is cropped; a produced frame is not
                yield crop_of(f) if (not whole and f.size == pixfmt.frame_samples) else f
            else:
                yield crop_of(f) if (crop is not None and f.shape[:2] == (H, W) and (H, W) != (h, w)) else f
    finally:
        runner.close()


def _chain(first, it):
    yield first
    for f in it:
        yield f


def _chain_all(held, it):
    for f in held:
        yield f
    for f in it:
        yield f


def _active_generic_segment(model, factor, window, isBGR, divisor, tta, max_batch, area, profile_of, size):
    """``(segment, watch)`` of the active picture for a model without the HIP backend: the forwards on ``window`` of the frames, every
    produced window composed into a full frame with the bars of the nearer original (``active.compose_numpy``); ``watch(a, b)``
    (``area`` given: called once per segment, cut or not) examines the frames the device path uploads and, at a violation, switches
    ``segment`` to the whole frame for good.  ``area=None`` (a fixed window): ``watch`` is None."""
    from .active import compose_numpy
    y0, x0, h, w = window
    inner = _generic_segment(model, factor, lambda f: np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]), isBGR, divisor, tta, max_batch)
    whole = _generic_segment(model, factor, lambda f: f, isBGR, divisor, tta, max_batch)
    st = {"on": True, "seg": 0}

    def segment(a, b):
        if not st["on"]:
            return whole(a, b)
        return [compose_numpy(a if k <= factor // 2 else b, window, win_u8=m) for k, m in enumerate(inner(a, b), 1)]

    def watch(a, b):
        st["seg"] += 1
        if st["on"] and any([area.check(profile_of(f), *size) for f in ((a, b) if st["seg"] == 1 else (b,))]):
            area.fallback_at, st["on"] = st["seg"] - 1, False
    return segment, (None if area is None else watch)


def inference_nx(img0, img1, model, factor: int = 4, isBGR: bool = True, divisor: Optional[int] = 64, tta: bool = False) -> List[np.ndarray]:
    """Two uint8 [H,W,3] frames -> the ``factor - 1`` uint8 frames between them (t = 1/N ... (N-1)/N), by the recursion of
    davis-vid.py:102-106."""
    out = list(interpolate_video_nx([img0, img1], model, factor=factor, isBGR=isBGR, divisor=divisor, tta=tta))
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
