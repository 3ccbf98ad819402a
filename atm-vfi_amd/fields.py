"""Interlaced input: motion-compensated deinterlacing to field rate (50i -> 50p).  Nothing of the reference: an addition of this
project, opt-in like ``scene=``, ``active=``, ``shutter=`` and ``motion_scale=``.

Definitions (all exact; ``bob_numpy`` / ``rows_numpy`` / ``weave_numpy`` here, ``atmvfi_field_bob`` / ``atmvfi_field_rows`` of
csrc/fields.hip and the per-pixel models of tests/cpu_fields.py agree bit for bit).

Fields.  A woven frame j of H >= 2 rows holds two fields: with ``order="tff"`` field 2j is the even rows (0, 2, ...) and field 2j + 1
the odd rows; ``"bff"`` the other way round.  ``field_parity(k, order) = (k + (0 if tff else 1)) & 1`` is the row parity of field k's
real rows; field k belongs to frame ``k // 2``; n frames give 2n fields and 2n output frames, output k at time ``k / (2 fps)``.

Bob, ``F = bob(S, p)``: a picture of the woven frame's size with field p's lines kept and the others filled from that field alone.
Per plane, rows y in [0, h): ``F[y] = S[y]`` if ``y & 1 == p``; else ``S[1]`` if ``y == 0``; else ``S[h - 2]`` if ``y == h - 1``; else
``0.5f * (S[y - 1] + S[y + 1])`` (the fp32 sum rounded once; the halving is exact).  The canvas form is what the network reads:
``D[c][Y][X] = F[c][clamp(Y - pad_top, 0, h - 1)][clamp(X - pad_left, 0, w - 1)]`` -- replicate padding of the BOBBED picture, not of
the woven one.

Rows, ``rows(dst, src, p)``: per plane, rows ``y = p (mod 2)`` of ``src`` replace those of ``dst``.  Bytes are moved.

Weave (output k).  The loop's ordinary way out for a produced frame -- ``frame_f32_to_u8``, or ``yuv_encode`` of the stream's format --
is applied to a prediction canvas P; then ``rows`` brings field k's own lines back from the source frame's STORED samples.  An RGB
uint8 frame is one plane of ``3 W`` bytes per row, a planar 4:2:2 / 4:4:4 frame three planes of H rows each (their encodes make a row
from that row alone, so the other rows are what the encode of P wrote); a ``Packed`` stream weaves at the planar level, between the
encode and ``yuv_pack``.

Modes.  ``mode="bob"``: ``P = bob(C_j, parity(k))``, ``C_j`` the canvas of frame ``j = k // 2``; no forward runs.  ``mode="mc"``:
fields 0 and 2n - 1 as bob; every other k uses ``P = forward(B_{k-1}, B_{k+1})["I_t"]`` with ``B_i = bob(C_{i // 2}, parity(i))`` in
canvas form -- fields k - 1 and k + 1 have the parity opposite to field k, so their real lines are exactly the lines field k is
missing, and the network's middle frame of the two is a motion-compensated estimate of them at the right instant.  The unrounded
padded fp32 prediction is used as returned.  ``scene=SceneCuts()``: signatures of the woven frames; a cut between frames j and j + 1
makes fields 2j + 1 and 2j + 2 bob, no forward runs for them, and ``scene.cuts`` holds j.

Quality is NOT verified here: there is no checkpoint, no interlaced footage and no dataset; the tests establish that the mode computes
this definition.
"""
from __future__ import annotations

from collections import deque
from typing import Optional

import numpy as np

from .pixfmt import DeepRGB, Packed, as_surface

ORDERS, MODES = ("tff", "bff"), ("mc", "bob")


def field_parity(k: int, order: str = "tff") -> int:
    """The row parity of field ``k``'s real rows."""
    if order not in ORDERS:
        raise ValueError(f"field_parity: unknown field order {order!r} (tff, bff)")
    return (int(k) + (0 if order == "tff" else 1)) & 1


def bob_numpy(S, parity: int, canvas=None) -> np.ndarray:
    """``bob(S, parity)`` of fp32 pictures ``S`` [..., h, w] (h >= 2), in float32 with the module's expression: the picture form
    [..., h, w]; with ``canvas=(pad_top, pad_left, Hp, Wp)`` the canvas form [..., Hp, Wp], the replicate padding of the bobbed
    picture.  The bits of ``atmvfi_field_bob``."""
    S = np.asarray(S)
    if S.dtype != np.float32 or S.ndim < 2 or S.shape[-2] < 2:
        raise ValueError(f"bob_numpy: float32 pictures [..., h >= 2, w] expected, got {S.dtype} {tuple(S.shape)}")
    if parity not in (0, 1):
        raise ValueError(f"bob_numpy: parity must be 0 or 1 (got {parity!r})")
    h, w = S.shape[-2:]
    F = S.copy()
    y = np.arange(1 - parity, h, 2)                  # the rows of the other field
    inner = y[(y > 0) & (y < h - 1)]
    F[..., inner, :] = np.float32(0.5) * (S[..., inner - 1, :] + S[..., inner + 1, :])
    if parity == 1:
        F[..., 0, :] = S[..., 1, :]
    if (h - 1) & 1 != parity:
        F[..., h - 1, :] = S[..., h - 2, :]
    if canvas is None:
        return F
    top, left, hp, wp = (int(v) for v in canvas)
    if top < 0 or left < 0 or top + h > hp or left + w > wp:
        raise ValueError(f"bob_numpy: a {h} x {w} picture at ({top}, {left}) does not fit a {hp} x {wp} canvas")
    ys, xs = np.clip(np.arange(hp) - top, 0, h - 1), np.clip(np.arange(wp) - left, 0, w - 1)
    return np.ascontiguousarray(F[..., ys[:, None], xs[None, :]])


def rows_numpy(dst, src, parity: int):
    """``rows(dst, src, parity)`` of one plane (arrays [rows, ...] of one shape and type), in place; returns ``dst``."""
    if parity not in (0, 1):
        raise ValueError(f"rows_numpy: parity must be 0 or 1 (got {parity!r})")
    if dst.shape != src.shape or dst.dtype != src.dtype:
        raise ValueError(f"rows_numpy: planes of one shape and type expected, got {dst.dtype} {tuple(dst.shape)} and {src.dtype} {tuple(src.shape)}")
    dst[parity::2] = src[parity::2]
    return dst


def check_stream(who: str, pixfmt, keep_depth: bool, order: str = "tff", mode: str = "mc", height: Optional[int] = None):
    """Every refusal of ``deinterlace_video`` that the arguments alone decide (``ValueError`` with the reason)."""
    if order not in ORDERS:
        raise ValueError(f"{who}: unknown field order {order!r} (tff, bff)")
    if mode not in MODES:
        raise ValueError(f"{who}: unknown mode {mode!r} (mc, bob)")
    if isinstance(pixfmt, DeepRGB):
        raise ValueError(f"{who}: a DeepRGB pixfmt is not deinterlaced here (uint8 RGB, planar 4:2:2 / 4:4:4 and packed 4:2:2 are)")
    if pixfmt is not None:
        if pixfmt.subsampling == "420":
            raise ValueError(f"{who}: interlaced 4:2:0 is not supported in any layout (its chroma rows are shared between the two fields and "
                             "its decode filters vertically; 4:2:2 and 4:4:4 are taken)")
        if pixfmt.depth > 8 and not keep_depth:
            raise ValueError(f"{who}: a 10-bit pixfmt needs the depth kept: pass keep_depth=True (the real lines of an output are copies "
                             "of the source's samples, which an 8-bit output cannot hold)")
        height = pixfmt.height
    if height is not None and height < 2:
        raise ValueError(f"{who}: a frame of {height} row(s) has no two fields (H must be at least 2)")


def _out_format(pixfmt):
    from .yuv import out_format
    return None if pixfmt is None else out_format(pixfmt, pixfmt.depth > 8)


def _planes_of(frame, fmt):
    """The planes of a frame as 2-D views of its stored samples: one [H, 3 W] plane of a uint8 RGB frame, three of a planar one."""
    if fmt is None:
        return [frame.reshape(frame.shape[0], -1)]
    return list(fmt.planes(frame))


def weave_numpy(frame, pixfmt, parity: int, produced) -> np.ndarray:
    """Output k of the loop from ``produced`` -- the loop's ordinary way out applied to the prediction canvas, a frame of the output
    format -- and the source ``frame`` (of ``pixfmt``; None: uint8 [H,W,3]): a copy of ``produced`` in which the rows of ``parity`` are
    the source's stored samples, plane by plane.  A ``Packed`` frame is woven as the planar frame it unpacks to and packed again."""
    if isinstance(pixfmt, Packed):
        from .yuv import pack_numpy, unpack_numpy
        out = _out_format(pixfmt)
        return pack_numpy(weave_numpy(unpack_numpy(frame, pixfmt), pixfmt.planar, parity, unpack_numpy(produced, out)), out)
    out_fmt = _out_format(pixfmt)
    out = np.array(produced, copy=True)
    if pixfmt is None and (out.shape != np.shape(frame) or out.dtype != np.asarray(frame).dtype):
        raise ValueError(f"weave_numpy: the produced frame {out.dtype} {tuple(out.shape)} is not of the source's kind")
    for d, s in zip(_planes_of(out, out_fmt), _planes_of(np.asarray(frame), pixfmt)):
        rows_numpy(d, s, parity)
    return out


def plane_geometry(dst_fmt, src_fmt, height: Optional[int] = None, width: Optional[int] = None):
    """``HipOps.field_rows``' geometry between a frame of ``src_fmt`` and one of ``dst_fmt`` (planar ``Format`` / ``Surface`` of one size,
    depth and subsampling; both None: uint8 RGB frames [height, width, 3])."""
    if src_fmt is None:
        return [(0, 0, 3 * width, 3 * width, 3 * width, height)]
    d, s = as_surface(dst_fmt), as_surface(src_fmt)
    b, H, W = s.itemsize, s.height, s.width
    ch, cw = s.chroma_shape
    return [(0, 0, d.pitch, s.pitch, W * b, H),
            (d.chroma_offset, s.chroma_offset, d.chroma_pitch, s.chroma_pitch, cw * b, ch),
            (d.chroma_offset + d.chroma_pitch * ch, s.chroma_offset + s.chroma_pitch * ch, d.chroma_pitch, s.chroma_pitch, cw * b, ch)]


# ------------------------------------------------------------------------------------------------ the two backends
class _HostFields:
    """A model without the HIP backend (any callable ``forward(im0, im1) -> {"I_t"}``, as ``segments.HostBackend``): the numpy twins."""

    def __init__(self, model, st, pixfmt, packed, divisor, order, scene):
        import torch
        from .segments import _canvas
        self.torch, self.model, self.st, self.pixfmt, self.packed, self.order = torch, model, st, pixfmt, packed, order
        self.dev = next(model.parameters()).device
        top, left, hp, wp = _canvas(st.H, st.W, divisor)
        self.canvas, self.fields, self.pending = (top, left, hp, wp), {}, deque()

    def admit(self, frame):
        e = {"f": frame}
        if self.pixfmt is not None:
            (self.packed or self.pixfmt).check(frame, "deinterlace_video")
        elif frame.shape != (self.st.H, self.st.W, 3) or frame.dtype != np.uint8:
            raise ValueError(f"deinterlace_video: expected uint8 [{self.st.H},{self.st.W},3] frames, got {frame.dtype} {tuple(frame.shape)}")
        return e

    def _planar(self, e):
        if self.packed is None:
            return e["f"]
        if "planar" not in e:
            from .yuv import unpack_numpy
            e["planar"] = unpack_numpy(e["f"], self.packed)
        return e["planar"]

    def _rgb(self, e):
        if self.pixfmt is None:
            return e["f"]
        if "rgb" not in e:
            from .yuv import decode_numpy
            e["rgb"] = decode_numpy(self._planar(e), self.pixfmt)
        return e["rgb"]

    def signature(self, e):
        from .scene import signature_numpy
        return signature_numpy(self._rgb(e), (0, 0, self.st.H, self.st.W), bgr=self.st.isBGR)

    def prepare(self, e, j):
        """the woven picture of frame j as the network's fp32 [3,h,w], and its two field canvases"""
        torch = self.torch
        if self.st.deep:
            from .yuv import decode_numpy_f32
            pic = np.ascontiguousarray(decode_numpy_f32(self._planar(e), self.pixfmt).transpose(2, 0, 1))
        else:
            img = self._rgb(e)
            if self.st.isBGR:
                img = img[:, :, ::-1]
            pic = (torch.tensor(np.ascontiguousarray(img.transpose(2, 0, 1))) / 255.).numpy()
        for k in (2 * j, 2 * j + 1):
            self.fields[k % 4] = bob_numpy(pic, field_parity(k, self.order), self.canvas)

    def _store(self, P):
        """the loop's ordinary way out of a canvas: a frame of the output format (a packed stream: its planar frame)"""
        top, left, _, _ = self.canvas
        p = np.ascontiguousarray(P[:, top:top + self.st.H, left:left + self.st.W].transpose(1, 2, 0))
        if self.st.deep:
            from .yuv import encode_numpy
            return encode_numpy(p, self.st.out_fmt)
        u8 = np.clip(np.rint(p * np.float32(255)), 0, 255).astype(np.uint8)
        if self.pixfmt is None:
            return np.ascontiguousarray(u8[:, :, ::-1]) if self.st.isBGR else u8
        from .yuv import encode_numpy
        return encode_numpy(u8, self.st.out_fmt)

    def emit(self, k, e, bob):
        torch = self.torch
        if bob:
            P = self.fields[k % 4]
        else:
            a, b = (torch.from_numpy(self.fields[i % 4]).unsqueeze(0).to(self.dev) for i in (k - 1, k + 1))
            with torch.no_grad():
                P = self.model.forward(a, b)["I_t"][0].detach().float().cpu().numpy()
        out = weave_numpy(self._planar(e), self.pixfmt, field_parity(k, self.order), self._store(P))
        if self.packed is not None:
            from .yuv import pack_numpy
            out = pack_numpy(out, self.st.packed)
        self.pending.append(out)

    def release(self, e):
        pass

    def pop(self):
        return self.pending.popleft()

    def close(self):
        pass


class _DeviceFields:
    """The HIP path.  ``_Uploader`` brings every woven frame to the device once (with its signature probe for ``scene``); the existing
    convert writes ONE scratch canvas, ``field_bob`` splits it into two slots of a four-slot ``FramePool`` (field i lives in slot
    ``i % 4``: fields k - 1, k, k + 1 are resident when output k is made), and ``forward_pooled`` runs on (k - 1, k + 1) -- every bobbed
    field serves two pairs, so the steady state is one frame encode per output and one replayed plan pair.  ``pool=False``: the pair is
    gathered and ``forward`` called.  The way out: the existing encode into one of two output ring entries, ``field_rows`` from the upload
    slot's resident source bytes (a packed stream: its unpacked planar bytes, into the planar scratch, then ``yuv_pack``), the device ->
    host copy on a side stream.  An upload slot's ``free`` event is recorded again once both fields of its frame have left: the ring does
    not overwrite source bytes that ``field_rows`` is still to read."""

    def __init__(self, model, ops, dev, st, pixfmt, packed, divisor, order, scene, pool):
        import torch
        from .multiframe import FramePool
        from .segments import _Uploader, _canvas
        self.torch, self.model, self.ops, self.dev, self.st, self.pixfmt, self.order = torch, model, ops, dev, st, pixfmt, order
        self.use_pool = bool(pool) and hasattr(model, "forward_pooled")
        self.top, self.left, hp, wp = _canvas(st.H, st.W, divisor, 16 if getattr(model, "global_motion", True) else 8, self.use_pool)
        with torch.cuda.device(dev):
            u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
            self.scratch = torch.empty(3, hp, wp, dtype=torch.float32, device=dev)
            self.pool = FramePool(model, hp, wp, 4) if self.use_pool else None
            self.frames = self.pool.frames if self.use_pool else torch.empty(4, 3, hp, wp, dtype=torch.float32, device=dev)
            self.gather = None if self.use_pool else torch.empty(2, 3, hp, wp, dtype=torch.float32, device=dev)
            out_shape = (st.H, st.W, 3) if pixfmt is None else (st.out_fmt.frame_bytes,)
            self.pack, self.planar = st.packed, None
            if self.pack is not None:
                self.planar, out_shape = u8(st.out_fmt.frame_bytes), (self.pack.nbytes,)
            self.out_d = u8(2, *out_shape)
            self.out_h = [torch.empty(*out_shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.out_evt = [torch.cuda.Event() for _ in range(2)]
            self.done, self.copy_out = torch.cuda.Event(), torch.cuda.Stream(dev)
            self.up = _Uploader(dev, st.H, st.W, depth=4, signature=(ops, (0, 0, st.H, st.W), bool(st.isBGR)) if scene else None,
                                pixfmt=None if pixfmt is None else (ops, pixfmt), deep=st.deep, caller="deinterlace_video", packed=packed)
        self.geometry = plane_geometry(st.out_fmt, pixfmt, st.H, st.W)
        self.u16 = (st.deep if self.pack is None else self.pack.itemsize == 2)
        self.sent, self.pending = 0, deque()

    def admit(self, frame):
        return {"f": frame, "slot": self.up.upload(frame)}

    def signature(self, e):
        return self.up.signature(e["slot"])

    def prepare(self, e, j):
        ops, even = self.ops, 2 * j + field_parity(2 * j, self.order)      # the field of frame j with the even rows

        def convert(d, surface=None):
            if self.st.deep:                         # d: the frame's planar bytes
                ops.yuv_decode(d, self.pixfmt, dst=self.scratch, pad_top=self.top, pad_left=self.left, keep_depth=True)
            else:
                ops.frame_u8_to_f32(d, self.scratch, self.top, self.left, self.st.isBGR)
            ops.field_bob(self.scratch, self.frames[even % 4], self.frames[(even ^ 1) % 4], self.top, self.left, self.st.H, self.st.W)
        with self.torch.cuda.device(self.dev):
            self.up.take(e["slot"], convert)
        if self.pool is not None:
            for k in (2 * j, 2 * j + 1):
                self.pool.invalidate(k % 4)

    def _forward(self, left, right):
        if self.use_pool:
            return self.model.forward_pooled(self.pool, [left], [right])["I_t"]
        self.ops.pool_blocks(self.frames, [left, right], self.gather)
        return self.model.forward(self.gather[:1], self.gather[1:])["I_t"]

    def emit(self, k, e, bob):
        torch, ops, ring = self.torch, self.ops, self.sent & 1
        self.sent += 1
        slot = e["slot"]
        with torch.cuda.device(self.dev):
            cur = torch.cuda.current_stream(self.dev)
            P = self.frames[k % 4] if bob else self._forward((k - 1) % 4, (k + 1) % 4)[0]
            dst = self.out_d[ring] if self.pack is None else self.planar
            if self.pixfmt is None:
                ops.frame_f32_to_u8(P, dst, self.top, self.left, self.st.isBGR)
                ops.field_rows(dst.view(-1), slot["d"].view(-1), self.geometry, field_parity(k, self.order))
            else:
                ops.yuv_encode(dst, self.st.out_fmt, src=P, pad_top=self.top, pad_left=self.left)
                ops.field_rows(dst, slot["yuv"], self.geometry, field_parity(k, self.order))
                if self.pack is not None:
                    ops.yuv_pack(self.planar, self.pack, dst=self.out_d[ring])
            self.done.record(cur)
            self.copy_out.wait_event(self.done)
            with torch.cuda.stream(self.copy_out):
                self.out_h[ring].copy_(self.out_d[ring], non_blocking=True)
                self.out_evt[ring].record(self.copy_out)
            cur.wait_event(self.out_evt[ring])       # the entry is rewritten two outputs on
        self.pending.append(ring)

    def release(self, e):
        """both fields of the frame have left: its upload slot may be overwritten once what is enqueued has run"""
        e["slot"]["free"].record(self.torch.cuda.current_stream(self.dev))

    def pop(self):
        ring = self.pending.popleft()
        self.out_evt[ring].synchronize()
        arr = self.out_h[ring].numpy().copy()
        return arr.view(np.uint16) if self.u16 else arr

    def close(self):
        if self.pool is not None:
            self.pool.release()


# ------------------------------------------------------------------------------------------------ the loop
def deinterlace_video(frames, model, order: str = "tff", mode: str = "mc", isBGR: bool = True, divisor: int = 64, pixfmt=None,
                      keep_depth: bool = False, scene=None, pool: bool = True):
    """Woven interlaced frames -> progressive frames at field rate: a generator of 2n frames in the input's own format (uint8
    [H,W,3]; with a ``pixfmt`` arrays of ``yuv.out_format(pixfmt, keep_depth)``: a ``Surface`` or ``Packed`` at its default pitch).  Output
    k holds field k's own lines as the source's stored samples and, on the lines between, the module's prediction: the network's
    middle frame of the bobbed fields k - 1 and k + 1 (``mode="mc"``; one forward per output; fields 0 and 2n - 1 and the fields either
    side of a ``scene`` cut are bob) or the field's own line average (``mode="bob"``; no forward).  ``order``: "tff" or "bff".

    Accepted: uint8 RGB / BGR; 8-bit planar 4:2:2 and 4:4:4 ``Format``s and planar ``Surface``s of those at any pitch; ``Packed`` uyvy /
    yuy2; the 10-bit forms of all of these (y210, v210 included) with ``keep_depth=True``.  Refused (``ValueError``): 4:2:0 in any layout,
    10-bit without ``keep_depth``, ``DeepRGB``, H < 2, an unknown ``order`` or ``mode``.

    With the HIP backend everything runs on the device (``_DeviceFields``); ``pool=False`` gathers each pair and calls ``forward`` (the
    same frames).  A model without it gets the same frames through the numpy twins.  Outputs are delivered one behind the enqueue, so
    the device always has the next output's work queued."""
    from .host_io import _hip_ops_of
    from .segments import open_stream, planar_of
    check_stream("deinterlace_video", pixfmt, keep_depth, order, mode)
    if scene is not None:
        scene.begin()
    it = iter(frames)
    first = next(it, None)
    if first is None:
        return
    if pixfmt is None:
        first = np.asarray(first)
        if first.ndim != 3 or first.shape[2] != 3 or first.dtype != np.uint8:
            raise ValueError(f"deinterlace_video: uint8 [H,W,3] frames expected, got {first.dtype} {tuple(first.shape)}")
        check_stream("deinterlace_video", None, keep_depth, order, mode, height=first.shape[0])
    st = open_stream(first, None, pixfmt, keep_depth, isBGR, "deinterlace_video")
    packed, planar = planar_of(pixfmt)               # (a packed 4:2:2 stream is its planar stream from here on)
    ops, dev = _hip_ops_of(model)
    if ops is None or not hasattr(ops, "field_bob"):
        be = _HostFields(model, st, planar, packed, divisor, order, scene)
    else:
        be = _DeviceFields(model, ops, dev, st, planar, packed, divisor, order, scene, pool)
    try:
        cur, nxt = be.admit(first), next(it, None)
        be.prepare(cur, 0)
        nxt = None if nxt is None else be.admit(nxt)
        j, cut_before, sig_next = 0, False, None
        while cur is not None:
            be.emit(2 * j, cur, mode == "bob" or j == 0 or cut_before)
            if len(be.pending) > 1:
                yield be.pop()
            cut_after = False
            if nxt is not None:
                be.prepare(nxt, j + 1)               # overwrites fields 2j - 2 and 2j - 1: output 2j was their last reader
                if scene is not None:
                    sig = be.signature(cur) if j == 0 else sig_next
                    sig_next = be.signature(nxt)
                    cut_after = scene.judge(sig, sig_next, st.H, st.W)
                ahead = next(it, None)               # its upload runs under this frame's second output
                ahead = None if ahead is None else be.admit(ahead)
            else:
                ahead = None
            be.emit(2 * j + 1, cur, mode == "bob" or nxt is None or cut_after)
            be.release(cur)
            yield be.pop()
            cur, nxt, cut_before, j = nxt, ahead, cut_after, j + 1
        while be.pending:
            yield be.pop()
    finally:
        be.close()
