"""Per-sample loop models of the active picture on YUV frames (include/atmvfi.h atmvfi_yuv_borders / atmvfi_yuv_compose;
atm-vfi_amd/active.py), the yardsticks of their tests: written sample by sample from the definitions over the frame's BYTES, not the way
``active.yuv_borders_numpy`` / ``yuv_compose_numpy`` (plane views, whole-array reductions, slices) or the kernels (per-lane column
maxima, wave butterflies, rectangles of bytes, the encode kernel at an origin) compute them.  The window's samples are those of the
per-pixel encode models (cpu_yuv_surface.encode for 4:2:0 layouts, cpu_yuv_sub.encode for 4:2:2 / 4:4:4)."""
from __future__ import annotations

import numpy as np

import cpu_yuv_sub
import cpu_yuv_surface

STEPS = {"420": (2, 2), "422": (1, 2), "444": (1, 1)}        # luma rows, columns per chroma sample


def layout(H, W, depth=8, sub="420", chroma="planar", msb=False, pitch=None, chroma_pitch=None, chroma_offset=None):
    """-> dict: the definition's defaults filled in, everything in bytes; planes Y, U, V (planar) or Y and one plane of pairs"""
    assert sub == "420" or (chroma == "planar" and not msb)
    sy, sx = STEPS[sub]
    b, ch, cw = (2 if depth == 10 else 1), (H + sy - 1) // sy, (W + sx - 1) // sx
    crow = (cw if chroma == "planar" else 2 * cw) * b
    pitch = W * b if pitch is None else pitch
    chroma_pitch = crow if chroma_pitch is None else chroma_pitch
    chroma_offset = pitch * H if chroma_offset is None else chroma_offset
    last = chroma_offset + chroma_pitch * ((2 * ch if chroma == "planar" else ch) - 1)
    return dict(H=H, W=W, depth=depth, b=b, sub=sub, ch=ch, cw=cw, chroma=chroma, msb=bool(msb), pitch=pitch, chroma_pitch=chroma_pitch,
                chroma_offset=chroma_offset, nbytes=last + crow)


def tight(L, h=None, w=None):
    return layout(L["H"] if h is None else h, L["W"] if w is None else w, L["depth"], L["sub"], L["chroma"], L["msb"])


def offset(L, plane, r, c):
    """the byte offset of sample (r, c) of plane "y" / "u" / "v" """
    if plane == "y":
        return L["pitch"] * r + L["b"] * c
    if L["chroma"] == "planar":
        return L["chroma_offset"] + L["chroma_pitch"] * (r + (L["ch"] if plane == "v" else 0)) + L["b"] * c
    second = (plane == "v") == (L["chroma"] == "uv")
    return L["chroma_offset"] + L["chroma_pitch"] * r + L["b"] * (2 * c + (1 if second else 0))


def raw_bytes(buf, L):
    raw = np.ascontiguousarray(np.asarray(buf)).view(np.uint8).reshape(-1)
    assert raw.size == L["nbytes"], (raw.size, L["nbytes"])
    return raw


def stored(raw, L, plane, r, c):
    """the stored sample (msb: still shifted) from the frame's bytes, little-endian at depth 10"""
    o = offset(L, plane, r, c)
    return int(raw[o]) if L["b"] == 1 else int(raw[o]) | (int(raw[o + 1]) << 8)


def random_frame(L, seed=0, poison=None, top=None):
    """A seeded uniform-random frame of ``L`` as the 1-D sample array (uint8 / uint16), every sample in 0..``top`` (default: its whole
    range); msb: the low six bits random too.  Padding bytes: ``poison`` (a byte value) or random."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, L["nbytes"]).astype(np.uint8) if poison is None else np.full(L["nbytes"], poison, np.uint8)
    top = (1023 if L["b"] == 2 else 255) if top is None else top
    for plane, rows, cols in (("y", L["H"], L["W"]), ("u", L["ch"], L["cw"]), ("v", L["ch"], L["cw"])):
        vals = rng.integers(0, top + 1, (rows, cols))
        junk = rng.integers(0, 64, (rows, cols))
        for r in range(rows):
            for c in range(cols):
                o, v = offset(L, plane, r, c), int(vals[r, c])
                if L["msb"]:
                    v = (v << 6) | int(junk[r, c])
                raw[o] = v & 255
                if L["b"] == 2:
                    raw[o + 1] = v >> 8
    return raw.view("<u2").astype(np.uint16) if L["b"] == 2 else raw


def set_luma(buf, L, y, x, v):
    """store the luma VALUE ``v`` at (y, x) of the 1-D sample array ``buf`` (in place)"""
    assert offset(L, "y", y, x) % L["b"] == 0
    buf[offset(L, "y", y, x) // L["b"]] = (v << 6) if L["msb"] else v


# ------------------------------------------------------------------------------------------------ borders
def borders_model(buf, L) -> np.ndarray:
    """int32[H + W], sample by sample over the luma plane's bytes: the largest sample value per row, then per column."""
    raw, H, W = raw_bytes(buf, L), L["H"], L["W"]
    assert H >= 16 and W >= 16
    out = [0] * (H + W)
    for y in range(H):
        for x in range(W):
            v = stored(raw, L, "y", y, x)
            if L["msb"]:
                v >>= 6
            if v > out[y]:
                out[y] = v
            if v > out[H + x]:
                out[H + x] = v
    return np.array(out, np.int32)


def borders_model_lines(buf, L) -> np.ndarray:
    """The same, line by line (frames too large for the sample loop): a row's samples gathered from its own bytes."""
    raw, H, W, b = raw_bytes(buf, L), L["H"], L["W"], L["b"]
    rows, cols = np.zeros(H, np.int64), np.zeros(W, np.int64)
    for y in range(H):
        line = raw[L["pitch"] * y:L["pitch"] * y + W * b]
        v = line.astype(np.int64) if b == 1 else line[0::2].astype(np.int64) | (line[1::2].astype(np.int64) << 8)
        if L["msb"]:
            v = v >> 6
        rows[y] = v.max()
        cols = np.maximum(cols, v)
    return np.concatenate([rows, cols]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ compose
def window_ok(L, window) -> bool:
    """origin on multiples of the subsampling step, end on a multiple or at the frame's edge"""
    (sy, sx), (y0, x0, h, w) = STEPS[L["sub"]], window
    return (y0 >= 0 and x0 >= 0 and h >= 1 and w >= 1 and y0 + h <= L["H"] and x0 + w <= L["W"] and y0 % sy == 0 and x0 % sx == 0 and
            ((y0 + h) % sy == 0 or y0 + h == L["H"]) and ((x0 + w) % sx == 0 or x0 + w == L["W"]))


def encode_window(px, L, h, w, matrix="bt601", full_range=0, siting="centre"):
    """int [h,w,3] pixels -> the bytes of the tight h x w frame of ``L``'s kind, by the per-pixel encode models"""
    if L["sub"] == "420":
        return cpu_yuv_surface.encode(px, cpu_yuv_surface.layout(h, w, L["depth"], L["chroma"], L["msb"]), matrix, full_range, siting)
    return cpu_yuv_sub.encode(px, cpu_yuv_sub.layout(h, w, L["depth"], L["sub"]), matrix, full_range, siting)


def compose_model(border, LB, window, win_bytes) -> np.ndarray:
    """The TIGHT frame of ``LB``'s kind as bytes, sample by sample: the window's sample from ``win_bytes`` (the tight h x w frame,
    ``encode_window``), every other one the sample of ``border`` (a frame of ``LB``) as it is stored -- of an msb word the value's ten bits, the low six
    zero, as ``yuv.repack`` writes it.  Every byte once."""
    assert window_ok(LB, window)
    y0, x0, h, w = window
    (sy, sx), LT, LW = STEPS[LB["sub"]], tight(LB), tight(LB, h, w)
    src, win = raw_bytes(border, LB), raw_bytes(win_bytes, LW)
    out, written = np.zeros(LT["nbytes"], np.uint8), np.zeros(LT["nbytes"], np.int32)
    cy0, cx0 = y0 // sy, x0 // sx
    for plane, rows, cols, oy, ox, wh, ww in (("y", LB["H"], LB["W"], y0, x0, h, w), ("u", LB["ch"], LB["cw"], cy0, cx0, LW["ch"], LW["cw"]),
                                              ("v", LB["ch"], LB["cw"], cy0, cx0, LW["ch"], LW["cw"])):
        for r in range(rows):
            for c in range(cols):
                inside = oy <= r < oy + wh and ox <= c < ox + ww
                o = offset(LT, plane, r, c)
                s = offset(LW, plane, r - oy, c - ox) if inside else offset(LB, plane, r, c)
                for k in range(LB["b"]):
                    out[o + k] = (win if inside else src)[s + k]
                    written[o + k] += 1
                if LB["msb"]:                          # the sample's VALUE moves: the six low bits of an msb word are not part of it
                    out[o] &= 0xc0
    assert (written == 1).all()
    return out


# ------------------------------------------------------------------------------------------------ the loops' identities
def letterboxed_yuv(yuv, fmt, frames):
    """uint8 [H,W,3] frames -> frames of ``fmt`` (a ``yuv.Format`` or ``Surface``): ``yuv.encode_numpy`` (10 bit: of f / 255 in fp32),
    moved into the surface's layout; padding bytes are 0xAB."""
    t = yuv.as_surface(fmt).tight() if isinstance(fmt, yuv.Surface) else fmt
    out = []
    for f in frames:
        e = yuv.encode_numpy(f.astype(np.float32) / np.float32(255) if fmt.depth == 10 else f, t)
        if isinstance(fmt, yuv.Surface) and not fmt.is_tight:
            buf = np.full(fmt.frame_bytes, 0xAB, np.uint8).view(fmt.dtype)
            for d, s in zip(fmt.planes(buf), t.planes(e)):
                d[...] = s
            e = buf
        out.append(e)
    return out


def check_composed(yuv, fmt, out_fmt, window, g, cropped, near):
    """a produced frame ``g`` of ``out_fmt``: inside the window the crop run's frame, outside the nearer original's samples"""
    y0, x0, h, w = window
    assert g.dtype == out_fmt.dtype and g.size == out_fmt.frame_samples
    assert np.array_equal(yuv.crop(g, out_fmt, y0, x0, h, w), cropped)
    (sy, sx), tight = out_fmt.steps, yuv.repack(near, fmt, out_fmt)
    for k, (a, b) in enumerate(zip(out_fmt.planes(g), out_fmt.planes(tight))):
        mask = np.ones(a.shape, bool)
        if k == 0:
            mask[y0:y0 + h, x0:x0 + w] = False
        else:
            mask[y0 // sy:-(-(y0 + h) // sy), x0 // sx:-(-(x0 + w) // sx)] = False
        assert mask.any() and np.array_equal(a[mask], b[mask]), k


def check_nx(yuv, fmt, out_fmt, window, got, video, cropped, factor, segments=None):
    """``got``: the loop's frames with ``active=``; ``cropped``: the same loop's with ``crop=`` of the (centred) window"""
    n_seg = len(video) - 1 if segments is None else segments
    through = yuv.passes_through(fmt)
    for s in range(n_seg):
        for k in range(factor):
            g = got[s * factor + k]
            if k == 0:
                assert (g is video[s]) if through else np.array_equal(g, yuv.repack(video[s], fmt, out_fmt)), (s, k)
            else:
                check_composed(yuv, fmt, out_fmt, window, g, cropped[s * factor + k], video[s] if k <= factor // 2 else video[s + 1])


def check_retimed(yuv, fmt, out_fmt, window, got, video, cropped, slots, n, kept=None, upto=None):
    """the same for the retimed loop: ``slots`` = ``retime.retime_slots`` of the run, ``kept`` the kept frames' indices"""
    kept = list(range(len(video))) if kept is None else kept
    through = yuv.passes_through(fmt)
    assert len(got) == len(cropped) == len(slots)
    for i, (j, p) in enumerate(slots[:upto]):
        a, b = video[kept[j]], video[kept[min(j + 1, len(kept) - 1)]]
        if p in (0, n):
            o = a if p == 0 else b
            assert (got[i] is o) if through else np.array_equal(got[i], yuv.repack(o, fmt, out_fmt)), (i, j, p)
        else:
            check_composed(yuv, fmt, out_fmt, window, got[i], cropped[i], a if p <= n // 2 else b)
