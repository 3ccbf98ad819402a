"""The per-sample model of deep RGB frames (include/atmvfi.h atmvfi_rgb16_decode / atmvfi_rgb16_encode): plain loops over pixels and
components, written from the definition and independently of the vectorised twins in atm-vfi_amd/rgb16.py, which -- like the kernels --
are held to it bit for bit.  Frames are 1-D uint16 arrays of 3 H W samples; fp32 arithmetic is numpy's float32 scalars."""
import numpy as np

LAYOUTS = ("rgb48", "bgr48", "gbrp")
DEPTHS = (10, 12, 16)
# what the kernel tests run on: the aligned fast path, W % 4 != 0, and odd small sizes
SHAPES = [(16, 16), (18, 22), (1, 1), (3, 5), (2, 8)]


def top_of(depth: int) -> int:
    return (1 << depth) - 1


def sample_index(layout: str, H: int, W: int, y: int, x: int, c: int) -> int:
    """where component c (0 R, 1 G, 2 B) of pixel (y, x) lives in the 1-D frame"""
    if layout == "rgb48":
        return (y * W + x) * 3 + c
    if layout == "bgr48":
        return (y * W + x) * 3 + (2 - c)
    plane = {1: 0, 2: 1, 0: 2}[c]                   # G, B, R
    return plane * H * W + y * W + x


def random_frame(rng, H: int, W: int, depth: int, over: bool = False) -> np.ndarray:
    """random codes with both ends present; ``over``: some samples above the depth's top (10 and 12 bit)"""
    n = 3 * H * W
    f = rng.integers(0, top_of(depth) + 1, n, dtype=np.int64)
    f[rng.integers(0, n)] = 0
    f[rng.integers(0, n)] = top_of(depth)
    if over and depth < 16:
        k = rng.integers(0, n, max(1, n // 8))
        f[k] = rng.integers(top_of(depth) + 1, 65536, k.size)
    return f.astype(np.uint16)


def decode_loop(frame, layout, depth, H, W, window=None, canvas=None, pad_top=0, pad_left=0, want_f32=True, want_u8=True):
    """-> (fp32 [3,Hp,Wp] or None, uint8 [h,w,3] or None).  ``canvas=(Hp, Wp)`` (default: the window, no padding): the window at
    (pad_top, pad_left), every other canvas pixel the window's nearest edge pixel."""
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    Hp, Wp = (h, w) if canvas is None else canvas
    top = top_of(depth)
    topf = np.float32(top)
    f32 = np.empty((3, Hp, Wp), np.float32) if want_f32 else None
    u8 = np.empty((h, w, 3), np.uint8) if want_u8 else None
    if want_f32:
        for y in range(Hp):
            wy = min(max(y - pad_top, 0), h - 1)
            for x in range(Wp):
                wx = min(max(x - pad_left, 0), w - 1)
                for c in range(3):
                    q = min(int(frame[sample_index(layout, H, W, y0 + wy, x0 + wx, c)]), top)
                    f32[c, y, x] = np.float32(q) / topf
    if want_u8:
        for y in range(h):
            for x in range(w):
                for c in range(3):
                    q = min(int(frame[sample_index(layout, H, W, y0 + y, x0 + x, c)]), top)
                    u8[y, x, c] = q >> (depth - 8)
    return f32, u8


def encode_loop(canvas, layout, depth, H, W, pad_top=0, pad_left=0) -> np.ndarray:
    """fp32 [3,Hp,Wp] -> the 1-D frame: clip(rint(fl32(x * top)), 0, top), half to even; only the picture is read"""
    top = top_of(depth)
    topf = np.float32(top)
    out = np.empty(3 * H * W, np.uint16)
    for y in range(H):
        for x in range(W):
            for c in range(3):
                v = np.float32(canvas[c, y + pad_top, x + pad_left]) * topf           # one fp32 product
                r = float(np.rint(np.float64(v)))                                      # exact: v is an fp32 number
                out[sample_index(layout, H, W, y, x, c)] = int(min(max(r, 0.0), float(top)))
    return out


def ties(depth: int):
    """fp32 values x whose product with top is an exact .5 tie in fp32: (x, the even neighbour it rounds to).  For k + 0.5 to survive
    fl32(x * top) the product must be exact, so x is built as (k + 0.5) / top only where that quotient, rounded to fp32 and multiplied
    back in fp32, gives k + 0.5 again; the smallest such k are returned."""
    topf = np.float32(top_of(depth))
    out = []
    k = 0
    while len(out) < 8 and k < top_of(depth):
        t = np.float32(k) + np.float32(0.5)
        x = np.float32(t / topf)
        if np.float32(x * topf) == t:
            out.append((x, k if k % 2 == 0 else k + 1))
        k += 1
    return out
