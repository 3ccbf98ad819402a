"""Loop-style numpy models of the active-picture kernels (include/atmvfi.h atmvfi_frame_borders / atmvfi_frame_compose;
atm-vfi_amd/active.py), the yardsticks of their tests: written line by line and pixel by pixel from the definitions, not the way
``active.borders_numpy`` / ``compose_numpy`` (whole-array reductions, slices) or the kernels (per-lane column maxima, wave butterflies,
12-byte groups) compute them -- plus the canvases of tests/golden/active_ref.npz, their statistics, and the synthetic letterboxed
videos of the loop tests."""
from __future__ import annotations

import os

import numpy as np

import cpu_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIVE_REF = os.path.join(ROOT, "tests", "golden", "active_ref.npz")
BAR_ROWS, BAR_COLS = 40, 37              # the bars of the fixture's canvases: rows above and below, columns left and right
BLACKS, QUALITIES = (0, 16), (95, 90, 75)
KEEP = 8                                 # bar lines nearer than this to the picture are not bar statistics; content edges are this deep


def luma_pixel(px, bgr: bool) -> int:
    """(77 R + 150 G + 29 B + 128) >> 8 of one pixel."""
    c0, c1, c2 = int(px[0]), int(px[1]), int(px[2])
    red, blue = (c2, c0) if bgr else (c0, c2)
    return (77 * red + 150 * c1 + 29 * blue + 128) // 256


def borders_model(frame: np.ndarray, bgr: bool = False) -> np.ndarray:
    """int32[H + W]: row by row, then column by column, the largest luma of the line."""
    H, W = frame.shape[:2]
    assert frame.dtype == np.uint8 and frame.shape[2] == 3 and H >= 16 and W >= 16
    out = np.zeros(H + W, np.int64)
    for y in range(H):
        out[y] = int(cpu_scene.luma(frame[y], bgr).max())
    for x in range(W):
        out[H + x] = int(cpu_scene.luma(frame[:, x], bgr).max())
    assert out.max() <= 255 and out[:H].max() == out[H:].max()
    return out.astype(np.int32)


def borders_model_pixels(frame: np.ndarray, bgr: bool = False) -> np.ndarray:
    """The same, pixel by pixel (small frames only)."""
    H, W = frame.shape[:2]
    out = np.zeros(H + W, np.int64)
    for y in range(H):
        for x in range(W):
            v = luma_pixel(frame[y, x], bgr)
            out[y] = max(out[y], v)
            out[H + x] = max(out[H + x], v)
    return out.astype(np.int32)


def to_u8(v) -> int:
    """``frame_f32_to_u8``'s value: x * 255 in fp32, round half to even, clamp."""
    q = float(np.float32(v) * np.float32(255.0))
    return int(min(255.0, max(0.0, float(np.rint(q)))))


def compose_model(border: np.ndarray, window, src=None, win_u8=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False) -> np.ndarray:
    """uint8 [H,W,3], pixel by pixel: ``border`` outside the window, the produced pixel inside."""
    H, W = border.shape[:2]
    y0, x0, h, w = window
    assert (src is None) != (win_u8 is None) and 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W
    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            wy, wx = y - y0, x - x0
            if not (0 <= wy < h and 0 <= wx < w):
                out[y, x] = border[y, x]
            elif win_u8 is not None:
                out[y, x] = win_u8[wy, wx]
            else:
                rgb = [to_u8(src[c, wy + pad_top, wx + pad_left]) for c in range(3)]
                out[y, x] = rgb[::-1] if bgr else rgb
    return out


# ------------------------------------------------------------------------------------------------ the fixture
def canvas(picture: np.ndarray, black: int) -> np.ndarray:
    """``picture`` (RGB) in a letterbox + pillarbox canvas: BAR_ROWS rows above and below, BAR_COLS columns left and right, all
    ``black``."""
    h, w = picture.shape[:2]
    c = np.full((h + 2 * BAR_ROWS, w + 2 * BAR_COLS, 3), black, np.uint8)
    c[BAR_ROWS:BAR_ROWS + h, BAR_COLS:BAR_COLS + w] = picture
    return c


def decoded_canvases():
    """(name, black, quality) -> the decoded uint8 RGB canvas: the canvas plus the committed int8 residual."""
    z = np.load(ACTIVE_REF)
    out = {}
    for name, pic in cpu_scene.pictures().items():
        for black in BLACKS:
            base = canvas(pic, black).astype(np.int16)
            for q in QUALITIES:
                out[(name, black, q)] = (base + z[f"{name}.b{black}.q{q}"]).astype(np.uint8)
    return out


def fixture_statistics():
    """(bars, content): ``bars`` one (label, value) per decoded canvas, the largest maximum of a bar line at least KEEP lines from the
    picture; ``content`` one per decoded canvas, the smallest line maximum among the picture's outermost KEEP rows and columns on each
    side.  Line maxima by the loop model."""
    bars, content = [], []
    for (name, black, q), c in decoded_canvases().items():
        H, W = c.shape[:2]
        prof = borders_model(c, bgr=False)
        rows, cols = prof[:H], prof[H:]
        far = np.concatenate([rows[:BAR_ROWS - KEEP], rows[H - BAR_ROWS + KEEP:], cols[:BAR_COLS - KEEP], cols[W - BAR_COLS + KEEP:]])
        edge = np.concatenate([rows[BAR_ROWS:BAR_ROWS + KEEP], rows[H - BAR_ROWS - KEEP:H - BAR_ROWS],
                               cols[BAR_COLS:BAR_COLS + KEEP], cols[W - BAR_COLS - KEEP:W - BAR_COLS]])
        label = f"{name} black {black} q{q}"
        bars.append((label, int(far.max())))
        content.append((label, int(edge.min())))
    return bars, content


# ------------------------------------------------------------------------------------------------ synthetic letterboxed videos
def letterboxed(n: int, H: int, W: int, rows, seed: int, tone: int = 150, noise: int = 3, cols=None, span: int = 60):
    """``n`` uint8 frames [H,W,3]: a ``cpu_scene.shot`` (tone >= 60 everywhere for the defaults: tone - span / 2 - 4 >= 116) in rows
    ``rows[0] .. rows[1] - 1`` (and columns ``cols``, default all), bars of seeded noise in 0 .. ``noise`` around it, different in every
    frame.  Returns (letterboxed frames, the pictures alone)."""
    r0, r1 = rows
    c0, c1 = cols or (0, W)
    inner = cpu_scene.shot(n, r1 - r0, c1 - c0, seed=seed, tone=tone, span=span)
    rng = np.random.default_rng(1000 + seed)
    full = []
    for f in inner:
        c = rng.integers(0, noise + 1, (H, W, 3), dtype=np.uint8)
        c[r0:r1, c0:c1] = f
        full.append(c)
    return full, inner
