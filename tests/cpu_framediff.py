"""Loop-style model of the frame difference (include/atmvfi.h atmvfi_frame_difference; atm-vfi_amd/retime.py), the yardstick of its
tests: written pixel by pixel from the definition, not the way ``retime.difference_numpy`` (reduceat) or the kernel (per-lane column
sums, segmented scans) compute it -- plus the pictures of tests/golden/dedup_ref.npz and the duplicate / motion sets the default
thresholds are placed from."""
from __future__ import annotations

import os

import numpy as np

import cpu_scene

ROOT = cpu_scene.ROOT
DEDUP_REF = os.path.join(ROOT, "tests", "golden", "dedup_ref.npz")


def luma_of(px, bgr: bool) -> int:
    red, green, blue = int(px[2 if bgr else 0]), int(px[1]), int(px[0 if bgr else 2])
    return (77 * red + 150 * green + 29 * blue + 128) // 256


def difference_model(a: np.ndarray, b: np.ndarray, y0: int = 0, x0: int = 0, h=None, w=None, bgr: bool = True) -> np.ndarray:
    """int32[258]: one pixel at a time, every pixel added to the cell that the definition's row and column ranges put it in."""
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    H, W = a.shape[:2]
    h = H - y0 if h is None else h
    w = W - x0 if w is None else w
    assert h >= 16 and w >= 16 and y0 >= 0 and x0 >= 0 and y0 + h <= H and x0 + w <= W
    cell_of_row = [next(i for i in range(16) if (i * h) // 16 <= r < ((i + 1) * h) // 16) for r in range(h)]
    cell_of_col = [next(j for j in range(16) if (j * w) // 16 <= c < ((j + 1) * w) // 16) for c in range(w)]
    out = [0] * 258
    for r in range(h):
        ra, rb = a[y0 + r], b[y0 + r]
        for c in range(w):
            d = abs(luma_of(ra[x0 + c], bgr) - luma_of(rb[x0 + c], bgr))
            out[16 * cell_of_row[r] + cell_of_col[c]] += d
            out[256] = max(out[256], d)
            out[257] += d != 0
    assert max(out) < 2 ** 31
    return np.array(out, dtype=np.int32)


def difference_fast(a, b, y0=0, x0=0, h=None, w=None, bgr=True) -> np.ndarray:
    """The same numbers for windows too large for the pixel loop: whole-array luma (cpu_scene.luma), cells sliced one by one as
    cpu_scene.signature_model slices them.  tests/test_retime_cpu.py holds it to ``difference_model`` on the small cases."""
    H, W = a.shape[:2]
    h = H - y0 if h is None else h
    w = W - x0 if w is None else w
    d = np.abs(cpu_scene.luma(a, bgr) - cpu_scene.luma(b, bgr))[y0:y0 + h, x0:x0 + w]
    out = np.zeros(258, np.int64)
    for i in range(16):
        for j in range(16):
            out[16 * i + j] = int(d[(i * h) // 16:((i + 1) * h) // 16, (j * w) // 16:((j + 1) * w) // 16].sum())
    out[256], out[257] = int(d.max()), int(np.count_nonzero(d))
    assert out[:256].sum() == d.sum() and out.max() < 2 ** 31
    return out.astype(np.int32)


def reencodes():
    """(name, quality) -> the decoded uint8 RGB [300,207,3] JPEG re-encode of a picture of scene_ref.npz (tools/gen_dedup_golden.py
    stores decoded - original as int8)."""
    P, z = cpu_scene.pictures(), np.load(DEDUP_REF)
    out = {}
    for key in z.files:
        name, q = key.rsplit(".q", 1)
        out[(name, int(q))] = (P[name].astype(np.int16) + z[key]).astype(np.uint8)
    return out


def duplicate_pairs():
    """(label, a, b): every picture against its q95 and q90 re-encodes, and against itself plus uniform noise of +-1, +-2, +-3."""
    P, R = cpu_scene.pictures(), reencodes()
    rng = np.random.default_rng(0)
    pairs = []
    for name, pic in P.items():
        for q in (95, 90):
            pairs.append((f"{name} / q{q}", pic, R[(name, q)]))
        for amp in (1, 2, 3):
            noise = rng.integers(-amp, amp + 1, pic.shape)
            pairs.append((f"{name} / noise +-{amp}", pic, np.clip(pic.astype(np.int64) + noise, 0, 255).astype(np.uint8)))
    return pairs


def motion_pairs():
    """(label, a, b): the 128-pixel window [40:168, 40:168] of each picture against the same window panned by one pixel."""
    return [(f"{name} panned by 1", np.ascontiguousarray(pic[40:168, 40:168]), np.ascontiguousarray(pic[40:168, 41:169]))
            for name, pic in cpu_scene.pictures().items()]


def primed(frame: np.ndarray, seed: int, amp: int = 2) -> np.ndarray:
    """A duplicate of ``frame`` within the duplicate set: uniform noise of +-``amp``."""
    noise = np.random.default_rng(seed).integers(-amp, amp + 1, frame.shape)
    return np.clip(frame.astype(np.int64) + noise, 0, 255).astype(np.uint8)
