"""Loop-style numpy model of the frame signature (include/atmvfi.h atmvfi_frame_signature; atm-vfi_amd/scene.py), the yardstick of its
tests: written cell by cell and bin by bin from the definition, not the way ``scene.signature_numpy`` (reduceat / bincount) or the
kernel (per-lane column sums, LDS histogram copies) compute it -- plus the pictures of tests/golden/scene_ref.npz and the synthetic
two-shot videos of the loop tests."""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_REF = os.path.join(ROOT, "tests", "golden", "scene_ref.npz")


def luma(frame: np.ndarray, bgr: bool) -> np.ndarray:
    """int64 [H,W]: (77 R + 150 G + 29 B + 128) >> 8, channel by channel."""
    f = frame.astype(np.int64)
    red, green, blue = f[..., 2 if bgr else 0], f[..., 1], f[..., 0 if bgr else 2]
    return (77 * red + 150 * green + 29 * blue + 128) // 256


def signature_model(frame: np.ndarray, y0: int = 0, x0: int = 0, h=None, w=None, bgr: bool = False) -> np.ndarray:
    H, W = frame.shape[:2]
    h = H - y0 if h is None else h
    w = W - x0 if w is None else w
    assert h >= 16 and w >= 16 and y0 >= 0 and x0 >= 0 and y0 + h <= H and x0 + w <= W
    y = luma(frame, bgr)[y0:y0 + h, x0:x0 + w]
    sig = np.zeros(288, np.int64)
    for i in range(16):
        for j in range(16):
            cell = y[(i * h) // 16:((i + 1) * h) // 16, (j * w) // 16:((j + 1) * w) // 16]
            sig[16 * i + j] = int(cell.sum())
    for b in range(32):
        sig[256 + b] = int(np.count_nonzero((y >= 8 * b) & (y < 8 * b + 8)))
    assert sig[:256].sum() == y.sum() and sig[256:].sum() == h * w and sig.max() < 2 ** 31
    return sig.astype(np.int32)


def pictures():
    """name -> uint8 RGB [300,207,3] of tests/golden/scene_ref.npz."""
    z = np.load(SCENE_REF)
    return {k: z[k] for k in z.files}


def pan_windows(frame: np.ndarray, frac: float, side: int = 128):
    """Two ``side``-square windows of a picture offset horizontally by ``frac`` of their side, centred vertically: a pan."""
    H, W = frame.shape[:2]
    off = int(round(side * frac))
    y = (H - side) // 2
    x = (W - side - off) // 2
    return frame[y:y + side, x:x + side], frame[y:y + side, x + off:x + off + side]


def shot(n: int, h: int, w: int, seed: int, tone: int, span: int = 60):
    """``n`` uint8 frames of one synthetic shot: a smooth texture around luma ``tone`` (+- span / 2) drifting one pixel per frame.
    Two shots of different ``tone`` differ in tone, not just in seed: the histogram term cannot tell two i.i.d. textures apart."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w + n]
    base = np.zeros((h, w + n, 3))
    for c in range(3):
        fy, fx, ph = rng.uniform(0.05, 0.3), rng.uniform(0.05, 0.3), rng.uniform(0, 6.28)
        base[..., c] = tone + span / 2 * np.sin(fy * yy + fx * xx + ph) + rng.uniform(-4, 4)
    base = np.clip(np.round(base), 0, 255).astype(np.uint8)
    return [np.ascontiguousarray(base[:, k:k + w]) for k in range(n)]


def expected_two_shot(nx, A, B, factor: int, s: int = 1, crop_of=lambda f: f):
    """The frames of video A ++ B with the cut between them detected, from ``nx(shot)`` = the loop on one shot alone:
    list(nx(A)) + [A_last] * (N / 2) + [B_0] * (N / 2 - 1) + list(nx(B)).  A and B must each be whole segments long (len = k s + 1)."""
    assert (len(A) - 1) % s == 0 and (len(B) - 1) % s == 0
    a = list(nx(A)) if len(A) > 1 else [crop_of(A[0])]
    b = list(nx(B)) if len(B) > 1 else [crop_of(B[0])]
    return a + [crop_of(A[-1])] * (factor // 2) + [crop_of(B[0])] * (factor // 2 - 1) + b
