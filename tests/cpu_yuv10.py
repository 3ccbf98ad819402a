"""The depth-keeping 10-bit YUV 4:2:0 <-> RGB definition of include/atmvfi.h (atmvfi_yuv_decode with keep_depth / atmvfi_yuv_encode at depth 10) as
explicit per-pixel Python loops over plain ints: the model that ``atm-vfi_amd/yuv.py``'s ``decode_numpy_f32`` / ``encode_numpy`` and
the HIP kernels of csrc/yuv10.hip are held to, bit for bit.  Written from the definition, not from ``yuv.py``: it carries its own
coefficient table (the README's) and shares nothing with the package or with ``cpu_yuv`` but ``random_frame``."""
import numpy as np

from cpu_yuv import random_frame  # noqa: F401  (re-exported: the tests draw their frames here)

# matrix -> decode [kY, kRV, kGU, kGV, kBU], encode rows Y / U / V over (R, G, B): 10-bit limited range, 14 fractional bits
TABLE10 = {
    "bt601": ([19133, 26226, -6438, -13359, 33148], [[4195, 8235, 1599], [-2421, -4754, 7175], [7175, -6008, -1167]]),
    "bt709": ([19133, 29459, -3504, -8757, 34711], [[2983, 10034, 1013], [-1644, -5531, 7175], [7175, -6517, -658]]),
}


def clip10(v):
    return 0 if v < 0 else (1023 if v > 1023 else v)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def split(buf, H, W):
    ch, cw = (H + 1) // 2, (W + 1) // 2
    flat = [int(v) for v in np.asarray(buf).reshape(-1)]
    assert len(flat) == H * W + 2 * ch * cw
    Y = [flat[r * W:(r + 1) * W] for r in range(H)]
    U = [flat[H * W + r * cw:H * W + (r + 1) * cw] for r in range(ch)]
    V = [flat[H * W + ch * cw + r * cw:H * W + ch * cw + (r + 1) * cw] for r in range(ch)]
    return Y, U, V, ch, cw


def decode_q(buf, H, W, matrix="bt601", siting="centre", window=None, track=None):
    """-> int [h,w,3], the 10-bit RGB levels of the window (y0, x0, h, w) of the frame (default: all of it).  Chroma neighbours clamp
    at the frame's edges.  ``track`` (a list): the largest accumulator magnitude seen is appended."""
    Y, U, V, ch, cw = split(buf, H, W)
    kY, kRV, kGU, kGV, kBU = TABLE10[matrix][0]
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    assert y0 % 2 == 0 and x0 % 2 == 0 and y0 >= 0 and x0 >= 0 and y0 + h <= H and x0 + w <= W
    out = np.zeros((h, w, 3), np.int64)
    big = 0
    for y in range(y0, y0 + h):
        r0 = y >> 1
        r1 = clamp(r0 + (1 if y & 1 else -1), 0, ch - 1)
        for x in range(x0, x0 + w):
            q0 = x >> 1
            if siting == "centre":
                q1 = clamp(q0 + (1 if x & 1 else -1), 0, cw - 1)
                wx0, wx1 = 3, 1
            else:
                q1 = min(q0 + 1, cw - 1)
                wx0, wx1 = (2, 2) if x & 1 else (4, 0)
            up = []
            for c in (U, V):
                up.append((3 * (wx0 * c[r0][q0] + wx1 * c[r0][q1]) + 1 * (wx0 * c[r1][q0] + wx1 * c[r1][q1]) + 8) >> 4)
            yy, u, v = Y[y][x] - 64, up[0] - 512, up[1] - 512
            acc = (kY * yy + kRV * v + (1 << 13), kY * yy + kGU * u + kGV * v + (1 << 13), kY * yy + kBU * u + (1 << 13))
            big = max(big, *(abs(a) for a in acc))
            out[y - y0, x - x0] = [clip10(a >> 14) for a in acc]
    if track is not None:
        track.append(big)
    return out


def decode(buf, H, W, matrix="bt601", siting="centre", window=None):
    """-> float32 [h,w,3] = q / 1023, the fp32 division"""
    return decode_q(buf, H, W, matrix, siting, window).astype(np.float32) / np.float32(1023)


def f32_to_q(x):
    """clip(rint(fl32(x * 1023)), 0, 1023) of an fp32 array in fp32 arithmetic, half to even: the encode's source pixel"""
    return np.clip(np.rint(np.asarray(x, np.float32) * np.float32(1023.0)), 0, 1023).astype(np.int64)


def encode_q(q, matrix="bt601", siting="centre", track=None):
    """int [H,W,3] 10-bit RGB levels -> packed 10-bit I420, 1-D uint16"""
    q = np.asarray(q)
    H, W = q.shape[:2]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    eY, eU, eV = TABLE10[matrix][1]
    big = 0

    def px(y, x):
        return [int(v) for v in q[y, x]]
    out = []
    for y in range(H):
        for x in range(W):
            p = px(y, x)
            acc = eY[0] * p[0] + eY[1] * p[1] + eY[2] * p[2] + (1 << 13)
            big = max(big, abs(acc))
            out.append(clip10((acc >> 14) + 64))
    for e in (eU, eV):
        for j in range(ch):
            for i in range(cw):
                rows = (2 * j, min(2 * j + 1, H - 1))
                if siting == "centre":
                    taps, sh = [(2 * i, 1), (min(2 * i + 1, W - 1), 1)], 2
                else:
                    taps, sh = [(max(2 * i - 1, 0), 1), (2 * i, 2), (min(2 * i + 1, W - 1), 1)], 3
                s = [0, 0, 0]
                for r in rows:
                    for col, wgt in taps:
                        p = px(r, col)
                        for c in range(3):
                            s[c] += wgt * p[c]
                acc = e[0] * s[0] + e[1] * s[1] + e[2] * s[2] + (1 << (13 + sh))
                big = max(big, abs(acc))
                out.append(clip10((acc >> (14 + sh)) + 512))
    if track is not None:
        track.append(big)
    return np.array(out, np.uint16)


def encode(rgb_f32, matrix="bt601", siting="centre"):
    """float32 [H,W,3] -> packed 10-bit I420, 1-D uint16"""
    return encode_q(f32_to_q(rgb_f32), matrix, siting)


def random_rgb(H, W, seed=0):
    """A seeded fp32 [H,W,3] picture: uniform over [-0.05, 1.05] (both clamps occur), every eighth value an exact level k / 1023."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.05, 1.05, (H, W, 3)).astype(np.float32)
    lv = (rng.integers(0, 1024, (H, W, 3)).astype(np.float32) / np.float32(1023))
    return np.where(rng.integers(0, 8, (H, W, 3)) == 0, lv, x).astype(np.float32)


def replicate_pad(img, hp, wp, pad_top, pad_left):
    """[h,w,3] -> planar [3,hp,wp] with the picture at (pad_top, pad_left) and replicate padding"""
    h, w = img.shape[:2]
    ys = np.clip(np.arange(hp) - pad_top, 0, h - 1)
    xs = np.clip(np.arange(wp) - pad_left, 0, w - 1)
    return np.ascontiguousarray(img[ys][:, xs].transpose(2, 0, 1))
