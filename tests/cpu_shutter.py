"""The loop model of the synthetic shutter (atm-vfi_amd/shutter.py; csrc/shutter.hip): the light tables from their float64 derivation,
accumulate / resolve one value at a time, and the timeline by brute force over every sample of the stream -- written from the
definition (README "Synthetic shutter"), independently of shutter.py's streaming plan and vectorised arithmetic."""
import math
from fractions import Fraction

import numpy as np


def derived_table(light):
    """LUT[q], q = 0..255: 257 q ("code"), or rint(65535 eotf(q / 255)) of the sRGB curve in float64 ("linear")."""
    if light == "code":
        return [257 * q for q in range(256)]
    out = []
    for q in range(256):
        x = q / 255.0
        e = x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4
        out.append(int(np.rint(65535.0 * e)))
    return out


def tie_margin():
    """how close 65535 eotf(q / 255) comes to a rounding tie, over all q"""
    worst = 1.0
    for q in range(256):
        x = q / 255.0
        v = 65535.0 * (x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4)
        worst = min(worst, abs(v - math.floor(v) - 0.5))
    return worst


def thresholds(lut):
    """thr[k], k = 1..255 (thr[0] is not part of the definition)"""
    return [None] + [(lut[k - 1] + lut[k] + 1) >> 1 for k in range(1, 256)]


def inverse_value(v, lut):
    """the number of k in 1..255 with v >= thr[k]"""
    thr = thresholds(lut)
    return sum(1 for k in range(1, 256) if v >= thr[k])


_INVERSE = {}


def inverse_table(lut):
    """inverse_value for every v in 0..65535 by one sweep (thr is increasing), kept per table"""
    key = tuple(lut)
    if key not in _INVERSE:
        thr, out, k = thresholds(lut), [], 0
        for v in range(65536):
            while k < 255 and v >= thr[k + 1]:
                k += 1
            out.append(k)
        _INVERSE[key] = out
    return _INVERSE[key]


def pixel_of_f32(x):
    """frame_f32_to_u8's pixel of one fp32 value: clamp(rint(fl32(x * 255))), half to even"""
    r = int(np.rint(np.float32(x) * np.float32(255.0)))
    return 0 if r < 0 else (255 if r > 255 else r)


def pixels_of_canvas(canvas, pad_top, pad_left, h, w):
    """uint8 [h,w,3] RGB of the window of an fp32 planar [3,Hp,Wp] canvas, one value at a time"""
    out = np.zeros((h, w, 3), np.uint8)
    for c in range(3):
        for y in range(h):
            for x in range(w):
                out[y, x, c] = pixel_of_f32(canvas[c, y + pad_top, x + pad_left])
    return out


def accumulate_model(acc, rgb, weight, lut, first):
    """acc: a list of 3 h w Python ints, planar R, G, B (None when ``first``: nothing is read); rgb: uint8 [h,w,3] R, G, B."""
    h, w = rgb.shape[:2]
    flat = rgb.tolist()
    out = [0] * (3 * h * w)
    for c in range(3):
        for y in range(h):
            row = flat[y]
            for x in range(w):
                i = (c * h + y) * w + x
                out[i] = weight * lut[row[x][c]] + (0 if first else acc[i])
    return out


def resolve_model(acc, h, w, total, lut):
    """uint8 [h,w,3] R, G, B of a planar accumulator"""
    inv = inverse_table(lut)
    out = np.zeros((h, w, 3), np.uint8)
    for c in range(3):
        for y in range(h):
            for x in range(w):
                a = acc[(c * h + y) * w + x]
                assert 0 <= a <= 65535 * total
                out[y, x, c] = inv[(a + (total >> 1)) // total]
    return out


def blend_model(frames, weights, light):
    """the blend of uint8 frames of any one shape, one value at a time"""
    lut = derived_table(light)
    inv = inverse_table(lut)
    total = sum(weights)
    flat = [np.asarray(f).reshape(-1).tolist() for f in frames]
    out = []
    for i in range(len(flat[0])):
        acc = sum(w * lut[f[i]] for f, w in zip(flat, weights))
        out.append(inv[(acc + (total >> 1)) // total])
    return np.array(out, np.uint8).reshape(np.asarray(frames[0]).shape)


def slots_model(kept, fps_in, fps_out, levels, angle, cuts=()):
    """[(m, (j_m, p_m), [(j, p, weight), ...])] by brute force: every sample of the whole stream against every output's window."""
    kept = list(kept)
    fi, fo, n = Fraction(fps_in), Fraction(fps_out), 1 << levels
    J = len(kept) - 1
    cuts = set(cuts)

    def shot(j, p):
        return sum(1 for c in cuts if c < j) + (1 if j in cuts and 2 * p > n else 0)
    samples = []                                     # (time, j, p, weight, shot)
    for j in range(J):
        g = kept[j + 1] - kept[j]
        for p in range(n):
            samples.append(((kept[j] + Fraction(g * p, n)) / fi, j, p, g, shot(j, p)))
    if J >= 1:
        samples.append((Fraction(kept[J]) / fi, J - 1, n, kept[J] - kept[J - 1], shot(J - 1, n)))
    E = Fraction(angle) / 360 / fo
    out, m = [], 0
    while Fraction(m) / fo <= Fraction(kept[-1]) / fi:
        T = Fraction(m) / fo
        u = T * fi
        if u == kept[-1]:
            pos = (J - 1, n) if J >= 1 else (0, 0)
        else:
            j = max(k for k in range(J) if kept[k] <= u)
            pos = (j, math.floor((u - kept[j]) / (kept[j + 1] - kept[j]) * n + Fraction(1, 2)))
        # the shot of the position; (j, N) of a non-last segment is sample (j + 1, 0)
        own = shot(*pos) if J >= 1 else 0
        S = [(j, p, w) for t, j, p, w, s in samples if T - E / 2 <= t < T + E / 2 and s == own]
        if not S:
            S = [(pos[0], pos[1], kept[pos[0] + 1] - kept[pos[0]] if J >= 1 else 1)]
        out.append((m, pos, S))
        m += 1
    return out
