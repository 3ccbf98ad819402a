"""The YUV 4:2:0 <-> RGB definition of include/atmvfi.h as explicit per-pixel Python loops over plain ints: the model that
``atm-vfi_amd/yuv.py``'s vectorised twins and the HIP kernels are held to, bit for bit.  Written from the definition, not from
``yuv.py``: it carries its own coefficient table (the README's) and shares no code with the package."""
import numpy as np

# (matrix, full_range) -> decode [kY, kRV, kGU, kGV, kBU], encode rows Y / U / V over (R, G, B)
TABLE = {
    ("bt601", 0): ([19077, 26149, -6419, -13320, 33050], [[4207, 8260, 1604], [-2428, -4768, 7196], [7196, -6026, -1170]]),
    ("bt601", 1): ([16384, 22970, -5638, -11700, 29032], [[4899, 9617, 1868], [-2765, -5427, 8192], [8192, -6860, -1332]]),
    ("bt709", 0): ([19077, 29372, -3494, -8731, 34610], [[2991, 10064, 1016], [-1649, -5547, 7196], [7196, -6536, -660]]),
    ("bt709", 1): ([16384, 25802, -3069, -7670, 30402], [[3483, 11718, 1183], [-1877, -6315, 8192], [8192, -7441, -751]]),
}


def clip8(v):
    return 0 if v < 0 else (255 if v > 255 else v)


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


def decode(buf, H, W, matrix="bt601", full_range=0, siting="centre", depth=8, bgr=False):
    """-> uint8 [H,W,3]"""
    Y, U, V, ch, cw = split(buf, H, W)
    kY, kRV, kGU, kGV, kBU = TABLE[matrix, int(full_range)][0]
    if depth == 10:
        yo, mid, T = 64, 512, 16
    else:
        yo, mid, T = (0 if full_range else 16), 128, 14
    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        r0 = y >> 1
        r1 = clamp(r0 + (1 if y & 1 else -1), 0, ch - 1)
        for x in range(W):
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
            yy, u, v = Y[y][x] - yo, up[0] - mid, up[1] - mid
            half = 1 << (T - 1)
            R = clip8((kY * yy + kRV * v + half) >> T)
            G = clip8((kY * yy + kGU * u + kGV * v + half) >> T)
            B = clip8((kY * yy + kBU * u + half) >> T)
            out[y, x] = (B, G, R) if bgr else (R, G, B)
    return out


def encode(rgb, matrix="bt601", full_range=0, siting="centre", bgr=False):
    """uint8 [H,W,3] -> packed I420, 1-D uint8"""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    eY, eU, eV = TABLE[matrix, int(full_range)][1]
    yo = 0 if full_range else 16

    def px(y, x):
        p = [int(v) for v in rgb[y, x]]
        return p[::-1] if bgr else p
    out = []
    for y in range(H):
        for x in range(W):
            p = px(y, x)
            out.append(clip8(((eY[0] * p[0] + eY[1] * p[1] + eY[2] * p[2] + (1 << 13)) >> 14) + yo))
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
                out.append(clip8(((e[0] * s[0] + e[1] * s[1] + e[2] * s[2] + (1 << (13 + sh))) >> (14 + sh)) + 128))
    return np.array(out, np.uint8)


def f32_to_u8(x):
    """clamp(rint(x * 255)) of an fp32 array in fp32 arithmetic, half to even: atmvfi_frame_f32_to_u8's pixel"""
    return np.clip(np.rint(np.asarray(x, np.float32) * np.float32(255.0)), 0, 255).astype(np.uint8)


def random_frame(H, W, depth=8, seed=0):
    """A seeded uniform-random packed I420 frame over the whole sample range."""
    rng = np.random.default_rng(seed)
    n = H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
    return rng.integers(0, 1024 if depth == 10 else 256, n).astype(np.uint16 if depth == 10 else np.uint8)
