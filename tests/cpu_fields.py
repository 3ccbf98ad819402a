"""Per-pixel models of the interlaced-input definitions (atm-vfi_amd/fields.py; csrc/fields.hip): plain Python loops over rows and columns,
written from the definitions and not from the twins.  Shared by tests/test_fields_cpu.py and tests/test_gpu_fields.py.

``mutant`` switches one deliberate mistake on (the GPU tests show that each is caught by their inputs):
  "parity"  the parity of bob / rows flipped          "edge"     the edge row averaged (with its clamped neighbour) instead of copied
  "padding" the canvas padding replicated from the woven picture instead of the bobbed one
  "order"   bff read as tff                            "k2"       the forward's neighbours k - 2 / k + 2 instead of k - 1 / k + 1
"""
import numpy as np

F32 = np.float32


def parity_model(k, order, mutant=None):
    assert order in ("tff", "bff")
    tff = order == "tff" or mutant == "order"
    return (k + (0 if tff else 1)) & 1


def bob_model(S, p, mutant=None):
    """S: float32 [planes, h, w] -> bob(S, p), element by element."""
    planes, h, w = S.shape
    assert h >= 2 and p in (0, 1)
    if mutant == "parity":
        p ^= 1
    F = np.empty_like(S)
    for c in range(planes):
        for y in range(h):
            for x in range(w):
                if y & 1 == p:
                    v = S[c, y, x]
                elif y == 0 and mutant != "edge":
                    v = S[c, 1, x]
                elif y == h - 1 and mutant != "edge":
                    v = S[c, h - 2, x]
                else:
                    v = F32(0.5) * F32(S[c, max(y - 1, 0), x] + S[c, min(y + 1, h - 1), x])
                F[c, y, x] = v
    return F


def canvas_model(S, p, pad_top, pad_left, Hp, Wp, mutant=None):
    """The canvas form: D[c][Y][X] = bob(S, p)[c][clamp(Y - pad_top)][clamp(X - pad_left)]."""
    planes, h, w = S.shape
    F = bob_model(S, p, mutant)
    D = np.empty((planes, Hp, Wp), F32)
    for c in range(planes):
        for Y in range(Hp):
            for X in range(Wp):
                y, x = min(max(Y - pad_top, 0), h - 1), min(max(X - pad_left, 0), w - 1)
                inside = 0 <= Y - pad_top < h and 0 <= X - pad_left < w
                D[c, Y, X] = S[c, y, x] if (mutant == "padding" and not inside) else F[c, y, x]
    return D


def rows_model(dst, src, p, mutant=None):
    """One plane [rows, cols]: rows of parity p of src replace those of dst (a new array)."""
    if mutant == "parity":
        p ^= 1
    out = dst.copy()
    for y in range(dst.shape[0]):
        if y & 1 == p:
            for x in range(dst.shape[1]):
                out[y, x] = src[y, x]
    return out


def rows_bytes_model(dst, src, geometry, p):
    """``atmvfi_field_rows`` on flat uint8 arrays: (dst_offset, src_offset, dst_pitch, src_pitch, row_bytes, rows) per plane."""
    out = dst.copy()
    for doff, soff, dp, sp, rb, rows in geometry:
        for y in range(rows):
            if y & 1 == p:
                for x in range(rb):
                    out[doff + y * dp + x] = src[soff + y * sp + x]
    return out


def predictions_model(pictures, order, mode, forward, canvas, cuts=(), mutant=None):
    """The prediction canvas P of every output k of n woven pictures (float32 [3,h,w] each): ``forward(B0, B1) -> I_t`` on canvases
    [3,Hp,Wp]; ``cuts``: the frame indices j with a cut between j and j + 1.  -> [(P, parity(k), was_bob)]."""
    n = len(pictures)
    B = lambda i: canvas_model(pictures[i // 2], parity_model(i, order, mutant), *canvas, mutant=mutant)
    out = []
    d = 2 if mutant == "k2" else 1
    for k in range(2 * n):
        j = k // 2
        bob = mode == "bob" or k == 0 or k == 2 * n - 1
        if k & 1 and j in cuts:                  # field 2j + 1 of a cut between j and j + 1
            bob = True
        if not k & 1 and (j - 1) in cuts:        # field 2j + 2 of a cut between j and j + 1, as field 2(j + 1)
            bob = True
        if not bob and not (0 <= k - d and k + d < 2 * n):
            bob = True
        P = B(k) if bob else forward(B(k - d), B(k + d))
        out.append((P, parity_model(k, order, mutant), bob))
    return out


def hostile(shape, seed):
    """float32 values well outside [0, 1], of mixed magnitude and sign (no two neighbouring rows alike)."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(F32)


def interlaced_video(n, h, w, seed=5, tone=120):
    """n woven uint8 RGB frames of a drifting texture: even rows from time 2j, odd rows from time 2j + 1 (tff material)."""
    import cpu_scene as CS
    prog = CS.shot(2 * n, h, w, seed=seed, tone=tone)
    out = []
    for j in range(n):
        f = prog[2 * j].copy()
        f[1::2] = prog[2 * j + 1][1::2]
        out.append(f)
    return out


# ------------------------------------------------------------------------------------------------ the reference parity fixture
import os

FIELDS_REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fields_ref.npz")
REF_CASES = (("lite", "lite"), ("base", "base"))             # (name, variant): both with the global branch on
REF_H, REF_W, REF_N, REF_DIVISOR, REF_STEP = 64, 96, 4, 64, 2


def reference_video():
    """Four woven 64 x 96 uint8 RGB frames of a moving ``pairs`` picture: even rows from time 2j, odd rows from time 2j + 1."""
    import pairs
    prog = pairs.uint8_video(2 * REF_N, REF_H, REF_W, seed=7)
    out = []
    for j in range(REF_N):
        f = prog[2 * j].copy()
        f[1::2] = prog[2 * j + 1][1::2]
        out.append(f)
    return out


def reference_pictures():
    """The woven pictures as the network's fp32 [3,h,w] (u8 / 255 in float32)."""
    return [(f.transpose(2, 0, 1).astype(F32) / F32(255)) for f in reference_video()]
