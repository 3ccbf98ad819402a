"""Per-sample loop model of the packed 4:2:2 layouts (atm-vfi_amd/pixfmt.py Packed; include/atmvfi.h atmvfi_yuv_unpack / atmvfi_yuv_pack):
plain Python loops over samples, written from the layout table and -- for v210 -- as a literal transcription of its word table,
independently of the vectorised twins ``yuv.unpack_numpy`` / ``pack_numpy``.  A frame here is its BYTES (1-D uint8, little-endian);
a planar frame is a 1-D array of uint8 / uint16 sample values, Y [H,W] then U [H,W/2] then V [H,W/2].

The layouts are row-separable by definition (a row of the packed frame holds the samples of that row of the three planes and nothing
else), so the frame functions run the row loops row by row; ``memo`` (a dict) lets a tall frame built from a few distinct rows pay for
each distinct row once."""
import numpy as np

LAYOUTS = ("uyvy", "yuy2", "y210", "v210")
DEPTH = {"uyvy": 8, "yuy2": 8, "y210": 10, "v210": 10}
# memory order of a pixel pair's four samples
PAIR_ORDER = {"uyvy": ("U", "Y0", "V", "Y1"), "yuy2": ("Y0", "U", "Y1", "V"), "y210": ("Y0", "U", "Y1", "V")}
# a v210 group: four little-endian 32-bit words for 6 pixels, three components each in bits 0-9, 10-19, 20-29
V210_WORDS = ((("Cb", 0), ("Y", 0), ("Cr", 0)),
              (("Y", 1), ("Cb", 1), ("Y", 2)),
              (("Cr", 1), ("Y", 3), ("Cb", 2)),
              (("Y", 4), ("Cr", 2), ("Y", 5)))


def row_bytes(layout, W):
    return {"uyvy": 2 * W, "yuy2": 2 * W, "y210": 4 * W, "v210": -(-W // 6) * 16}[layout]


def default_pitch(layout, W):
    return -(-W // 48) * 128 if layout == "v210" else row_bytes(layout, W)


def planar_dtype(layout):
    return np.uint16 if DEPTH[layout] == 10 else np.uint8


def unpack_row(row, layout, W):
    """the bytes of one packed row (at least its own bytes) -> (Y, U, V) lists of sample values"""
    Y, U, V = [0] * W, [0] * (W // 2), [0] * (W // 2)
    if layout == "v210":
        for g in range(-(-W // 6)):
            for k, word in enumerate(V210_WORDS):
                o = 16 * g + 4 * k
                w = int(row[o]) | int(row[o + 1]) << 8 | int(row[o + 2]) << 16 | int(row[o + 3]) << 24
                for slot, (kind, i) in enumerate(word):
                    value = (w >> (10 * slot)) & 0x3FF
                    if kind == "Y":
                        if 6 * g + i < W:
                            Y[6 * g + i] = value
                    elif 2 * (3 * g + i) < W:        # Cb_i / Cr_i of the group belong to its pixels 2i and 2i + 1
                        (U if kind == "Cb" else V)[3 * g + i] = value
        return Y, U, V
    size = 2 if layout == "y210" else 1
    for p in range(W // 2):
        for slot, name in enumerate(PAIR_ORDER[layout]):
            o = (4 * p + slot) * size
            s = int(row[o]) if size == 1 else (int(row[o]) | int(row[o + 1]) << 8) >> 6
            if name == "Y0":
                Y[2 * p] = s
            elif name == "Y1":
                Y[2 * p + 1] = s
            elif name == "U":
                U[p] = s
            else:
                V[p] = s
    return Y, U, V


def pack_row(Y, U, V, layout, W):
    """sample values of one row -> the bytes of the packed row at the default pitch; what holds no sample is zero"""
    out = bytearray(default_pitch(layout, W))
    if layout == "v210":
        for g in range(-(-W // 6)):
            for k, word in enumerate(V210_WORDS):
                w = 0
                for slot, (kind, i) in enumerate(word):
                    if kind == "Y":
                        value = int(Y[6 * g + i]) if 6 * g + i < W else 0
                    else:
                        value = int((U if kind == "Cb" else V)[3 * g + i]) if 2 * (3 * g + i) < W else 0
                    w |= (value & 0x3FF) << (10 * slot)
                out[16 * g + 4 * k:16 * g + 4 * k + 4] = w.to_bytes(4, "little")
        return out
    size = 2 if layout == "y210" else 1
    for p in range(W // 2):
        named = {"Y0": Y[2 * p], "Y1": Y[2 * p + 1], "U": U[p], "V": V[p]}
        for slot, name in enumerate(PAIR_ORDER[layout]):
            o = (4 * p + slot) * size
            if size == 1:
                out[o] = int(named[name]) & 0xFF
            else:
                out[o:o + 2] = ((int(named[name]) << 6) & 0xFFFF).to_bytes(2, "little")
    return out


def unpack_loop(frame, layout, H, W, pitch=None, memo=None):
    """packed frame bytes (1-D uint8, ``pitch * H``) -> the planar frame (1-D uint8 / uint16)"""
    pitch = default_pitch(layout, W) if pitch is None else pitch
    frame = np.asarray(frame, np.uint8)
    assert frame.shape == (pitch * H,)
    n = row_bytes(layout, W)
    Ys, Us, Vs = [], [], []
    for y in range(H):
        row = frame[y * pitch:y * pitch + n].tobytes()          # (nothing beyond the row's own bytes is looked at)
        if memo is None or row not in memo:
            got = tuple(np.array(p, dtype=planar_dtype(layout)) for p in unpack_row(row, layout, W))
            if memo is not None:
                memo[row] = got
        else:
            got = memo[row]
        Ys.append(got[0])
        Us.append(got[1])
        Vs.append(got[2])
    return np.concatenate(Ys + Us + Vs)


def pack_loop(planar, layout, H, W, memo=None):
    """the planar frame -> packed frame bytes at the default pitch (1-D uint8)"""
    planar = np.asarray(planar)
    cw = W // 2
    assert planar.shape == (2 * H * W,) and planar.dtype == planar_dtype(layout)
    Y, U, V = planar[:H * W].reshape(H, W), planar[H * W:H * W + H * cw].reshape(H, cw), planar[H * W + H * cw:].reshape(H, cw)
    out = bytearray()
    for y in range(H):
        key = (Y[y].tobytes(), U[y].tobytes(), V[y].tobytes())
        if memo is None or key not in memo:
            row = pack_row(Y[y].tolist(), U[y].tolist(), V[y].tolist(), layout, W)
            if memo is not None:
                memo[key] = row
        else:
            row = memo[key]
        out += row
    return np.frombuffer(bytes(out), np.uint8).copy()


def sample_mask(layout, H, W, pitch=None):
    """uint8 [pitch * H]: the BITS of a packed frame that hold a sample"""
    pitch = default_pitch(layout, W) if pitch is None else pitch
    row = bytearray(pitch)
    if layout == "v210":
        for g in range(-(-W // 6)):
            for k, word in enumerate(V210_WORDS):
                w = 0
                for slot, (kind, i) in enumerate(word):
                    if (6 * g + i < W) if kind == "Y" else (2 * (3 * g + i) < W):
                        w |= 0x3FF << (10 * slot)
                row[16 * g + 4 * k:16 * g + 4 * k + 4] = w.to_bytes(4, "little")
    elif layout == "y210":
        for s in range(2 * W):
            row[2 * s:2 * s + 2] = (0xFFC0).to_bytes(2, "little")
    else:
        for s in range(2 * W):
            row[s] = 0xFF
    return np.tile(np.frombuffer(bytes(row), np.uint8), H)


def poisoned(frame, layout, H, W, pitch):
    """a default-pitch frame's bytes at ``pitch`` with every bit that holds no sample SET (0xFF row padding, v210's bits 30-31 and unused
    component slots, y210's low six bits)"""
    d = default_pitch(layout, W)
    n = row_bytes(layout, W)
    src = np.asarray(frame, np.uint8).reshape(H, d)
    out = np.full((H, pitch), 0xFF, np.uint8)
    out[:, :n] = src[:, :n]
    out = out.reshape(-1)
    return out | ~sample_mask(layout, H, W, pitch)


def random_planar(rng, layout, H, W):
    return rng.integers(0, 1 << DEPTH[layout], 2 * H * W).astype(planar_dtype(layout))


def tall_planar(rng, layout, H, W, distinct=6):
    """a planar frame of H rows drawn (without a period) from ``distinct`` random rows: what ``memo`` makes affordable"""
    cw = W // 2
    rows = rng.integers(0, 1 << DEPTH[layout], (distinct, 2 * W)).astype(planar_dtype(layout))
    pick = rng.integers(0, distinct, H)
    return np.concatenate([rows[pick, :W].reshape(-1), rows[pick, W:W + cw].reshape(-1), rows[pick, W + cw:].reshape(-1)])
