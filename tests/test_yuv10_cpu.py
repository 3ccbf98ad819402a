"""CPU: 10-bit depth kept end to end (``keep_depth``; include/atmvfi.h atmvfi_yuv_decode with keep_depth / atmvfi_yuv_encode at depth 10, csrc/yuv.hip, yuv_encode.hip):
the coefficient table in all its places, the numpy twins against the per-pixel model of tests/cpu_yuv10.py, accumulator bounds, grey
neutrality and round trips, the q / 1023 shortcut of the kernel, ties and clamps of the encode, the ABI's host-side checks, and the
loops / ``interpolate_y4m`` with ``keep_depth=True`` through the generic (no-GPU) path."""
import ctypes
import importlib
import inspect
import io
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cpu_scene as CS
import cpu_yuv10 as C10

mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")
yuv = importlib.import_module("atm-vfi_amd.yuv")

COMBOS = list(itertools.product(("bt601", "bt709"), ("centre", "left")))
SIZES = [(1, 1), (2, 2), (3, 5), (17, 31), (34, 50)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ coefficients
def _ints(text):
    return [int(v) for v in re.findall(r"-?\d+", text)]


def test_coefficients_table_derivation_header_and_kernel_agree():
    assert set(yuv.COEFFS10) == {"bt601", "bt709"}
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    src = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "yuv_common.h")).read()
    table = re.search(r"kCoeffs10\[2\]\s*=\s*\{(.*?)\n\};", src, flags=re.S).group(1)
    rows = [_ints(line) for line in table.splitlines() if re.search(r"\{\{", line)]
    assert len(rows) == 2
    for k, m in enumerate(("bt601", "bt709")):
        dec, enc = yuv.COEFFS10[m]
        want = C10.TABLE10[m]
        assert list(dec) == want[0] and [list(r) for r in enc] == want[1]
        flat = want[0] + [v for r in want[1] for v in r]
        # from (Kr, Kb), written out once more here: luma scaled by 876 / 1023, chroma by 896 / 1023
        kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[m]
        kg = 1 - kr - kb
        sy, sc = 876 / 1023, 896 / 1023
        want_dec = [1 / sy, 2 * (1 - kr) / sc, -2 * (1 - kb) * kb / kg / sc, -2 * (1 - kr) * kr / kg / sc, 2 * (1 - kb) / sc]
        want_enc = [[kr * sy, kg * sy, kb * sy], [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc],
                    [0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]]
        assert want[0] == [int(np.rint(v * 16384)) for v in want_dec]
        assert want[1] == [[int(np.rint(v * 16384)) for v in r] for r in want_enc]
        assert yuv.derive_coeffs(m, False, 10) == (want[0], want[1]) == yuv.derive_coeffs(m, depth=10)
        assert [sum(r) for r in want[1]][1:] == [0, 0]                       # greys carry no chroma
        assert max(abs(v) for v in flat) < 1 << 17                           # __mul24's operand range, with samples below 2^14
        # the header's table line and the kernel's table row
        line = re.search(m + r" 10 bit(.*)", hdr).group(1)
        assert _ints(line) == flat, (m, line)
        assert rows[k] == flat, (m, rows[k])
    # the 8-bit derivation is untouched and 10-bit full range stays refused
    assert yuv.derive_coeffs("bt601", False) == (list(yuv.COEFFS["bt601", False][0]), [list(r) for r in yuv.COEFFS["bt601", False][1]])
    with pytest.raises(ValueError):
        yuv.derive_coeffs("bt601", True, 10)
    with pytest.raises(ValueError):
        yuv.derive_coeffs("bt601", False, 12)


# ------------------------------------------------------------------------------------------------ twins
def windows_of(H, W):
    """even-origin windows: the whole frame, one strictly inside (when there is room) and ones touching each frame edge"""
    out = [(0, 0, H, W)]
    if H >= 8 and W >= 8:
        out += [(2, 4, H - 6, W - 8), (0, 0, H - 3, W - 3), (4, 2, H - 4, W - 2), (H // 2 // 2 * 2, W // 2 // 2 * 2, H - H // 2 // 2 * 2, 3),
                (2, 0, 1, W)]
    return out


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_numpy_twins_are_the_loop_model(H, W):
    for k, (m, s) in enumerate(COMBOS):
        fmt = yuv.Format(H, W, m, False, s, 10)
        buf = C10.random_frame(H, W, 10, seed=H * W + k)
        full = C10.decode(buf, H, W, m, s)
        got = yuv.decode_numpy_f32(buf, fmt)
        assert got.shape == (H, W, 3) and same_bits(got, full), (m, s)
        for win in windows_of(H, W):
            y0, x0, h, w = win
            part = yuv.decode_numpy_f32(buf, fmt, window=win)
            assert same_bits(part, C10.decode(buf, H, W, m, s, window=win)), (m, s, win)
            assert same_bits(part, full[y0:y0 + h, x0:x0 + w]), (m, s, win)                  # a window of the whole frame's decode
        rgb = C10.random_rgb(H, W, seed=k)
        enc = yuv.encode_numpy(rgb, fmt)
        assert enc.dtype == np.uint16 and enc.shape == (fmt.frame_samples,) and np.array_equal(enc, C10.encode(rgb, m, s)), (m, s)
        assert int(enc.max()) <= 1023
    fmt = yuv.Format(H, W, depth=10)
    with pytest.raises(ValueError):
        yuv.encode_numpy(np.zeros((H, W, 3), np.uint8), fmt)                                 # uint8 into 10 bit keeps raising
    with pytest.raises(ValueError):
        yuv.encode_numpy(np.zeros((H + 1, W, 3), np.float32), fmt)
    with pytest.raises(ValueError):
        yuv.encode_numpy(np.zeros((H, W, 3), np.float32), fmt.as_8bit())                     # fp32 into 8 bit is not a thing
    with pytest.raises(ValueError):
        yuv.decode_numpy_f32(C10.random_frame(H, W, 8), fmt.as_8bit())


def test_window_refusals_of_the_twin():
    fmt = yuv.Format(10, 14, depth=10)
    buf = C10.random_frame(10, 14, 10)
    for win in ((1, 0, 4, 4), (0, 3, 4, 4)):
        with pytest.raises(ValueError, match="even"):
            yuv.decode_numpy_f32(buf, fmt, window=win)
    for win in ((8, 0, 4, 4), (0, 0, 4, 16), (0, 0, 0, 4), (-2, 0, 4, 4)):
        with pytest.raises(ValueError, match="outside"):
            yuv.decode_numpy_f32(buf, fmt, window=win)


def test_accumulators_stay_far_below_2_31_on_the_extremes():
    """Extreme samples (all 0 / all 1023 per plane, in every combination) and a random full-range frame; extreme pixels for the encode."""
    H, W = 4, 6
    n, c = H * W, 2 * 3
    for m, s in COMBOS:
        seen = []
        for ylv, ulv, vlv in itertools.product((0, 1023), repeat=3):
            buf = np.concatenate([np.full(n, ylv), np.full(c, ulv), np.full(c, vlv)]).astype(np.uint16)
            C10.decode_q(buf, H, W, m, s, track=seen)
        C10.decode_q(C10.random_frame(17, 31, 10, seed=3), 17, 31, m, s, track=seen)
        for rgb in itertools.product((0, 1023), repeat=3):
            C10.encode_q(np.broadcast_to(np.array(rgb), (H, W, 3)), m, s, track=seen)
        C10.encode_q(np.random.default_rng(4).integers(0, 1024, (17, 31, 3)), m, s, track=seen)
        print(m, s, "largest accumulator", max(seen), "= 2 ^ %.2f" % np.log2(max(seen)))
        assert max(seen) < 1 << 31
        assert max(seen) < 1 << 28          # the left-sited chroma sums are 8 pixels: 2^13 * 2^14 with signs cancelling, never near int32


def test_greys_are_neutral_and_round_trip_within_one_level():
    lv = np.arange(1024)
    for m, s in COMBOS:
        ramp = np.repeat(lv[None, :, None], 4, 0).repeat(3, 2)                  # [4,1024,3]
        fmt = yuv.Format(4, 1024, m, False, s, 10)
        enc = yuv.encode_numpy((ramp / 1023).astype(np.float32), fmt)
        assert np.array_equal(enc, C10.encode_q(ramp, m, s))
        Y, U, V = fmt.planes(enc)
        assert (U == 512).all() and (V == 512).all()                           # for all 1024 levels
        # flat greys (so that the chroma filters see one value): decode(encode(g)) within 1 level
        fm = yuv.Format(2, 2, m, False, s, 10)
        for g in range(1024):
            flat = np.full((2, 2, 3), g / 1023, np.float32)
            back = np.rint(yuv.decode_numpy_f32(yuv.encode_numpy(flat, fm), fm) * np.float32(1023)).astype(int)
            assert np.abs(back - g).max() <= 1, (m, s, g)


def test_flat_colours_round_trip_within_two_levels():
    """20 000 seeded random flat colours per (matrix, siting).  Each colour is a 2 x 2 block of a tall two-pixel-wide picture, so the
    twin encodes every block from its own four pixels (the left-sited taps clamp inside the two columns).  Decoding a FLAT frame
    upsamples constant chroma planes to themselves ((3 (4 c) + 4 c + 8) >> 4 = c), which leaves the matrix: applied here per block
    from the definition, and through the twins themselves on 200 true flat frames."""
    rng = np.random.default_rng(2024)
    cols = rng.integers(0, 1024, (20000, 3))
    for m, s in COMBOS:
        img = np.repeat(cols, 2, axis=0)[:, None, :].repeat(2, 1)                  # [2 * 20000, 2, 3]
        fm = yuv.Format(img.shape[0], 2, m, False, s, 10)
        Y, U, V = fm.planes(yuv.encode_numpy((img / 1023).astype(np.float32), fm))
        kY, kRV, kGU, kGV, kBU = C10.TABLE10[m][0]
        y, u, v = Y.astype(np.int64) - 64, (U.astype(np.int64) - 512).repeat(2, 0).repeat(2, 1), (V.astype(np.int64) - 512).repeat(2, 0).repeat(2, 1)
        r = np.clip((kY * y + kRV * v + 8192) >> 14, 0, 1023)
        g = np.clip((kY * y + kGU * u + kGV * v + 8192) >> 14, 0, 1023)
        b = np.clip((kY * y + kBU * u + 8192) >> 14, 0, 1023)
        worst = np.abs(np.stack([r, g, b], -1) - img).max()
        print(m, s, "worst round trip of 20000 flat colours:", worst, "levels")
        assert worst <= 2, (m, s, worst)
        fs = yuv.Format(4, 6, m, False, s, 10)
        for k, col in enumerate(cols[:200]):
            flat = np.broadcast_to((col / 1023).astype(np.float32), (4, 6, 3)).copy()
            bk = np.rint(yuv.decode_numpy_f32(yuv.encode_numpy(flat, fs), fs) * np.float32(1023)).astype(int)
            assert np.abs(bk - col).max() <= 2, (m, s, col)
            assert np.array_equal(bk[0, 0], [r[2 * k, 0], g[2 * k, 0], b[2 * k, 0]])       # the per-block matrix above is the twin's decode


def fl(x):
    """the float32 nearest to the rational x, ties to even"""
    c = np.float32(float(x))
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        d = abs(Fraction(float(cand)) - x)
        if best is None or d < best[0] or (d == best[0] and not (int(cand.view(np.uint32)) & 1)):
            best = (d, cand)
    return best[1]


def test_the_kernels_multiply_add_form_of_q_over_1023_is_the_fp32_division():
    """csrc/yuv_common.h writes q / 1023 as y = fl(q r), fl(y + fl(q - 1023 y) r) with r = fl(1 / 1023) and fused multiply-adds (one
    rounding each).  In exact rational arithmetic, for every q in 0..1023: the bits of the fp32 division; and the encode's pixel of
    that value is q again."""
    Fr = Fraction
    r = fl(Fr(1, 1023))
    assert float(r).hex() == "0x1.0040100000000p-10"
    src = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "yuv_common.h")).read()
    assert "0x1.00401p-10f" in src and "-1023.0f" in src                       # the kernel's constants
    plain = 0
    for q in range(1024):
        want = np.float32(q) / np.float32(1023)
        assert want.view(np.uint32) == fl(Fr(q, 1023)).view(np.uint32)
        y = fl(q * Fr(float(r)))
        e = fl(q - 1023 * Fr(float(y)))
        got = fl(Fr(float(y)) + Fr(float(e)) * Fr(float(r)))
        assert got.view(np.uint32) == want.view(np.uint32), q
        plain += int(y.view(np.uint32) != want.view(np.uint32))
        assert int(np.rint(np.float32(want * np.float32(1023)))) == q           # rint(fl32(fl32(q / 1023) * 1023)) == q
    assert plain > 0                                                            # the bare product is not enough


def test_encode_ties_and_clamps():
    """Inputs on both sides of (k + 0.5) / 1023, exact ties (half to even), and values below 0 and above 1."""
    k = np.arange(1023, dtype=np.float64)
    x = ((k + 0.5) / 1023.0).astype(np.float32)
    vals, want, tie_levels = [], [], []
    for i in range(1023):
        for v in (np.nextafter(x[i], np.float32(0)), x[i], np.nextafter(x[i], np.float32(2))):
            p = Fraction(float(np.float32(v * np.float32(1023.0))))             # fl32(x * 1023), exactly; then rint, half to even
            lo = int(p // 1)
            frac = p - lo
            lvl = lo + 1 if frac > Fraction(1, 2) else (lo if frac < Fraction(1, 2) else lo + (lo & 1))
            if frac == Fraction(1, 2):
                tie_levels.append((lo, lvl))
            vals.append(v)
            want.append(lvl)
    assert len(tie_levels) > 20 and all(lvl % 2 == 0 for _, lvl in tie_levels)                     # true ties occur; they go to even
    assert any(lvl == lo for lo, lvl in tie_levels) and any(lvl == lo + 1 for lo, lvl in tie_levels)        # ... down and up
    assert set(range(1, 1023)) <= set(want)
    for v, lvl in ((-0.0, 0), (-1e-3, 0), (-7.5, 0), (-1e30, 0), (1.0, 1023), (1.0004, 1023), (1.5, 1023), (1e30, 1023)):
        vals.append(np.float32(v))
        want.append(lvl)
    vals, want = np.array(vals, np.float32), np.array(want)
    assert np.array_equal(C10.f32_to_q(vals), want)
    # through the twin: a grey picture of those values is the encoding of the expected levels
    img = np.repeat(vals[None, :, None], 2, 0).repeat(3, 2)
    lv = np.repeat(want[None, :, None], 2, 0).repeat(3, 2)
    for m, s in COMBOS:
        fmt = yuv.Format(2, len(vals), m, False, s, 10)
        assert np.array_equal(yuv.encode_numpy(img, fmt), C10.encode_q(lv, m, s)), (m, s)


# ------------------------------------------------------------------------------------------------ ABI
def test_yuv10_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    for name in ("atmvfi_yuv_decode", "atmvfi_yuv_encode"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in hip_ops.SIGNATURES and hasattr(lib, name)
        assert lib.atmvfi_plan_fn_id(name.encode()) >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 29
    mk = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert " yuv.hip" in mk and " yuv_encode.hip" in mk
    assert callable(hip_ops.HipOps.yuv420p10_to_f32) and callable(hip_ops.HipOps.f32_to_yuv420p10)
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error

    def dec(yuv_=P, H=64, W=96, matrix=0, siting=0, y0=0, x0=0, h=64, w=96, dst=P, Hp=64, Wp=96, pt=0, pl=0):
        d = hip_ops.YuvDesc(H=H, W=W, depth=10, matrix=matrix, siting=siting)
        rc = lib.atmvfi_yuv_decode(ctypes.byref(d), yuv_, 1, 0, y0, x0, h, w, None, 0, dst, Hp, Wp, pt, pl, None)       # keep_depth
        assert rc == -1 and err().startswith(b"yuv_decode: ")           # the shared checks, under the entry point's own name
        return rc

    def enc(src=P, Hp=64, Wp=96, pt=0, pl=0, H=64, W=96, matrix=0, siting=0, yuv_=P):
        d = hip_ops.YuvDesc(H=H, W=W, depth=10, matrix=matrix, siting=siting)
        rc = lib.atmvfi_yuv_encode(ctypes.byref(d), None, 0, src, Hp, Wp, pt, pl, yuv_, None)
        assert rc == -1 and err().startswith(b"yuv_encode: ")
        return rc
    assert dec(yuv_=None) == -1 and b"null source" in err()
    assert dec(dst=None) == -1 and b"both outputs are null" in err()           # (the general message: the call has two outputs)
    assert dec(H=0) == -1 and b"at least 1" in err()
    assert dec(W=0) == -1 and b"at least 1" in err()
    assert dec(h=0) == -1 and b"at least 1" in err()
    assert dec(w=-4) == -1 and b"at least 1" in err()
    assert dec(matrix=2) == -1 and b"unknown matrix" in err()
    assert dec(siting=-1) == -1 and b"unknown siting" in err()
    assert dec(y0=2) == -1 and b"outside the" in err()
    assert dec(x0=4, w=96) == -1 and b"outside the" in err()
    assert dec(y0=-2, h=8) == -1 and b"outside the" in err()
    assert dec(y0=1, h=8) == -1 and b"must be even" in err()
    assert dec(x0=3, w=8) == -1 and b"must be even" in err()
    assert dec(Hp=63) == -1 and b"smaller than the window" in err()
    assert dec(pl=1) == -1 and b"smaller than the window" in err()
    assert dec(pt=-1) == -1 and b"smaller than the window" in err()
    assert dec(dst=P + 2) == -1 and b"4-byte aligned" in err()
    assert dec(H=100000, W=100000, h=100000, w=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()
    assert dec(x0=-2, w=8) == -1 and b"outside the" in err()                                    # (asserted for its siblings before)
    assert dec(y0=34, h=32) == -1 and b"outside the" in err()
    assert enc(src=None) == -1 and b"exactly one of src_u8 and src" in err()   # (the general message: the call has two sources)
    assert enc(yuv_=None) == -1 and b"null destination" in err()
    assert enc(H=0) == -1 and b"at least 1" in err()
    assert enc(W=-1) == -1 and b"at least 1" in err()
    assert enc(matrix=-1) == -1 and b"unknown matrix" in err()
    assert enc(siting=3) == -1 and b"unknown siting" in err()
    assert enc(Wp=95) == -1 and b"smaller than the frame" in err()
    assert enc(pt=1) == -1 and b"smaller than the frame" in err()
    assert enc(pl=-4) == -1 and b"smaller than the frame" in err()
    assert enc(src=P + 1) == -1 and b"4-byte aligned" in err()
    assert enc(H=100000, W=100000, Hp=100000, Wp=100000) == -1 and b"too large" in err()


# ------------------------------------------------------------------------------------------------ the loops, generic path
class Mean(torch.nn.Module):
    """A CPU model without the HIP backend (tests/test_yuv_cpu.py's stand-in): the pair mean."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.pairs = 0

    def forward(self, a, b):
        self.pairs += a.shape[0]
        return {"I_t": (a + b) / 2}


H, W = 24, 40
FMT8 = yuv.Format(H, W, "bt709", False, "left")
FMT = yuv.Format(H, W, "bt709", False, "left", 10)


def ten_bit(frames_rgb, seed):
    """10-bit I420 frames of a uint8 RGB shot: encoded at 10 bits, with the two low bits of every sample filled at random so that
    nothing about them is 8-bit material"""
    rng = np.random.default_rng(seed)
    out = []
    for f in frames_rgb:
        v = yuv.encode_numpy((f.astype(np.float32) / np.float32(255)), FMT)
        out.append(((v & ~np.uint16(3)) | rng.integers(0, 4, v.shape).astype(np.uint16)).astype(np.uint16))
    return out


SHOT_A = ten_bit(CS.shot(5, H, W, seed=1, tone=60), 1)
SHOT_B = ten_bit(CS.shot(5, H, W, seed=2, tone=190), 2)


def twin_chain(a, b, factor, window, tta=False):
    """The produced frames of one segment from the numpy twins and the same fp32 arithmetic as the generic loop: decode the window,
    recursive pair means (Mean() is the model: padding and flips change nothing about a per-pixel mean), encode."""
    y0, x0, h, w = window
    fr = {0: yuv.decode_numpy_f32(a, FMT, window=window), factor: yuv.decode_numpy_f32(b, FMT, window=window)}
    for level in mf.nx_levels(factor):
        for l, r, o in level:
            fr[o] = ((torch.from_numpy(fr[l]) + torch.from_numpy(fr[r])) / 2).numpy()
    out = []
    for pos in range(1, factor):
        p = torch.from_numpy(fr[pos])
        if tta:
            p = (p + p) / 2
        out.append(yuv.encode_numpy(p.numpy(), FMT.cropped(h, w)))
    return out


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("kw", [dict(), dict(time_interval=2), dict(crop=(16, 32)), dict(tta=True), dict(time_interval=2, crop=(16, 32))],
                         ids=lambda k: "-".join(k) or "plain")
def test_loops_keep_the_depth_through_the_generic_path(factor, kw):
    video = SHOT_A + SHOT_B
    keep = [v.copy() for v in video]
    window = y0, x0, h, w = mf.centre_window(H, W, kw.get("crop"))
    out_fmt = FMT.cropped(h, w)
    s = kw.get("time_interval", 1)
    for sc_deep, sc_8 in ((None, None), (scene.SceneCuts(), scene.SceneCuts())):
        model = Mean()
        got = list(mf.interpolate_video_nx(iter(video), model, factor=factor, pixfmt=FMT, scene=sc_deep, keep_depth=True, **kw))
        ref_model = Mean()
        ref = list(mf.interpolate_video_nx(iter(video), ref_model, factor=factor, pixfmt=FMT, scene=sc_8, **kw))        # the 8-bit path
        n_seg = (len(video) - 1) // s
        assert len(got) == len(ref) == factor * n_seg + 1 and model.pairs == ref_model.pairs
        cut = set()
        if sc_deep is not None:             # signatures, and so cut decisions, are those of the 8-bit path
            assert sc_deep.cuts == sc_8.cuts == [(len(SHOT_A) - 1) // s] and sc_deep.stats == sc_8.stats
            cut = set(sc_deep.cuts)
        for seg in range(n_seg):
            a, b = video[seg * s], video[(seg + 1) * s]
            g = got[seg * factor:(seg + 1) * factor]
            assert np.array_equal(g[0], yuv.crop(a, FMT, y0, x0, h, w)) and g[0].dtype == np.uint16       # an original
            if kw.get("crop") is None:
                assert g[0] is a                                                                          # ... by identity
            if seg in cut:                                                                                # copies of the 10-bit originals
                for pos in range(1, factor):
                    src = a if pos <= factor // 2 else b
                    assert g[pos] is not src and g[pos].dtype == np.uint16 and np.array_equal(g[pos], yuv.crop(src, FMT, y0, x0, h, w))
            else:
                want = twin_chain(a, b, factor, window, tta=bool(kw.get("tta")))
                for pos in range(1, factor):
                    assert g[pos].dtype == np.uint16 and g[pos].shape == (out_fmt.frame_samples,)
                    assert np.array_equal(g[pos], want[pos - 1]), (seg, pos)
                    assert ref[seg * factor + pos].dtype == np.uint8                                      # the default stays 8-bit
        last = got[-1]
        assert np.array_equal(last, yuv.crop(video[n_seg * s], FMT, y0, x0, h, w))
        if kw.get("crop") is None:
            assert last is video[n_seg * s]
    assert all(np.array_equal(a, b) for a, b in zip(video, keep))        # the caller's buffers are untouched


def test_keep_depth_changes_nothing_for_eight_bit_or_rgb_frames():
    rgb = CS.shot(4, H, W, seed=3, tone=90)
    video8 = [yuv.encode_numpy(f, FMT8) for f in rgb]
    for frames, kw in ((video8, dict(pixfmt=FMT8)), (rgb, dict(isBGR=False))):
        for extra in (dict(), dict(crop=(16, 32), tta=True)):
            a = list(mf.interpolate_video_nx(iter(frames), Mean(), factor=4, **kw, **extra))
            b = list(mf.interpolate_video_nx(iter(frames), Mean(), factor=4, keep_depth=True, **kw, **extra))
            assert len(a) == len(b) == 13 and all(x.dtype == y.dtype == np.uint8 and np.array_equal(x, y) for x, y in zip(a, b))
    # ... and the default for 10-bit input is what it was: 8-bit produced frames
    a = list(mf.interpolate_video_nx(iter(SHOT_A[:3]), Mean(), factor=2, pixfmt=FMT))
    b = list(mf.interpolate_video_nx(iter(SHOT_A[:3]), Mean(), factor=2, pixfmt=FMT, keep_depth=False))
    assert [x.dtype for x in a] == [np.uint16, np.uint8, np.uint16, np.uint8, np.uint16] and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_keep_depth_defaults_to_false_in_every_signature():
    for fn in (host_io.interpolate_video_2x, host_io.interpolate_video_nx, mf.interpolate_video_nx, host_io.FramePipeline.__init__,
               yuv.interpolate_y4m):
        assert inspect.signature(fn).parameters["keep_depth"].default is False, fn
    # video_2x / video_nx hand it on through **kw
    for fn in (host_io.video_2x, mf.video_nx):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(fn).parameters.values()), fn
    tool = open(os.path.join(CS.ROOT, "tools", "interp_y4m.py")).read()
    assert '"--keep-depth"' in tool and "keep_depth=a.keep_depth" in tool


class Cap:
    """cv2.VideoCapture's read() / get() over a list of frames"""

    def __init__(self, frames, fps=25):
        self.frames, self.k, self.fps, self.released = frames, 0, fps, False

    def isOpened(self):
        return True

    def read(self):
        if self.k >= len(self.frames):
            return False, None
        self.k += 1
        return True, self.frames[self.k - 1]

    def get(self, prop):
        return {host_io.CAP_PROP_FPS: self.fps, host_io.CAP_PROP_FRAME_WIDTH: W, host_io.CAP_PROP_FRAME_HEIGHT: H}[prop]

    def release(self):
        self.released = True


def test_video_nx_hands_keep_depth_on():
    seen = {}

    def interp(frames, model, **kw):
        seen.update(kw)
        return iter(())

    class Sink:
        def write(self, f):
            pass

        def release(self):
            pass
    mf.video_nx(Cap([]), lambda rate, size: Sink(), Mean(), factor=4, interpolator=interp, keep_depth=True, pixfmt=FMT)
    assert seen["keep_depth"] is True and seen["pixfmt"] is FMT
    seen.clear()
    host_io.video_2x(Cap([]), lambda rate, size: Sink(), Mean(), interpolator=interp, keep_depth=True, pixfmt=FMT)
    assert seen["keep_depth"] is True


@pytest.mark.parametrize("factor,kw", [(2, {}), (4, {}), (2, dict(crop=(16, 32))), (4, dict(time_interval=2))])
def test_interpolate_y4m_keeps_c420p10(factor, kw):
    fmt = yuv.Format(H, W, "bt601", False, "centre", 10)           # what a C420p10 header says (24 rows: bt601 by height)
    video = [v.copy() for v in SHOT_A]
    src, dst = io.BytesIO(), io.BytesIO()
    wr = yuv.Y4MWriter(src, fmt, Fraction(30000, 1001), aspect="4:3")
    for f in video:
        wr.write(f)
    src.seek(0)
    called = []
    orig = yuv.to_8bit
    yuv.to_8bit = lambda *a, **k: called.append(1) or orig(*a, **k)
    try:
        info = yuv.interpolate_y4m(src, dst, Mean(), factor=factor, keep_depth=True, **kw)
    finally:
        yuv.to_8bit = orig
    assert not called                                              # nothing is re-quantised
    s = kw.get("time_interval", 1)
    y0, x0, h, w = mf.centre_window(H, W, kw.get("crop"))
    n_out = factor * ((len(video) - 1) // s) + 1
    assert info == {"fps_in": Fraction(30000, 1001), "fps_out": Fraction(30000, 1001) * factor / s, "size": (w, h),
                    "frames_in": len(video), "frames_out": n_out}
    dst.seek(0)
    rd = yuv.Y4MReader(dst)
    assert rd.fmt == fmt.cropped(h, w) and rd.ctag == "420p10" and rd.fps == Fraction(30000 * factor, 1001 * s) and rd.aspect == "4:3"
    got = list(rd)
    want = list(mf.interpolate_video_nx(iter(video), Mean(), factor=factor, pixfmt=fmt, keep_depth=True, **kw))
    assert len(got) == len(want) == n_out and all(g.dtype == np.uint16 and np.array_equal(g, w_) for g, w_ in zip(got, want))
    for k in range(0, n_out, factor):                              # originals: the input's bytes
        assert got[k].astype("<u2").tobytes() == yuv.crop(video[k // factor * s], fmt, y0, x0, h, w).astype("<u2").tobytes()
    if not kw:                                                     # uncropped: every original frame record is byte-equal to the input's
        rec = 6 + fmt.frame_bytes
        head_in, head_out = len(src.getvalue().split(b"\n", 1)[0]) + 1, len(dst.getvalue().split(b"\n", 1)[0]) + 1
        for k in range(len(video)):
            assert dst.getvalue()[head_out + k * factor * rec:head_out + (k * factor + 1) * rec] == src.getvalue()[head_in + k * rec:head_in + (k + 1) * rec]
    # without keep_depth the same stream still comes back 8-bit
    src.seek(0)
    dst8 = io.BytesIO()
    yuv.interpolate_y4m(src, dst8, Mean(), factor=factor, **kw)
    dst8.seek(0)
    rd8 = yuv.Y4MReader(dst8)
    assert rd8.fmt == fmt.as_8bit().cropped(h, w) and rd8.ctag == "420jpeg"


def test_a_smooth_ten_bit_ramp_keeps_more_than_256_luma_levels():
    """The point of the feature: a smooth 10-bit grey ramp clip.  With ``keep_depth`` the produced frames carry more than 256 distinct
    Y values; without it they cannot (8-bit samples)."""
    h, w = 16, 1024
    fmt = yuv.Format(h, w, "bt709", False, "centre", 10)
    frames = []
    for shift in (0, 1, 2):          # a ramp over every 10-bit grey, drifting by one level per frame
        lv = np.clip(np.arange(w) + shift, 0, 1023)
        img = np.repeat(lv[None, :, None], h, 0).repeat(3, 2)
        frames.append(yuv.encode_numpy((img / 1023).astype(np.float32), fmt))
    assert len(np.unique(fmt.planes(frames[0])[0])) > 800
    deep = list(mf.interpolate_video_nx(iter(frames), Mean(), factor=2, pixfmt=fmt, keep_depth=True))
    flat = list(mf.interpolate_video_nx(iter(frames), Mean(), factor=2, pixfmt=fmt))
    for k in (1, 3):
        n_deep = len(np.unique(fmt.planes(deep[k])[0]))
        n_flat = len(np.unique(fmt.as_8bit().planes(flat[k])[0]))
        print(f"produced frame {k}: {n_deep} distinct Y values with keep_depth, {n_flat} without")
        assert deep[k].dtype == np.uint16 and n_deep > 256
        assert flat[k].dtype == np.uint8 and n_flat <= 256
        U, V = fmt.planes(deep[k])[1:]
        assert (U == 512).all() and (V == 512).all()
