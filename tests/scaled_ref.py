"""Half-resolution motion (atm-vfi_amd/scaled.py, atmvfi_frame_half / atmvfi_synth_up2): a float64 reference of the synthesis with an
ELEMENTWISE error bound derived from the kernel's fp32 arithmetic, an fp32 emulation of that arithmetic with switchable mutants (built on
warp_ref's taps, not on the package's twin), and the hostile input families.  Built on warp_ref.py and pointwise_ref.py.

THE BOUND.  U = 2^-24; one fp32 rounding of x errs by at most U |x|; g(n) = n U / (1 - n U) bounds n roundings in a row ((1 + U)^n - 1).
Inputs (the half-size maps, the full-size frames) are fp32 numbers taken as exact.  Every step carries (value64, error bound):
  residual at a half-size pixel   r = s - (m1 a + q c), q = fl(1 - m1):  e_q = U |1 - m1|;  the two products, the sum and the subtraction
                                  each add U |their result| (products and sums of bounded operands: ``_mul``, ``_add``);
  x2 up-sampling                  v = sum of four w_ij v_ij with exact weights (0.0625 .. 0.5625, sum 1).  A tap passes through at most four
                                  roundings (wx v, the row sum, wy (.), the final sum): g(4) sum |w_ij v_ij|, plus the same convex
                                  combination of the taps' own bounds;
  flows                           doubling is exact: e_f = 2 e_up(flow);
  coordinate                      the kernel's sampling coordinate differs from the exact p = x + f by e_f plus warp_ref.delta at |p| + e_f
                                  (ref_coord's five roundings; delta is monotone in |p|) -- delta carries warp_bound's only slack (4 |p| for
                                  3 |p|), nothing is added here;
  sample                          warp_ref.warp_bound with that coordinate error: (delta + e_f) x the neighbourhood slopes + 6 U S + U |w00 tap00|;
                                  0 where a coordinate is not finite (the contract there is 0.0 exactly);
  blend                           (m a + (1 - m) c) + r with e_m = e_up(m1), e_(1-m) = e_m + U |1 - m|: two products, two sums (``_mul``, ``_add``);
  clamp                           1-Lipschitz: the bound passes through.
Second-order terms are kept (``_mul`` multiplies the bounds out), so no slack is needed for them."""
import importlib

import numpy as np

import warp_ref as WR

U = WR.U
F32 = np.float32
scaled = importlib.import_module("atm-vfi_amd.scaled")


def g(n: int) -> float:
    return n * U / (1.0 - n * U)


def _mul(x, ex, y, ey):
    """fl(x~ y~) for |x~ - x| <= ex, |y~ - y| <= ey -> (x y, bound)."""
    e = np.abs(x) * ey + np.abs(y) * ex + ex * ey
    return x * y, e + U * (np.abs(x * y) + e)


def _add(x, ex, y, ey, sign=1.0):
    e = ex + ey
    return x + sign * y, e + U * (np.abs(x + sign * y) + e)


def taps(n: int):
    """The x2 rule restated here, output index by output index (nothing of the package): -> (i0, i1, w0, w1) for x = 0 .. 2n - 1."""
    i0, i1, w0, w1 = [], [], [], []
    for x in range(2 * n):
        if x % 2 == 0:
            i0.append(max(x // 2 - 1, 0)); i1.append(x // 2); w0.append(0.25); w1.append(0.75)
        else:
            i0.append((x - 1) // 2); i1.append(min((x + 1) // 2, n - 1)); w0.append(0.75); w1.append(0.25)
    return np.asarray(i0), np.asarray(i1), np.asarray(w0, F32), np.asarray(w1, F32)


def up2_64(v: np.ndarray, ev=None):
    """[...,h,w] float64 -> (value, bound) [...,2h,2w] of the kernel's x2 up-sampling."""
    r0, r1, wy0, wy1 = taps(v.shape[-2])
    c0, c1, wx0, wx1 = taps(v.shape[-1])
    wy0, wy1, wx0, wx1 = (a.astype(np.float64) for a in (wy0[:, None], wy1[:, None], wx0, wx1))

    def comb(t):
        return wy0 * (wx0 * t[..., r0, :][..., c0] + wx1 * t[..., r0, :][..., c1]) + wy1 * (wx0 * t[..., r1, :][..., c0] + wx1 * t[..., r1, :][..., c1])
    with np.errstate(invalid="ignore", over="ignore"):
        out, mag = comb(v), comb(np.abs(v))
        bound = g(4) * mag + (comb(ev) if ev is not None else 0.0)
    return out, bound


def residual64(half: dict):
    s, a, c, m1 = (np.asarray(half[k], np.float64) for k in ("it_sum", "I_t_0", "I_t_1", "occ_mask1"))
    q, eq = 1.0 - m1, U * np.abs(1.0 - m1)
    p1, e1 = _mul(m1, 0.0, a, 0.0)
    p2, e2 = _mul(q, eq, c, 0.0)
    bl, eb = _add(p1, e1, p2, e2)
    return _add(s, 0.0, bl, eb, -1.0)


def _sample64(frames: np.ndarray, f: np.ndarray, ef: np.ndarray):
    """flow_warp of ``frames`` [B,3,H,W] by the float64 flow f [B,2,H,W] known to ef -> (value, bound, dead)."""
    _, _, h, w = frames.shape
    ref = WR.warp64(frames, f)
    with np.errstate(invalid="ignore", over="ignore"):
        efx, efy = np.where(ref["dead"], 0.0, ef[:, 0]), np.where(ref["dead"], 0.0, ef[:, 1])
        dx = WR.delta(np.abs(ref["px"]) + efx, w) + efx
        dy = WR.delta(np.abs(ref["py"]) + efy, h) + efy
        bound = dx[:, None] * ref["Dx"] + dy[:, None] * ref["Dy"] + 6 * U * ref["S"] + U * ref["T00"]
    return ref["v"], np.where(ref["dead"][:, None], 0.0, bound), ref["dead"]


def synth64(half: dict, store0: np.ndarray, store1: np.ndarray, slots0=None, slots1=None) -> dict:
    """-> {"I_t": (v, bound), "opt_flow_0": ..., "opt_flow_1": ..., "occ_mask1": ..., "dead": [B,H,W] "a flow of the pixel is not finite"}.
    ``half``: fp32 arrays it_sum, I_t_0, I_t_1 [B,3,h,w], opt_flow_0/1 [B,2,h,w], occ_mask1 [B,1,h,w]."""
    b = half["it_sum"].shape[0]
    left = store0[list(range(b)) if slots0 is None else list(slots0)]
    right = store1[list(range(b)) if slots1 is None else list(slots1)]
    out = {}
    flows = []
    for k in ("opt_flow_0", "opt_flow_1"):
        v, e = up2_64(np.asarray(half[k], np.float64))
        flows.append((2.0 * v, 2.0 * e))
        out[k] = flows[-1]
    m, em = up2_64(np.asarray(half["occ_mask1"], np.float64))
    out["occ_mask1"] = (m, em)
    r, er = up2_64(*residual64(half))
    a, ea, dead_a = _sample64(left, *flows[0])
    c, ec, dead_c = _sample64(right, *flows[1])
    with np.errstate(invalid="ignore", over="ignore"):
        p1, e1 = _mul(m, em, a, ea)
        p2, e2 = _mul(1.0 - m, em + U * np.abs(1.0 - m), c, ec)
        bl, eb = _add(p1, e1, p2, e2)
        v, ev = _add(bl, eb, r, er)
    out["I_t"] = (np.clip(v, 0.0, 1.0), ev)
    out["dead"] = dead_a | dead_c
    return out


# ------------------------------------------------------------------------------------------------------------------- the fp32 emulation
MUTANTS = ("flow_not_doubled", "align_corners", "nearest_mask", "no_residual", "mask_swapped", "edge_unclamped")


def _up2_32(t: np.ndarray, mutant=None) -> np.ndarray:
    t = t.astype(F32)
    if mutant == "align_corners":
        return WR.resize32(t, 2 * t.shape[-2], 2 * t.shape[-1])
    if mutant == "nearest":
        return np.repeat(np.repeat(t, 2, axis=-2), 2, axis=-1)

    def taps_of(n):
        i0, i1, w0, w1 = taps(n)
        if mutant == "edge_unclamped":               # x/2 - 1 and (x + 1)/2 as they are: -1 and n wrap around the row
            x = np.arange(2 * n)
            i0, i1 = np.where(x & 1, (x - 1) // 2, x // 2 - 1) % n, np.where(x & 1, (x + 1) // 2, x // 2) % n
        return i0, i1, w0, w1
    r0, r1, wy0, wy1 = taps_of(t.shape[-2])
    c0, c1, wx0, wx1 = taps_of(t.shape[-1])
    with np.errstate(invalid="ignore", over="ignore"):
        top = (wx0 * t[..., r0, :][..., c0] + wx1 * t[..., r0, :][..., c1]).astype(F32)
        bot = (wx0 * t[..., r1, :][..., c0] + wx1 * t[..., r1, :][..., c1]).astype(F32)
        return (wy0[:, None] * top + wy1[:, None] * bot).astype(F32)


def synth32(half: dict, store0: np.ndarray, store1: np.ndarray, slots0=None, slots1=None, mutant=None) -> dict:
    """The kernel's arithmetic, one fp32 rounding per operation, the warps by warp_ref.warp32."""
    b = half["it_sum"].shape[0]
    left = store0[list(range(b)) if slots0 is None else list(slots0)]
    right = store1[list(range(b)) if slots1 is None else list(slots1)]
    s, a0, c0, m1 = (half[k].astype(F32) for k in ("it_sum", "I_t_0", "I_t_1", "occ_mask1"))
    one = F32(1.0)
    upm = mutant if mutant in ("align_corners", "edge_unclamped") else None
    scale = one if mutant == "flow_not_doubled" else F32(2.0)
    with np.errstate(invalid="ignore", over="ignore"):
        res = (s - (m1 * a0 + (one - m1) * c0)).astype(F32)
        f0 = (_up2_32(half["opt_flow_0"], upm) * scale).astype(F32)
        f1 = (_up2_32(half["opt_flow_1"], upm) * scale).astype(F32)
        m = _up2_32(m1, "nearest" if mutant == "nearest_mask" else upm)
        r = np.zeros_like(left) if mutant == "no_residual" else _up2_32(res, upm)
        a, c = WR.warp32(left, f0), WR.warp32(right, f1)
        if mutant == "mask_swapped":
            a, c = c, a
        v = ((m * a + (one - m) * c) + r).astype(F32)
        it = np.fmin(np.fmax(v, F32(0.0)), one).astype(F32)
    return {"I_t": it, "opt_flow_0": f0, "opt_flow_1": f1, "occ_mask1": m}


# ----------------------------------------------------------------------------------------------------------------------- input families
FLOW_FAMILIES = ("gauss", "const_int", "const_ulp", "blocks", "outside", "wild", "far")
FINITE_FAMILIES = FLOW_FAMILIES[:5] + ("far",)
MASK_FAMILIES = ("rand", "zeros", "ones", "binary")


def half_flow(name: str, b: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[b,2,h,w] fp32 HALF-SIZE flows (the full-size flow is twice their up-sampling; a constant c up-samples to c exactly).
    gauss: sigma 3.  const_int: one constant k / 2 per sample and axis, k an integer in -3 .. 3: every full-size tap lies exactly on a
    pixel.  const_ulp: the same one fp32 ulp up or down (a zero stays zero: its neighbours are subnormal, where a rounding's error is
    absolute and the bound's relative model does not apply).  blocks: 3 x 3 blocks of constants k / 2 +- ulp over +-(size + 2) (exact inside a
    block, blended across its borders; targets on -1, size - 1, size and beyond).  outside: constants that put every target beyond
    (-1, size) on one axis.  wild: gauss with 6 % of the pixels' components from warp_ref.WILD_VALUES (NaN, +-Inf, +-3e38, 2^31 ...).  far:
    zero flow with one pixel in eight thrown 20 .. 60 half-pixels away (tiles whose taps leave the staged box, mixed with near ones)."""
    rng = np.random.default_rng([FLOW_FAMILIES.index(name), b, h, w, seed])
    if name == "gauss":
        return rng.normal(0.0, 3.0, (b, 2, h, w)).astype(F32)
    if name in ("const_int", "const_ulp"):
        f = np.broadcast_to((rng.integers(-3, 4, (b, 2, 1, 1)) * 0.5).astype(F32), (b, 2, h, w)).copy()
        if name == "const_ulp":
            f = np.where(f == 0, f, np.nextafter(f, np.where(rng.integers(0, 2, (b, 2, 1, 1)) == 1, np.inf, -np.inf).astype(F32)))
        return f
    if name == "blocks":
        f = np.zeros((b, 2, h, w), F32)
        for axis, size in ((0, 2 * w), (1, 2 * h)):
            for y0 in range(0, h, 3):
                for x0 in range(0, w, 3):
                    k = (rng.integers(-(size + 2), size + 3, b) * 0.5).astype(F32)
                    k = np.where(k == 0, k, np.nextafter(k, np.asarray([-np.inf, 0.0, np.inf], F32)[rng.integers(0, 3, b)] + k))
                    f[:, axis, y0:y0 + 3, x0:x0 + 3] = k[:, None, None]
        return f
    if name == "outside":
        f = rng.normal(0.0, 1.0, (b, 2, h, w)).astype(F32)
        f[:, 0] += np.where(rng.integers(0, 2, (b, 1, 1)) == 1, w + 1.0, -(w + 1.0)).astype(F32)
        return f
    if name == "wild":
        f = rng.normal(0.0, 3.0, (b, 2, h, w)).astype(F32)
        hit = rng.random((b, 2, h, w)) < 0.06
        vals = np.asarray(WR.WILD_VALUES, F32)[rng.integers(0, len(WR.WILD_VALUES), (b, 2, h, w))]
        return np.where(hit, vals, f).astype(F32)
    if name == "far":
        f = np.zeros((b, 2, h, w), F32)
        hit = rng.random((b, 1, h, w)) < 0.125
        jump = (rng.integers(20, 61, (b, 2, h, w)) * np.where(rng.integers(0, 2, (b, 2, h, w)) == 1, 1, -1)).astype(F32)
        return np.where(hit, jump, f).astype(F32)
    raise ValueError(name)


def half_mask(name: str, b: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng([MASK_FAMILIES.index(name), b, h, w, seed, 77])
    if name == "rand":
        return rng.random((b, 1, h, w)).astype(F32)
    if name == "zeros":
        return np.zeros((b, 1, h, w), F32)
    if name == "ones":
        return np.ones((b, 1, h, w), F32)
    return rng.integers(0, 2, (b, 1, h, w)).astype(F32)


def make_case(b: int, h: int, w: int, flow: str = "gauss", mask: str = "rand", stores: int = None, residual: float = 1.5, seed: int = 0,
              flow1: str = None) -> dict:
    """One synthetic call: half-size maps as a forward would return them (it_sum = blend of the half-size warps + a residual uniform in
    +-``residual``, which drives the sum outside [0, 1]; ``flow1``: the second flow's family, default ``flow``) and two full-size stores of ``stores`` (default b) random frames.
    -> {"half": dict of fp32 arrays, "store0", "store1"}."""
    rng = np.random.default_rng([b, h, w, seed, 5])
    s = b if stores is None else stores
    m1 = half_mask(mask, b, h, w, seed)
    a, c = rng.random((b, 3, h, w)).astype(F32), rng.random((b, 3, h, w)).astype(F32)
    it_sum = (m1 * a + (F32(1.0) - m1) * c + rng.uniform(-residual, residual, (b, 3, h, w)).astype(F32)).astype(F32)
    half = {"it_sum": it_sum, "I_t_0": a, "I_t_1": c, "opt_flow_0": half_flow(flow, b, h, w, seed), "opt_flow_1": half_flow(flow1 or flow, b, h, w, seed + 1),
            "occ_mask1": m1}
    return {"half": half, "store0": rng.random((s, 3, 2 * h, 2 * w)).astype(F32), "store1": rng.random((s, 3, 2 * h, 2 * w)).astype(F32)}


def as_forward_dict(half: dict) -> dict:
    """The arrays of ``make_case`` under the keys of ``forward``'s dict (what scaled.synth_up2_numpy and HipOps.synth_up2 take)."""
    return {"im_t_list": [half["it_sum"]], **{k: half[k] for k in ("I_t_0", "I_t_1", "opt_flow_0", "opt_flow_1", "occ_mask1")}}


def worst(got: dict, ref: dict) -> dict:
    """Worst error / bound ratio per output (inf: NaN in ``got`` or an error where the bound is 0).  A flow output whose exact value is
    not finite must be non-finite too (inf ratio otherwise); one beyond fp32's range is not compared."""
    out = {}
    for k in ("I_t", "opt_flow_0", "opt_flow_1", "occ_mask1"):
        if k not in got:
            continue
        g_, v, e = np.asarray(got[k]), ref[k][0], ref[k][1]
        if k.startswith("opt_flow"):
            lost = ~np.isfinite(v)
            if np.isfinite(g_[lost]).any():
                out[k] = float("inf")
                continue
            skip = lost | (np.abs(np.where(lost, 0.0, v)) > float(np.finfo(F32).max))
            g_, v, e = np.where(skip, 0.0, g_), np.where(skip, 0.0, v), np.where(skip, 0.0, e)
        out[k] = WR.worst_ratio(g_, v, e)
    return out


def tie_pixels() -> np.ndarray:
    """fp32 values p_k, k = 0 .. 254, with fl(p_k * 255) == k + 0.5 exactly: frame_f32_to_u8's ties (half to even)."""
    out = []
    for k in range(255):
        p = F32((k + 0.5) / 255.0)
        cands = [p]
        for _ in range(4):
            cands += [np.nextafter(cands[-1], F32(2.0)), np.nextafter(cands[0], F32(-1.0))]
            cands.sort()
        hit = [q for q in cands if F32(q * F32(255.0)) == F32(k + 0.5)]
        if hit:
            out.append(hit[0])
    return np.asarray(out, F32)
