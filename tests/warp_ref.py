"""Plain float64 references of the warp and resize kernels (flow_warp in all its forms, warp_blend's samples and blend, the
align_corners=True resize, the flow up-sampling of flow_warp_up2, the image pyramid), the ELEMENTWISE error bounds that follow from the
kernels' fp32 arithmetic, an fp32 emulation of that arithmetic (numpy, one rounding per operation, with switchable mutants), the
staged-box rule of the tiled warps restated in Python, and the hostile input families.  No grid_sample, no F.interpolate and nothing of
the package is used in here: the references are explicit gathers.  See "fp64 bounds of the warp and resize kernels" in DESIGN_NOTES.md.

Arrays are numpy: images [B,C,H,W], flows [B,2,H,W] (x, y); the GPU tests convert at their boundary."""
import numpy as np
import torch

import pointwise_ref as R

U = R.U                                       # 2^-24: the relative error of one fp32 rounding to nearest
F32 = np.float32
PADDINGS = ("zeros", "border", "reflection")
NB = 3                                        # padding of the extended image: the 4 x 4 neighbourhood of floor -2 .. size reaches -3 .. size + 2


# ------------------------------------------------------------------------------------------------------------------ the extended image
def extend(src: np.ndarray, padding: str) -> np.ndarray:
    """[B,C,H,W] float64 -> [B,C,H+2 NB,W+2 NB]: the image as the padding mode continues it over the plane (zeros; the border pixel
    repeated; mirrored about the centres of the border pixels)."""
    mode = {"zeros": "constant", "border": "edge", "reflection": "reflect"}[padding]
    return np.pad(src.astype(np.float64), ((0, 0), (0, 0), (NB, NB), (NB, NB)), mode=mode)


def neighbourhood(ext: np.ndarray, x0: np.ndarray, y0: np.ndarray) -> np.ndarray:
    """ext [B,C,Hp,Wp] (extended by NB), x0 / y0 integer [B,Ho,Wo] -> [B,C,Ho,Wo,4,4]: rows y0-1 .. y0+2, columns x0-1 .. x0+2."""
    b = np.arange(ext.shape[0])[:, None, None, None, None]
    yy = (y0 + NB)[..., None, None] + np.arange(-1, 3)[:, None]
    xx = (x0 + NB)[..., None, None] + np.arange(-1, 3)[None, :]
    return np.moveaxis(ext[b, :, yy, xx], -1, 1)


def interpolate(ext: np.ndarray, px: np.ndarray, py: np.ndarray, w: int, h: int):
    """Bilinear interpolation of the extended image at float64 coordinates [B,Ho,Wo] (already mapped by the padding mode; anything
    beyond floor -2 .. size lies in the constant part of the extension and is moved there).
    -> v, S = sum |weight tap|, Dx, Dy (largest |horizontal| / |vertical| neighbour difference over the 4 x 4 neighbourhood of the
    taps), T00 = |w00 tap00|, each [B,C,Ho,Wo]."""
    px, py = np.clip(px, -2.0, w + 0.5), np.clip(py, -2.0, h + 0.5)
    fx, fy = np.floor(px), np.floor(py)
    ax, ay = (px - fx)[:, None], (py - fy)[:, None]
    blk = neighbourhood(ext, fx.astype(np.int64), fy.astype(np.int64))
    t00, t01 = (1 - ax) * (1 - ay) * blk[..., 1, 1], ax * (1 - ay) * blk[..., 1, 2]
    t10, t11 = (1 - ax) * ay * blk[..., 2, 1], ax * ay * blk[..., 2, 2]
    v = t00 + t01 + t10 + t11
    s = np.abs(t00) + np.abs(t01) + np.abs(t10) + np.abs(t11)
    dx = np.abs(blk[..., :, 1:] - blk[..., :, :-1]).max(axis=(-1, -2))
    dy = np.abs(blk[..., 1:, :] - blk[..., :-1, :]).max(axis=(-1, -2))
    return v, s, dx, dy, np.abs(t00)


# ------------------------------------------------------------------------------------------------------------------------------- warps
def coords64(flow: np.ndarray):
    """The sampling coordinates x + double(flow_x), y + double(flow_y), [B,H,W] each: no normalisation round trip."""
    _, _, h, w = flow.shape
    return np.arange(w)[None, None, :] + flow[:, 0].astype(np.float64), np.arange(h)[None, :, None] + flow[:, 1].astype(np.float64)


def reflect64(c: np.ndarray, size: int) -> np.ndarray:
    """Reflection about 0 and size - 1 (grid_sample's reflect_coordinates for align_corners=True), float64."""
    span = float(size - 1)
    a = np.abs(c)
    extra, flips = np.fmod(a, span), np.floor(a / span)
    return np.where(np.fmod(flips, 2.0) == 1.0, span - extra, extra)


def delta(p: np.ndarray, size: int, reflection: bool = False) -> np.ndarray:
    """Bound on the kernel's sampling coordinate minus the exact p, from ref_coord's arithmetic (warp.hip ``ref_coord``, and the
    same expression in flow_warp_ex_kernel):  g = 2 p / (size - 1) - 1,  ix = ((g + 1) / 2) (size - 1).  Five roundings (2 p and / 2
    are exact): the add x + flow (U |p|), the division (U |g + 1| in g, i.e. U |g + 1| (size - 1) / 2 in pixels), the -1 (U |g|), the
    +1 (U |g + 1|) and the multiplication (U |p|); with |g + 1| (size - 1) / 2 = |p| their first-order sum is
        U (4 |p| + |g| (size - 1) / 2)  =  U (3 |p| + (|g| + |g + 1|) (size - 1) / 2)
    and the bound takes 4 |p| for the 3 |p| of the second form as its only slack (it pays for the second-order terms).
    ix - floor(ix) is exact.  The border and reflection maps do not stretch distances; reflection's ``hi - extra`` is one more rounding
    of a value <= |c|: U |c|."""
    p = np.abs(p)
    g = 2.0 * p / (size - 1) - 1.0
    d = U * (4.0 * p + (np.abs(g) + np.abs(g + 1.0)) * (size - 1) / 2.0)
    return d + U * p if reflection else d


def warp64(src: np.ndarray, flow: np.ndarray, padding: str = "zeros"):
    """-> dict(v, S, Dx, Dy, T00 [B,C,H,W]; px, py the exact coordinates and dead = "a coordinate is not finite" [B,H,W]).
    zeros: bilinear interpolation of the image extended by zeros, a continuous function of the plane: 0.0 at or beyond -1 and size and
    at a non-finite coordinate.  border: clip to [0, size - 1], then interpolate.  reflection: reflect about 0 and size - 1, clip,
    interpolate."""
    _, _, h, w = src.shape
    px, py = coords64(flow)
    dead = ~(np.isfinite(px) & np.isfinite(py))
    qx, qy = np.where(dead, -2.0, px), np.where(dead, -2.0, py)
    if padding == "reflection":
        qx, qy = reflect64(qx, w), reflect64(qy, h)
    if padding != "zeros":
        qx, qy = np.clip(qx, 0.0, w - 1.0), np.clip(qy, 0.0, h - 1.0)
    v, s, dx, dy, t00 = interpolate(extend(src, padding), qx, qy, w, h)
    if padding == "zeros":
        v, s, t00 = (np.where(dead[:, None], 0.0, t) for t in (v, s, t00))
    return {"v": v, "S": s, "Dx": dx, "Dy": dy, "T00": t00, "px": px, "py": py, "dead": dead}


def warp_bound(ref: dict, w: int, h: int, padding: str = "zeros") -> np.ndarray:
    """bound = delta_x Dx + delta_y Dy + 6 U S + U |w00 tap00|, elementwise.
    The first two: the value moves by at most the coordinate error times the steepest slope nearby (bilinear interpolation is
    piecewise linear with slopes <= the neighbour differences; the 4 x 4 neighbourhood covers a coordinate that crosses into the next
    cell).  6 U S: per tap two roundings of the weight, one of weight x tap, and the three additions of sample_plane (the first
    ``v += `` adds to zero).  U |w00 tap00|: w00 = (1 - ax) (1 - ay) alone has THREE roundings (two subtractions and the product).
    Zero where a coordinate is not finite (zeros padding): the contract there is 0.0 exactly."""
    refl = padding == "reflection"
    with np.errstate(invalid="ignore", over="ignore"):
        dxy = delta(ref["px"], w, refl)[:, None] * ref["Dx"] + delta(ref["py"], h, refl)[:, None] * ref["Dy"]
    bound = dxy + 6 * U * ref["S"] + U * ref["T00"]
    return np.where(ref["dead"][:, None], 0.0, bound) if padding == "zeros" else bound


def must_be_zero(ref: dict, w: int, h: int) -> np.ndarray:
    """[B,H,W] bool: a coordinate is non-finite or more than delta outside (-1, size): the zero-padding warps give 0.0 exactly."""
    out = ref["dead"].copy()
    for p, size in ((ref["px"], w), (ref["py"], h)):
        with np.errstate(invalid="ignore", over="ignore"):
            d = delta(np.where(np.isfinite(p), p, 0.0), size)
            out |= np.isfinite(p) & ((p <= -1.0 - d) | (p >= size + d))
    return out


# -------------------------------------------------------------------------------------------------------------------- resize / pyramid
def resize64(src: np.ndarray, ho: int, wo: int, value_scale: float = 1.0, src_bound: np.ndarray = None):
    """align_corners=True bilinear resize in float64 -> (v, bound) [B,C,Ho,Wo].  Coordinate r = o (Hi - 1) / (Ho - 1) (0 when Ho == 1);
    the kernel's is fl(fl((Hi - 1) / (Ho - 1)) o): delta = 2 U |r|.  The value: hy (hx s00 + lx s01) + ly (hx s10 + lx s11) puts at most
    six roundings on a tap (hx, hx s, the inner sum, hy, hy (...), the outer sum): 6 U S; ``* value_scale`` one more: U |v|.
    ``src_bound``: the error bound of the source's own elements (a pyramid level made by the kernel); the weights are >= 0 and sum to
    1, so the largest bound over the neighbourhood of the taps is added."""
    b, c, hi, wi = src.shape
    ry = np.arange(ho) * ((hi - 1) / (ho - 1)) if ho > 1 else np.zeros(ho)
    rx = np.arange(wo) * ((wi - 1) / (wo - 1)) if wo > 1 else np.zeros(wo)
    py, px = np.broadcast_to(ry[None, :, None], (b, ho, wo)), np.broadcast_to(rx[None, None, :], (b, ho, wo))
    v, s, dx, dy, _ = interpolate(extend(src, "border"), px, py, wi, hi)
    bound = (2 * U * px)[:, None] * dx + (2 * U * py)[:, None] * dy + 6 * U * s
    if src_bound is not None:
        fx, fy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
        bound = bound + neighbourhood(extend(src_bound, "border"), fx, fy).max(axis=(-1, -2))
    v = v * value_scale
    return v, bound * abs(value_scale) + U * np.abs(v)


def pyramid64(frames: np.ndarray, direct_level2: bool = False):
    """The x0.5 levels 1..3 of [N,3,H,W] -> [(v1, bound1), (v2, bound2), (v3, bound3)]: three applications of resize64, level l of size
    (H >> l, W >> l); the bound of level l is its own plus the largest bound of level l - 1 over the taps it reads.
    MUTANT ``direct_level2``: level 2 resized from the frame itself."""
    out, cur, cb = [], frames.astype(np.float64), None
    h, w = frames.shape[2:]
    for l in (1, 2, 3):
        if direct_level2 and l == 2:
            cur, cb = resize64(frames.astype(np.float64), h >> 2, w >> 2)
        else:
            cur, cb = resize64(cur, h >> l, w >> l, 1.0, cb)
        out.append((cur, cb))
    return out


# ------------------------------------------------------------------------------------------------------------------------------- blend
def blend64(r: np.ndarray, a: dict, c: dict, bound_a: np.ndarray, bound_c: np.ndarray):
    """warp_blend's it = m1 a + m2 c with m1 = sigmoid(r), m2 = 1 - m1 (r [B,H,W]; a, c the warp64 results of the two frames).
    bound = m1 bound_a + m2 bound_c + bound_m (|a| + |c|) + 3 U (|m1 a| + |m2 c|): the samples' own errors weighted by the masks,
    the masks' error (pointwise_ref.sigmoid_mask64; m2 = fl(1 - m1) adds U m2) on both products, and the three roundings of the two
    products and the sum."""
    m1, bm = R.sigmoid_mask64(torch.from_numpy(np.ascontiguousarray(r)))
    m1, bm = m1.numpy()[:, None], bm.numpy()[:, None]
    m2 = 1.0 - m1
    bm = bm + U * m2
    it = m1 * a["v"] + m2 * c["v"]
    bound = m1 * bound_a + m2 * bound_c + bm * (np.abs(a["v"]) + np.abs(c["v"])) + 3 * U * (np.abs(m1 * a["v"]) + np.abs(m2 * c["v"]))
    return it, bound


# ------------------------------------------------------------------------------------------------------------------- the fp32 emulation
WARP_MUTANTS = ("trunc", "swap_ax", "swap_ay", "x1_le_W", "y1_le_H", "stride", "no_nan_test", "no_far", "border_size", "reflect_no_flip")
TAIL = 7.0            # what the emulated loads find past the end of the image tensor (a real kernel finds its neighbour's data)


def _ref_coord32(p, size):
    """ref_coord of warp.hip, one fp32 rounding per operation."""
    hi = F32(size - 1)
    g = (F32(2.0) * p) / hi - F32(1.0)
    return g, ((g + F32(1.0)) / F32(2.0)) * hi


def _to_int32(f):
    """The float -> int conversion of the hardware: saturating, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        f = np.where(np.isnan(f), 0.0, f.astype(np.float64))
    return np.clip(f, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def pad_coord32(c, size, mode, mutant=None):
    """pad_coord of warp.hip (mode 0 zeros, 1 border, 2 reflection) on fp32 arrays."""
    if mode == 0:
        return c
    hi = F32(size - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 2:
            a = np.abs(c)
            extra = np.fmod(a, hi).astype(F32)
            flips = _to_int32(np.floor(a / hi))
            c = extra if mutant == "reflect_no_flip" else np.where(flips & 1, hi - extra, extra).astype(F32)
        top = F32(size) if mutant == "border_size" else hi
        return np.fmin(top, np.fmax(c, F32(0.0)))


def taps32(flow: np.ndarray, padding: str = "zeros", mutant: str = None):
    """make_taps (flow_warp_ex_kernel calls it with its padding map) on a whole flow field -> dict of [B,H,W] arrays: x0, y0 (int64), the four
    weights (fp32), the four in-flags, and the mask of flow_warp_ex (the fp32 expression 2 p / (size - 1) - 1 inside [-1, 1])."""
    _, _, h, w = flow.shape
    flow = flow.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        px = np.arange(w, dtype=F32)[None, None, :] + flow[:, 0]
        py = np.arange(h, dtype=F32)[None, :, None] + flow[:, 1]
        (gx, ix), (gy, iy) = _ref_coord32(px, w), _ref_coord32(py, h)
        mask = (gx >= -1) & (gy >= -1) & (gx <= 1) & (gy <= 1)
        mode = PADDINGS.index(padding)
        ix, iy = pad_coord32(ix, w, mode, mutant), pad_coord32(iy, h, mode, mutant)
        fx0, fy0 = (np.trunc(ix), np.trunc(iy)) if mutant == "trunc" else (np.floor(ix), np.floor(iy))
        if mutant == "no_far":                       # no clamp, no far test: the conversion saturates and turns NaN into 0
            x0, y0 = _to_int32(fx0), _to_int32(fy0)
            far = np.zeros(ix.shape, bool)
        else:
            cx = np.fmin(np.fmax(fx0, F32(-2.0)), F32(w) + F32(1.0))
            cy = np.fmin(np.fmax(fy0, F32(-2.0)), F32(h) + F32(1.0))
            x0, y0 = cx.astype(np.int64), cy.astype(np.int64)
            far = (cx != fx0) | (cy != fy0)
            if mutant != "no_nan_test":
                far |= np.isnan(ix) | np.isnan(iy)
        ax, ay = (ix - fx0).astype(F32), (iy - fy0).astype(F32)
        if mutant == "swap_ax":
            ax = F32(1.0) - ax
        if mutant == "swap_ay":
            ay = F32(1.0) - ay
        one = F32(1.0)
        wts = ((one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay)
    xin0, xin1 = (x0 >= 0) & (x0 < w), (x0 + 1 >= 0) & ((x0 + 1 <= w) if mutant == "x1_le_W" else (x0 + 1 < w))
    yin0, yin1 = (y0 >= 0) & (y0 < h), (y0 + 1 >= 0) & ((y0 + 1 <= h) if mutant == "y1_le_H" else (y0 + 1 < h))
    ins = tuple(~far & a & b for a, b in ((xin0, yin0), (xin1, yin0), (xin0, yin1), (xin1, yin1)))
    return {"x0": x0, "y0": y0, "w": wts, "in": ins, "mask": mask}


def sample32(src: np.ndarray, t: dict, mutant: str = None) -> np.ndarray:
    """sample_plane on every plane of src [B,C,H,W]: ``b = p + y0 * W + x0``, taps b[0], b[1], b[W], b[W + 1] of the FLAT tensor (a tap
    admitted wrongly reads what lies there: the next row, the next plane, or TAIL past the end), accumulated in sample_plane's order."""
    b, c, h, w = src.shape
    stride = w + 1 if mutant == "stride" else w
    flat = np.concatenate([src.astype(F32).reshape(-1), np.full(2 * w + 4, TAIL, F32)])
    base = (np.arange(b * c).reshape(b, c, 1, 1) * (h * w)) + (t["y0"] * stride + t["x0"])[:, None]
    v = np.zeros((b, c, h, w), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for off, wt, live in zip((0, 1, stride, stride + 1), t["w"], t["in"]):
            live = np.broadcast_to(live[:, None], v.shape)
            tap = flat[np.clip(base + off, 0, flat.size - 1)]
            v = np.where(live, v + tap * wt[:, None], v).astype(F32)
    return v


def warp32(src, flow, padding="zeros", mutant=None) -> np.ndarray:
    return sample32(src, taps32(flow, padding, mutant), mutant)


def mask_unnormalised32(flow: np.ndarray) -> np.ndarray:
    """MUTANT of flow_warp_ex's mask: taken on the pixel coordinate (0 <= p <= size - 1) instead of the normalised one."""
    _, _, h, w = flow.shape
    px = np.arange(w, dtype=F32)[None, None, :] + flow[:, 0].astype(F32)
    py = np.arange(h, dtype=F32)[None, :, None] + flow[:, 1].astype(F32)
    return (px >= 0) & (py >= 0) & (px <= w - 1) & (py <= h - 1)


def mask64(flow: np.ndarray):
    """-> (inside, decided) [B,H,W]: the float64 predicate |g| <= 1 on both axes, and where it is decided: every axis has
    ||g| - 1| > 4 U (or one axis is decidedly outside / not a number, which settles the conjunction)."""
    _, _, h, w = flow.shape
    px, py = coords64(flow)
    with np.errstate(invalid="ignore"):
        gx, gy = np.abs(2 * px / (w - 1) - 1), np.abs(2 * py / (h - 1) - 1)
        out = ~(gx <= 1 + 4 * U) | ~(gy <= 1 + 4 * U)                  # NaN counts as outside: the kernel's comparisons are false
        sure_in = (gx < 1 - 4 * U) & (gy < 1 - 4 * U)
        inside = (gx <= 1) & (gy <= 1)
    return inside, out | sure_in


def resize32(src: np.ndarray, ho: int, wo: int, value_scale: float = 1.0, mutant: str = None) -> np.ndarray:
    """resize_ac_kernel, one fp32 rounding per operation.  MUTANT ``ac_false``: the scale Hi / Ho with the half-pixel offset of
    align_corners=False."""
    src = src.astype(F32)
    b, c, hi, wi = src.shape

    def axis(n_in, n_out):
        o = np.arange(n_out, dtype=F32)
        if mutant == "ac_false":
            r = np.fmax((o + F32(0.5)) * (F32(n_in) / F32(n_out)) - F32(0.5), F32(0.0))
        else:
            r = (F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)) * o
        i0 = r.astype(np.int64)
        return i0, np.where(i0 < n_in - 1, 1, 0), (r - i0.astype(F32)).astype(F32)

    (y0, yp, ly), (x0, xp, lx) = axis(hi, ho), axis(wi, wo)
    hy, hx = (F32(1.0) - ly)[:, None], (F32(1.0) - lx)[None, :]
    ly, lx = ly[:, None], lx[None, :]
    ya, yb, xa, xb = y0[:, None], (y0 + yp)[:, None], x0[None, :], (x0 + xp)[None, :]
    v = hy * (hx * src[:, :, ya, xa] + lx * src[:, :, ya, xb]) + ly * (hx * src[:, :, yb, xa] + lx * src[:, :, yb, xb])
    return (v * F32(value_scale)).astype(F32)


def pyramid32(frames: np.ndarray, mutant: str = None):
    """image_pyramid_kernel: three sequential resize32 (bit-identical by the kernel's own promise).  MUTANT ``l2_direct``."""
    h, w = frames.shape[2:]
    l1 = resize32(frames, h >> 1, w >> 1)
    l2 = resize32(frames if mutant == "l2_direct" else l1, h >> 2, w >> 2)
    return [l1, l2, resize32(l2, h >> 3, w >> 3)]


# ------------------------------------------------------------------------------------------------- the staged-box rule of the tiled warps
WT_W, WT_H, WB_W, WB_H = 32, 8, 64, 24       # warp.hip: constexpr int WT_W = 32, WT_H = 8; WB_W = 64, WB_H = 24


def staged_boxes(flow: np.ndarray):
    """The decision of flow_warp_tiled_kernel / warp_blend_tiled_kernel per workgroup, restated from warp.hip:
      * ``tile_pixel``: workgroup (b, ty, tx) owns pixels x = 32 tx + (lane & 31), y = 8 ty + (lane >> 5), live when x < W && y < H;
      * ``box_add``: a lane counts when it is live and one of its four taps is inside (``any``); it contributes
        xlo = max(x0, 0), xhi = min(x0 + 1, W - 1), ylo = max(y0, 0), yhi = min(y0 + 1, H - 1) to the tile's extremes;
      * ``box_get``: no lane counted (``bx[0] > bx[1]``) -> the empty box, ok; else ax0 = xlo & ~3, nv = ((xhi - ax0) >> 2) + 1,
        h = yhi - ylo + 1, ok = nv <= 64 / 4 && h <= 24 (``b.ok = b.nv <= WB_W / 4 && b.h <= WB_H``).
    -> dict (b, ty, tx) -> {"state": "empty" | "fits" | "falls back", "ax0", "y0", "nv", "h", "lanes"} (lanes = how many counted)."""
    t = taps32(flow)
    bsz, _, h, w = flow.shape
    anyin = t["in"][0] | t["in"][1] | t["in"][2] | t["in"][3]
    out = {}
    for b in range(bsz):
        for ty in range((h + WT_H - 1) // WT_H):
            for tx in range((w + WT_W - 1) // WT_W):
                sl = (b, slice(ty * WT_H, min((ty + 1) * WT_H, h)), slice(tx * WT_W, min((tx + 1) * WT_W, w)))
                live = anyin[sl]
                if not live.any():
                    out[(b, ty, tx)] = {"state": "empty", "ax0": 0, "y0": 0, "nv": 0, "h": 0, "lanes": 0}
                    continue
                x0, y0 = t["x0"][sl][live], t["y0"][sl][live]
                xlo, xhi = int(np.maximum(x0, 0).min()), int(np.minimum(x0 + 1, w - 1).max())
                ylo, yhi = int(np.maximum(y0, 0).min()), int(np.minimum(y0 + 1, h - 1).max())
                ax0 = xlo & ~3
                nv, bh = ((xhi - ax0) >> 2) + 1, yhi - ylo + 1
                ok = nv <= WB_W // 4 and bh <= WB_H
                out[(b, ty, tx)] = {"state": "fits" if ok else "falls back", "ax0": ax0, "y0": ylo, "nv": nv, "h": bh, "xlo": xlo, "xhi": xhi,
                                    "lanes": int(live.sum())}
    return out


BOX_SHAPE = (1, 3, 40, 96)                   # 5 x 3 tiles of 32 x 8
# case -> (tile (ty, tx), state wanted, checks on the box); the targets of every case are written out in boundary_flow
BOX_CASES = {
    "a_fits_64x24": ((0, 0), "fits", {"ax0": 8, "nv": 16, "h": 24}),
    "b_65_columns": ((0, 1), "falls back", {"ax0": 8, "nv": 17, "h": 24}),
    "c_25_rows": ((0, 2), "falls back", {"ax0": 8, "nv": 16, "h": 25}),
    "d_left_tap_3_mod_4": ((1, 0), "fits", {"ax0": 8, "xlo": 11, "nv": 16}),
    "d2_left_tap_3_mod_4_one_more": ((1, 1), "falls back", {"ax0": 8, "xlo": 11, "nv": 17}),
    "e_last_load_ends_at_W": ((1, 2), "fits", {"ax0": 40, "xhi": 95, "nv": 14}),
    "f_clipped_at_last_row": ((2, 0), "fits", {"y0": 20, "h": 20}),
    "g_all_outside": ((2, 1), "empty", {}),
    "g2_normal_neighbour": ((2, 2), "fits", {}),
    "h_single_live_lane": ((3, 0), "fits", {"lanes": 1, "nv": 1, "h": 2}),
}


def boundary_flow(shift: int = 0) -> np.ndarray:
    """A flow field [1,2,40,96] built tile by tile for BOX_CASES (tiles not named have zero flow).  In a tile every lane aims at the
    point (base + 0.25) of its case, except the lanes named below, which pin the box's extremes: a target (tx + .25, ty + .25) has
    taps x0 = tx, tx + 1 and y0 = ty, ty + 1.  ``shift`` rotates the cases over the tiles (the second flow of warp_blend)."""
    _, _, h, w = BOX_SHAPE
    tgt_x = np.tile(np.arange(w, dtype=np.float64), (h, 1))
    tgt_y = np.tile(np.arange(h, dtype=np.float64)[:, None], (1, w))
    tiles = [(ty, tx) for ty in range(h // WT_H) for tx in range(w // WT_W)]

    def aim(tile, base, pins):
        ty, tx = tiles[(tiles.index(tile) + shift) % len(tiles)]
        ys, xs = slice(ty * WT_H, (ty + 1) * WT_H), slice(tx * WT_W, (tx + 1) * WT_W)
        tgt_x[ys, xs], tgt_y[ys, xs] = base[0] + 0.25, base[1] + 0.25
        for k, (x, y) in enumerate(pins):                       # lane k * 37 % 256: spread over the tile's four waves
            lane = k * 37 % 256
            tgt_x[ty * WT_H + lane // 32, tx * WT_W + lane % 32] = x
            tgt_y[ty * WT_H + lane // 32, tx * WT_W + lane % 32] = y

    aim((0, 0), (30, 10), [(8.25, 4.25), (70.25, 26.25)])                  # columns 8 .. 71, rows 4 .. 27
    aim((0, 1), (30, 10), [(8.25, 4.25), (71.25, 26.25)])                  # columns 8 .. 72: 65 columns
    aim((0, 2), (30, 10), [(8.25, 4.25), (70.25, 27.25)])                  # rows 4 .. 28: 25 rows
    aim((1, 0), (30, 10), [(11.25, 8.25), (70.25, 12.25)])                 # left tap 11, aligned to 8: columns 8 .. 71
    aim((1, 1), (30, 10), [(11.25, 8.25), (71.25, 12.25)])                 # left tap 11 .. 72: the alignment's three columns push it out
    aim((1, 2), (60, 10), [(40.25, 8.25), (95.0, 12.25), (95.5, 9.0)])     # columns 40 .. 95: the last 16-byte load ends at W = 96
    aim((2, 0), (30, 30), [(30.25, 20.25), (31.0, 39.25), (30.5, 39.0)])   # rows 20 .. 39: y0 + 1 = 40 is clipped to H - 1
    aim((2, 1), (-5, -5), [(200.0, 3.0), (3.0, -1.25), (-1.25, 3.0), (96.25, 3.0), (3.0, 40.25)])   # nothing inside
    aim((2, 2), (70, 20), [])
    aim((3, 0), (-5, 50), [(17.5, 5.5)])                                   # one live lane
    flow = np.stack([tgt_x - np.arange(w)[None, :], tgt_y - np.arange(h)[:, None]])[None]
    assert np.array_equal(flow.astype(F32).astype(np.float64), flow)
    return flow.astype(F32)


def case_tile(name: str, shift: int = 0):
    """(b, ty, tx) of a BOX_CASES entry in boundary_flow(shift)."""
    _, _, h, w = BOX_SHAPE
    tiles = [(ty, tx) for ty in range(h // WT_H) for tx in range(w // WT_W)]
    return (0, *tiles[(tiles.index(BOX_CASES[name][0]) + shift) % len(tiles)])


def check_box_cases(flow: np.ndarray, shift: int = 0):
    """Every constructed tile is on the intended side of the staged-box rule, with the intended box."""
    boxes = staged_boxes(flow)
    for name, (_, state, fields) in BOX_CASES.items():
        got = boxes[case_tile(name, shift)]
        assert got["state"] == state, f"{name}: the tile is '{got['state']}', constructed to be '{state}': {got}"
        for k, v in fields.items():
            assert got[k] == v, f"{name}: {k} = {got[k]}, constructed to be {v}: {got}"
    return boxes


# ----------------------------------------------------------------------------------------------------------------------- input families
FLOW_FAMILIES = ("gauss", "integers", "ulp", "halves", "edges", "wild")
FINITE_FAMILIES = FLOW_FAMILIES[:5]
IMAGE_FAMILIES = ("rand", "ramp", "checker", "hot")
WILD_VALUES = (np.inf, -np.inf, np.nan, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31, 1e9, 0.0)


def flow_family(name: str, b: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[b,2,h,w] fp32.  gauss: sigma 6 px.  integers: targets uniform over -2 .. size + 1 on both axes (taps exactly on pixels, on -1,
    size - 1, size).  ulp: the same targets, the flow one fp32 ulp up or down.  halves: targets at multiples of 0.5 over +-2 size.
    edges: targets uniform in [-1.5, 0.5] and [size - 1.5, size + 0.5].  wild: one component from WILD_VALUES, the other Gaussian."""
    rng = np.random.default_rng([FLOW_FAMILIES.index(name), b, h, w, seed])
    xs, ys = np.arange(w, dtype=np.float64)[None, None, :], np.arange(h, dtype=np.float64)[None, :, None]
    if name == "gauss":
        return rng.normal(0.0, 6.0, (b, 2, h, w)).astype(F32)
    if name in ("integers", "ulp"):
        flow = np.stack([rng.integers(-2, w + 2, (b, h, w)) - xs, rng.integers(-2, h + 2, (b, h, w)) - ys], 1).astype(F32)
        if name == "ulp":
            flow = np.nextafter(flow, np.where(rng.integers(0, 2, flow.shape) == 1, np.inf, -np.inf).astype(F32))
        return flow
    if name == "halves":
        return np.stack([rng.integers(-4 * w, 4 * w + 1, (b, h, w)) * 0.5 - xs, rng.integers(-4 * h, 4 * h + 1, (b, h, w)) * 0.5 - ys], 1).astype(F32)
    if name == "edges":
        tx = rng.uniform(-1.5, 0.5, (b, h, w)) + np.where(rng.integers(0, 2, (b, h, w)) == 1, float(w), 0.0)
        ty = rng.uniform(-1.5, 0.5, (b, h, w)) + np.where(rng.integers(0, 2, (b, h, w)) == 1, float(h), 0.0)
        return np.stack([tx - xs, ty - ys], 1).astype(F32)
    if name == "wild":
        flow = rng.normal(0.0, 6.0, (b, 2, h, w)).astype(F32)
        which = rng.integers(0, 2, (b, h, w))
        vals = np.asarray(WILD_VALUES, F32)[rng.integers(0, len(WILD_VALUES), (b, h, w))]
        flow[:, 0] = np.where(which == 0, vals, flow[:, 0])
        flow[:, 1] = np.where(which == 1, vals, flow[:, 1])
        return flow
    raise ValueError(name)


def image_family(name: str, b: int, c: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[b,c,h,w] fp32.  rand: uniform in [0, 1).  ramp: 0.37 x + 1.1 y + 3 (bilinear interpolation reproduces it: the warp's error is the
    coordinate error times the slope).  checker: +-1 (the largest Dx, Dy).  hot: single 1.0 pixels at the four corners and the centre of a
    zero image (each tap's weight visible on its own)."""
    x, y = np.arange(w, dtype=np.float64)[None, None, None, :], np.arange(h, dtype=np.float64)[None, None, :, None]
    if name == "rand":
        return np.random.default_rng([IMAGE_FAMILIES.index(name), b, c, h, w, seed]).random((b, c, h, w)).astype(F32)
    if name == "ramp":
        return np.ascontiguousarray(np.broadcast_to(0.37 * x + 1.1 * y + 3.0, (b, c, h, w)), F32)
    if name == "checker":
        return np.ascontiguousarray(np.broadcast_to(1.0 - 2.0 * ((x + y) % 2), (b, c, h, w)), F32)
    if name == "hot":
        im = np.zeros((b, c, h, w), F32)
        for yy, xx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
            im[:, :, yy, xx] = 1.0
        return im
    raise ValueError(name)


def worst_ratio(got, ref, bound) -> float:
    """pointwise_ref.worst_ratio on numpy arrays or tensors: NaN in ``got``, or an error at bound 0, is an infinite ratio."""
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return R.worst_ratio(as_t(got).cpu(), as_t(ref), as_t(bound))
