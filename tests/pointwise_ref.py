"""fp64 references and derived elementwise error bounds of the fp32 pointwise kernels -- test infrastructure only.

The f16x3 contractions have an exact model (tests/f16x3_model.py).  The fp32 kernels around them -- LayerNorm, depth-wise 3x3 + GELU,
the motion head and the ``2 * sigmoid - 1`` residual sites -- are held here to a plain float64 restatement of the same operation and to
a bound that is DERIVED from the arithmetic the kernel performs, never fitted to what it returns.  Conventions:

* ``U = 2^-24`` is the unit roundoff of fp32 (one rounding to nearest changes a value by at most ``U`` of its magnitude);
* a "bound" is always a tensor of the result's shape; a test asserts ``|got - ref| <= bound`` elementwise and reports
  ``worst_ratio`` = max ``err / bound``;
* everything is plain torch in float64 and runs on whatever device its arguments live on (the two large dw-conv cases of
  tests/test_gpu_pointwise_fp64.py evaluate reference and bound on the GPU);
* the bounds are first order in ``U`` (products of two error terms, ~1e-14, are dropped).

tests/test_pointwise_ref_cpu.py shows without a GPU that fp32 torch stays inside every bound on the input families below and that
a subtly wrong kernel (one-pass variance, tanh-form GELU, a moved select threshold, a coefficient off in its 6th digit, an early clamp,
an fp16 sigmoid) does not.
"""
from __future__ import annotations

import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
# Gradual underflow: a result below the smallest normal number 2^-126 is rounded to a multiple of 2^-149, i.e. by up to 2^-150 whatever
# its magnitude.  Two such roundings (0.5 * x, then the product) -> 2^-149 in the GELU bound.  (torch's own fp32 GELU returns 0 for the
# smallest subnormal where the exact value is 2^-150: without this term no fp32 evaluation can meet a purely relative bound there.)
UNDERFLOW = 2.0 ** -149
# Below the smallest normal number fp32 carries no relative accuracy at all, and 1 / (1 + expf(-r)) is 0 as soon as expf overflows
# (-r > 88.72, sigmoid(r) < 2^-128): the absolute term of a bound on sigmoid itself.
FLT_MIN = 2.0 ** -126
SQRT2 = math.sqrt(2.0)

# ----------------------------------------------------------------------------------------------------------------------------- GELU
# E of gelu_erf2 (common.h erf_2range), the sum of three terms:
#   1.2e-7   erf_2range's stated contract: |erf_2range(z) - erf(z)| at the fp32 argument z (tools/fit_erf.py, exactly rounded exp2);
#   2^-26    one ulp of a v_exp_f32 result below 0.25: range B (|z| >= 1) computes 1 - 2^P(|z|) and 2^P ~ erfc(|z|) <= erfc(1) = 0.157;
#   4.4e-8   the rounding of z = x * 0.70710678f (one product and the constant's own rounding, <= 1.5 U relative) propagated through
#            erf: |d erf| = |dz| erf'(z) <= 1.5 U max z erf'(z) = 1.5 x 5.96e-8 x 0.484.
E_ERF2 = 1.8e-7
# E of gelu_erf (the motion head): 0.5 x (1 + erff(x * 0.70710678f)) with the library erff at 1 ulp of a value below 1 (2^-24 = 6.0e-8)
# plus the same 4.4e-8 for the argument: 1.04e-7 <= 1.2e-7.
E_ERFF = 1.2e-7
GELU_SLOPE = 1.13          # max |GELU'(a)| = 1.1289 at a = +-1.41: an error of the argument grows by at most this factor


def gelu64(a: torch.Tensor) -> torch.Tensor:
    """Exact GELU in float64: 0.5 a erfc(-a / sqrt 2) (1 + erf cancels for negative a; erfc does not)."""
    a = a.double()
    return 0.5 * a * torch.special.erfc(-a / SQRT2)


def gelu_bound(a: torch.Tensor, E: float = E_ERF2) -> torch.Tensor:
    """|gelu_fp32(a) - gelu64(a)| <= 0.5 |a| E + 2^-23 |gelu64(a)| + 2^-149 for the fp32 value a.

    The kernel forms 0.5f * a * (1.0f + e) with |e - erf(a / sqrt 2)| <= E: the error of e enters as 0.5 |a| E; the sum 1 + e and the
    final product are one fp32 rounding each, 2 U = 2^-23 relative to the result (0.5f * a is exact unless it underflows); the last
    term is ``UNDERFLOW`` above."""
    a = a.double()
    return 0.5 * a.abs() * E + 2.0 ** -23 * gelu64(a).abs() + UNDERFLOW


def gelu_tanh64(a: torch.Tensor) -> torch.Tensor:
    """The tanh approximation of GELU (a MUTANT: ~3e-4 away from the exact one)."""
    a = a.double()
    return 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a ** 3)))


COMMON_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "atm-vfi_amd", "csrc", "common.h")


def parse_erf_2range(path: str = COMMON_H) -> dict:
    """Coefficients and thresholds of ``erf_2range`` / ``gelu_erf2`` as written in common.h (so the emulation cannot drift):
    {"a": Horner coefficients of range A in u = z^2, highest first, "b": those of range B in |z|, "clamp", "select", "rsqrt2"}."""
    src = open(path).read()
    body = src[src.index("float erf_2range(float z)"):]
    body = body[:body.index("gelu_erf2(float x)") + 200]
    num = r"(-?[0-9.]+(?:e[+-]?[0-9]+)?)f"
    out = {}
    for name, var in (("a", "u"), ("b", "ac")):
        p = "p" + name
        first = re.search(r"float %s = fmaf\(%s, %s, %s\);" % (p, num, var, num), body)
        rest = re.findall(r"\b%s = fmaf\(%s, %s, %s\);" % (p, p, var, num), body)
        assert first and rest, "common.h: the Horner chain of erf_2range's range %s was not found" % name.upper()
        out[name] = [float(first.group(1)), float(first.group(2))] + [float(r) for r in rest]
    out["clamp"] = float(re.search(r"fminf\(az, %s\)" % num, body).group(1))
    out["select"] = float(re.search(r"az < %s \? ea : eb" % num, body).group(1))
    out["rsqrt2"] = float(re.search(r"erf_2range\(x \* %s\)" % num, body).group(1))
    assert len(out["a"]) == 6 and len(out["b"]) == 8, out
    return out


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64, so this is one rounding of a * b + c (up to the
    double rounding of the float64 sum, as in tools/fit_erf.py)."""
    return _f32(a.astype(np.float64) * b.astype(np.float64) + np.float64(np.float32(c)))


def gelu_erf2_emulated(x, coef: dict = None, select: float = None, clamp: float = None, b_last_shift: float = 0.0) -> np.ndarray:
    """numpy emulation of common.h's gelu_erf2 on fp32 ``x`` (a torch tensor or array), operation by operation, each in fp32, every
    fmaf with one rounding, v_exp_f32 as a correctly rounded exp2.  ``select`` / ``clamp`` / ``b_last_shift`` build the MUTANTS."""
    coef = coef or parse_erf_2range()
    select = coef["select"] if select is None else select
    clamp = coef["clamp"] if clamp is None else clamp
    x = np.asarray(torch.as_tensor(x).detach().cpu().float().numpy(), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        z = _f32(x.astype(np.float64) * np.float64(np.float32(coef["rsqrt2"])))
        az = np.abs(z)
        u = _f32(az.astype(np.float64) * az)
        pa = _fma32(np.full_like(u, np.float32(coef["a"][0])), u, coef["a"][1])
        for c in coef["a"][2:]:
            pa = _fma32(pa, u, c)
        ea = _f32(az.astype(np.float64) * pa)
        ac = np.minimum(az, np.float32(clamp))
        cb = list(coef["b"])
        cb[-1] += b_last_shift
        pb = _fma32(np.full_like(ac, np.float32(cb[0])), ac, cb[1])
        for c in cb[2:]:
            pb = _fma32(pb, ac, c)
        eb = _f32(1.0 - _f32(np.exp2(pb.astype(np.float64))).astype(np.float64))
        e = np.copysign(np.where(az < np.float32(select), ea, eb), z)
        half_x = _f32(0.5 * x.astype(np.float64))
        one_e = _f32(1.0 + e.astype(np.float64))
        return _f32(half_x.astype(np.float64) * one_e)


def _ulp_neighbourhood(centre: float, ulps: int) -> np.ndarray:
    c = np.array([centre], dtype=np.float32).view(np.int32)[0]
    return (np.arange(-ulps, ulps + 1, dtype=np.int64) + int(c)).astype(np.int32).view(np.float32)


GELU_JOINT_ULPS = 4096
GELU_SPECIALS = (0.0, 2.0 ** -149, 1e-38, 1e-30, 6.0, 10.0, 20.0, 1e30)
GELU_GRID_POINTS = 2 ** 22


def gelu_sweep() -> torch.Tensor:
    """The hostile arguments of GELU, fp32, 1-D: both signs of every float within 4096 ulps of sqrt 2 and of 4 sqrt 2 (x there puts
    z = x / sqrt 2 on erf_2range's joints |z| = 1 and |z| = 4), of 0, the smallest subnormal, 1e-38, 1e-30, 6, 10, 20, 1e30, and 2^22
    evenly spaced points on [-8, 8].  No Inf or NaN, |x| <= 1e30."""
    parts = []
    for centre in (SQRT2, 4.0 * SQRT2):
        nb = _ulp_neighbourhood(centre, GELU_JOINT_ULPS)
        parts += [nb, -nb]
    sp = np.array(GELU_SPECIALS, dtype=np.float32)
    parts += [sp, -sp, np.linspace(-8.0, 8.0, GELU_GRID_POINTS).astype(np.float32)]
    return torch.from_numpy(np.concatenate(parts).astype(np.float32))


def tile_to(values: torch.Tensor, numel: int) -> torch.Tensor:
    """``values`` (1-D) repeated cyclically to ``numel`` elements."""
    reps = (numel + values.numel() - 1) // values.numel()
    return values.repeat(reps)[:numel]


# ------------------------------------------------------------------------------------------------------------------ dw-conv + GELU
DWCONV_ROUNDINGS = 12


def dwconv_acc64(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor):
    """(a, S) of the depth-wise 3x3 convolution (zero padding 1) of NHWC ``x`` with ``w`` [C,1,3,3] and bias ``b``, in float64:
    a = b + sum v w over the nine taps, S = |b| + sum |v w|.  Nine shifted-slice multiply-adds on a zero-padded tensor."""
    x = x.double()
    n, h, wd, c = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    wk = w.double().reshape(c, 3, 3)
    a = b.double().expand(n, h, wd, c).clone()
    s = b.double().abs().expand(n, h, wd, c).clone()
    for ky in range(3):
        for kx in range(3):
            t = xp[:, ky:ky + h, kx:kx + wd, :] * wk[:, ky, kx]
            a += t
            s += t.abs()
    return a, s


def dwconv_gelu64(x, w, b):
    """-> (reference, bound) of GELU(dwconv3x3(x) + b).

    bound = 1.13 x 12 U S + gelu_bound(a).  The accumulator starts from the bias and takes nine multiply-adds: ten roundings at most
    (nine sums and, in the per-pixel kernel, which does not fuse, the products -- each product's rounding is relative to one term, so
    it adds U S in all), each bounded by U times a partial sum <= S; 12 leaves slack for the order and FMA / non-FMA difference
    between the three kernels.  GELU carries an argument error through with a factor of at most max |GELU'| = 1.13, and adds its own
    ``gelu_bound``."""
    a, s = dwconv_acc64(x, w, b)
    return gelu64(a), GELU_SLOPE * DWCONV_ROUNDINGS * U * s + gelu_bound(a)


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-5


def layernorm64(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """-> (y, bound) of LayerNorm over the last dimension of ``x`` [rows, C], two passes in float64, eps 1e-5, biased variance.

    With mu, rstd = 1 / sqrt(var + eps), yhat = (x - mu) rstd and y = yhat gamma + beta:

        bound = |gamma| (rstd (log2 C + 2) U max|x_row|  +  (log2 C + 8) U |yhat|)  +  2 U |y|

    First term: the fp32 mean is a tree sum of C values (depth log2 C; + 2 for the division by C and the rounding of x - mean), its
    error <= (log2 C + 2) U max|x_row| shifts every x - mean by the same amount and is multiplied by rstd -- this is the term a
    large common offset makes large, and the one a one-pass variance E[x^2] - mu^2 cannot meet.  Second term: the relative error of
    rstd (half that of the tree-summed variance, whose squares each carry 3 U: (log2 C + 3 + 2) / 2 U, plus division, sqrt and
    reciprocal) and the two products (x - mean) * rstd * gamma, <= (log2 C + 8) U of |yhat gamma|.  Last: the product's and the final
    sum's rounding, relative to |y| to first order."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    c = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    yhat = (x - mu) * rstd
    y = yhat * gamma + beta
    l2 = math.log2(c)
    xmax = x.abs().amax(-1, keepdim=True)
    bound = gamma.abs() * (rstd * (l2 + 2) * U * xmax + (l2 + 8) * U * yhat.abs()) + 2 * U * y.abs()
    return y, bound


def layernorm_two_pass_f32(x, gamma, beta):
    """Well-behaved fp32 LayerNorm written out (mean, then the variance of the centred values)."""
    x = x.float()
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    return d * (1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32))) * gamma.float() + beta.float()


def layernorm_one_pass_f32(x, gamma, beta):
    """MUTANT: variance as E[x^2] - mean^2 in fp32 (cancels on rows with an offset mean)."""
    x = x.float()
    mu = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mu * mu).clamp_min(0)
    return (x - mu) * (1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32))) * gamma.float() + beta.float()


LN_FAMILIES = ("plain", "mean1000", "mean100_sigma0.01", "sigma1e-4", "constant", "outlier1e4", "scale1e12")
LN_ROWS = 64
LN_WIDTHS = (224, 448, 512, 672)     # one partial vector / has1 on 48 of 64 lanes / both vectors full / loop path


def layernorm_family(name: str, c: int, gen: torch.Generator) -> torch.Tensor:
    """64 fp32 rows of ``c`` channels of one hostile family."""
    n = torch.randn(LN_ROWS, c, generator=gen)
    if name == "plain":
        return (torch.rand(LN_ROWS, c, generator=gen) * 2 - 1) * 3.0
    if name == "mean1000":
        return 1000.0 + n
    if name == "mean100_sigma0.01":
        return 100.0 + 0.01 * n
    if name == "sigma1e-4":
        return 1e-4 * n
    if name == "constant":
        return (0.1 * torch.arange(LN_ROWS, dtype=torch.float32))[:, None].expand(LN_ROWS, c).contiguous()
    if name == "outlier1e4":
        n[torch.arange(LN_ROWS), torch.randint(0, c, (LN_ROWS,), generator=gen)] = 1e4
        return n
    if name == "scale1e12":
        return 1e12 * n
    raise KeyError(name)


def layernorm_inputs(c: int, seed: int = 0):
    """-> (x [7 * 64, c] with the families stacked in LN_FAMILIES order, gamma, beta), fp32, seeded."""
    gen = torch.Generator().manual_seed(1000 + c + seed)
    x = torch.cat([layernorm_family(f, c, gen) for f in LN_FAMILIES], 0)
    gamma = 1 + (torch.rand(c, generator=gen) * 2 - 1) * 0.2
    beta = (torch.rand(c, generator=gen) * 2 - 1) * 0.2
    return x, gamma, beta


# ----------------------------------------------------------------------------------------------------------------- residual sigmoid
SIGMOID_SPECIALS = (float("inf"), 0.0, 88.8, 103.9)


def sigmoid_sweep() -> torch.Tensor:
    """The hostile arguments of the sigmoid sites, fp32, 1-D: 2^16 points on [-110, 110] (saturation on both sides, expf overflow
    beyond 88.72), 2^12 points on [-1e-3, 1e-3] (2 sigmoid - 1 cancels), +-Inf, +-0, +-88.8, +-103.9."""
    sp = torch.tensor(SIGMOID_SPECIALS, dtype=torch.float32)
    return torch.cat([torch.linspace(-110.0, 110.0, 2 ** 16, dtype=torch.float64).float(),
                      torch.linspace(-1e-3, 1e-3, 2 ** 12, dtype=torch.float64).float(), sp, -sp])


def residual_sigmoid64(it: torch.Tensor, r: torch.Tensor):
    """-> (v, bound) of v = it + (2 sigmoid(r) - 1) = it + tanh(r / 2), float64.

        bound = 8 U sigmoid(r) + U |2 sigmoid(r) - 1| + U |v|

    sigmoid = 1 / (1 + expf(-r)): expf at 1 ulp (2 U relative; the build has no fast-math), the sum and the division one rounding
    each -- <= 4 U relative on sigmoid, doubled by the factor 2 (exact): 8 U sigmoid.  The subtraction 2 s - 1 and the sum with ``it``
    are one rounding each, relative to their own results.  Where expf overflows (r < -88.72) sigmoid is 0 instead of < 2^-128: far
    below U |2 sigmoid - 1| = U."""
    it, r = it.double(), r.double()
    s = torch.sigmoid(r)
    t = torch.tanh(0.5 * r)
    v = it + t
    return v, 8 * U * s + U * t.abs() + U * v.abs()


def sigmoid_mask64(r: torch.Tensor):
    """-> (sigmoid(r), bound) in float64 for a site that stores the sigmoid itself (warp_blend's mask1): 4 U sigmoid(r) (expf, sum and
    division as above) + 2^-126: below the smallest normal number fp32 keeps no relative accuracy and expf(-r) overflows."""
    s = torch.sigmoid(r.double())
    return s, 4 * U * s + FLT_MIN


def blend_const64(r: torch.Tensor, c0: torch.Tensor, c1: torch.Tensor):
    """-> (it, bound) of warp_blend's ``it`` for zero flows and per-channel constant images c0, c1 in [0, 1] ([3] each), r [B,H,W]:
    it = s c0 + (1 - s) c1, s = sigmoid(r), shape [B,3,H,W].

    bound = 12 U, the sum of
      * 6 U for the two samples.  A bilinear sample of a constant plane is c (w00 + w01 + w10 + w11).  At zero flow the round trip of
        the sampling coordinate leaves a fraction within ~1e-5 of 0 or of 1 (and exactly 0 on the image's border, where g = -1 and
        g = 1 are exact), so one weight carries the value: its two factors 1 - a and their product are values in [0.5, 1], rounded by
        at most U / 2 each (1.5 U), its product with c by U c, and the three sums with the ~1e-5 c terms by U c each: 5.5 U c <= 6 U c
        per sample; they enter weighted by s and 1 - s with c <= 1;
      * 4 U for the masks: m1 = s (1 + d), |d| <= 4 U (expf, sum, division), m2 = fl(1 - m1) moves ``it`` by
        4 U s |c0 - c1| + U (1 - s) c1 <= 4 U;
      * 2 U for the roundings of the two products (U (s c0 + (1 - s) c1) together) and of the final sum (U it)."""
    s = torch.sigmoid(r.double())[:, None]
    it = s * c0.double()[None, :, None, None] + (1 - s) * c1.double()[None, :, None, None]
    return it, torch.full_like(it, 12 * U)


def sigmoid_f16(r: torch.Tensor) -> torch.Tensor:
    """MUTANT: the sigmoid evaluated in fp16."""
    return torch.sigmoid(r.float()).half().float()


# ---------------------------------------------------------------------------------------------------------------------- motion head
def motion_head64(motion: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor):
    """-> (y [rows, 2], bound [rows, 2]) of the motion head (tests/cpu_ops.py CpuOps.motion_head) in float64: for each of the two
    motion components, y = b1 + sum_j w1[j] GELU(b0[j] + sum_h w0[j, h] m[h]),  motion [rows, heads, 2], w0 [hid, heads], w1 [1, hid].

    Running-error bound of the kernel's sequential fp32 sums (attention.hip motion_head_kernel):
      * hidden unit: n = heads products added one by one to the bias -- the earliest term meets n sums and one product rounding, so
        |d ax| <= (n + 2) U (|b0| + sum |w0 m|)   (+ 1 of slack covers fused or unfused products);
      * GELU (library erff): |d g| <= 1.13 |d ax| + gelu_bound(ax, E = 1.2e-7);
      * output: hid products added to b1: |d y| <= sum |w1[j]| |d g_j| + (hid + 2) U (|b1| + sum |w1[j] g_j|)."""
    m = motion.double().permute(0, 2, 1)                                   # [rows, 2, heads]
    w0d, b0d, w1d, b1d = w0.double(), b0.double(), w1.double().reshape(-1), b1.double().reshape(-1)[0]
    hid, heads = w0d.shape
    t = m[:, :, None, :] * w0d[None, None]                                 # [rows, 2, hid, heads]
    ax = t.sum(-1) + b0d
    d_ax = (heads + 2) * U * (t.abs().sum(-1) + b0d.abs())
    g = gelu64(ax)
    d_g = GELU_SLOPE * d_ax + gelu_bound(ax, E_ERFF)
    p = g * w1d
    y = p.sum(-1) + b1d
    bound = (d_g * w1d.abs()).sum(-1) + (hid + 2) * U * (p.abs().sum(-1) + b1d.abs())
    return y, bound


# -------------------------------------------------------------------------------------------------------------------------- helpers
def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of |got - ref| / bound (0 where the error is exactly 0, inf where ``got`` is NaN or the bound is exceeded
    at bound 0)."""
    err = (got.double() - ref.double()).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")).max().item()


def split_on_device(rows: torch.Tensor):
    """(hi, lo') of finite fp32 ``rows`` as fp16 tensors on the rows' own device: the arithmetic of f16x3_model.split.  x - hi and its
    1024-fold are exact in fp32 (hi is x rounded to 11 bits), so each plane is ONE rounding to fp16, as in the model."""
    hi = rows.clamp(-65504.0, 65504.0).half()
    lo = (rows * 1024.0 - hi.float() * 1024.0).clamp(-65504.0, 65504.0).half()
    return hi, lo


class _Rows:
    """What assert_split_of reads of a Planes object, for a sample of its rows."""

    def __init__(self, rows):
        self._rows = rows

    def to_rows(self):
        return self._rows


def assert_planes_split_of(planes, rows: torch.Tensor, what: str):
    """The plane pair is bit for bit the split of the fp32 rows [R, C] (finite values) -- everywhere by the same arithmetic on the device,
    and by the fp64 model's ``assert_split_of`` on the whole result when it is small, else on its first and last 512 rows (the last
    strip) and 1024 rows in between."""
    import f16x3_model as M
    got = planes.to_rows()
    hi, lo = split_on_device(rows)
    c = rows.shape[1]
    nhi, nlo = int((got[0, :, :c] != hi).sum()), int((got[1, :, :c] != lo).sum())
    assert nhi == 0 and nlo == 0, f"{what}: planes differ from the split of the fp32 rows at {nhi} (hi) / {nlo} (lo') places"
    n = rows.shape[0]
    if n <= 4096:
        M.assert_split_of(planes, rows, what)
        return
    idx = torch.cat([torch.arange(512), torch.arange(n - 512, n),
                     torch.randint(512, n - 512, (1024,), generator=torch.Generator().manual_seed(1))]).to(rows.device)
    M.assert_split_of(_Rows(got[:, idx]), rows[idx], what)


# ----------------------------------------------------------------------------------------------------------- shared seeded inputs
DWCONV_SMALL_SHAPES = ((1, 9, 11, 100), (1, 11, 9, 64))      # per-pixel kernel (C % 64 != 0) / 8-row strips, partial strip and x-block
DWCONV_SCALES = (1e-3, 2.0, 30.0)


def uniform(gen: torch.Generator, *shape, scale: float = 1.0) -> torch.Tensor:
    return (torch.rand(*shape, generator=gen) * 2 - 1) * scale


def dwconv_params(c: int, seed: int = 0):
    """-> (w [C,1,3,3] of scale 0.5, bias [C] of scale 0.3), seeded."""
    gen = torch.Generator().manual_seed(2000 + c + seed)
    return uniform(gen, c, 1, 3, 3, scale=0.5), uniform(gen, c, scale=0.3)


def dwconv_input(shape, scale: float, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(3000 + sum(shape) + seed)
    return uniform(gen, *shape, scale=scale)


def centre_tap_params(c: int):
    """Weights 1 on the centre tap and 0 elsewhere, zero bias: the accumulator is the input exactly and the output is GELU alone."""
    w = torch.zeros(c, 1, 3, 3)
    w[:, 0, 1, 1] = 1.0
    return w, torch.zeros(c)


def motion_head_inputs(rows: int, scale: float, heads: int = 8):
    """-> (motion [rows, heads, 2] of the given scale, w0 [heads/2, heads], b0, w1 [1, heads/2], b1), seeded: the geometry of
    test_gpu_ops.py::test_motion_head."""
    gen = torch.Generator().manual_seed(4000 + int(scale))
    hid = heads // 2
    return (uniform(gen, rows, heads, 2, scale=scale), uniform(gen, hid, heads), uniform(gen, hid), uniform(gen, 1, hid),
            uniform(gen, 1))


def residual_inputs(numel: int):
    """-> (r, it) 1-D fp32 of ``numel`` elements: the sigmoid sweep repeated cyclically, ``it`` uniform in [0, 1]."""
    gen = torch.Generator().manual_seed(5000)
    return tile_to(sigmoid_sweep(), numel), torch.rand(numel, generator=gen)
