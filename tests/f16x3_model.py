"""Exact fp64 model of the f16x3 arithmetic (include/atmvfi.h) -- CPU only, test infrastructure only.

Every fp32 operand of a contraction is split as x = hi + lo'/1024 with hi = fp16(x), lo' = fp16((x - hi) * 1024), both rounded to
nearest even and saturating at +-65504 (an infinity stays one in hi and makes lo' NaN: common.h split_pair).  A product is
hi*hi + (hi*lo' + lo'*hi) / 1024: the first sum goes into one fp32 accumulator ``acc``, the two cross terms into another, ``cor``,
and the kernels fold them as acc + cor / 1024; lo'*lo' is never formed.  The functions below compute ``acc`` and ``cor`` EXACTLY
(fp64 over fp16 x fp16 products) from the split of the actual operands, then the epilogue (bias, PReLU, residual) in fp64.

Input families (all seeded): ``exact`` (a dyadic grid on which no fp32 accumulation can round -- ``certificate`` proves it for the
operands actually used), ``wide`` (log-uniform magnitudes), ``edge`` (fp16 saturation / subnormal boundaries) and ``cancel``
(sums near 0 with large terms).  ``mutants`` are what a subtly wrong engine would compute; tests/test_f16x3_model_cpu.py shows
that each of them misses the GPU tolerance on every exact-family configuration of tests/test_gpu_f16x3_contract.py by > 10x.

``stem_chain`` / ``tail_chain`` and the ``chain_exact`` / ``chain_rich_last`` families (at the end) model the two kernels that chain
layers on chip, on operands for which the hidden layers are exact: tests/test_gpu_f16x3_chains.py.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

F16_MAX = 65504.0
EPS32 = 2.0 ** -24           # half an ulp of fp32, relative: the bound of one rounding
EDGE_VALUES = [2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 65472.0, 65487.99, 65488.0, 65504.0,
               65519.99, 65520.0, 7e4, -0.0]


# ------------------------------------------------------------------ the split
def _sat16(t: np.ndarray) -> np.ndarray:
    """fp16 of fp64 values that are exact in fp32, rounded to nearest even, finite values saturating at +-65504 (FP16_OVFL), an
    infinity or NaN passed on."""
    t = np.asarray(t, dtype=np.float64)
    fin = np.isfinite(t)
    return np.where(fin, np.clip(t, -F16_MAX, F16_MAX), t).astype(np.float16)


def split(x) -> tuple:
    """(hi, lo') of fp32 values as fp16 tensors, the library's split: hi = fp16(x), lo' = fp16(fp32(x * 1024) - hi * 1024)."""
    x32 = torch.as_tensor(x).detach().cpu().float().numpy()
    hi = _sat16(x32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = np.where(np.isinf(x32), x32.astype(np.float16), hi)
        xs = (x32 * np.float32(1024.0)).astype(np.float64)            # fp32 product: overflows to inf beyond 2^118
        lo = _sat16(xs - hi.astype(np.float64) * 1024.0)
    return torch.from_numpy(hi.copy()), torch.from_numpy(lo.copy())


def dequant(x) -> torch.Tensor:
    """hi + lo'/1024 in fp64: the value the engines contract with."""
    h, l = split(x)
    return h.double() + l.double() / 1024.0


# ------------------------------------------------------------------ mutants (what a subtly wrong engine computes)
def lo_4bits(lo: torch.Tensor) -> torch.Tensor:
    """lo' truncated to 4 significant bits (an fp8-like cross-term operand)."""
    m, e = torch.frexp(lo.double())
    return torch.ldexp(torch.trunc(m * 16.0) / 16.0, e)


MUTANTS = ("lo4", "one_cross", "last_chunk")


def _operands(x, w, x_cdim: int, w_cdim: int, mutant: Optional[str]) -> tuple:
    xh, xl = (t.double() for t in split(x))
    wh, wl = (t.double() for t in split(w))
    xl2 = xl                         # lo' of x in the lo'*hi cross term
    if mutant == "lo4":
        xl, wl = lo_4bits(xl), lo_4bits(wl)
        xl2 = xl
    elif mutant == "one_cross":
        xl2 = torch.zeros_like(xl)
    elif mutant == "last_chunk":
        c = x.shape[x_cdim]
        c0 = (c - 1) // 32 * 32
        xl = xl.clone()
        wl = wl.clone()
        xl.narrow(x_cdim, c0, c - c0).zero_()
        wl.narrow(w_cdim, c0, c - c0).zero_()
        xl2 = xl
    elif mutant is not None:
        raise ValueError(mutant)
    return xh, xl, xl2, wh, wl


@dataclass
class Result:
    y: torch.Tensor          # the model's output (fp64)
    acc: torch.Tensor        # exact sum of hi*hi
    cor: torch.Tensor        # exact sum of the cross terms
    bias: torch.Tensor       # broadcast bias (0 without)
    slope: torch.Tensor      # broadcast |PReLU slope| bound factor max(1, |slope|)
    res: torch.Tensor        # residual (0 without)
    abs_xw: torch.Tensor     # sum |x| |w| over the dequantised operands (statistical rule)
    kparts: Optional[torch.Tensor] = None   # sum over k-steps of |partial fold| (split-K bound), when asked for

    def exact_tol(self) -> torch.Tensor:
        """Elementwise bound for the exact family: the final epilogue roundings only."""
        return 4 * EPS32 * ((self.acc.abs() + self.cor.abs() / 1024 + self.bias.abs()) * self.slope + self.res.abs())

    def splitk_tol(self) -> torch.Tensor:
        """Exact family with split-K: every range folds acc + cor/1024 once and the reduce adds <= 8 of them in order, so the bound
        grows to (8 + 2) roundings of the sum of |partial folds| (each range is a union of k-steps)."""
        return 10 * EPS32 * ((self.kparts + self.bias.abs()) * self.slope + self.res.abs())


def _epilogue(acc, cor, bias, slope, residual, cdim_last: bool = True):
    y = acc + cor / 1024.0
    b = torch.zeros_like(y) if bias is None else bias.double().expand_as(y)
    y = y + b
    sl = torch.ones_like(y) if slope is None else slope.double().expand_as(y)
    if slope is not None:
        y = torch.where(y > 0, y, y * sl)
    r = torch.zeros_like(y) if residual is None else residual.double().expand_as(y)
    return y + r, b, sl.abs().clamp_min(1.0), r


def _prelu32(x: torch.Tensor, slope: torch.Tensor, cdim: int) -> torch.Tensor:
    """fp32 PReLU per input channel (the in_prelu of the loaders; x * slope rounds to fp32)."""
    shape = [1] * x.dim()
    shape[cdim] = -1
    s = slope.float().reshape(shape)
    return torch.where(x > 0, x, x * s)


# ------------------------------------------------------------------ contractions
def conv(x, w, bias=None, slope=None, stride=1, pad=1, dil=1, in_prelu=None, residual=None, mutant=None, kparts=False) -> Result:
    """Conv2d on NHWC fp32 ``x`` [N,H,W,Cin] with OIHW ``w``; output NHWC [N,Ho,Wo,Cout].  ``in_prelu``: per-input-channel PReLU
    before the split.  ``kparts``: also the per-(tap, 32-channel chunk) partial folds for the split-K bound."""
    x = x.float()
    if in_prelu is not None:
        x = _prelu32(x, in_prelu[:x.shape[3]], 3)
    xh, xl, xl2, wh, wl = _operands(x, w.float(), 3, 1, mutant)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    cv = lambda a, b: F.conv2d(nchw(a), b, stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1)
    acc = cv(xh, wh)
    cor = cv(xh, wl) + cv(xl2, wh)
    xd = xh + xl / 1024
    abs_xw = cv(xd.abs(), (wh + wl / 1024).abs())
    y, b, sl, r = _epilogue(acc, cor, bias, slope, residual)
    res = Result(y, acc, cor, b, sl, r, abs_xw)
    if kparts:
        cin, kh, kw = w.shape[1], w.shape[2], w.shape[3]
        ho, wo = acc.shape[1], acc.shape[2]
        pd = lambda a: F.pad(nchw(a), (pad, pad, pad, pad))
        ph, pl = pd(xh), pd(xl2)
        tot = torch.zeros_like(acc)
        taps = [(ky, kx) for ky in range(kh) for kx in range(kw)] if kparts != "chunk" else [None]
        for tap in taps:
            for c0 in range(0, cin, 32):
                cs = slice(c0, c0 + 32)
                if tap is None:       # whole 32-channel chunks with all their taps (conv3x3_planes' split-K ranges)
                    one = lambda a, b: cv(a[..., cs], b[:, cs])
                    part = one(xh, wh) + (one(xh, wl) + one(xl2, wh)) / 1024
                else:
                    ky, kx = tap
                    one = lambda a, b: F.conv2d(a[:, cs, ky * dil:, kx * dil:], b[:, cs, ky:ky + 1, kx:kx + 1],
                                                stride=stride)[:, :, :ho, :wo].permute(0, 2, 3, 1)
                    part = one(ph, wh) + (one(ph, wl) + one(pl, wh)) / 1024
                tot += part.abs()
        res.kparts = tot
    return res


def linear(x, w, bias=None, residual=None, mutant=None, kparts=False) -> Result:
    """x [M,K] fp32, w [Cout,K]: rows of the GEMM before any row group / scatter map (the caller places them)."""
    xh, xl, xl2, wh, wl = _operands(x.float(), w.float(), 1, 1, mutant)
    acc = xh @ wh.t()
    cor = xh @ wl.t() + xl2 @ wh.t()
    abs_xw = (xh + xl / 1024).abs() @ (wh + wl / 1024).abs().t()
    y, b, sl, r = _epilogue(acc, cor, bias, None, residual)
    res = Result(y, acc, cor, b, sl, r, abs_xw)
    if kparts:
        tot = torch.zeros_like(acc)
        for c0 in range(0, x.shape[1], 32):
            s = slice(c0, c0 + 32)
            tot += (xh[:, s] @ wh[:, s].t() + (xh[:, s] @ wl[:, s].t() + xl2[:, s] @ wh[:, s].t()) / 1024).abs()
        res.kparts = tot
    return res


def deconv2x2(x, w, bias=None, slope=None, in_prelu=None, mutant=None, kparts=False) -> Result:
    """ConvTranspose2d(k2, s2) of NHWC ``x`` [N,H,W,Cin] with IOHW ``w`` [Cin,Cout,2,2]: NHWC [N,2H,2W,Cout]."""
    x = x.float()
    if in_prelu is not None:
        x = _prelu32(x, in_prelu[:x.shape[3]], 3)
    xh, xl, xl2, wh, wl = _operands(x, w.float(), 3, 0, mutant)
    n, h, wd, _ = x.shape
    co = w.shape[1]

    def dc(a, b):
        t = torch.einsum("nijc,coab->niajbo", a, b)
        return t.reshape(n, 2 * h, 2 * wd, co)
    acc = dc(xh, wh)
    cor = dc(xh, wl) + dc(xl2, wh)
    abs_xw = dc((xh + xl / 1024).abs(), (wh + wl / 1024).abs())
    y, b, sl, r = _epilogue(acc, cor, bias, slope, None)
    res = Result(y, acc, cor, b, sl, r, abs_xw)
    if kparts:
        tot = torch.zeros_like(acc)
        for c0 in range(0, x.shape[3], 32):
            s = slice(c0, c0 + 32)
            tot += (dc(xh[..., s], wh[s]) + (dc(xh[..., s], wl[s]) + dc(xl2[..., s], wh[s])) / 1024).abs()
        res.kparts = tot
    return res


def head1x1(x, w, bias=None) -> torch.Tensor:
    """atmvfi_head1x1_planes: split activations (x = hi + lo'/1024, exact in fp32) times the UNSPLIT fp32 weight [Cout][Cin] in fp32
    FMAs; returned in fp64 (the FMA chain's rounding is the statistical rule's business)."""
    y = dequant(x) @ w.double().t()
    return y if bias is None else y + bias.double()


def attention(qkv, labels, bw, nw, ws, heads, hd, kv_shift, mutant=None):
    """window_attention_f16x3: S = Q K^T on the split of Q and K (acc + cor/1024), logits S / sqrt(hd) - 100 * (label_q != label_k),
    P = exp(logits - max) (unnormalised, <= 1) split again for P V with the split of V, divided by sum P.  Returns (out, motion, sum
    |P||V| / sum P) in fp64; ``qkv`` [Bw*N, 3C] in window order."""
    n, c = ws * ws, heads * hd
    t = qkv.float().reshape(bw, n, 3, heads, hd)
    src = (torch.arange(bw) + kv_shift) % bw
    q = t[:, :, 0].permute(0, 2, 1, 3)
    k = t[src, :, 1].permute(0, 2, 1, 3)
    v = t[src, :, 2].permute(0, 2, 1, 3)
    qh, ql, ql2, kh, kl = _operands(q, k, 3, 3, mutant)
    s = qh @ kh.transpose(-2, -1) + (qh @ kl.transpose(-2, -1) + ql2 @ kh.transpose(-2, -1)) / 1024
    s = s * (1.0 / math.sqrt(hd))
    if labels is not None:
        mask = (labels[:, :, None] != labels[:, None, :]).double() * -100.0
        s = (s.reshape(bw // nw, nw, heads, n, n) + mask[None, :, None]).reshape(bw, heads, n, n)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    den = p.sum(-1, keepdim=True)
    ph, pl, pl2, vh, vl = _operands(p.float(), v.transpose(-2, -1).contiguous(), 3, 3, mutant)
    vh, vl = vh.transpose(-2, -1), vl.transpose(-2, -1)
    o = (ph @ vh + (ph @ vl + pl2 @ vh) / 1024) / den
    absr = ((ph + pl / 1024).abs() @ (vh + vl / 1024).abs()) / den
    idx = torch.arange(n)
    cx, cy = (idx % ws).double(), (idx // ws).double()
    rel = torch.stack([cx[None, :] - cx[:, None], cy[None, :] - cy[:, None]])
    a = p / den
    m = (a[:, :, None] * rel[None, None]).sum(-1)
    return (o.transpose(1, 2).reshape(bw * n, c), m.permute(0, 3, 1, 2).reshape(bw * n, heads, 2),
            absr.transpose(1, 2).reshape(bw * n, c))


def naive_conv(x, w, bias, slope, stride, pad, dil):
    """Loop form of ``conv`` (fp64 sums of the split products) for small shapes: the model's own check."""
    xh, xl = (t.double() for t in split(x))
    wh, wl = (t.double() for t in split(w))
    n, h, wd, cin = x.shape
    co, _, kh, kw = w.shape
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (wd + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    y = torch.zeros(n, ho, wo, co, dtype=torch.float64)
    for b in range(n):
        for oy in range(ho):
            for ox in range(wo):
                for o in range(co):
                    acc = cor = 0.0
                    for ky in range(kh):
                        for kx in range(kw):
                            iy, ix = oy * stride - pad + ky * dil, ox * stride - pad + kx * dil
                            if not (0 <= iy < h and 0 <= ix < wd):
                                continue
                            for c in range(cin):
                                acc += float(xh[b, iy, ix, c] * wh[o, c, ky, kx])
                                cor += float(xh[b, iy, ix, c] * wl[o, c, ky, kx] + xl[b, iy, ix, c] * wh[o, c, ky, kx])
                    v = acc + cor / 1024 + (0.0 if bias is None else float(bias[o]))
                    if slope is not None and v <= 0:
                        v *= float(slope[o])
                    y[b, oy, ox, o] = v
    return y


# ------------------------------------------------------------------ exactness certificate
def _grid_exp(t: torch.Tensor) -> int:
    """Largest e with every element of fp16-valued ``t`` an integer multiple of 2^e (fp16 values are multiples of 2^-24)."""
    n = (t.double() * 2.0 ** 24).round().to(torch.int64)
    n = n[n != 0]
    if n.numel() == 0:
        return 64
    low = n & -n
    return int(torch.log2(low.double()).min().item()) - 24


def certificate(x, w, contract, ratio: float = 2.0 ** 24) -> dict:
    """Proof that no fp32 rounding can touch either accumulator: from split() of the ACTUAL operands, every term of acc is an integer
    multiple of q_acc = 2^(e(x_hi) + e(w_hi)) and every term of cor of q_cor = min(2^(e(x_hi) + e(w_lo')), 2^(e(x_lo') + e(w_hi))),
    and for every output sum |terms| <= 2^24 q.  Then each partial sum, whatever the order or grouping (MFMA blocks, k-steps,
    split-K ranges before their fold), is an integer multiple of q below 2^24 q: exact in fp32.  ``contract(a, b)`` is the contraction
    (a linear map in each argument) applied to same-layout fp64 operands."""
    xh, xl = (t.double() for t in split(x))
    wh, wl = (t.double() for t in split(w))
    finite = all(torch.isfinite(t).all() for t in (xh, xl, wh, wl))
    q_acc = _grid_exp(xh) + _grid_exp(wh)
    q_cor = min(_grid_exp(xh) + _grid_exp(wl), _grid_exp(xl) + _grid_exp(wh))
    s_acc = contract(xh.abs(), wh.abs()).max().item()
    s_cor = (contract(xh.abs(), wl.abs()) + contract(xl.abs(), wh.abs())).max().item()
    ok = bool(finite) and s_acc <= ratio * 2.0 ** q_acc and s_cor <= ratio * 2.0 ** q_cor
    return {"ok": ok, "q_acc": q_acc, "q_cor": q_cor, "sum_acc": s_acc, "sum_cor": s_cor}


def conv_contract(stride=1, pad=1, dil=1):
    return lambda a, b: F.conv2d(a.permute(0, 3, 1, 2), b, stride=stride, padding=pad, dilation=dil)


def linear_contract(a, b):
    return a @ b.t()


def deconv_contract(a, b):
    return torch.einsum("nijc,coab->nijoab", a, b)


# ------------------------------------------------------------------ input families
def exact(gen: torch.Generator, *shape, bmax: int = 127, bmin: int = 0) -> torch.Tensor:
    """hi = a 2^-3 (2 <= |a| <= 7, random sign), lo' = b 2^-11 (|b| <= bmax): x = hi + lo'/1024 is an fp32 value of <= 22 bits whose
    residual is below half an fp16 ulp of hi, so split(x) == (hi, lo') exactly.  bmax 127: K <= 9 000 keeps cor below 2^24 q;
    bmax 63: K <= 19 000.  bmin: smallest |b|."""
    a = torch.randint(2, 8, shape, generator=gen).double() * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    b = torch.randint(bmin, bmax + 1, shape, generator=gen).double() * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return (a * 2.0 ** -3 + b * 2.0 ** -21).float()


def exact_bias(gen: torch.Generator, n: int) -> torch.Tensor:
    """Bias on the acc grid (multiples of 2^-6)."""
    return (torch.randint(-64, 65, (n,), generator=gen).double() * 2.0 ** -6).float()


def pow2_slopes(gen: torch.Generator, n: int) -> torch.Tensor:
    """PReLU slopes that round nothing: 2^-3 .. 2^1 (and a few 0)."""
    e = torch.randint(-3, 2, (n,), generator=gen).double()
    s = 2.0 ** e
    s[torch.rand(n, generator=gen) < 0.1] = 0.0
    return s.float()


def wide(gen: torch.Generator, *shape, lo: float = -26.0, hi: float = 12.0) -> torch.Tensor:
    """Log-uniform magnitudes 2^lo .. 2^hi, random signs."""
    e = torch.rand(*shape, generator=gen).double() * (hi - lo) + lo
    s = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (s * 2.0 ** e).float()


def edge(gen: torch.Generator, *shape, frac: float = 0.25) -> torch.Tensor:
    """U(-1, 1) with a fraction ``frac`` of the elements replaced by the boundary values of the split (random signs)."""
    x = torch.rand(*shape, generator=gen) * 2 - 1
    vals = torch.tensor(EDGE_VALUES, dtype=torch.float32)
    pick = vals[torch.randint(0, len(EDGE_VALUES), shape, generator=gen)]
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return torch.where(torch.rand(*shape, generator=gen) < frac, pick * sign, x)


def cancel(gen: torch.Generator, x: torch.Tensor, w: torch.Tensor, cdim_x: int, cdim_w: int, rel: float = 2.0 ** -18):
    """Rows whose sum of x w is near 0 while sum |x||w| is large: the second half of the contraction channels repeats the first
    half of x (times 1 + O(rel)) against the NEGATED first half of w.  Needs an even channel count."""
    c = x.shape[cdim_x]
    h = c // 2
    x = x.clone()
    w = w.clone()
    xa = x.narrow(cdim_x, 0, h)
    x.narrow(cdim_x, h, h).copy_(xa * (1 + rel * (torch.rand(xa.shape, generator=gen) * 2 - 1)))
    w.narrow(cdim_w, h, h).copy_(-w.narrow(cdim_w, 0, h))
    return x, w


def stat_bound(abs_xw: torch.Tensor, cpu32_err: float) -> torch.Tensor:
    """The statistical rule of the wide / edge / cancel families (test_conv3x3_f16x3_large_and_ragged's): per element
    8 x max(largest error of plain fp32 on CPU against fp64 on the dequantised operands, 2^-24 sum |x||w|)."""
    return 8 * torch.clamp(EPS32 * abs_xw, min=cpu32_err)


# ------------------------------------------------------------------ the exact-family configurations of the GPU tests
def _case(id, kind, seed, **kw):
    return dict(id=id, kind=kind, seed=seed, **kw)


CASES_GEMM32 = [        # atmvfi_gemm f16x3 on fp32 input (gemm_f16x3.hip); "wns": forced tile widths
    _case("lin_M1000_N200_K100_res", "linear", 1, M=1000, K=100, N=200, bias=True, res=True, wns=[0, 1, 3, 8]),
    _case("lin_M1920_K96_scatter", "linear", 2, M=1920, K=96, N=96, bias=True, scatter=True),
    _case("conv_40to24_s2_inprelu", "conv", 3, NHW=(2, 10, 12), cin=40, cout=24, k=3, stride=2, pad=1, dil=1, bias=True, prelu=True,
          in_prelu=True),
    _case("conv_48to48_s4_d2", "conv", 4, NHW=(2, 24, 40), cin=48, cout=48, k=3, stride=4, pad=2, dil=2, bias=True, prelu=True),
    _case("conv_64to5_1x1", "conv", 5, NHW=(2, 10, 14), cin=64, cout=5, k=1, stride=1, pad=0, dil=1, bias=True),
    _case("deconv_128to64_inprelu", "deconv", 6, NHW=(2, 6, 10), cin=128, cout=64, bias=True, prelu=True, in_prelu=True),
]
CASES_PLANES = [        # atmvfi_gemm on split-plane input: gemm_split / gemm_pp / gemm_duo; "splitk": also with a workspace
    _case("lin_M1000_N200_K100_res", "linear", 11, M=1000, K=100, N=200, bias=True, res=True),
    _case("lin_M1920_K96_scatter", "linear", 12, M=1920, K=96, N=96, bias=True, scatter=True),
    _case("lin_M66000_N136_K64_persistent", "linear", 13, M=66000, K=64, N=136, bias=True, res=True),
    _case("lin_M512_N256_K2048_splitk", "linear", 14, M=512, K=2048, N=256, bias=True, res=True, splitk=True),
    _case("conv_two_sources_s2_splitk", "conv", 15, NHW=(1, 64, 64), cin=288, cout=128, k=3, stride=2, pad=1, dil=1, bias=True,
          prelu=True, two_sources=2, splitk=True),
    _case("conv_48to48_s4_d2", "conv", 16, NHW=(2, 24, 40), cin=48, cout=48, k=3, stride=4, pad=2, dil=2, bias=True, prelu=True),
    _case("conv_64to5_1x1", "conv", 17, NHW=(2, 10, 14), cin=64, cout=5, k=1, stride=1, pad=0, dil=1, bias=True),
    _case("deconv_101to101", "deconv", 18, NHW=(1, 15, 22), cin=101, cout=101, bias=True, prelu=True),
    _case("deconv_1024to61_splitk", "deconv", 19, NHW=(1, 32, 32), cin=1024, cout=61, bias=True, prelu=True, splitk=True),
]
CASES_CONV3 = [         # 3x3 / stride 1: conv3x3_f16x3 and conv3x3_planes; channel tails Cin % 32 = 1, 5, 8, 0
    _case("c3_33to20_tail1", "conv", 21, NHW=(2, 19, 21), cin=33, cout=20, k=3, stride=1, pad=1, dil=1, bias=True, prelu=True),
    _case("c3_37to123_tail5", "conv", 22, NHW=(2, 19, 21), cin=37, cout=123, k=3, stride=1, pad=1, dil=1, bias=True, prelu=True),
    _case("c3_40to48_tail8", "conv", 23, NHW=(1, 23, 17), cin=40, cout=48, k=3, stride=1, pad=1, dil=1, bias=True, prelu=True),
    _case("c3_64to123_tail0", "conv", 24, NHW=(2, 17, 33), cin=64, cout=123, k=3, stride=1, pad=1, dil=1, bias=True, prelu=True),
    _case("c3_712to352_splitk", "conv", 25, NHW=(1, 16, 16), cin=712, cout=352, k=3, stride=1, pad=1, dil=1, bias=True, prelu=True,
          kparts="chunk"),
]
CASE_CONV3_PERSISTENT = _case("c3_64to32_272x272", "conv", 26, NHW=(1, 272, 272), cin=64, cout=32, k=3, stride=1, pad=1, dil=1,
                              bias=True, prelu=True)
ALL_EXACT_CASES = CASES_GEMM32 + CASES_PLANES + CASES_CONV3 + [CASE_CONV3_PERSISTENT]


def case_operands(cfg) -> dict:
    """The seeded CPU operands of an exact-family configuration: x, w and the optional bias / slope / in_prelu / residual / row_map."""
    g = torch.Generator().manual_seed(1000 + cfg["seed"])
    bmax = cfg.get("bmax", 127)
    bmin = 0
    o = {}
    if cfg["kind"] == "linear":
        o["x"] = exact(g, cfg["M"], cfg["K"], bmax=bmax, bmin=bmin)
        o["w"] = exact(g, cfg["N"], cfg["K"], bmax=bmax, bmin=bmin)
        n = cfg["N"]
    else:
        nb, h, wd = cfg["NHW"]
        o["x"] = exact(g, nb, h, wd, cfg["cin"], bmax=bmax, bmin=bmin)
        o["w"] = exact(g, cfg["cout"], cfg["cin"], cfg["k"], cfg["k"], bmax=bmax, bmin=bmin) if cfg["kind"] == "conv" else \
            exact(g, cfg["cin"], cfg["cout"], 2, 2, bmax=bmax, bmin=bmin)
        n = cfg["cout"]
    if cfg.get("bias"):
        o["bias"] = exact_bias(g, n)
    if cfg.get("prelu"):
        o["slope"] = pow2_slopes(g, n)
    if cfg.get("in_prelu"):
        o["in_prelu"] = pow2_slopes(g, cfg["cin"])
    if cfg.get("res"):
        o["residual"] = exact_bias(g, cfg["M"] * n).reshape(cfg["M"], n)
    if cfg.get("scatter"):
        o["row_map"] = torch.randperm(cfg["M"], generator=g).to(torch.int32)
    return o


def case_model(cfg, o: dict, mutant=None) -> Result:
    kp = cfg.get("kparts") or bool(cfg.get("splitk"))
    if cfg["kind"] == "linear":
        return linear(o["x"], o["w"], o.get("bias"), o.get("residual"), mutant=mutant, kparts=kp)
    if cfg["kind"] == "conv":
        return conv(o["x"], o["w"], o.get("bias"), o.get("slope"), cfg["stride"], cfg["pad"], cfg["dil"], o.get("in_prelu"),
                    mutant=mutant, kparts=kp)
    return deconv2x2(o["x"], o["w"], o.get("bias"), o.get("slope"), o.get("in_prelu"), mutant=mutant, kparts=kp)


def case_contract(cfg):
    """The contraction of a configuration for ``certificate`` (operands as they reach the split: after in_prelu)."""
    if cfg["kind"] == "linear":
        return linear_contract
    if cfg["kind"] == "conv":
        return conv_contract(cfg["stride"], cfg["pad"], cfg["dil"])
    return deconv_contract


def case_split_operand(cfg, o: dict) -> torch.Tensor:
    x = o["x"]
    if "in_prelu" in o:
        x = _prelu32(x.float(), o["in_prelu"], 3)
    return x


_CACHE = {}


def build_case(cfg):
    """(x, w, model Result) of a configuration, cached per process; also fills cfg["dev_args"] (the optional operands to move to the
    device) and cfg["row_map_cpu"]."""
    key = cfg["id"] + cfg["kind"] + str(cfg["seed"])
    if key not in _CACHE:
        o = case_operands(cfg)
        _CACHE[key] = (o, case_model(cfg, o))
    o, res = _CACHE[key]
    cfg["dev_args"] = lambda x, w: {k: v for k, v in o.items() if k not in ("x", "w")}
    cfg["row_map_cpu"] = o.get("row_map")
    if cfg["kind"] == "linear":
        cfg["rows_out"] = cfg["M"]
    return o["x"], o["w"], res


def gather_rows(out: torch.Tensor, row_map: Optional[torch.Tensor]) -> torch.Tensor:
    """Output rows in GEMM row order (undo a scatter map that is a permutation)."""
    return out if row_map is None else out[row_map.long()]


def assert_split_of(planes, values, what: str, c0: int = 0):
    """The plane pair holds exactly split(values) in channels c0 .. c0 + C (rows x C fp32 values, any shape [..., C])."""
    v = values.detach().float().cpu()
    c = v.shape[-1]
    v = v.reshape(-1, c)
    hi, lo = split(v)
    got = planes.to_rows().cpu()[:, :v.shape[0], c0:c0 + c]
    same = lambda a, b: torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))
    assert same(got[0], hi), f"{what}: hi plane differs from split() of the fp32 result at {int((got[0].float() != hi.float()).sum())} places"
    assert same(got[1], lo), f"{what}: lo' plane differs from split() of the fp32 result at {int((got[1].float() != lo.float()).sum())} places"


# ------------------------------------------------------------------ exact chains: the fused stem and the fused refiner tail
# Both kernels chain layers on chip (stem.hip: three 3x3 layers, the two hidden maps in LDS; conv3x3_planes.hip + pointwise.hip: the
# activated tile of refine_head.0 times W2, then the nine shifted tap contributions), so a hidden layer cannot be observed.  The chain
# families below choose operands for which NO fp32 operation of a hidden layer rounds -- neither accumulator (``certificate``), nor
# the fold acc + cor/1024, nor + bias, nor the PReLU product, nor the re-split -- so the model predicts every hidden value bit for
# bit and the next layer's input is known exactly (``layer_exactness`` is that proof, tests/test_f16x3_model_cpu.py runs it for every
# case).  Budget: a value of b bits fed through a layer whose sum of |terms| is 2^g times its grid needs b + g <= 24 bits in the
# accumulator and <= 22 after the PReLU for the re-split, hence ternary weights, biases on 2^-1, hidden slopes {1, -1, 2}, 13-bit inputs.
STRUCTURAL_MUTANTS = ("pad_bias", "parity")
STEM_STRIDES = (1, 1, 2)


def stem_chain(x, params, mutant=None, mutant_layer=None) -> list:
    """feat_extracts.0.0 -> 0.1 -> 1.0 as three ``conv`` calls (3x3, pad 1, strides 1, 1, 2) on NHWC frames ``x`` [F,H,W,3], each
    fed with the fp32 value of the one before; ``params`` = three (weight OIHW, bias, slope).  -> the three ``Result``s.
    ``mutant`` in MUTANTS: that engine mutant in layer ``mutant_layer`` (0..2) only.  "pad_bias": hidden layer ``mutant_layer``
    (0 or 1) is PReLU(conv(0) + bias) outside the image instead of 0 (the next layer's zero padding).  "parity": layer 3 reads the
    layer-2 columns one to the right, i.e. at the other parity."""
    if mutant is not None and mutant not in MUTANTS + STRUCTURAL_MUTANTS:
        raise ValueError(mutant)
    out = []
    a = x.float()
    for i, ((w, b, p), st) in enumerate(zip(params, STEM_STRIDES)):
        m = mutant if (i == mutant_layer and mutant in MUTANTS) else None
        if mutant == "pad_bias" and i > 0 and mutant_layer == i - 1:
            pb, pp = params[i - 1][1].float(), params[i - 1][2].float()
            n, h, wd, c = a.shape
            ap = torch.where(pb > 0, pb, pb * pp).reshape(1, 1, 1, c).expand(n, h + 2, wd + 2, c).clone()
            ap[:, 1:-1, 1:-1] = a
            r = conv(ap, w, b, p, stride=st, pad=0)
        else:
            if mutant == "parity" and i == 2:
                a = torch.cat([a[:, :, 1:], torch.zeros_like(a[:, :, :1])], 2)
            r = conv(a, w, b, p, stride=st, pad=1, mutant=m)
        out.append(r)
        a = r.y.float()
    return out


def readout_matrix(wb) -> torch.Tensor:
    """refine_head.1's weight [3, C, 3, 3] as W2[(ky * 3 + kx) * 3 + o][c] (27 x C)."""
    return wb.float().permute(2, 3, 0, 1).reshape(27, wb.shape[1])


def tail_sum(contrib, n: int, h: int, w: int) -> torch.Tensor:
    """refine_tail's sum: ``contrib`` [n*h*w, 27] (column (ky * 3 + kx) * 3 + o) -> [n, 3, h, w], each output pixel adding the
    contributions of its nine neighbours p + (ky - 1, kx - 1) that lie inside the image, in (ky, kx) order."""
    t = contrib.double().reshape(n, h, w, 9, 3)
    pre = torch.zeros(n, h, w, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dy, dx = ky - 1, kx - 1
            y0, y1, x0, x1 = max(0, -dy), h - max(0, dy), max(0, -dx), w - max(0, dx)
            pre[:, y0:y1, x0:x1] += t[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx, ky * 3 + kx]
    return pre.permute(0, 3, 1, 2).contiguous()


def tail_chain(x_planes_values, wa, ba, pa, wb, mutant=None, which=None, terms: int = 3) -> tuple:
    """atmvfi_conv3p's read-out + the sum of atmvfi_refine_tail on the plane values ``x`` [n,h,w,Cin]: ``conv`` for
    refine_head.0 (wa, ba, pa), ``linear`` of its activated rows (fp32) with W2 = ``readout_matrix(wb)`` -- the 27 tap contributions
    per pixel, what ``contrib`` holds, transposed -- and their sum per output pixel (no bias: refine_tail adds it).  -> (Result of the
    conv, Result of the W2 product [n*h*w, 27], summed pre-activation [n,3,h,w]).  ``mutant`` goes into product ``which`` (0: the
    conv, 1: W2).  ``terms`` = 1: the main product on hi(x), hi(w) (the f16 mode, tests/f16_model.py); W2 stays three-term."""
    x = x_planes_values.float()
    n, h, w, _ = x.shape
    if terms == 1:
        x, wa = split(x)[0].float(), split(wa)[0].float()
    ra = conv(x, wa, ba, pa, mutant=mutant if which == 0 else None)
    rc = linear(ra.y.float().reshape(n * h * w, -1), readout_matrix(wb), mutant=mutant if which == 1 else None)
    return ra, rc, tail_sum(rc.y, n, h, w)


def _is_f32(t: torch.Tensor) -> bool:
    return bool((t.float().double() == t).all())


def layer_exactness(x, w, res: Result, contract, resplit: bool = True) -> dict:
    """Is the layer ``res`` = model(x, w) EXACT in the kernel's fp32 arithmetic?  ``cert``: no rounding in either accumulator
    (``certificate`` on the operands actually used); ``fold`` / ``bias`` / ``prelu``: acc + cor/1024, + bias and the PReLU product
    are fp32 values (so whatever way the compiler contracts them, each step is exact); ``resplit``: hi + lo'/1024 of the fp32
    result is the result.  ``ok``: all of them.  Also the share of the activation operand with lo' != 0 and of negative
    pre-activations (conditions on the inputs: a chain whose lo' is all zero, or whose PReLU never multiplies, tests less)."""
    cert = certificate(x, w, contract)
    fold = res.acc + res.cor / 1024.0
    pre = fold + res.bias
    d = {"cert": cert["ok"], "fold": _is_f32(fold), "bias": _is_f32(pre), "prelu": _is_f32(res.y),
         "resplit": (not resplit) or bool((dequant(res.y.float()) == res.y).all()),
         "lo_share": float((split(x)[1] != 0).double().mean()), "neg_share": float((pre < 0).double().mean()), "certificate": cert}
    d["ok"] = all(d[k] for k in ("cert", "fold", "bias", "prelu", "resplit"))
    return d


def sum_exactness(contrib, n, h, w, bias, slope) -> dict:
    """refine_tail's nine-term sum, + bias and PReLU product on exact contributions: every partial sum is a multiple of the
    contributions' grid q below 2^24 q (so no order of adding rounds), and the two epilogue steps are fp32 values."""
    c = contrib.double()
    k = (c * 2.0 ** 40).round().to(torch.int64)          # the contributions are multiples of 2^-40 below 2^20 (asserted)
    assert bool((k.double() * 2.0 ** -40 == c).all()) and float(c.abs().max()) < 2.0 ** 20
    k = k[k != 0]
    q = 2.0 ** (int(torch.log2((k & -k).double()).min().item()) - 40) if k.numel() else 1.0
    pre = tail_sum(c, n, h, w)
    sabs = tail_sum(c.abs(), n, h, w)
    b = bias.double().reshape(1, 3, 1, 1)
    s = slope.double().reshape(1, 3, 1, 1)
    v = pre + b
    y = torch.where(v > 0, v, v * s)
    d = {"sum": float(sabs.max()) <= 2.0 ** 24 * q, "bias": _is_f32(v), "prelu": _is_f32(y), "q": q, "sum_abs": float(sabs.max()),
         "neg_share": float((v < 0).double().mean())}
    d["ok"] = d["sum"] and d["bias"] and d["prelu"]
    return d


def ternary(gen: torch.Generator, *shape, period: int, keep: int = 1, phase: int = 0) -> torch.Tensor:
    """Weights in {-1, 0, +1}, signs from ``gen``: position i is nonzero where (r_i + phase) % period < keep, with r_i drawn from
    a seed of the SHAPE alone -- density keep / period, and the cases of ``period`` consecutive phases reach every position."""
    r = torch.randint(0, period, shape, generator=torch.Generator().manual_seed(7919 * period + math.prod(shape)))
    s = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (s * (((r + phase) % period) < keep)).float()


def chain_values(gen: torch.Generator, *shape, signed: bool = False, amin: int = 1, amax: int = 7) -> torch.Tensor:
    """13-bit inputs a 2^-3 + b 2^-13 (amin <= a <= amax, |b| <= 7): hi = fp16 keeps 11 bits, so lo' != 0 wherever |x| >= 1/4 and b is not
    a multiple of the fp16 ulp there (2^-12 below 1/2, 2^-11 above).  Coarser than ``exact``'s 2^-21 on purpose: three layers deep the
    sums must still fit 24 bits."""
    a = torch.randint(amin, amax + 1, shape, generator=gen).double()
    b = torch.randint(-7, 8, shape, generator=gen).double()
    x = a * 2.0 ** -3 + b * 2.0 ** -13
    if signed:
        x = x * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return x.float()


def half_bias(gen: torch.Generator, n: int, amax: int = 4) -> torch.Tensor:
    return (torch.randint(-amax, amax + 1, (n,), generator=gen).double() * 0.5).float()


def chain_slopes(gen: torch.Generator, n: int, choices=(1.0, -1.0, 2.0)) -> torch.Tensor:
    """PReLU slopes whose product keeps the grid (a hidden layer's 1/2 would cost the next layer one of its 24 bits; the last
    layer of a chain may take it)."""
    return torch.tensor(choices, dtype=torch.float32)[torch.randint(0, len(choices), (n,), generator=gen)]


CHAIN_FAMILIES = ("chain_exact", "chain_rich_last")
STEM_SHAPES = [(1, 2, 2), (1, 16, 32), (1, 18, 34), (1, 36, 52), (3, 70, 34), (3, 176, 256), (4, 176, 384)]      # F, H, W (full resolution)
STEM_PERIODS = (5, 4, 3, 7)             # layer 1: 4 of 5 weights nonzero; layers 2, 3: 1 of 3, 1 of 7
CASES_STEM = [_case(f"stem_{c0}_{c1}_f{f}_{h}x{w}", "stem", 40 + 10 * (c0 == 16) + i, c0=c0, c1=c1, FHW=(f, h, w), phase=i,
                    nan_lane=(i == 3))
              for c0, c1 in ((24, 48), (16, 32)) for i, (f, h, w) in enumerate(STEM_SHAPES)]
TAIL_SHAPES = [(64, 32, 1, 16, 16), (128, 64, 2, 17, 50), (64, 32, 2, 21, 35), (128, 64, 1, 40, 72), (64, 32, 1, 272, 272),
               (128, 64, 1, 16, 16), (64, 32, 2, 17, 50), (128, 64, 2, 21, 35)]             # Cin, C, n, h, w
TAIL_PERIODS = (4, 2)                   # refine_head.0: 1 of 4 weights nonzero; W2: 1 of 2
CASES_TAIL = [_case(f"tail_{cin}_{c}_n{n}_{h}x{w}", "tail", 70 + i, cin=cin, c=c, NHW=(n, h, w), phase=i // 2)
              for i, (cin, c, n, h, w) in enumerate(TAIL_SHAPES)]
CASE_TAIL_F16 = dict(CASES_TAIL[2], id=CASES_TAIL[2]["id"] + "_terms1", terms=1)


def stem_operands(cfg, family: str) -> dict:
    """Seeded operands of a stem case: frames ``x`` [F,H,W,3] and ``params``, three (weight, bias, slope).  Both families share the
    frames and the two hidden layers; ``chain_rich_last`` replaces layer 3 by full-precision operands (``exact`` weights with their
    7-bit lo' in the even cases, uniform ones in the odd cases; uniform bias and slopes)."""
    assert family in CHAIN_FAMILIES
    g = torch.Generator().manual_seed(2000 + cfg["seed"])
    c0, c1, (f, h, w), ph = cfg["c0"], cfg["c1"], cfg["FHW"], cfg["phase"]
    x = chain_values(g, f, h, w, 3, amin=2, amax=3)
    p5, k5, p2, p3 = STEM_PERIODS
    ws = [ternary(g, c0, 3, 3, 3, period=p5, keep=k5, phase=ph), ternary(g, c0, c0, 3, 3, period=p2, phase=ph),
          ternary(g, c1, c0, 3, 3, period=p3, phase=ph)]
    bs = [half_bias(g, c) for c in (c0, c0, c1)]
    # two channels of layer 1 sit near +-9: there the 13-bit grid leaves lo' five significant bits, which is what lets the lo4
    # mutant (a 4-bit lo' operand) show in layer 2 at all
    bs[0][(ph + 1) % c0], bs[0][(ph + 9) % c0] = 8.5, -9.0
    ps = [chain_slopes(g, c0), chain_slopes(g, c0), chain_slopes(g, c1, (1.0, 0.5, -1.0, 2.0))]
    if family == "chain_rich_last":
        g2 = torch.Generator().manual_seed(3000 + cfg["seed"])
        ws[2] = exact(g2, c1, c0, 3, 3) * 0.25 if ph % 2 == 0 else (torch.rand(c1, c0, 3, 3, generator=g2) * 2 - 1) * 0.25
        bs[2] = (torch.rand(c1, generator=g2) * 2 - 1) * 0.3
        ps[2] = 0.25 + (torch.rand(c1, generator=g2) * 2 - 1) * 0.2
    return {"x": x, "params": list(zip(ws, bs, ps))}


def tail_operands(cfg, family: str) -> dict:
    """Seeded operands of a tail case: plane values ``x`` [n,h,w,Cin], refine_head.0 (wa, ba, pa), refine_head.1 (wb, bb, pb) and
    ``it`` [n,3,h,w].  W2 is ternary x 2^-6 (the sigmoid's argument stays O(1)) in ``chain_exact``; in ``chain_rich_last`` it is
    ``exact`` x 2^-6 (even cases) or uniform (odd cases) with uniform bias and slope."""
    assert family in CHAIN_FAMILIES
    g = torch.Generator().manual_seed(2000 + cfg["seed"])
    cin, c, (n, h, w), ph = cfg["cin"], cfg["c"], cfg["NHW"], cfg["phase"]
    pa_, pb_ = TAIL_PERIODS
    o = {"x": chain_values(g, n, h, w, cin, signed=True), "wa": ternary(g, c, cin, 3, 3, period=pa_, phase=ph), "ba": half_bias(g, c),
         "pa": chain_slopes(g, c), "wb": ternary(g, 3, c, 3, 3, period=pb_, phase=ph) * 2.0 ** -6, "bb": half_bias(g, 3, 2),
         "pb": chain_slopes(g, 3, (1.0, 0.5, 2.0)), "it": torch.rand(n, 3, h, w, generator=g)}
    if family == "chain_rich_last":
        g2 = torch.Generator().manual_seed(3000 + cfg["seed"])
        o["wb"] = exact(g2, 3, c, 3, 3) * 2.0 ** -6 if ph % 2 == 0 else (torch.rand(3, c, 3, 3, generator=g2) * 2 - 1) * 2.0 ** -6
        o["bb"] = (torch.rand(3, generator=g2) * 2 - 1) * 0.2
        o["pb"] = 0.25 + (torch.rand(3, generator=g2) * 2 - 1) * 0.2
    return o


def build_chain(cfg, family: str, mutant=None, where=None) -> dict:
    """Operands + model of a chain case (cached per process without a mutant).  stem: "res" = the three Results; tail: "ra", "rc",
    "pre" of ``tail_chain``."""
    key = (cfg["id"], family)
    if mutant is None and key in _CACHE:
        return _CACHE[key]
    if cfg["kind"] == "stem":
        o = stem_operands(cfg, family)
        o["res"] = stem_chain(o["x"], o["params"], mutant, where)
    else:
        o = tail_operands(cfg, family)
        o["ra"], o["rc"], o["pre"] = tail_chain(o["x"], o["wa"], o["ba"], o["pa"], o["wb"], mutant, where, cfg.get("terms", 3))
    if mutant is None:
        _CACHE[key] = o
    return o


def stem_exactness(o: dict, layers=(0, 1, 2)) -> list:
    """``layer_exactness`` of the given layers of a built stem case (each on the operands that layer actually sees)."""
    out = []
    a = o["x"]
    for i, ((w, b, p), st, r) in enumerate(zip(o["params"], STEM_STRIDES, o["res"])):
        if i in layers:
            out.append(layer_exactness(a, w, r, conv_contract(st, 1, 1), resplit=i < 2))
        a = r.y.float()
    return out


def split_quantisation(y: torch.Tensor) -> torch.Tensor:
    """Bound of |hi + lo'/1024 - v| for an fp32 v near ``y`` inside fp16's range: both halves round to nearest, ~22 significant bits
    (2^-21 relative, as tests/test_gpu_ops.py holds the split to), and lo'/1024 has the absolute granularity 2^-34."""
    return 2.0 ** -21 * y.abs() + 2.0 ** -34


# ------------------------------------------------------------------ the bounds the GPU chain tests apply (shared with the CPU teeth)
def stem_last_bound(o: dict) -> torch.Tensor:
    """``chain_rich_last``: elementwise bound of |planes.to_float() - y3|.  Layer 3's input is known exactly, so this is the
    statistical rule on layer 3 alone -- cpu32_err derived as test_statistical_families does, plain fp32 on the CPU on the
    dequantised operands against the model -- plus the quantisation of the output split."""
    (w, b, p), r = o["params"][2], o["res"][2]
    xd = dequant(o["res"][1].y.float()).float().permute(0, 3, 1, 2)
    cpu32 = F.prelu(F.conv2d(xd, dequant(w).float(), b.float(), stride=2, padding=1), p.float()).permute(0, 2, 3, 1)
    return stat_bound(r.abs_xw, (cpu32.double() - r.y).abs().max().item()) + split_quantisation(r.y)


def tail_contrib_bound(o: dict, fold_exact: bool) -> torch.Tensor:
    """Elementwise bound of |contrib^T - rc.y| [n*h*w, 27].  The activated tile is known exactly, so only W2's product counts: where
    its certificate holds the epilogue roundings (``exact_tol``; 0 where the fold is exact too: bit for bit), else the statistical
    rule with plain fp32 on the CPU as the yardstick."""
    rc = o["rc"]
    act, w2 = o["ra"].y.float().reshape(rc.y.shape[0], -1), readout_matrix(o["wb"])
    if certificate(act, w2, linear_contract)["ok"]:
        return torch.zeros_like(rc.y) if fold_exact else rc.exact_tol()
    cpu32 = dequant(act).float() @ dequant(w2).float().t()
    return stat_bound(rc.abs_xw, (cpu32.double() - rc.y).abs().max().item())


def tail_preact(o: dict, n: int, h: int, w: int, contrib_bound: torch.Tensor) -> tuple:
    """-> (r, bound of the kernel's r): r = PReLU(sum of the nine contributions + bias) of the model in fp64 [n,3,h,w], and how far
    refine_tail's fp32 r can be from it: the contributions' own bounds, summed like the contributions, plus 11 roundings (nine
    additions, the bias, the PReLU product) of at most 2^-24 (sum |contributions| + |bias|) each, all times max(1, |slope|).  Exactly 0
    where ``sum_exactness`` holds and the contributions are exact."""
    b, s = o["bb"].double().reshape(1, 3, 1, 1), o["pb"].double().reshape(1, 3, 1, 1)
    v = o["pre"] + b
    r = torch.where(v > 0, v, v * s)
    if float(contrib_bound.max()) == 0.0:
        return r, torch.zeros_like(r)
    rb = (tail_sum(contrib_bound, n, h, w) + 11 * EPS32 * (tail_sum(o["rc"].y.abs(), n, h, w) + b.abs())) * s.abs().clamp_min(1.0)
    return r, rb
