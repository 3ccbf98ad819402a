"""float64 reference, derived bounds, fp32 emulations with mutants and input builders for window attention (csrc/attention.hip) --
CPU only, test infrastructure only.  tests/test_attention_ref_cpu.py shows that the bounds hold for well-behaved fp32 arithmetic and
that each mutant leaves them; tests/test_gpu_attention_fp64.py holds the two kernels to them.

The operation: qkv [Bw*N, 3C] in window order (N = ws^2, C = heads * hd; q, k, v thirds; head h at columns h*hd), window b attends to
the K/V rows of window (b + kv_shift) % Bw, logits l = q.k / sqrt(hd) - 100 * (label_q != label_k) with labels[b % nW], softmax over
the N keys, out = sum_k a_k v_k, motion = sum_k a_k (k_xy - q_xy) with token t at (t % ws, t // ws).

Bounds, U = 2^-24, first order.  A logit is known to dl <= U (c A + |l|) with A_k = sum_d |q_d k_d| / sqrt(hd) (c roundings of the
dot product, one of the scaling, one of the mask add); a normalised weight a_k = e^{l_k} / sum_j e^{l_j} moves by
a_k (dl_k - sum_j a_j dl_j), i.e. the logit error enters TWICE, so with R = max_k (A_k + |l_k|) per (row, head)

    B32        = K U absr (8 + 2 R)                       exact-fp32 kernel against attention64; absr = sum_k a_k |v_k|
    B32 motion = K U max(absm, 1) (8 + 2 R)               absm = sum_k a_k k_xy + q_xy >= 0 (the form the x3 kernel computes)
    Bx3        = K (U absr_model (8 + 2 R) + 2^-34 sum_k |v_k| / den)       f16x3 kernel against f16x3_model.attention
    Bx3 motion = K (U max(absm, 1) (8 + 2 R) + 2^-34 sum_k k_xy / den)      (the key positions are four more V columns)
    Bx3/fp64   = K (Bx3[absr, K = 1] + 2^-22 absr (1 + 2 max_k A_k) + 2^-35)  f16x3 kernel against attention64 (the walk test)

the 8 being one rounding per product and add of the rest (exp, sum, reciprocal, P V, the fold acc + cor / 1024), K the constant that
absorbs c and the accumulation orders.  The 2^-34 term is real: the kernel splits the UNNORMALISED numerators p = e^{l - max} in
(0, 1] to fp16 hi + lo'/1024, and lo' goes subnormal (grid 2^-24) for small p, so p is only known to 2^-34 absolutely; the kernel's
fp32 p and the model's p can round to different sides of that grid, whatever U absr says (den = sum_k p_k >= 1 divides it).  The
2^-22 term of the last bound is the three-term product of the f16x3 arithmetic itself (lo' * lo' is never formed): once on P V and,
through the logits, twice on Q K.  Its 2^-35 was not in the formula this work started from: below 2^-14 BOTH halves of a split V
element are subnormal, so V itself is carried to half a grid step of 2^-34 absolutely, not to 22 bits (ws 1, Q = 0, where the output
IS one V element, showed 39x the bound without it; the model, which splits like the library, is not affected).

K is NOT fitted to a kernel: it is the smallest power of two at least twice the worst ratio of an fp32 CPU emulation of the same
pipeline (``emulate32`` / ``emulate_x3``: torch fp32 matmuls, whose accumulation order is not the MFMA's) against the bound with
K = 1, over every input of the GPU tests (the x3-vs-fp64 bound: over the walk inputs, the only ones it is used on).  Measured
(tests/test_attention_ref_cpu.py asserts worst <= K / 2 and reports the figures through record_property):

    emulate32  / B32          1.53 (hot ws 9 / hd 72)    -> K32 = 4          motion 0.58 (hot ws 13 / hd 68) -> K32_MOTION = 2
    emulate_x3 / Bx3          1.15 (hot ws 11 / hd 84)   -> KX3 = 4          motion 0.54 (hot ws 14 / hd 64) -> KX3_MOTION = 2
    emulate_x3 / Bx3/fp64     0.27 (walk ws 8 / hd 72), motion 0.11          -> KX3_FP64 = 1; the model / the same bound: 0.08, 0.05

-100 is not -inf: a masked key at logit +60 - 100 beats an unmasked one at -60, and the ``hot`` family plants such a row in every
input that has labels (asserted: a masked key with a normalised weight above 1e-3), so a kernel that masked with -inf fails.
"""
from __future__ import annotations

import importlib
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

import f16x3_model as M

windows = importlib.import_module("atm-vfi_amd.windows")

U = 2.0 ** -24
PGRID = 2.0 ** -34            # the absolute grid of a split softmax numerator (fp16 lo' subnormal, / 1024)
SPLIT3 = 2.0 ** -22           # the three-term f16x3 product against the full one
VGRID = 2.0 ** -35            # half the absolute grid of a split V element (hi and lo' both subnormal below 2^-14)
LOG2E = 1.4426950408889634
LDS_LIMIT = 160 * 1024
HEADS = 8

# one constant per bound: the smallest power of two >= 2 x the worst CPU-emulation ratio (module docstring, DESIGN_NOTES)
K32, K32_MOTION, KX3, KX3_MOTION, KX3_FP64 = 4.0, 2.0, 4.0, 2.0, 1.0


# ------------------------------------------------------------------ what the launchers decide (launch_attn / launch_attn_x3)
def tiles(ws: int) -> int:
    return (ws * ws + 15) // 16


def dch(hd: int) -> int:
    return (hd + 31) // 32


def lds_bytes(engine: str, ws: int, hd: int, motion: bool) -> int:
    """Dynamic LDS of a launch, as launch_attn / launch_attn_x3 compute it."""
    npad = 16 * tiles(ws)
    if engine == "f32":
        dpad = (hd + 15) // 16 * 16
        return (npad * ((dpad // 4 + 15) // 16 * 16) * 4 + dpad * ((npad // 4 + 15) // 16 * 16) * 4 + npad) * 4
    d32, dt, vrows = dch(hd), (hd + (4 if motion else 0) + 15) // 16, 32 * ((tiles(ws) + 1) // 2)
    ks = (4 if d32 <= 1 else 8 if d32 == 2 else 16) * 16
    vs = 32 * dt + (0 if dt & 1 else 32)
    return 2 * npad * ks + 2 * vrows * vs + npad * 4


def admissible(engine: str, ws: int, hd: int, motion: bool = True) -> bool:
    return (1 <= ws <= 16 and hd % 4 == 0 and 0 < hd <= (64 if tiles(ws) >= 13 else 128)
            and lds_bytes(engine, ws, hd, motion) <= LDS_LIMIT)


def key_xy(ws: int) -> torch.Tensor:
    """[N, 2] fp64: token t sits at (t % ws, t // ws)."""
    idx = torch.arange(ws * ws)
    return torch.stack([idx % ws, idx // ws], -1).double()


# ------------------------------------------------------------------ window subsets
def gather_windows(qkv, labels, bw: int, nw: int, n: int, kv_shift: int, wins: Sequence[int]):
    """The sub-problem of windows ``wins``: their q rows beside the k / v rows of windows (b + kv_shift) % Bw, one label row per
    window.  Returns (qkv', labels', Bw' = nW' = len(wins), kv_shift' = 0); output row i*N + t is row wins[i]*N + t of the whole."""
    c3 = qkv.shape[1]
    c = c3 // 3
    w = torch.as_tensor(list(wins), dtype=torch.long)
    t = qkv.reshape(bw, n, c3)
    sub = torch.cat([t[w][:, :, :c], t[(w + kv_shift) % bw][:, :, c:]], -1).reshape(len(w) * n, c3).contiguous()
    lab = None if labels is None else labels[w % nw].contiguous()
    return sub, lab, len(w), len(w), 0


def rows_of(wins: Sequence[int], n: int) -> torch.Tensor:
    """Row indices [len(wins) * N] of the windows in a whole [Bw*N, ...] tensor."""
    w = torch.as_tensor(list(wins), dtype=torch.long)
    return (w[:, None] * n + torch.arange(n)[None, :]).reshape(-1)


def _heads_view(qkv, bw, n, heads, hd, kv_shift, dtype):
    t = qkv.to(dtype).reshape(bw, n, 3, heads, hd)
    src = (torch.arange(bw) + kv_shift) % bw
    return t[:, :, 0].permute(0, 2, 1, 3), t[src, :, 1].permute(0, 2, 1, 3), t[src, :, 2].permute(0, 2, 1, 3)


def _mask(labels, bw, nw):
    """[Bw, 1, N, N] bool: label_q != label_k with labels[b % nW]; None without labels."""
    if labels is None:
        return None
    lab = labels[torch.arange(bw) % nw]
    return (lab[:, :, None] != lab[:, None, :])[:, None]


# ------------------------------------------------------------------ the float64 reference
@dataclass
class Ref64:
    out: torch.Tensor        # [rows, C]
    motion: torch.Tensor     # [rows, heads, 2]
    absr: torch.Tensor       # [rows, C]         sum_k a_k |v_k|
    absm: torch.Tensor       # [rows, heads, 2]  sum_k a_k k_xy + q_xy
    R: torch.Tensor          # [rows, heads]     max_k (A_k + |l_k|)
    amax: torch.Tensor       # [rows, heads]     max_k A_k
    vsum_den: torch.Tensor   # [rows, C]         sum_k |v_k| / den, den = sum_k e^{l_k - max}
    kxy_den: torch.Tensor    # [rows, heads, 2]  sum_k k_xy / den
    masked_wmax: float       # largest normalised weight of a masked key
    logit_absmax: float      # largest |q.k| / sqrt(hd) (before the mask)

    def per_channel(self, t: torch.Tensor) -> torch.Tensor:
        """[rows, heads] -> [rows, C]."""
        hd = self.out.shape[1] // t.shape[1]
        return t[:, :, None].expand(-1, -1, hd).reshape(t.shape[0], -1)


def attention64(qkv, labels, bw: int, nw: int, ws: int, heads: int, hd: int, kv_shift: int,
                windows: Optional[Sequence[int]] = None) -> Ref64:
    """Plain float64 window attention on the fp32 inputs.  ``windows``: only those (rows in that order); window b needs its own rows
    and those of window (b + kv_shift) % Bw.  ``labels``: int [nW, N] (a geometry's or synthetic) or None."""
    n = ws * ws
    if windows is not None:
        qkv, labels, bw, nw, kv_shift = gather_windows(qkv, labels, bw, nw, n, kv_shift, windows)
    q, k, v = _heads_view(qkv, bw, n, heads, hd, kv_shift, torch.float64)
    rs = 1.0 / math.sqrt(hd)
    dot = (q @ k.transpose(-2, -1)) * rs
    a_k = (q.abs() @ k.abs().transpose(-2, -1)) * rs
    mask = _mask(labels, bw, nw)
    l = dot if mask is None else dot - 100.0 * mask.double()
    p = torch.exp(l - l.max(-1, keepdim=True).values)
    den = p.sum(-1, keepdim=True)
    a = p / den
    kxy = key_xy(ws)
    ek = a @ kxy                                                   # [Bw, heads, N, 2]
    rows = lambda t: t.transpose(1, 2).reshape(bw * n, -1)
    rows_h = lambda t: t.permute(0, 2, 1, 3).reshape(bw * n, heads, -1)
    return Ref64(out=rows(a @ v), motion=rows_h(ek - kxy), absr=rows(a @ v.abs()), absm=rows_h(ek + kxy),
                 R=rows_h((a_k + l.abs()).max(-1, keepdim=True).values)[..., 0], amax=rows_h(a_k.max(-1, keepdim=True).values)[..., 0],
                 vsum_den=rows(v.abs().sum(-2, keepdim=True) / den), kxy_den=rows_h(kxy.sum(0) / den),
                 masked_wmax=0.0 if mask is None else float((a * mask).max()), logit_absmax=float(dot.abs().max()))


# ------------------------------------------------------------------ the bounds (module docstring)
def bound32(ref: Ref64, K: float = K32) -> torch.Tensor:
    return K * U * ref.absr * (8 + 2 * ref.per_channel(ref.R))


def bound32_motion(ref: Ref64, K: float = K32_MOTION) -> torch.Tensor:
    return K * U * ref.absm.clamp_min(1.0) * (8 + 2 * ref.R[..., None])


def bound_x3(ref: Ref64, absr_model: torch.Tensor, K: float = KX3) -> torch.Tensor:
    return K * (U * absr_model * (8 + 2 * ref.per_channel(ref.R)) + PGRID * ref.vsum_den)


def bound_x3_motion(ref: Ref64, K: float = KX3_MOTION) -> torch.Tensor:
    return K * (U * ref.absm.clamp_min(1.0) * (8 + 2 * ref.R[..., None]) + PGRID * ref.kxy_den)


def bound_x3_fp64(ref: Ref64, K: float = KX3_FP64) -> torch.Tensor:
    """One K on the whole expression (its Bx3 part is taken at K = 1, not at KX3)."""
    return bound_x3(ref, ref.absr, K) + K * (SPLIT3 * ref.absr * (1 + 2 * ref.per_channel(ref.amax)) + VGRID)


def bound_x3_fp64_motion(ref: Ref64, K: float = KX3_FP64) -> torch.Tensor:
    return bound_x3_motion(ref, K) + K * SPLIT3 * ref.absm.clamp_min(1.0) * (1 + 2 * ref.amax[..., None])


def worst(err: torch.Tensor, bound: torch.Tensor) -> float:
    """Largest err / bound; an element with bound 0 must have err 0."""
    assert bool(((bound > 0) | (err == 0)).all()), "a non-zero error where the bound is 0"
    return float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------ fp32 restatements of the two pipelines, with mutants
MUTANTS_BOTH = ("mask_inf", "pad_keys_unmasked", "labels_of_window_0", "scale_of_padded_hd", "motion_q_of_tile")
MUTANTS_X3_ONLY = ("p_hi_only", "v_lo_other_window")
MUTANTS32, MUTANTS_X3 = MUTANTS_BOTH, MUTANTS_BOTH + MUTANTS_X3_ONLY


def _emulation_setup(qkv, labels, bw, nw, ws, heads, hd, kv_shift, mutant, windows, allowed):
    if mutant is not None and mutant not in allowed:
        raise ValueError(mutant)
    n = ws * ws
    if mutant == "labels_of_window_0" and labels is not None:
        labels = labels[:1].expand(nw, n)
    if windows is not None:
        qkv, labels, bw, nw, kv_shift = gather_windows(qkv, labels, bw, nw, n, kv_shift, windows)
    q, k, v = _heads_view(qkv, bw, n, heads, hd, kv_shift, torch.float32)
    hd_scale = 32 * dch(hd) if mutant == "scale_of_padded_hd" else hd
    scale = np.float32(1.0) / np.sqrt(np.float32(hd_scale))          # launch_attn: 1.0f / sqrtf((float)hd)
    kxy = key_xy(ws).float()
    qxy = kxy[torch.arange(n) % 16] if mutant == "motion_q_of_tile" else kxy
    return bw, n, q, k, v, _mask(labels, bw, nw), scale, kxy, qxy


def _masked_logits(s, mask, minus, n, ws, mutant):
    """Add the mask (``minus``, or -inf for the mutant); the mutant's 16 NT - N padded keys join max and sum at logit 0."""
    if mask is not None:
        s = s + torch.where(mask, torch.tensor(-math.inf if mutant == "mask_inf" else minus, dtype=torch.float32), torch.tensor(0.0))
    npad = 16 * tiles(ws) - n
    if mutant == "pad_keys_unmasked" and npad:
        s = torch.cat([s, torch.zeros(*s.shape[:-1], npad)], -1)
    return s


def _rows(o, m, bw, n, heads):
    return o.transpose(1, 2).reshape(bw * n, -1), m.permute(0, 2, 1, 3).reshape(bw * n, heads, 2)


def emulate32(qkv, labels, bw, nw, ws, heads, hd, kv_shift, mutant: Optional[str] = None, windows=None):
    """window_attn_kernel in fp32 torch: S = Q K^T, times scale, mask, softmax with expf and a reciprocal, motion from the normalised
    weights, O = P V.  Returns (out [rows, C], motion [rows, heads, 2]) in fp32."""
    bw, n, q, k, v, mask, scale, kxy, qxy = _emulation_setup(qkv, labels, bw, nw, ws, heads, hd, kv_shift, mutant, windows, MUTANTS32)
    s = _masked_logits((q @ k.transpose(-2, -1)) * torch.tensor(scale), mask, -100.0, n, ws, mutant)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    inv = 1.0 / p.sum(-1, keepdim=True)
    p = p[..., :n] * inv
    rel = kxy[None, :, :] - qxy[:, None, :]                            # [q, key, 2]
    m = (p[..., None] * rel).sum(-2)
    return _rows(p @ v, m, bw, n, heads)


def _split32(x):
    h, l = M.split(x)
    return h.float(), l.float()


def emulate_x3(qkv, labels, bw, nw, ws, heads, hd, kv_shift, mutant: Optional[str] = None, windows=None):
    """window_attn_x3_kernel in fp32 torch: acc / cor in fp32 from f16x3_model.split operands, s = acc + cor / 1024; base-2 softmax
    numerators with sl2 = scale * log2(e) and the mask -100 log2(e); P split UNNORMALISED, P V with the key-position columns
    (kx, ky, 0, 0) appended to V, then times 1 / sum; motion = o[hd .. hd + 1] - q_xy."""
    bw, n, q, k, v, mask, scale, kxy, qxy = _emulation_setup(qkv, labels, bw, nw, ws, heads, hd, kv_shift, mutant, windows, MUTANTS_X3)
    (qh, ql), (kh, kl) = _split32(q), _split32(k)
    kht, klt = kh.transpose(-2, -1), kl.transpose(-2, -1)
    s = qh @ kht + (qh @ klt + ql @ kht) * torch.tensor(1.0 / 1024.0)
    sl2 = np.float32(scale * np.float32(LOG2E))
    x = _masked_logits(s * torch.tensor(sl2), mask, float(np.float32(-100.0) * np.float32(LOG2E)), n, ws, mutant)
    p = torch.exp2(x - x.max(-1, keepdim=True).values)
    inv = 1.0 / p.sum(-1, keepdim=True)
    ph, pl = _split32(p[..., :n].contiguous())
    if mutant == "p_hi_only":
        pl = torch.zeros_like(pl)
    vh, vl = _split32(v)
    if mutant == "v_lo_other_window":
        vl = vl.roll(1, 0)
    cols = torch.cat([kxy, torch.zeros(n, 2)], -1).expand(bw, heads, n, 4)
    vh, vl = torch.cat([vh, cols], -1), torch.cat([vl, torch.zeros_like(cols)], -1)
    o = (ph @ vh + (ph @ vl + pl @ vh) * torch.tensor(1.0 / 1024.0)) * inv
    return _rows(o[..., :hd], o[..., hd:hd + 2] - qxy, bw, n, heads)


# ------------------------------------------------------------------ input builders
@dataclass
class Case:
    name: str
    qkv: torch.Tensor                  # [Bw*N, 3C] fp32
    labels: Optional[torch.Tensor]     # int32 [nW, N]
    bw: int
    nw: int
    ws: int
    heads: int
    hd: int
    kv_shift: int
    expect_out: Optional[torch.Tensor] = None       # closed forms (one_hot): fp32 rows of V / integer motion
    expect_motion: Optional[torch.Tensor] = None

    @property
    def n(self):
        return self.ws * self.ws

    @property
    def c(self):
        return self.heads * self.hd

    @property
    def args(self):
        return (self.labels, self.bw, self.nw, self.ws, self.heads, self.hd, self.kv_shift)


# every reachable tile count NT (1 2 3 4 6 7 8 9 11 13 15 16), every DCH (DCH 3 persistent at 9/72 and 11/84, one item per
# workgroup at 13/68), hd mod 16 in {0, 4, 8, 12}; each admissible for BOTH engines with a motion output (test_attention_ref_cpu)
PAIRS = [(1, 32), (2, 4), (3, 8), (5, 12), (6, 20), (7, 36), (9, 72), (10, 100), (11, 84), (12, 100), (13, 68), (14, 64), (15, 40),
         (16, 52)]
WALK_PAIRS = [(4, 16), (8, 48), (8, 72), (11, 32)]
LOGIT_SCALE = 60.0


def geometry(ws: int):
    """Two frames of a map of about two windows per side whose size is no multiple of ws, shifted by ws // 2: padded and shifted
    windows carry labels.  (ws 1: every size is a multiple and there is nothing to shift -- no labels, one key.)"""
    if ws == 1:
        return windows.build_window_geometry(2, 2, 2, 1, 0)
    return windows.build_window_geometry(2, 2 * ws - 1, 2 * ws - max(1, ws // 3), ws, ws // 2)


def _hot_qk(g, rows, c, hd):
    """q, k of magnitude sqrt(60): q.k / sqrt(hd) has a standard deviation of 60 / sqrt(hd) and reaches about +-60 (beyond, at the
    small head dims), as tests/test_gpu_f16x3_contract.py's attention inputs."""
    return (torch.rand(rows, 2 * c, generator=g) * 2 - 1) * (LOGIT_SCALE * 3.0 / hd ** 0.5) ** 0.5


def _reach(qkv, bw, n, heads, hd, kv_shift):
    """Few keys and a large head dim leave the largest |logit| well below 60 (ws 1 / hd 32: 64 logits in all): scale q and k up so
    that it is 60.  Inputs that reach it on their own stay as they are."""
    q, k, _ = _heads_view(qkv, bw, n, heads, hd, kv_shift, torch.float64)
    top = float((q @ k.transpose(-2, -1)).abs().max()) / math.sqrt(hd)
    if top < LOGIT_SCALE:
        qkv[:, :2 * heads * hd] *= (LOGIT_SCALE / top) ** 0.5


def _plant_masked_winner(qkv, labels, bw, nw, n, heads, hd, kv_shift, g):
    """In head 0 of every window whose labels differ: the first query's row and the K rows it meets are set so that the first key of
    ANOTHER label sits at logit +60 (-100 by the mask) and every other key at about -58: the masked key wins the softmax."""
    c = heads * hd
    m = (LOGIT_SCALE / hd ** 0.5) ** 0.5
    for b in range(bw):
        lab = labels[b % nw]
        other = (lab != lab[0]).nonzero()
        if other.numel() == 0:
            continue
        k0, bk = int(other[0]), (b + kv_shift) % bw
        sig = (torch.randint(0, 2, (hd,), generator=g) * 2 - 1).float()
        qkv[b * n, 0:hd] = m * sig
        kr = -m * sig[None, :] * (0.95 + 0.05 * torch.rand(n, hd, generator=g))
        kr[k0] = m * sig
        qkv[bk * n:(bk + 1) * n, c:c + hd] = kr


_CASES: dict = {}
_REFS: dict = {}


def _cached(name, make):
    if name not in _CASES:
        _CASES[name] = make()
    return _CASES[name]


def reference(case: Case, windows_: Optional[Sequence[int]] = None) -> Ref64:
    """attention64 of a case, computed once per process and shared (callers leave it unchanged)."""
    key = (case.name, None if windows_ is None else tuple(windows_))
    if key not in _REFS:
        _REFS[key] = attention64(case.qkv, *case.args, windows=windows_)
    return _REFS[key]


def hot(ws: int, hd: int, vfam: str = "wide", heads: int = HEADS) -> Case:
    """Logits to about +-60, V log-uniform over 2^-20 .. 2^8 (``wide``) or at the fp16 boundaries of the split (``edge``: the f16x3
    engine only, it saturates by contract), two frames cross-attending, a planted masked winner (asserted)."""
    def make():
        g = torch.Generator().manual_seed(7000 + 131 * ws + hd + (vfam == "edge"))
        geo = geometry(ws)
        bw, n, c = 2 * geo.n_windows, ws * ws, heads * hd
        qkv = torch.empty(bw * n, 3 * c)
        qkv[:, :2 * c] = _hot_qk(g, bw * n, c, hd)
        qkv[:, 2 * c:] = M.wide(g, bw * n, c, lo=-20.0, hi=8.0) if vfam == "wide" else M.edge(g, bw * n, c, frac=0.1)
        _reach(qkv, bw, n, heads, hd, bw // 2)
        if geo.labels is not None:
            _plant_masked_winner(qkv, geo.labels, bw, geo.n_windows, n, heads, hd, bw // 2, g)
        case = Case(f"hot_{vfam}_ws{ws}_hd{hd}", qkv, geo.labels, bw, geo.n_windows, ws, heads, hd, bw // 2)
        ref = reference(case)
        assert ref.logit_absmax > 0.5 * LOGIT_SCALE, "the logits do not reach the intended range"
        assert geo.labels is None or ref.masked_wmax > 1e-3, "no masked key carries weight: -100 could not be told from -inf"
        return case
    return _cached(f"hot_{vfam}_ws{ws}_hd{hd}_{heads}", make)


def uniform(ws: int, hd: int, heads: int = HEADS) -> Case:
    """Q = 0: every same-label key weighs the same (a masked one e^-100 of that)."""
    def make():
        g = torch.Generator().manual_seed(8000 + 131 * ws + hd)
        geo = geometry(ws)
        bw, n, c = 2 * geo.n_windows, ws * ws, heads * hd
        qkv = torch.zeros(bw * n, 3 * c)
        qkv[:, c:2 * c] = _hot_qk(g, bw * n, c, hd)[:, :c]
        qkv[:, 2 * c:] = M.wide(g, bw * n, c, lo=-20.0, hi=8.0)
        return Case(f"uniform_ws{ws}_hd{hd}", qkv, geo.labels, bw, geo.n_windows, ws, heads, hd, bw // 2)
    return _cached(f"uniform_ws{ws}_hd{hd}_{heads}", make)


def uniform_closed_form(case: Case, dequant: bool = False):
    """(out, motion) fp64 of a ``uniform`` case from its definition: the mean of V / of the key positions over the keys weighted
    1 (same label) or e^-100 (masked).  ``dequant``: of the f16x3 value hi + lo'/1024 of V (what that engine contracts with)."""
    bw, n, heads, hd = case.bw, case.n, case.heads, case.hd
    _, _, v = _heads_view(M.dequant(case.qkv) if dequant else case.qkv, bw, n, heads, hd, case.kv_shift, torch.float64)
    mask = _mask(case.labels, bw, case.nw)
    wgt = torch.ones(bw, 1, n, n, dtype=torch.float64) if mask is None else torch.where(mask, math.exp(-100.0), 1.0).double()
    wgt = wgt / wgt.sum(-1, keepdim=True)
    kxy = key_xy(case.ws)
    o, m = _rows(wgt @ v, (wgt @ kxy - kxy).expand(bw, heads, n, 2), bw, n, heads)
    return o, m


ONE_HOT_LEAD = 110.0          # e^-104 is 0 in fp32; 110 leaves room for the roundings of the scaling


def one_hot_codes(n: int, hd: int, seed: int = 0) -> Optional[torch.Tensor]:
    """[N, hd] codes in {+-1}^hd whose pairwise scalar products u_a.u_b leave 64 (hd - u_a.u_b) / sqrt(hd) >= 110, by seeded greedy
    search; None when the search finds no such set."""
    need = math.ceil(ONE_HOT_LEAD * math.sqrt(hd) / 64.0)
    g = torch.Generator().manual_seed(9000 + 1009 * n + hd + seed)
    got = torch.empty(0, hd)
    for _ in range(64):
        cand = (torch.randint(0, 2, (4 * n + 64, hd), generator=g) * 2 - 1).float()
        for u in cand:
            if got.shape[0] == 0 or float((got @ u).max()) <= hd - need:
                got = torch.cat([got, u[None]])
                if got.shape[0] == n:
                    return got
    return None


def one_hot(ws: int, hd: int, labelled: bool, vfam: str = "wide", heads: int = HEADS) -> Optional[Case]:
    """Q row q = 8 u_pi(q), K row k = 8 u_k (times a sign pattern per head): every product is exact in either engine, key pi(q) leads
    every other logit by >= 110 (asserted from the float64 logits, mask included), so the softmax is exactly one-hot in fp32:
    out = V[pi(q)] (its f16x3 value for that engine), motion = pi(q)_xy - q_xy.  ``labelled``: with the geometry's labels, pi a
    permutation inside each label class of the query's window; otherwise no labels.  None when no code set exists (named in
    ONE_HOT_WITHOUT_CODES)."""
    def make():
        n = ws * ws
        codes = one_hot_codes(n, hd)
        if codes is None:
            return None
        g = torch.Generator().manual_seed(9500 + 131 * ws + hd + labelled + 2 * (vfam == "edge"))
        geo = geometry(ws)
        labels = geo.labels if labelled else None
        bw, nw, c, kv_shift = 2 * geo.n_windows, geo.n_windows, heads * hd, geo.n_windows
        sig = (torch.randint(0, 2, (heads, hd), generator=g) * 2 - 1).float()
        pi = torch.empty(bw, n, dtype=torch.long)
        for b in range(bw):
            if labels is None:
                pi[b] = torch.randperm(n, generator=g)
            else:
                lab = labels[b % nw]
                for cls in lab.unique():
                    idx = (lab == cls).nonzero()[:, 0]
                    pi[b, idx] = idx[torch.randperm(idx.numel(), generator=g)]
        qkv = torch.empty(bw, n, 3, heads, hd)
        qkv[:, :, 1] = 8.0 * codes[None, :, None, :] * sig[None, None]
        qkv[:, :, 0] = 8.0 * codes[pi][:, :, None, :] * sig[None, None]
        qkv[:, :, 2] = (M.wide(g, bw, n, heads, hd, lo=-20.0, hi=8.0) if vfam == "wide" else M.edge(g, bw, n, heads, hd, frac=0.1))
        v = qkv[:, :, 2]
        src = (torch.arange(bw) + kv_shift) % bw
        kxy = key_xy(ws)
        case = Case(f"one_hot_{'lab' if labelled else 'nolab'}_{vfam}_ws{ws}_hd{hd}", qkv.reshape(bw * n, 3 * c).contiguous(), labels,
                    bw, nw, ws, heads, hd, kv_shift,
                    expect_out=v[src[:, None], pi].reshape(bw * n, c).contiguous(),
                    expect_motion=(kxy[pi] - kxy[None])[:, :, None, :].expand(bw, n, heads, 2).reshape(bw * n, heads, 2).float().contiguous())
        # the precondition, from the float64 logits with the mask
        q, k, _ = _heads_view(case.qkv, bw, n, heads, hd, kv_shift, torch.float64)
        l = (q @ k.transpose(-2, -1)) / math.sqrt(hd)
        mask = _mask(labels, bw, nw)
        if mask is not None:
            l = l - 100.0 * mask.double()
        chosen = torch.gather(l, -1, pi[:, None, :, None].expand(bw, heads, n, 1))
        others = l.scatter(-1, pi[:, None, :, None].expand(bw, heads, n, 1), -math.inf)
        assert n == 1 or float((chosen - others.max(-1, keepdim=True).values).min()) >= ONE_HOT_LEAD, "one_hot: a key leads by less than 110"
        return case
    return _cached(f"one_hot_{labelled}_{vfam}_ws{ws}_hd{hd}_{heads}", make)


# pairs of PAIRS for which the seeded search finds no code set (left out of the one_hot tests BY NAME; test_attention_ref_cpu holds
# this list to what the search actually finds)
ONE_HOT_WITHOUT_CODES: list = []
ONE_HOT_PAIRS = [p for p in PAIRS if p not in ONE_HOT_WITHOUT_CODES]


def walk_grid_ceiling(ws: int, cus: int) -> int:
    """No persistent grid can exceed this: a CU holds 32 waves, a workgroup has NT of them."""
    return cus * (32 // tiles(ws))


def walk_bw(ws: int, cus: int, heads: int = HEADS, nw: int = 3) -> int:
    """Smallest Bw, a multiple of nW and none of 8, with vitems = ceil(Bw / 8) * 8 * heads >= 2 * ceiling + 8 * heads: every
    workgroup walks at least two items and the last round is ragged."""
    need = 2 * walk_grid_ceiling(ws, cus) + 8 * heads
    bw = (need + heads - 1) // heads
    while bw % nw or bw % 8 == 0 or (bw + 7) // 8 * 8 * heads < need:
        bw += 1
    return bw


def walk(ws: int, hd: int, cus: int, heads: int = HEADS) -> Case:
    """The persistent walk's input, sized from the device's CU count: hot logits, V uniform in +-1 (a cheap float64 reference and a
    negligible 2^-34 term), synthetic labels [3, N] with values 0..2 (every window position its own row), an odd kv_shift that is
    not Bw / 2."""
    def make():
        nw, n, c = 3, ws * ws, heads * hd
        bw = walk_bw(ws, cus, heads, nw)
        g = torch.Generator().manual_seed(9900 + 131 * ws + hd)
        qkv = torch.empty(bw * n, 3 * c)
        qkv[:, :2 * c] = _hot_qk(g, bw * n, c, hd)
        qkv[:, 2 * c:] = torch.rand(bw * n, c, generator=g) * 2 - 1
        labels = torch.randint(0, 3, (nw, n), generator=g).to(torch.int32)
        assert n == 1 or not (torch.equal(labels[0], labels[1]) or torch.equal(labels[1], labels[2]) or torch.equal(labels[0], labels[2]))
        kv_shift = 2 * (bw // 5) + 1
        _reach(qkv, bw, n, heads, hd, kv_shift)
        assert kv_shift % 2 == 1 and 2 * kv_shift != bw and 0 < kv_shift < bw and bw % 8 and bw % nw == 0
        return Case(f"walk_ws{ws}_hd{hd}_cu{cus}", qkv, labels, bw, nw, ws, heads, hd, kv_shift)
    return _cached(f"walk_ws{ws}_hd{hd}_cu{cus}_{heads}", make)


def walk_windows(bw: int, per_residue: int = 8) -> list:
    """>= 64 windows of a walk: for every residue b mod 8, ``per_residue`` windows spread evenly from the first to the last of that
    residue (first, middle and last rounds of the item walk whatever the grid), windows 0 and Bw - 1 among them."""
    wins = []
    for r in range(8):
        last = (bw - 1 - r) // 8
        wins += sorted({r + 8 * round(j * last / (per_residue - 1)) for j in range(per_residue)})
    assert 0 in wins and bw - 1 in wins
    return wins


def model_subset(case: Case, wins: Sequence[int]):
    """f16x3_model.attention on the windows ``wins`` only: (out, motion, absr) with rows in that order."""
    sub, lab, bw, nw, kv = gather_windows(case.qkv, case.labels, case.bw, case.nw, case.n, case.kv_shift, wins)
    return M.attention(sub, lab, bw, nw, case.ws, case.heads, case.hd, kv)
