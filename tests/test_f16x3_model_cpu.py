"""CPU: the fp64 f16x3 model (tests/f16x3_model.py) itself -- its split against the library's documented semantics, its contractions
against a naive loop, the exactness certificate of every exact-family configuration the GPU contract tests use, and the teeth of those
tests: every mutant engine misses their tolerance by more than 10x on every configuration."""
import numpy as np
import pytest
import torch

import f16x3_model as M


def test_split_edge_table():
    cases = [  # x, hi, lo'
        (1.0, 1.0, 0.0), (65504.0, 65504.0, 0.0), (65472.0, 65472.0, 0.0),
        (65488.0, 65472.0, 16384.0),               # exact tie: rounds to even (65472), so the limit is |x| > 65488
        (65488.0078125, 65504.0, -16376.0),        # the next fp32 value goes up
        (65519.9921875, 65504.0, 16376.0), (65520.0, 65504.0, 16384.0),
        (7e4, 65504.0, 65504.0),                   # both halves saturate
        (-7e4, -65504.0, -65504.0),
        (2.0 ** -14, 2.0 ** -14, 0.0), (2.0 ** -24, 2.0 ** -24, 0.0),
        (2.0 ** -25, 0.0, 2.0 ** -15),             # tie at half the smallest subnormal: to even (0)
        (3 * 2.0 ** -26, 2.0 ** -24, -2.0 ** -16),
        (2.0 ** -14 - 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 0.0),
        (1.0 + 2.0 ** -11, 1.0, 0.5),              # tie: to even
        (1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -9, -0.5),
    ]
    x = torch.tensor([c[0] for c in cases], dtype=torch.float32)
    hi, lo = M.split(x)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    for i, (v, h, l) in enumerate(cases):
        assert float(hi[i]) == h and float(lo[i]) == l, (v, float(hi[i]), float(lo[i]))
    hi, lo = M.split(torch.tensor([-0.0, float("inf"), float("-inf"), float("nan")]))
    assert float(hi[0]) == 0.0 and np.signbit(hi[0].numpy()) and float(lo[0]) == 0.0
    assert float(hi[1]) == float("inf") and float(hi[2]) == float("-inf") and torch.isnan(lo[1:]).all()
    assert torch.isnan(hi[3])


def test_split_matches_torch_half_after_clamp():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([M.wide(g, 20000, lo=-30.0, hi=20.0), M.edge(g, 5000, frac=1.0), (torch.rand(5000, generator=g) * 2 - 1)])
    hi, lo = M.split(x)
    h_ref = x.clamp(-65504, 65504).half()
    lo_ref = ((x - h_ref.float()) * 1024).clamp(-65504, 65504).half()      # x - hi and the product are exact in fp32
    assert torch.equal(hi, h_ref) and torch.equal(lo, lo_ref)
    ok = (x.abs() <= 65504) & (x.abs() >= 2.0 ** -14)
    err = (M.dequant(x) - x.double()).abs()
    assert (err[ok] <= 2.0 ** -21 * x.double().abs()[ok]).all()           # ~22 significant bits in fp16's normal range


def test_exact_family_splits_as_built():
    g = torch.Generator().manual_seed(4)
    a = torch.randint(2, 8, (4000,), generator=g).double() * (torch.randint(0, 2, (4000,), generator=g) * 2 - 1)
    b = torch.randint(-127, 128, (4000,), generator=g).double()
    x = (a * 2.0 ** -3 + b * 2.0 ** -21).float()
    hi, lo = M.split(x)
    assert torch.equal(hi.double(), a * 2.0 ** -3) and torch.equal(lo.double(), b * 2.0 ** -11)


@pytest.mark.parametrize("stride,pad,dil,k", [(1, 1, 1, 3), (2, 1, 1, 3), (4, 2, 2, 3), (1, 0, 1, 1)])
def test_conv_model_equals_naive_loop(stride, pad, dil, k):
    g = torch.Generator().manual_seed(stride * 10 + dil)
    x = M.wide(g, 2, 7, 6, 5, lo=-12.0, hi=4.0)
    w = M.wide(g, 3, 5, k, k, lo=-12.0, hi=2.0)
    b = torch.randn(3, generator=g)
    s = torch.rand(3, generator=g)
    res = M.conv(x, w, b, s, stride, pad, dil)
    ref = M.naive_conv(x, w, b, s, stride, pad, dil)
    assert torch.allclose(res.y, ref, rtol=1e-13, atol=1e-13)


def test_linear_and_deconv_models_equal_naive_sums():
    g = torch.Generator().manual_seed(5)
    x, w = M.wide(g, 6, 40, lo=-10.0, hi=5.0), M.wide(g, 7, 40, lo=-10.0, hi=2.0)
    xh, xl = (t.double() for t in M.split(x))
    wh, wl = (t.double() for t in M.split(w))
    ref = torch.tensor([[sum(float(xh[i, k] * wh[j, k]) for k in range(40)) + sum(float(xh[i, k] * wl[j, k] + xl[i, k] * wh[j, k])
                                                                                    for k in range(40)) / 1024 for j in range(7)] for i in range(6)],
                       dtype=torch.float64)
    assert torch.allclose(M.linear(x, w).y, ref, rtol=1e-13, atol=1e-13)
    xd, wd = M.wide(g, 1, 3, 2, 6, lo=-8.0, hi=3.0), M.wide(g, 6, 4, 2, 2, lo=-8.0, hi=1.0)
    y = M.deconv2x2(xd, wd).y
    assert tuple(y.shape) == (1, 6, 4, 4)
    ref = torch.nn.functional.conv_transpose2d(M.dequant(xd).permute(0, 3, 1, 2), M.dequant(wd), stride=2).permute(0, 2, 3, 1)
    absxw = torch.nn.functional.conv_transpose2d(M.dequant(xd).abs().permute(0, 3, 1, 2), M.dequant(wd).abs(), stride=2).permute(0, 2, 3, 1)
    assert ((y - ref).abs() <= 2.0 ** -20 * absxw).all()                      # differs by the omitted lo'*lo' term only


def test_attention_model_without_split_error_is_softmax_attention():
    """On operands that split exactly and a P that does too (hd = 1 row sums), the model is plain fp64 attention."""
    g = torch.Generator().manual_seed(6)
    ws, heads, hd, bw = 4, 2, 8, 2
    n, c = ws * ws, heads * hd
    qkv = torch.cat([M.exact(g, bw * n, 2 * c), M.exact(g, bw * n, c)], 1)
    y, mo, _ = M.attention(qkv, None, bw, 1, ws, heads, hd, 0)
    t = M.dequant(qkv).reshape(bw, n, 3, heads, hd)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    a = ((q @ k.transpose(-2, -1)) / hd ** 0.5).softmax(-1)
    ref = (a @ v).transpose(1, 2).reshape(bw * n, c)
    assert (y - ref).abs().max().item() <= 2.0 ** -20 * v.abs().max().item()     # P's own split: ~22 bits


@pytest.mark.parametrize("cfg", M.ALL_EXACT_CASES, ids=lambda c: c["id"] + f"_{c['seed']}")
def test_certificate_holds(cfg):
    o = M.case_operands(cfg)
    cert = M.certificate(M.case_split_operand(cfg, o), o["w"], M.case_contract(cfg))
    assert cert["ok"], cert


def test_certificate_rejects_inexact_operands():
    g = torch.Generator().manual_seed(7)
    x, w = M.wide(g, 50, 300), M.wide(g, 20, 300)
    assert not M.certificate(x, w, M.linear_contract)["ok"]
    x, w = M.exact(g, 4, 40000), M.exact(g, 3, 40000)           # bmax 127 is certified to K ~ 9 000 in the worst case
    assert not M.certificate(x, w, M.linear_contract)["ok"]
    x, w = M.exact(g, 4, 18000, bmax=63), M.exact(g, 3, 18000, bmax=63)
    assert M.certificate(x, w, M.linear_contract)["ok"]


@pytest.mark.parametrize("mutant", M.MUTANTS)
@pytest.mark.parametrize("cfg", M.ALL_EXACT_CASES, ids=lambda c: c["id"] + f"_{c['seed']}")
def test_mutants_miss_the_gpu_tolerance(cfg, mutant):
    """Teeth: on every exact-family configuration each mutant deviates from the model by > 10x the bound the GPU test applies to every
    engine's unsplit launch.  (The split-K launches of the same configurations are held to the wider summation-order bound
    ``Result.splitk_tol``; a mutant of the shared arithmetic is caught by the unsplit launches of the same engines.)"""
    o = M.case_operands(cfg)
    res = M.case_model(cfg, o)
    mut = M.case_model(cfg, o, mutant=mutant)
    dev = (mut.y - res.y).abs()
    worst = (dev / res.exact_tol()).max().item()
    assert worst > 10, f"{cfg['id']}: mutant {mutant} only {worst:.1f}x the tolerance"
