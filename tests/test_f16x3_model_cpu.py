"""CPU: the fp64 f16x3 model (tests/f16x3_model.py) itself -- its split against the library's documented semantics, its contractions
against a naive loop, the exactness certificate of every exact-family configuration the GPU contract tests use, and the teeth of those
tests: every mutant engine misses their tolerance by more than 10x on every configuration.  The same for the exact CHAINS of the
fused stem and the fused refiner tail (tests/test_gpu_f16x3_chains.py): every layer that test treats as exact is proven exact, and
every mutant of one layer, a hidden layer with a wrong padding and a layer 3 at the wrong parity fail its comparisons."""
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


# ------------------------------------------------------------------ the exact chains of the fused stem and the fused refiner tail
STEM_IDS = [c["id"] for c in M.CASES_STEM]
TAIL_CASES = M.CASES_TAIL + [M.CASE_TAIL_F16]
# Measured over all committed cases (both families share the hidden layers): share of activation-side lo' != 0 entering stem layers
# 1 / 2 / 3: 0.38-0.58 / 0.57-0.86 / 0.95-1.00; negative pre-activations per stem layer 0.30-0.71 (the 2 x 2 map, 4 to 48 values per
# layer, is left out of these floors); tail: lo' != 0 0.55 into refine_head.0 and 0.89-0.93 into W2, negative pre-activations
# 0.46-0.55, negative sums 0.23-0.70.  The floors sit clearly below.
STEM_LO_FLOOR, STEM_NEG_RANGE = (0.3, 0.5, 0.8), (0.2, 0.8)
TAIL_LO_FLOOR, TAIL_NEG_RANGE, TAIL_SUM_NEG_RANGE = (0.4, 0.7), (0.3, 0.7), (0.1, 0.9)


def tail_exactness(cfg, o):
    n, h, w = cfg["NHW"]
    x, wa = o["x"], o["wa"]
    if cfg.get("terms") == 1:
        x, wa = M.split(x)[0].float(), M.split(wa)[0].float()
    da = M.layer_exactness(x, wa, o["ra"], M.conv_contract(1, 1, 1))
    dc = M.layer_exactness(o["ra"].y.float().reshape(n * h * w, -1), M.readout_matrix(o["wb"]), o["rc"], M.linear_contract, resplit=False)
    return da, dc


@pytest.mark.parametrize("family", M.CHAIN_FAMILIES)
@pytest.mark.parametrize("cfg", M.CASES_STEM, ids=STEM_IDS)
def test_stem_chain_is_exact(cfg, family):
    """Every layer the GPU test treats as exact -- all three in chain_exact, the two hidden ones in chain_rich_last -- rounds nowhere:
    certificate, fold, bias, PReLU product, re-split; and the inputs are worth testing with (lo' and both PReLU branches)."""
    o = M.build_chain(cfg, family)
    layers = (0, 1, 2) if family == "chain_exact" else (0, 1)
    for i, d in zip(layers, M.stem_exactness(o, layers)):
        assert d["ok"], (cfg["id"], family, i, {k: v for k, v in d.items() if k != "certificate"}, d["certificate"])
        if cfg["FHW"][1] > 2:
            assert d["lo_share"] >= STEM_LO_FLOOR[i], (cfg["id"], i, d["lo_share"])
            assert STEM_NEG_RANGE[0] <= d["neg_share"] <= STEM_NEG_RANGE[1], (cfg["id"], i, d["neg_share"])
    if family == "chain_rich_last":
        hi, lo = M.split(o["params"][2][0])
        assert float((lo != 0).double().mean()) > 0.9, "the last layer's weights carry no lo'"
        assert not M.certificate(o["res"][1].y.float(), o["params"][2][0], M.conv_contract(2, 1, 1))["ok"]


@pytest.mark.parametrize("family", M.CHAIN_FAMILIES)
@pytest.mark.parametrize("cfg", TAIL_CASES, ids=lambda c: c["id"])
def test_tail_chain_is_exact(cfg, family):
    o = M.build_chain(cfg, family)
    n, h, w = cfg["NHW"]
    da, dc = tail_exactness(cfg, o)
    assert da["ok"], (cfg["id"], family, {k: v for k, v in da.items() if k != "certificate"}, da["certificate"])
    if cfg.get("terms") != 1:
        assert da["lo_share"] >= TAIL_LO_FLOOR[0]
    else:
        assert float(o["ra"].cor.abs().max()) == 0.0 and float((M.split(o["x"])[1] != 0).double().mean()) >= TAIL_LO_FLOOR[0]
    assert dc["lo_share"] >= TAIL_LO_FLOOR[1] and TAIL_NEG_RANGE[0] <= da["neg_share"] <= TAIL_NEG_RANGE[1], (da["neg_share"], dc["lo_share"])
    if family == "chain_exact":
        assert dc["cert"] and dc["fold"], (cfg["id"], dc["certificate"])
        s = M.sum_exactness(o["rc"].y, n, h, w, o["bb"], o["pb"])
        assert s["ok"], (cfg["id"], s)
        assert TAIL_SUM_NEG_RANGE[0] <= s["neg_share"] <= TAIL_SUM_NEG_RANGE[1], s["neg_share"]
        assert float(M.tail_contrib_bound(o, dc["fold"]).max()) == 0.0
        r, rb = M.tail_preact(o, n, h, w, torch.zeros_like(o["rc"].y))
        assert float(rb.max()) == 0.0
        assert float((r.abs() < 4).double().mean()) > 0.5, "most arguments of the sigmoid should lie where it does not saturate"
    else:
        assert not dc["cert"] and float((M.split(o["wb"])[1] != 0).double().mean()) > 0.9


def test_chain_weights_reach_every_position():
    """Over the committed cases of each variant / width, every (cout, cin, tap) of every ternary layer is nonzero at least once."""
    for c0 in (24, 16):
        ws = [M.stem_operands(c, "chain_exact")["params"] for c in M.CASES_STEM if c["c0"] == c0]
        for layer in range(3):
            assert bool((sum(p[layer][0].abs() for p in ws) > 0).all()), (c0, layer)
    for c in (64, 32):
        os_ = [M.tail_operands(cfg, "chain_exact") for cfg in M.CASES_TAIL if cfg["c"] == c]
        assert bool((sum(o["wa"].abs() for o in os_) > 0).all()) and bool((sum(o["wb"].abs() for o in os_) > 0).all()), c


def test_chains_equal_naive_loops():
    g = torch.Generator().manual_seed(8)
    x = M.wide(g, 2, 6, 4, 3, lo=-8.0, hi=1.0)
    params = [(M.wide(g, co, ci, 3, 3, lo=-8.0, hi=1.0), torch.randn(co, generator=g), torch.rand(co, generator=g)) for ci, co in ((3, 4), (4, 4), (4, 5))]
    res = M.stem_chain(x, params)
    a = x
    for (w, b, p), st, r in zip(params, M.STEM_STRIDES, res):
        ref = M.naive_conv(a, w, b, p, st, 1, 1)
        assert torch.allclose(r.y, ref, rtol=1e-13, atol=1e-13)
        a = r.y.float()
    assert tuple(res[2].y.shape) == (2, 3, 2, 5)
    n, h, w, cin, c = 2, 4, 5, 6, 32
    xt = M.wide(g, n, h, w, cin, lo=-6.0, hi=1.0)
    wa, ba, pa = M.wide(g, c, cin, 3, 3, lo=-6.0, hi=0.0), torch.randn(c, generator=g), torch.rand(c, generator=g)
    wb = M.wide(g, 3, c, 3, 3, lo=-6.0, hi=0.0)
    ra, rc, pre = M.tail_chain(xt, wa, ba, pa, wb)
    assert torch.allclose(ra.y, M.naive_conv(xt, wa, ba, pa, 1, 1, 1), rtol=1e-13, atol=1e-13)
    # refine_head.1 as a convolution of the activated map, zero padded: the nine-term sum of the contributions is that convolution
    want = M.naive_conv(ra.y.float(), wb, None, None, 1, 1, 1).permute(0, 3, 1, 2)
    assert torch.allclose(pre, want, rtol=1e-12, atol=1e-12)
    ah, al = (t.double() for t in M.split(ra.y.float().reshape(-1, c)))
    wh, wl = (t.double() for t in M.split(wb))
    p, tap, o_ = 7, 5, 2
    one = sum(float(ah[p, k] * wh[o_, k, tap // 3, tap % 3]) + float(ah[p, k] * wl[o_, k, tap // 3, tap % 3] + al[p, k] * wh[o_, k, tap // 3, tap % 3]) / 1024
              for k in range(c))
    assert abs(float(rc.y[p, tap * 3 + o_]) - one) <= 1e-12


TEETH_STEM = [c for c in M.CASES_STEM if 18 <= c["FHW"][1] <= 70]
STEM_MUTATIONS = [(m, layer) for layer in range(3) for m in M.MUTANTS] + [("pad_bias", 0), ("pad_bias", 1), ("parity", 2)]
# lo4 in layer 1 is the identity: frames that certify through three layers have 13 bits, so their lo' has at most 3 significant bits
# and a 4-bit lo' operand loses nothing (the same holds for the 13-bit plane values of the tail's main product).  Those lo' paths are
# held by one_cross and last_chunk (the stem's K = 27 is one chunk: all of lo').
STEM_UNREACHABLE = {("lo4", 0)}
TAIL_UNREACHABLE = {("lo4", 0)}
# chain_rich_last cannot reach 10x with lo4 in the LAST product (measured: 2.2x-4.6x the bound in the stem's layer 3, 4.0x-6.8x in W2):
# the statistical rule allows 8 x 2^-24 sum |x||w| and a 4-bit lo' loses ~2^-15 |x||w| per term with random signs, a ratio of about
# 64 / sqrt(K).  It still fails the GPU test (> 1x, asserted) and is proven on chain_exact, where any deviation fails.  lo4 in the
# stem's layer 2 touches only the few layer-1 values near +-9 whose lo' has five bits: 0.9x-2.4x behind the dense layer 3, reported and
# not asserted; chain_exact proves it (a third to nine tenths of the outputs move).
RICH_BELOW_10X = {("lo4", 2): 1.0, ("lo4", 1): 0.0}
TAIL_RICH_BELOW_10X = {("lo4", 1)}


@pytest.mark.parametrize("cfg", TEETH_STEM, ids=lambda c: c["id"])
def test_stem_chain_mutants_are_caught(cfg, record_property):
    """Teeth of the GPU stem tests.  chain_exact demands equality, so any deviation fails it: each mutant must move more than 16
    output values (how many is reported).  chain_rich_last: each must miss ``stem_last_bound`` by more than 10x."""
    table = {}
    for family in M.CHAIN_FAMILIES:
        o = M.build_chain(cfg, family)
        y = o["res"][2].y
        bound = M.stem_last_bound(o) if family == "chain_rich_last" else None
        for mutant, layer in STEM_MUTATIONS:
            dev = (M.build_chain(cfg, family, mutant, layer)["res"][2].y - y).abs()
            if (mutant, layer) in STEM_UNREACHABLE:
                assert float(dev.max()) == 0.0, "lo4 in layer 1 became reachable: take it off STEM_UNREACHABLE"
                continue
            if family == "chain_exact":
                table[f"{family}/{mutant}@{layer + 1}"] = f"{int((dev != 0).sum())} of {dev.numel()} differ"
                assert int((dev != 0).sum()) > 16, (cfg["id"], mutant, layer, int((dev != 0).sum()))
            else:
                worst = (dev / bound).max().item()
                table[f"{family}/{mutant}@{layer + 1}"] = f"{worst:.1f}x"
                assert worst > RICH_BELOW_10X.get((mutant, layer), 10), f"{cfg['id']}: {mutant} in layer {layer + 1} only {worst:.1f}x the bound"
    record_property("mutants", str(table))
    print(cfg["id"], table)


@pytest.mark.parametrize("cfg", [c for c in TAIL_CASES if c["NHW"][1] <= 72], ids=lambda c: c["id"])
def test_tail_chain_mutants_are_caught(cfg, record_property):
    """Teeth of the GPU tail tests on ``contrib``: chain_exact demands equality (more than 16 contributions must move);
    chain_rich_last applies ``tail_contrib_bound`` (more than 10x)."""
    table = {}
    for family in M.CHAIN_FAMILIES:
        o = M.build_chain(cfg, family)
        bound = M.tail_contrib_bound(o, True)
        assert (float(bound.max()) == 0.0) == (family == "chain_exact")
        for which in (0, 1):
            for mutant in M.MUTANTS:
                if which == 0 and cfg.get("terms") == 1:
                    continue            # the main product has no lo' in the f16 mode: nothing to mutate
                dev = (M.build_chain(cfg, family, mutant, which)["rc"].y - o["rc"].y).abs()
                if (mutant, which) in TAIL_UNREACHABLE:
                    assert float(dev.max()) == 0.0, "lo4 in the main product became reachable: take it off TAIL_UNREACHABLE"
                    continue
                if family == "chain_exact":
                    table[f"{family}/{mutant}@{'AW'[which]}"] = f"{int((dev != 0).sum())} of {dev.numel()} differ"
                    assert int((dev != 0).sum()) > 16, (cfg["id"], mutant, which)
                else:
                    worst = (dev / bound).max().item()
                    table[f"{family}/{mutant}@{'AW'[which]}"] = f"{worst:.1f}x"
                    assert worst > (1 if (mutant, which) in TAIL_RICH_BELOW_10X else 10), f"{cfg['id']}: {mutant} in product {which} only {worst:.1f}x the bound"
    record_property("mutants", str(table))
    print(cfg["id"], table)
