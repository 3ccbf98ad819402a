"""GPU: the two kernels that chain layers on chip -- atmvfi_stem_fused and atmvfi_conv3p's read-out + atmvfi_refine_tail -- held
to the exact chained f16x3 model of tests/f16x3_model.py (``stem_chain`` / ``tail_chain``).

``chain_exact``: operands for which no fp32 operation of ANY layer rounds (tests/test_f16x3_model_cpu.py proves it for every case
below: certificate, fold, bias, PReLU product, re-split), so the model predicts the hidden maps bit for bit and the kernel's output
must EQUAL the model's: the stem's planes are split(y3) in both halves, the tail's 27 tap contributions are the model's.
``chain_rich_last``: the hidden layers as above, the last contraction (layer 3 / W2) on full-precision weights with lo': its input
is known exactly, so the project's statistical rule applies to that one product alone.  The CPU file also shows the teeth: a 4-bit
lo', a dropped cross term, lo' dropped on the last k-chunk in any one layer, a hidden layer that is conv(0) + bias outside the image
and layer 3 at the wrong column parity all fail these comparisons.

CPU model time per case (fp64 torch on a multi-core x86 host): at most 0.2 s up to 70 x 34 / 40 x 72; stem F=3 176x256 0.6 s (24>48) /
0.4 s (16>32); stem F=4 176x384 1.4-1.6 s / 1.1 s; tail 64>32 at 272x272 0.6 s.  Worst kernel error / bound observed on an MI355X: 0.051
(stem, chain_rich_last), 0.071 (tail contributions, chain_rich_last), 0.54 (it_sum, chain_exact); each test records its own as the
``worst_ratio`` property."""
import importlib

import pytest
import torch

import f16x3_model as M
import pointwise_ref as R

pytestmark = pytest.mark.gpu

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
GEMM_CONV = 0
GUARD = 256            # fp16 elements on either side of the planes
SENTINEL = 1234.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def guarded_planes(rows, c, dev):
    """Zeroed ``Planes`` (one spare row) in the middle of a buffer whose ends hold a sentinel."""
    chunks = (c + 31) // 32
    n = 2 * chunks * (rows + 1) * 32
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float16, device=dev)
    buf[GUARD:GUARD + n] = 0
    return hip_ops.Planes(buf[GUARD:GUARD + n].view(2, chunks, rows + 1, 32), c, rows), buf


def check_planes_frame(out, buf, what):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f"{what}: the guard around the planes was written"
    assert out.t[:, :, out.rows:].abs().max().item() == 0, f"{what}: the spare row is not zero"
    if out.c % 32:
        assert out.t[:, -1, :, out.c % 32:].abs().max().item() == 0, f"{what}: the pad channels are not zero"


def where_differs(got, want, ho, wo):
    """The first places (frame, y, x, channel) at which two [rows, C] tensors differ: names the tile and the phase."""
    idx = (got.float() != want.float()).nonzero()[:6].tolist()
    return [(r // (ho * wo), r // wo % ho, r % wo, ch) for r, ch in idx]


def stem_frames(cfg, o, dev):
    """NHWC4 frames: the fourth lane, which stem.hip calls unused, carries finite junk (NaN in one case)."""
    f, h, w = cfg["FHW"]
    g = torch.Generator().manual_seed(cfg["seed"])
    x4 = torch.empty(f, h, w, 4)
    x4[..., :3] = o["x"]
    x4[..., 3] = float("nan") if cfg["nan_lane"] else (torch.rand(f, h, w, generator=g) * 2 - 1) * 1e3
    return x4.to(dev)


@pytest.mark.parametrize("family", M.CHAIN_FAMILIES)
@pytest.mark.parametrize("cfg", M.CASES_STEM, ids=lambda c: c["id"])
def test_stem_chain(cfg, family, dev, record_property):
    """atmvfi_stem_fused, both variants: a map smaller than a tile (2 x 2), exactly one 16 x 32 tile, 18 x 34 (four tiles, three of them
    ragged), several ragged tiles, several frames, and the two smallest shapes that reach the cross-tile hazards (frame patch over
    the layer-3 weight region, per-tile re-staging of those weights, the next patch requested under phase E): F=3 176x256 = 264
    tiles, so 8 of the 256 persistent workgroups walk two, and F=4 176x384 = 528 tiles, so every workgroup walks two or three."""
    f, h, w = cfg["FHW"]
    c1, ho, wo = cfg["c1"], h // 2, w // 2
    o = M.build_chain(cfg, family)
    y3 = o["res"][2].y.reshape(-1, c1)
    hip = hip_ops.HipOps(dev)
    pk = hip.pack_stem(*[t.to(dev) for layer in o["params"] for t in layer])
    x4 = stem_frames(cfg, o, dev)
    out, buf = guarded_planes(f * ho * wo, c1, dev)
    hip.stem_fused(x4, pk, out)
    torch.cuda.synchronize()
    what = f"{cfg['id']} {family}"
    check_planes_frame(out, buf, what)
    got = out.to_rows().cpu()[:, :, :c1]
    assert bool(torch.isfinite(got.float()).all()), f"{what}: the junk lane of the frames reached the output"
    if family == "chain_exact":
        hi, lo = M.split(y3.float())
        assert torch.equal(got[0].float(), hi.float()), f"{what}: hi differs from split(y3) at {int((got[0].float() != hi.float()).sum())} places, first (frame, y, x, c) {where_differs(got[0], hi, ho, wo)}"
        assert torch.equal(got[1].float(), lo.float()), f"{what}: lo' differs from split(y3) at {int((got[1].float() != lo.float()).sum())} places, first (frame, y, x, c) {where_differs(got[1], lo, ho, wo)}"
    else:
        val = out.to_float().cpu().double()
        ratio = R.worst_ratio(val, y3, M.stem_last_bound(o).reshape(-1, c1))
        record_property("worst_ratio", ratio)
        print(f"{what}: worst err/bound {ratio:.3f}")
        assert ratio <= 1.0, f"{what}: worst {ratio:.2f}x the statistical bound of layer 3"
    out2, buf2 = guarded_planes(f * ho * wo, c1, dev)
    hip.stem_fused(x4, pk, out2)
    torch.cuda.synchronize()
    assert torch.equal(buf, buf2), f"{what}: two launches of the fused stem differ"


def run_tail(cfg, family, dev, record_property):
    cin, c, (n, h, w) = cfg["cin"], cfg["c"], cfg["NHW"]
    px = n * h * w
    o = M.build_chain(cfg, family)
    hip = hip_ops.HipOps(dev)
    hip.plane_terms = cfg.get("terms", 3)
    xp = hip_ops.Planes.alloc(px, cin, dev)
    hip.split_planes(o["x"].reshape(px, cin).to(dev), xp)
    assert torch.equal(xp.to_float().cpu(), o["x"].reshape(px, cin)), "the plane values are not the case's operands"
    pw = hip.pack_weight(GEMM_CONV, o["wa"].to(dev))
    w2 = hip.pack_readout(o["wb"].to(dev))
    contrib = torch.full((27, px), float("nan"), device=dev)
    hip.conv3x3_planes_readout(xp, n, h, w, pw, o["ba"].to(dev), o["pa"].to(dev), w2, contrib)
    s, cl = torch.full((n, 3, h, w), 7.0, device=dev), torch.full((n, 3, h, w), 7.0, device=dev)
    hip.refine_tail(contrib, o["bb"].to(dev), o["pb"].to(dev), o["it"].to(dev), s, cl)
    torch.cuda.synchronize()
    what = f"{cfg['id']} {family}"
    got = contrib.t().cpu().double()
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} tap contributions were never written"
    # the 27 contributions per pixel: W2's product on a tile that is known exactly
    fold_exact = family == "chain_exact"            # test_tail_chain_is_exact proves certificate and fold for that family
    cb = M.tail_contrib_bound(o, fold_exact)
    want = o["rc"].y
    if float(cb.max()) == 0.0:
        bad = got != want
        assert not bad.any(), f"{what}: {int(bad.sum())} contributions differ from the exact model, first (pixel, tap * 3 + o) {bad.nonzero()[:6].tolist()}"
        ratio_c = 0.0
    else:
        ratio_c = R.worst_ratio(got, want, cb)
        assert ratio_c <= 1.0, f"{what}: contributions worst {ratio_c:.2f}x the bound of the W2 product"
    # refine_tail: sum, bias, PReLU, 2 sigmoid - 1, + I_t: the pointwise bound of tests/pointwise_ref.py at the model's argument, plus
    # what the argument's own error (0 in chain_exact) can move 2 sigmoid(r) - 1 = tanh(r / 2): at most half of it
    r, rb = M.tail_preact(o, n, h, w, cb)
    v, bound = R.residual_sigmoid64(o["it"], r)
    ratio_s = R.worst_ratio(s.cpu(), v, bound + 0.5 * rb)
    record_property("worst_ratio", max(ratio_c, ratio_s))
    record_property("per_stage", str({"contrib": round(ratio_c, 3), "it_sum": round(ratio_s, 3)}))
    print(f"{what}: worst err/bound contrib {ratio_c:.3f} it_sum {ratio_s:.3f}")
    assert ratio_s <= 1.0, f"{what}: it_sum worst {ratio_s:.2f}x the bound"
    assert torch.equal(cl, s.clamp(0, 1)), f"{what}: it_clamped is not clamp(it_sum, 0, 1) bit for bit"


@pytest.mark.parametrize("family", M.CHAIN_FAMILIES)
@pytest.mark.parametrize("cfg", M.CASES_TAIL, ids=lambda c: c["id"])
def test_tail_chain(cfg, family, dev, record_property):
    """atmvfi_conv3p's read-out + atmvfi_refine_tail, widths 128>64 and 64>32: one 16 x 16 tile, ragged tiles with several images,
    and 272 x 272 (289 tiles on 256 persistent workgroups)."""
    run_tail(cfg, family, dev, record_property)


@pytest.mark.parametrize("family", M.CHAIN_FAMILIES)
def test_tail_chain_f16_mode(family, dev, record_property):
    """The same with ``plane_terms`` = 1: the main product on hi(x), hi(w) alone (tests/f16_model.py), W2 still three-term."""
    run_tail(M.CASE_TAIL_F16, family, dev, record_property)
