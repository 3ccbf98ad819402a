"""GPU: the warp and resize kernels -- flow_warp (direct and LDS-tiled, planar and NHWC, fused with the flow up-sampling), flow_warp_ex's
padding modes and mask, warp_blend, the align_corners=True resize and the image pyramid -- against the plain float64 references of
tests/warp_ref.py at hostile coordinates (taps exactly on pixels, on -1, size - 1, size, one ulp beside them, on half pixels, hugging
the edges, non-finite), each held ELEMENTWISE to the bound that warp_ref derives from the kernel's arithmetic
(tests/test_warp_ref_cpu.py shows on the CPU that a faithful fp32 emulation stays inside these bounds and that subtly wrong kernels do
not).  Outputs are pre-filled with NaN, so an element that is not written fails.  Every test reports the worst err / bound in its
assertion message and as the ``worst_ratio`` property of its junit record."""
import functools
import importlib

import numpy as np
import pytest
import torch

import pointwise_ref as R
import warp_ref as W

pytestmark = pytest.mark.gpu

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip(dev):
    return hip_ops.HipOps(dev)


@pytest.fixture(autouse=True)
def tiles_restored(hip):
    """Whatever a test does with the A/B switch of the tiled warps, the next one starts from the product's setting."""
    try:
        yield
    finally:
        hip.warp_tiles = True


def report(record_property, what: str, worst: dict):
    ratio = max(worst.values())
    record_property("worst_ratio", ratio)
    record_property("per_case", str({k: round(v, 3) for k, v in worst.items()}))
    print(f"{what}: worst err/bound {ratio:.3f} { {k: round(v, 3) for k, v in worst.items()} }")
    return ratio


def forms(hip):
    """The direct and the LDS-tiled form of the planar warps, the switch restored whatever happens."""
    try:
        for tiles in (False, True):
            hip.warp_tiles = tiles
            yield "tiled" if tiles else "direct"
    finally:
        hip.warp_tiles = True


def nan_like(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def flow_layouts(flow: torch.Tensor):
    """The planar flow, and the same flow as channels 2..3 of an NHWC motion map (a permuted view)."""
    b, _, h, w = flow.shape
    mm = torch.full((b, h, w, 6), 5.0, device=flow.device)
    mm[..., 2:4] = flow.permute(0, 2, 3, 1)
    return {"planar": flow, "nhwc_pair": mm[..., 2:4].permute(0, 3, 1, 2)}


@functools.lru_cache(maxsize=None)
def warp_case(image: str, family: str, shape, padding: str = "zeros", seed: int = 0):
    """(src, flow, ref, bound, zero) of one case, numpy, computed once and shared (read only)."""
    b, c, h, w = shape
    src, flow = W.image_family(image, b, c, h, w, seed), W.flow_family(family, b, h, w, seed)
    ref = W.warp64(src, flow, padding)
    return src, flow, ref, W.warp_bound(ref, w, h, padding), W.must_be_zero(ref, w, h)


def check_warp(got: torch.Tensor, case, what: str) -> float:
    """err / bound of a zero-padding warp, with the zero contract and the NaN ban."""
    _, _, ref, bound, zero = case
    got = got.cpu().numpy()
    assert not np.isnan(got).any(), f"{what}: NaN (or an element that was not written) in the output"
    assert (got[np.broadcast_to(zero[:, None], got.shape)] == 0.0).all(), f"{what}: an element whose taps are all outside is not 0.0 exactly"
    return W.worst_ratio(got, ref["v"], bound)


WARP_SHAPES = [(1, 3, 8, 4096), (1, 1, 4096, 8), (2, 3, 9, 13), (1, 7, 24, 40), (1, 1, 2, 4), (1, 1, 2, 2)]
SMALL_SHAPES = [(2, 9, 13), (1, 24, 40), (1, 8, 4096)]            # (B, H, W): W % 4 != 0 / three tile rows, a ragged tile column / a 4K row
ids = lambda s: "x".join(str(v) for v in s)


# ------------------------------------------------------------------------------------------------------------------------- flow_warp
@pytest.mark.parametrize("family", W.FLOW_FAMILIES)
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=ids)
def test_flow_warp(shape, family, hip, dev, record_property):
    """(1,3,8,4096) / (1,1,4096,8): 4K rows and columns, the largest y0 * W + x0 and the largest round-trip error; (2,3,9,13): W % 4 != 0,
    direct whatever the switch; (1,7,24,40): three staging groups and a ragged last tile column; 2x4 and 2x2: the smallest accepted."""
    worst = {}
    for image in W.IMAGE_FAMILIES:
        case = warp_case(image, family, shape)
        src, flow = torch.from_numpy(case[0]).to(dev), torch.from_numpy(case[1]).to(dev)
        for form in forms(hip):
            assert hip._tiled_warp_ok(shape[3], src) == (form == "tiled" and shape[3] % 4 == 0)
            for layout, fv in flow_layouts(flow).items():
                dst = nan_like(shape, dev)
                hip.flow_warp(src, fv, dst)
                torch.cuda.synchronize()
                worst[(image, form, layout)] = check_warp(dst, case, f"flow_warp {ids(shape)} {family} {image} {form} {layout}")
    ratio = report(record_property, f"flow_warp {ids(shape)} {family}", worst)
    assert ratio <= 1.0, f"flow_warp {ids(shape)} {family}: worst err/bound {ratio:.3f} {worst}"


# ---------------------------------------------------------------------------------------------------------------------- flow_warp_ex
EX_SHAPES = [(2, 3, 9, 13), (1, 2, 24, 40), (1, 1, 8, 4096)]


@pytest.mark.parametrize("padding", W.PADDINGS)
@pytest.mark.parametrize("family", W.FINITE_FAMILIES)
@pytest.mark.parametrize("shape", EX_SHAPES, ids=ids)
def test_flow_warp_ex_padding_modes_and_mask(shape, family, padding, hip, dev, record_property):
    """Every family stays within +-8 spans of the image (halves reaches +-2 sizes).  The mask equals the fp32 expression
    2 p / (size - 1) - 1 in [-1, 1] element for element, and the float64 predicate wherever that is decided."""
    b, c, h, w = shape
    worst = {}
    for image in W.IMAGE_FAMILIES:
        src_np, flow_np, ref, bound, _ = warp_case(image, family, shape, padding)
        dst, mask = nan_like(shape, dev), torch.full((b, h, w), 7, dtype=torch.uint8, device=dev)
        hip.flow_warp_ex(torch.from_numpy(src_np).to(dev), torch.from_numpy(flow_np).to(dev), dst, mask=mask, padding_mode=padding)
        torch.cuda.synchronize()
        worst[image] = W.worst_ratio(dst.cpu().numpy(), ref["v"], bound)
        m = mask.cpu().numpy()
        assert np.isin(m, (0, 1)).all()
        assert np.array_equal(m.astype(bool), W.taps32(flow_np)["mask"]), "the mask is not the fp32 expression of the contract"
        inside, decided = W.mask64(flow_np)
        assert np.array_equal(m.astype(bool)[decided], inside[decided]), "the mask differs from the float64 predicate where that is decided"
    ratio = report(record_property, f"flow_warp_ex {padding} {ids(shape)} {family}", worst)
    assert ratio <= 1.0, f"flow_warp_ex {padding} {ids(shape)} {family}: worst err/bound {ratio:.3f} {worst}"


@pytest.mark.parametrize("padding", W.PADDINGS)
@pytest.mark.parametrize("shape", EX_SHAPES, ids=ids)
def test_flow_warp_ex_wild_coordinates(shape, padding, hip, dev, record_property):
    """zeros: the warp bound and the zero contract.  border / reflection: finite, and bit for bit the fp32 emulation of pad_coord (NaN and
    the infinities end on pixel 0 or size - 1 by fmaxf / fminf).  The mask as on the finite families."""
    b, c, h, w = shape
    worst = {}
    for image in W.IMAGE_FAMILIES:
        case = warp_case(image, "wild", shape, "zeros")
        src_np, flow_np = case[0], case[1]
        dst, mask = nan_like(shape, dev), torch.full((b, h, w), 7, dtype=torch.uint8, device=dev)
        hip.flow_warp_ex(torch.from_numpy(src_np).to(dev), torch.from_numpy(flow_np).to(dev), dst, mask=mask, padding_mode=padding)
        torch.cuda.synchronize()
        if padding == "zeros":
            worst[image] = check_warp(dst, case, f"flow_warp_ex zeros wild {image}")
        else:
            got = dst.cpu().numpy()
            assert np.isfinite(got).all(), f"{padding} {image}: a non-finite output"
            emu = W.warp32(src_np, flow_np, padding)
            worst[image] = 0.0 if np.array_equal(got, emu) else float("inf")
            assert np.array_equal(got, emu), f"{padding} {image}: differs from the fp32 emulation of pad_coord at {int((got != emu).sum())} elements"
        m = mask.cpu().numpy().astype(bool)
        assert np.array_equal(m, W.taps32(flow_np)["mask"])
        inside, decided = W.mask64(flow_np)
        assert np.array_equal(m[decided], inside[decided])
    ratio = report(record_property, f"flow_warp_ex {padding} {ids(shape)} wild", worst)
    assert ratio <= 1.0


# -------------------------------------------------------------------------------------------------------------------- flow_warp_nhwc
@pytest.mark.parametrize("family", W.FLOW_FAMILIES)
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=ids)
def test_flow_warp_nhwc_channel_slices(shape, c, family, hip, dev, record_property):
    """Source and destination are channel slices of wider maps (row pitch > C); the channels beside the destination stay untouched."""
    b, h, w = shape
    worst = {}
    for image in W.IMAGE_FAMILIES:
        case = warp_case(image, family, (b, c, h, w))
        wide_src = torch.full((b, h, w, c + 8), 3.0, device=dev)
        wide_src[..., 4:4 + c] = torch.from_numpy(case[0]).to(dev).permute(0, 2, 3, 1)
        wide_dst = nan_like((b, h, w, c + 12), dev)
        hip.flow_warp_nhwc(wide_src[..., 4:4 + c], torch.from_numpy(case[1]).to(dev), wide_dst[..., 8:8 + c])
        torch.cuda.synchronize()
        worst[image] = check_warp(wide_dst[..., 8:8 + c].permute(0, 3, 1, 2), case, f"flow_warp_nhwc C={c} {family} {image}")
        assert torch.isnan(wide_dst[..., :8]).all() and torch.isnan(wide_dst[..., 8 + c:]).all(), "a channel outside the slice was written"
    ratio = report(record_property, f"flow_warp_nhwc {ids(shape)} C={c} {family}", worst)
    assert ratio <= 1.0, f"flow_warp_nhwc {ids(shape)} C={c} {family}: worst err/bound {ratio:.3f} {worst}"


# --------------------------------------------------------------------------------------------------------------------- flow_warp_up2
@pytest.mark.parametrize("family", W.FINITE_FAMILIES)
@pytest.mark.parametrize("shape", [(2, 3, 17, 29), (1, 3, 16, 40), (1, 2, 2, 4)], ids=ids)
def test_flow_warp_up2(shape, family, hip, dev, record_property):
    """The warp half against the warp bound, the flow half against resize64(flow, 2H, 2W, 2.0); direct and tiled (W = 29: direct
    whatever the switch).  Finite flows: the up-sampled flow has no float64 reference at a NaN."""
    b, c, h, w = shape
    worst = {}
    flow_np = W.flow_family(family, b, h, w)
    up_ref, up_bound = W.resize64(flow_np, 2 * h, 2 * w, 2.0)
    for image in W.IMAGE_FAMILIES:
        case = warp_case(image, family, shape)
        src, flow = torch.from_numpy(case[0]).to(dev), torch.from_numpy(case[1]).to(dev)
        for form in forms(hip):
            dst, up = nan_like(shape, dev), nan_like((b, 2, 2 * h, 2 * w), dev)
            hip.flow_warp_up2(src, flow, dst, up)
            torch.cuda.synchronize()
            worst[(image, form, "warp")] = check_warp(dst, case, f"flow_warp_up2 {family} {image} {form}")
            worst[(image, form, "flow")] = W.worst_ratio(up.cpu().numpy(), up_ref, up_bound)
    ratio = report(record_property, f"flow_warp_up2 {ids(shape)} {family}", worst)
    assert ratio <= 1.0, f"flow_warp_up2 {ids(shape)} {family}: worst err/bound {ratio:.3f} {worst}"


# ------------------------------------------------------------------------------------------------------------------------ warp_blend
def sweep_for(n: int) -> torch.Tensor:
    """n arguments of the sigmoid: the whole sweep of pointwise_ref sampled evenly, its +-Inf / 0 / +-88.8 / +-103.9 kept."""
    sweep = R.sigmoid_sweep()
    r = sweep[torch.linspace(0, sweep.numel() - 9, n).long()]
    k = min(8, n)
    r[n - k:] = sweep[sweep.numel() - k:]
    return r


def run_warp_blend(hip, dev, im0, im1, flow0, flow1, r):
    """One launch with every output: -> dict of the planar outputs, pack15 (a 15-channel slice of a 16-channel map) and the plane sink."""
    b, _, h, w = im0.shape
    mm = torch.full((b, h, w, 8), 5.0, device=dev)
    mm[..., 0:2], mm[..., 2:4], mm[..., 4] = flow0.permute(0, 2, 3, 1), flow1.permute(0, 2, 3, 1), r
    o = {k: nan_like((b, 3, h, w), dev) for k in ("i0w", "i1w", "it")}
    o.update({k: nan_like((b, 2, h, w), dev) for k in ("f0", "f1")})
    o.update({k: nan_like((b, 1, h, w), dev) for k in ("m1", "m2")})
    o["orig0"], o["orig1"] = im0 * 0.5 + 0.125, im1 * 0.25 - 0.5
    o["pack"] = nan_like((b, h, w, 16), dev)
    o["planes"] = hip_ops.Planes.alloc(b * h * w, 16, dev)
    hip.warp_blend(im0, im1, mm[..., 0:5], o["i0w"], o["i1w"], o["it"], o["f0"], o["f1"], o["m1"], o["m2"], o["orig0"], o["orig1"],
                   o["pack"][..., :15], pack_planes=o["planes"])
    torch.cuda.synchronize()
    return o


def check_warp_blend(o, case0, case1, r, what: str) -> dict:
    """i0w / i1w against the warp bound, it against blend64, the masks and flows as test_gpu_pointwise_fp64 holds them, pack15 and the
    plane sink carrying exactly the planar outputs."""
    flow0, flow1 = (torch.from_numpy(c[1]).to(o["it"].device) for c in (case0, case1))
    worst = {"i0w": check_warp(o["i0w"], case0, what + " i0w"), "i1w": check_warp(o["i1w"], case1, what + " i1w")}
    it, bound = W.blend64(r.cpu().numpy(), case0[2], case1[2], case0[3], case1[3])
    assert not torch.isnan(o["it"]).any(), f"{what}: NaN in it"
    worst["it"] = W.worst_ratio(o["it"].cpu().numpy(), it, bound)
    assert same_bits(o["f0"], flow0) and same_bits(o["f1"], flow1), f"{what}: a flow output is not the motion map's flow"
    assert torch.equal(o["m2"], 1.0 - o["m1"]), f"{what}: mask2 is not 1 - mask1 bit for bit"
    s, sbound = R.sigmoid_mask64(r.cpu())
    worst["mask1"] = R.worst_ratio(o["m1"][:, 0].cpu(), s, sbound)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    want = torch.cat([nhwc(o["orig0"]), nhwc(o["i0w"]), nhwc(o["orig1"]), nhwc(o["i1w"]), nhwc(o["it"]), torch.zeros_like(nhwc(o["m1"]))], -1)
    assert same_bits(o["pack"][..., :15], want[..., :15]), f"{what}: pack15 does not carry the planar outputs"
    assert torch.isnan(o["pack"][..., 15]).all(), f"{what}: the channel beside pack15 was written"
    R.assert_planes_split_of(o["planes"], want.reshape(-1, 16), what + " plane sink")          # channel 16 of the plane pack: zero
    return worst


@pytest.mark.parametrize("family", W.FLOW_FAMILIES)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=ids)
def test_warp_blend_real_flows(shape, family, hip, dev, record_property):
    b, h, w = shape
    r = sweep_for(b * h * w).reshape(b, h, w).to(dev)
    worst = {}
    for img0, img1 in (("rand", "checker"), ("ramp", "hot")):
        case0, case1 = warp_case(img0, family, (b, 3, h, w)), warp_case(img1, family, (b, 3, h, w), "zeros", 1)
        im0, im1, flow0, flow1 = (torch.from_numpy(a).to(dev) for a in (case0[0], case1[0], case0[1], case1[1]))
        for form in forms(hip):
            assert hip._tiled_warp_ok(w, im0, im1) == (form == "tiled" and w % 4 == 0)
            o = run_warp_blend(hip, dev, im0, im1, flow0, flow1, r)
            for k, v in check_warp_blend(o, case0, case1, r, f"warp_blend {ids(shape)} {family} {img0}/{img1} {form}").items():
                worst[(img0, form, k)] = v
    ratio = report(record_property, f"warp_blend {ids(shape)} {family}", worst)
    assert ratio <= 1.0, f"warp_blend {ids(shape)} {family}: worst err/bound {ratio:.3f} {worst}"


# ---------------------------------------------------------------------------------------------------------------------------- resize
RESIZES = [((1, 2, 9, 13), (5, 7)), ((1, 2, 9, 13), (18, 26)), ((1, 2, 9, 13), (9, 13)), ((1, 2, 9, 13), (17, 25)), ((1, 2, 9, 13), (1, 7)),
           ((1, 2, 9, 13), (5, 1)), ((1, 2, 8, 4096), (16, 8192))]


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("sizes", RESIZES, ids=lambda s: f"{s[0][2]}x{s[0][3]}to{s[1][0]}x{s[1][1]}")
def test_resize_align_corners_fp64(sizes, scale, hip, dev, record_property):
    """From 9x13: down, x2, the identity (bit-exact), 17x25 (Ho - 1 a multiple of Hi - 1: every other output is a source pixel, exactly),
    Ho = 1, Wo = 1; a 4K row; each from a contiguous planar source and from the strided channel pair of an NHWC map."""
    (b, c, hi, wi), (ho, wo) = sizes
    worst = {}
    for image in W.IMAGE_FAMILIES:
        src_np = W.image_family(image, b, c, hi, wi)
        ref, bound = W.resize64(src_np, ho, wo, scale)
        src = torch.from_numpy(src_np).to(dev)
        mm = torch.full((b, hi, wi, 6), 5.0, device=dev)
        mm[..., 2:4] = src.permute(0, 2, 3, 1)
        for layout, view in (("planar", src), ("nhwc_pair", mm[..., 2:4].permute(0, 3, 1, 2))):
            dst = nan_like((b, c, ho, wo), dev)
            hip.resize(view, dst, scale)
            torch.cuda.synchronize()
            worst[(image, layout)] = W.worst_ratio(dst.cpu().numpy(), ref, bound)
            if (ho, wo) == (hi, wi):
                assert torch.equal(dst, src * scale), "the identity resize is not bit-exact"
            if (ho, wo) == (17, 25):
                assert torch.equal(dst[:, :, ::2, ::2], src * scale), "an output that lands on a source pixel is not that pixel"
    ratio = report(record_property, f"resize {hi}x{wi} -> {ho}x{wo} x{scale}", worst)
    assert ratio <= 1.0, f"resize {hi}x{wi} -> {ho}x{wo} x{scale}: worst err/bound {ratio:.3f} {worst}"


# --------------------------------------------------------------------------------------------------------------------- image pyramid
@pytest.mark.parametrize("with_pack", [False, True], ids=["levels", "levels_and_pack"])
@pytest.mark.parametrize("size", [(64, 96), (8, 8), (22, 26), (18, 30)], ids=ids)
def test_image_pyramid_fp64(size, with_pack, hip, dev, record_property):
    """(8, 8): level 3 is 1 x 1; (22, 26) and (18, 30): odd intermediate sizes (11 x 13 -> 5 x 6 -> 2 x 3; 9 x 15 -> 4 x 7 -> 2 x 3).  Each
    level against pyramid64's recursive bound."""
    h, w = size
    b = 2
    worst = {}
    for image in W.IMAGE_FAMILIES:
        frames = np.concatenate([W.image_family(image, b, 3, h, w), W.image_family(image, b, 3, h, w, 1)[:, :, ::-1].copy()])
        levels = W.pyramid64(frames)
        im0, im1 = torch.from_numpy(frames[:b]).to(dev), torch.from_numpy(frames[b:]).to(dev)
        lv = [nan_like((2 * b, 3, h >> l, w >> l), dev) for l in (1, 2, 3)]
        pack = nan_like((2 * b, h, w, 4), dev) if with_pack else None
        hip.image_pyramid(im0, im1, *lv, pack=pack)
        torch.cuda.synchronize()
        for l, (got, (ref, bound)) in enumerate(zip(lv, levels), 1):
            worst[(image, l)] = W.worst_ratio(got.cpu().numpy(), ref, bound)
        if with_pack:
            want = torch.cat([torch.from_numpy(frames).to(dev).permute(0, 2, 3, 1), torch.zeros(2 * b, h, w, 1, device=dev)], -1)
            assert same_bits(pack, want), "pack is not the NHWC4 stack of the two frames"
    ratio = report(record_property, f"image_pyramid {h}x{w}", worst)
    assert ratio <= 1.0, f"image_pyramid {h}x{w}: worst err/bound {ratio:.3f} {worst}"


# -------------------------------------------------------------------------------------------------------------------- one set of taps
@pytest.mark.parametrize("family", ["ulp", "edges"])
@pytest.mark.parametrize("shape", [(1, 24, 40), (1, 8, 4096)], ids=ids)
def test_every_zero_padding_form_has_the_same_taps(shape, family, hip, dev):
    """flow_warp, flow_warp_ex('zeros'), the warp half of flow_warp_up2, flow_warp_nhwc and warp_blend's i0w share make_taps: the same
    bits on the same inputs, in the direct and in the tiled form."""
    b, h, w = shape
    src_np, flow_np = W.image_family("rand", b, 3, h, w), W.flow_family(family, b, h, w)
    src, flow = torch.from_numpy(src_np).to(dev), torch.from_numpy(flow_np).to(dev)
    r = sweep_for(b * h * w).reshape(b, h, w).to(dev)
    outs = {}
    for form in forms(hip):
        d = nan_like((b, 3, h, w), dev)
        hip.flow_warp(src, flow, d)
        outs[f"flow_warp {form}"] = d
        d, up = nan_like((b, 3, h, w), dev), nan_like((b, 2, 2 * h, 2 * w), dev)
        hip.flow_warp_up2(src, flow, d, up)
        outs[f"flow_warp_up2 {form}"] = d
        outs[f"warp_blend i0w {form}"] = run_warp_blend(hip, dev, src, src.flip(1).contiguous(), flow, flow.flip(1).contiguous(), r)["i0w"]
    d = nan_like((b, 3, h, w), dev)
    hip.flow_warp_ex(src, flow, d, padding_mode="zeros")
    outs["flow_warp_ex zeros"] = d
    s4, d4 = torch.zeros(b, h, w, 4, device=dev), nan_like((b, h, w, 4), dev)
    s4[..., :3] = src.permute(0, 2, 3, 1)
    hip.flow_warp_nhwc(s4, flow, d4)
    outs["flow_warp_nhwc"] = d4[..., :3].permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    first = outs["flow_warp direct"]
    assert not torch.isnan(first).any()
    for k, v in outs.items():
        assert same_bits(v, first), f"{k} differs from the direct flow_warp at {int((v != first).sum())} elements"


# ------------------------------------------------------------------------------------------------------------- the staged-box boundary
def test_staged_box_boundary_tiles(hip, dev, record_property):
    """Flow fields constructed tile by tile (warp_ref.boundary_flow) put single 32 x 8 tiles on the boundary of the LDS box rule: exactly
    64 aligned columns x 24 rows (fits), 65 columns, 25 rows (fall back), a leftmost tap at x = 3 (mod 4) with and without room for the
    three columns the alignment eats, a box whose last 16-byte load ends at W, a box clipped at row H - 1, an empty box beside a normal
    one, a single live lane.  The restated rule confirms each tile's side; then the tiled flow_warp and warp_blend are held to the fp64
    bound and to the direct kernels' bits."""
    shape = W.BOX_SHAPE
    b, c, h, w = shape
    flows = [W.boundary_flow(0), W.boundary_flow(7)]
    for f, shift in zip(flows, (0, 7)):
        W.check_box_cases(f, shift)
    r = sweep_for(b * h * w).reshape(b, h, w).to(dev)
    worst = {}
    for img0, img1 in (("rand", "checker"), ("ramp", "hot")):
        cases = []
        for image, f in ((img0, flows[0]), (img1, flows[1])):
            src = W.image_family(image, b, c, h, w)
            ref = W.warp64(src, f)
            cases.append((src, f, ref, W.warp_bound(ref, w, h), W.must_be_zero(ref, w, h)))
        im0, im1, flow0, flow1 = (torch.from_numpy(a).to(dev) for a in (cases[0][0], cases[1][0], cases[0][1], cases[1][1]))
        res = {}
        for form in forms(hip):
            assert hip._tiled_warp_ok(w, im0, im1) == (form == "tiled")
            d0, d1 = nan_like(shape, dev), nan_like(shape, dev)
            hip.flow_warp(im0, flow0, d0)
            hip.flow_warp(im1, flow1, d1)
            o = run_warp_blend(hip, dev, im0, im1, flow0, flow1, r)
            worst[(img0, form, "flow_warp 0")] = check_warp(d0, cases[0], f"flow_warp {form} {img0}")
            worst[(img1, form, "flow_warp 1")] = check_warp(d1, cases[1], f"flow_warp {form} {img1}")
            for k, v in check_warp_blend(o, cases[0], cases[1], r, f"warp_blend {form} {img0}/{img1}").items():
                worst[(img0, form, k)] = v
            res[form] = [d0, d1, o["i0w"], o["i1w"], o["it"], o["pack"][..., :15], o["planes"].t.clone()]
        for i, (x, y) in enumerate(zip(res["direct"], res["tiled"])):
            assert torch.equal(x.contiguous().view(torch.int16 if x.dtype == torch.float16 else torch.int32),
                               y.contiguous().view(torch.int16 if y.dtype == torch.float16 else torch.int32)), f"{img0}/{img1}: tiled output {i} differs from the direct kernel's"
    ratio = report(record_property, "staged-box boundary tiles", worst)
    assert ratio <= 1.0, f"staged-box boundary tiles: worst err/bound {ratio:.3f} {worst}"
