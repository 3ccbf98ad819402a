"""CPU: the yardstick of tests/test_gpu_warp_fp64.py is sound.  A faithful fp32 emulation of the warp / resize kernels (numpy, one
rounding per operation) and fp32 torch stay inside the elementwise bounds of tests/warp_ref.py on every input family; the hand-written
float64 references agree with torch's float64 operators; every subtly wrong kernel (a switchable mutant of the emulation) leaves the
bound on a named family; the constructed tiles of the staged-box test are on the intended side of the restated rule."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import warp_ref as W

SHAPES = [(8, 4096), (4096, 8), (9, 13), (24, 40), (2, 2)]
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]
CH = 2


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def torch_warp(src, flow, padding, dtype):
    """grid_sample(align_corners=True) on the normalised grid 2 p / (size - 1) - 1, as a flow warp is commonly written."""
    src, flow = t(src).to(dtype), t(flow).to(dtype)
    _, _, h, w = src.shape
    px = torch.arange(w, dtype=dtype)[None, None, :] + flow[:, 0]
    py = torch.arange(h, dtype=dtype)[None, :, None] + flow[:, 1]
    grid = torch.stack([2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1], -1)
    return F.grid_sample(src, grid, mode="bilinear", padding_mode=padding, align_corners=True).numpy()


def ratios_over_images(fn, flow, padding, h, w, seed=0):
    """worst err / bound of fn(src, flow) per image family."""
    out = {}
    for im in W.IMAGE_FAMILIES:
        src = W.image_family(im, 1, CH, h, w, seed)
        ref = W.warp64(src, flow, padding)
        out[im] = W.worst_ratio(fn(src, flow), ref["v"], W.warp_bound(ref, w, h, padding))
    return out


# ------------------------------------------------------------------------------------------------------- the emulation inside the bounds
@pytest.mark.parametrize("family", W.FLOW_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_emulation_inside_the_warp_bound(shape, family, record_property):
    h, w = shape
    worst = {}
    for seed in (0, 1):
        flow = W.flow_family(family, 1, h, w, seed)
        worst[seed] = ratios_over_images(lambda s, f: W.warp32(s, f), flow, "zeros", h, w, seed)
    top = max(max(v.values()) for v in worst.values())
    record_property("worst_ratio", top)
    print(f"emulation zeros {h}x{w} {family}: worst err/bound per seed and image { {s: {k: round(v, 3) for k, v in d.items()} for s, d in worst.items()} }")
    assert top <= 1.0, f"{family} {h}x{w}: {worst}"


@pytest.mark.parametrize("padding", ["border", "reflection"])
@pytest.mark.parametrize("family", W.FINITE_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_emulation_inside_the_padding_mode_bounds(shape, family, padding, record_property):
    h, w = shape
    flow = W.flow_family(family, 1, h, w)
    worst = ratios_over_images(lambda s, f: W.warp32(s, f, padding), flow, padding, h, w)
    record_property("worst_ratio", max(worst.values()))
    print(f"emulation {padding} {h}x{w} {family}: worst err/bound per image { {k: round(v, 3) for k, v in worst.items()} }")
    assert max(worst.values()) <= 1.0, f"{padding} {family} {h}x{w}: {worst}"


def test_emulation_zero_contract_and_no_nan():
    """Where the reference is 0 because a coordinate is non-finite or more than delta outside, the emulation gives 0.0 exactly."""
    for h, w in SHAPES:
        for family in W.FLOW_FAMILIES:
            flow = W.flow_family(family, 1, h, w)
            src = W.image_family("rand", 1, CH, h, w) + 1.0
            got = W.warp32(src, flow)
            zero = W.must_be_zero(W.warp64(src, flow), w, h)
            assert not np.isnan(got).any()
            assert (got[np.broadcast_to(zero[:, None], got.shape)] == 0.0).all(), f"{family} {h}x{w}"
            if family == "wild":
                assert zero.sum() >= 0.5 * zero.size


# ---------------------------------------------------------------------------------------------------------- fp32 torch inside the bounds
@pytest.mark.parametrize("padding", W.PADDINGS)
@pytest.mark.parametrize("family", W.FINITE_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fp32_torch_inside_the_warp_bound(shape, family, padding, record_property):
    h, w = shape
    flow = W.flow_family(family, 1, h, w)
    worst = ratios_over_images(lambda s, f: torch_warp(s, f, padding, torch.float32), flow, padding, h, w)
    record_property("worst_ratio", max(worst.values()))
    print(f"fp32 torch {padding} {h}x{w} {family}: worst err/bound per image { {k: round(v, 3) for k, v in worst.items()} }")
    assert max(worst.values()) <= 1.0, f"{padding} {family} {h}x{w}: {worst}"


# ------------------------------------------------------------------------------------------- the references against torch's float64 operators
@pytest.mark.parametrize("padding", W.PADDINGS)
@pytest.mark.parametrize("family", ["gauss", "halves"])
@pytest.mark.parametrize("shape", [(9, 13), (24, 40), (2, 2)], ids=["9x13", "24x40", "2x2"])
def test_warp64_agrees_with_float64_grid_sample(shape, family, padding):
    """A cross-check of the hand-written gathers, not the reference: 1e-12 of the image's scale (the normalisation round trip of the
    float64 grid moves a coordinate by ~1e-14 px at these sizes)."""
    h, w = shape
    flow = W.flow_family(family, 2, h, w)
    for im in ("rand", "ramp"):
        src = W.image_family(im, 2, CH, h, w)
        v = W.warp64(src, flow, padding)["v"]
        gs = torch_warp(src, flow, padding, torch.float64)
        assert np.abs(v - gs).max() <= 1e-12 * max(1.0, np.abs(src).max()), f"{im}: {np.abs(v - gs).max()}"


RESIZES = [((9, 13), (5, 7)), ((9, 13), (18, 26)), ((9, 13), (9, 13)), ((9, 13), (17, 25)), ((9, 13), (1, 7)), ((9, 13), (5, 1)), ((8, 4096), (16, 8192))]


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("sizes", RESIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_references_emulation_and_torch(sizes, scale, record_property):
    (hi, wi), (ho, wo) = sizes
    worst = {}
    for im in W.IMAGE_FAMILIES:
        src = W.image_family(im, 1, CH, hi, wi)
        v, bound = W.resize64(src, ho, wo, scale)
        ft = F.interpolate(t(src).double(), size=(ho, wo), mode="bilinear", align_corners=True).numpy() * scale
        assert np.abs(v - ft).max() <= 1e-12 * max(1.0, np.abs(src).max())
        f32 = (F.interpolate(t(src), size=(ho, wo), mode="bilinear", align_corners=True) * scale).numpy()
        emu = W.resize32(src, ho, wo, scale)
        worst[im] = (round(W.worst_ratio(emu, v, bound), 3), round(W.worst_ratio(f32, v, bound), 3))
        if (ho, wo) == (hi, wi):
            assert np.array_equal(emu, src * np.float32(scale)), "the identity resize is not bit-exact"
        if (ho, wo) == (17, 25):
            assert np.array_equal(emu[:, :, ::2, ::2], src * np.float32(scale)), "an output on a source pixel is not that pixel"
    top = max(max(p) for p in worst.values())
    record_property("worst_ratio", top)
    print(f"resize {hi}x{wi} -> {ho}x{wo} x{scale}: worst err/bound (emulation, fp32 torch) per image {worst}")
    assert top <= 1.0, worst


PYRAMIDS = [(64, 96), (8, 8), (22, 26), (18, 30)]


@pytest.mark.parametrize("size", PYRAMIDS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_reference_emulation_and_torch(size, record_property):
    h, w = size
    worst = {}
    for im in W.IMAGE_FAMILIES:
        src = W.image_family(im, 2, 3, h, w)
        levels = W.pyramid64(src)
        emu = W.pyramid32(src)
        cur32, cur64 = t(src), t(src).double()
        for l, ((v, bound), e) in enumerate(zip(levels, emu), 1):
            assert v.shape[2:] == (h >> l, w >> l)
            cur32 = F.interpolate(cur32, scale_factor=0.5, mode="bilinear", align_corners=True)
            cur64 = F.interpolate(cur64, scale_factor=0.5, mode="bilinear", align_corners=True)
            assert np.abs(v - cur64.numpy()).max() <= 1e-12 * max(1.0, np.abs(src).max())
            worst[(im, l)] = (round(W.worst_ratio(e, v, bound), 3), round(W.worst_ratio(cur32.numpy(), v, bound), 3))
    top = max(max(p) for p in worst.values())
    record_property("worst_ratio", top)
    print(f"pyramid {h}x{w}: worst err/bound (emulation, fp32 torch) per image and level {worst}")
    assert top <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------------------- the mask
@pytest.mark.parametrize("family", W.FLOW_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mask_emulation_against_the_float64_predicate(shape, family):
    """The fp32 expression equals the float64 predicate wherever that is decided (||g| - 1| > 4 U), and torch's fp32 expression."""
    h, w = shape
    flow = W.flow_family(family, 1, h, w)
    m32 = W.taps32(flow)["mask"]
    inside, decided = W.mask64(flow)
    assert np.array_equal(m32[decided], inside[decided])
    f = t(flow)
    gx = 2 * (torch.arange(w, dtype=torch.float32)[None, None, :] + f[:, 0]) / (w - 1) - 1
    gy = 2 * (torch.arange(h, dtype=torch.float32)[None, :, None] + f[:, 1]) / (h - 1) - 1
    assert np.array_equal(m32, ((gx >= -1) & (gy >= -1) & (gx <= 1) & (gy <= 1)).numpy())
    if family in ("integers", "ulp") and h * w > 4:
        assert (~decided).any() and m32.any() and (~m32).any()


# ---------------------------------------------------------------------------------------------------------------------------- the mutants
# mutant -> (padding mode, the flow families on one of which it must leave the bound)
WARP_MUTANT_FAMILIES = {
    "trunc": ("zeros", ("edges", "integers")),                 # floor and trunc differ on (-1, 0)
    "swap_ax": ("zeros", ("gauss", "halves")),
    "swap_ay": ("zeros", ("gauss", "halves")),
    "x1_le_W": ("zeros", ("edges",)),                          # x0 = W - 1 with ax > 0 reads the next row's first pixel
    "y1_le_H": ("zeros", ("edges",)),                          # y0 = H - 1 with ay > 0 reads the next plane's first row
    "stride": ("zeros", ("gauss", "integers")),
    "no_far": ("zeros", ("wild",)),                            # a NaN coordinate converts to pixel 0 and its NaN weights reach the output
    "border_size": ("border", ("edges", "integers")),
    "reflect_no_flip": ("reflection", ("halves", "edges")),
}


@pytest.mark.parametrize("mutant", list(WARP_MUTANT_FAMILIES))
def test_warp_mutants_leave_the_bound(mutant):
    padding, families = WARP_MUTANT_FAMILIES[mutant]
    report = {}
    for family in families:
        for h, w in ((9, 13), (24, 40), (8, 4096)):
            flow = W.flow_family(family, 1, h, w)
            r = ratios_over_images(lambda s, f: W.warp32(s, f, padding, mutant), flow, padding, h, w)
            report[(family, h, w)] = max(r.values())
    print(f"mutant {mutant}: worst err/bound {report}")
    for family in families:
        assert max(v for k, v in report.items() if k[0] == family) > 1.0, f"mutant {mutant} stays inside the bound on {family}: {report}"
    if mutant == "no_far":
        flow = W.flow_family("wild", 1, 9, 13)
        assert np.isnan(W.warp32(W.image_family("rand", 1, CH, 9, 13), flow, "zeros", mutant)).any()


def test_nan_test_of_far_is_implied_by_the_clamp():
    """``far`` also tests ``!(ix == ix)``.  Removing that test alone changes nothing: fmaxf(NaN, -2) = -2, and ``cx != fx0`` is true for
    a NaN fx0, so the clamp comparison already marks a NaN coordinate as far (and x0 = -2 is outside whatever ``far`` says).  The
    mutant is EQUIVALENT -- bit-identical on every family, the wild one included -- and cannot leave the bound; what a lost NaN guard
    does is shown by the ``no_far`` mutant."""
    for h, w in ((9, 13), (24, 40)):
        for family in W.FLOW_FAMILIES:
            flow = W.flow_family(family, 1, h, w)
            src = W.image_family("rand", 1, CH, h, w)
            a, b = W.warp32(src, flow), W.warp32(src, flow, "zeros", "no_nan_test")
            assert np.array_equal(a, b) and not np.isnan(b).any()


def test_mask_mutant_on_unnormalised_coordinates():
    """p >= 0 for 2 p / (size - 1) - 1 >= -1: a coordinate one rounding below zero is inside by the contract, outside by the mutant."""
    caught = {}
    for family in ("ulp", "edges", "gauss"):
        flow = W.flow_family(family, 1, 24, 40)
        caught[family] = int((W.mask_unnormalised32(flow) != W.taps32(flow)["mask"]).sum())
    print(f"mask on un-normalised coordinates: elements that differ {caught}")
    assert caught["ulp"] > 0


def test_resize_and_pyramid_mutants_leave_the_bound():
    src = W.image_family("rand", 1, CH, 9, 13)
    for ho, wo in ((5, 7), (18, 26)):
        v, bound = W.resize64(src, ho, wo)
        assert W.worst_ratio(W.resize32(src, ho, wo, 1.0, "ac_false"), v, bound) > 1.0
    flow = W.flow_family("gauss", 1, 9, 13)
    v, bound = W.resize64(flow, 18, 26, 2.0)
    assert W.worst_ratio(W.resize32(flow, 18, 26, 2.0), v, bound) <= 1.0
    assert W.worst_ratio(W.resize32(flow, 18, 26, 1.0), v, bound) > 1.0, "an up-sampled flow that is not doubled stays inside the bound"
    for h, w in ((64, 96), (22, 26)):
        frames = W.image_family("rand", 2, 3, h, w)
        (_, _), (v2, b2), (_, _) = W.pyramid64(frames)
        assert W.worst_ratio(W.pyramid32(frames)[1], v2, b2) <= 1.0
        assert W.worst_ratio(W.pyramid32(frames, "l2_direct")[1], v2, b2) > 1.0, "level 2 taken from level 0 stays inside the bound"
        assert W.worst_ratio(W.pyramid64(frames, direct_level2=True)[1][0], v2, b2) > 1.0


# --------------------------------------------------------------------------------------------------------------------------- the box rule
@pytest.mark.parametrize("shift", [0, 7])
def test_constructed_tiles_are_on_the_intended_side_of_the_box_rule(shift):
    boxes = W.check_box_cases(W.boundary_flow(shift), shift)
    assert len(boxes) == 15
    named = {W.case_tile(n, shift) for n in W.BOX_CASES}
    assert all(b["state"] == "fits" and b["nv"] <= 10 and b["h"] <= 10 for k, b in boxes.items() if k not in named), "a zero-flow tile stages its own rows"


def test_box_rule_on_drawn_flows():
    """Gaussian flows of sigma 6 reach beyond the 64 x 24 box in some tiles and not in others; a far field leaves every tile empty."""
    states = [b["state"] for b in W.staged_boxes(W.flow_family("gauss", 1, 40, 96)).values()]
    assert "falls back" in states
    small = (W.flow_family("gauss", 1, 40, 96) / 6).astype(np.float32)
    assert all(b["state"] == "fits" for b in W.staged_boxes(small).values())
    assert all(b["state"] == "empty" for b in W.staged_boxes(np.full((1, 2, 40, 96), 500.0, np.float32)).values())
