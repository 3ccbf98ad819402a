"""GPU: the fp32 pointwise kernels -- depth-wise 3x3 + GELU (every kernel instance), LayerNorm, the ``2 * sigmoid - 1`` residual sites,
warp_blend's masks and the motion head -- against plain float64 references on hostile inputs, each held ELEMENTWISE to the bound that
tests/pointwise_ref.py derives from the kernel's arithmetic (tests/test_pointwise_ref_cpu.py shows on the CPU that well-behaved fp32
stays inside these bounds and that subtly wrong kernels do not).  Every test reports the worst ratio err / bound in its assertion
message and as the ``worst_ratio`` property of its junit record."""
import importlib

import pytest
import torch

import f16x3_model as M
import pointwise_ref as R

pytestmark = pytest.mark.gpu

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
windows = importlib.import_module("atm-vfi_amd.windows")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip(dev):
    return hip_ops.HipOps(dev)


def report(record_property, what: str, ratio: float, **more):
    record_property("worst_ratio", ratio)
    for k, v in more.items():
        record_property(k, v)
    print(f"{what}: worst err/bound {ratio:.3f} {more if more else ''}")


# ------------------------------------------------------------------ which dw-conv kernel a launch takes
def dwconv_instance(shape, planes_only: bool, dev) -> str:
    """The dispatch rule of atmvfi_dwconv3x3_gelu, restated (pointwise.hip, the body of that function: ``if (!out && C % 64 == 0 &&
    H >= 8)`` with ``RS = H % 17 == 0 ? 17 : ...`` and ``... < 8ll * atmvfi::cu_count()) RS = 8`` at lines 1244-1263, ``tall = ... >=
    8ll * atmvfi::cu_count()`` at lines 1266-1281, the per-pixel kernel below; cu_count() = the device's compute units rounded down to
    a multiple of 8, common.h:24-36)."""
    n, h, w, c = shape
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    cus = 256 if cus < 8 else cus // 8 * 8
    if c % 64:
        return "pixel"
    if planes_only and h >= 8:
        xgroups, cblocks = (w + 7) // 8, c // 32
        rs = 17 if h % 17 == 0 else 16 if h % 16 == 0 else 8 if h % 8 == 0 else 16 if h >= 16 else 8
        if n * ((h + rs - 1) // rs) * xgroups * cblocks < 8 * cus:
            rs = 8
        return f"dma<{rs}>"
    xblocks, cblocks = (w + 15) // 16, c // 64
    return "rows<16>" if n * ((h + 15) // 16) * xblocks * cblocks >= 8 * cus else "rows<8>"


# The two large shapes (26M and 18M elements) are the SMALLEST the dispatch thresholds allow on a 256-CU device: the 16-row sliding
# window needs N * ceil(H / 16) * ceil(W / 16) * C / 64 >= 2048 blocks (2 * 4 * 16 * 16 = 2048, with a 3-row last strip and a 10-wide
# last x-block), the 17- and 16-row LDS-DMA instances N * strips * ceil(W / 8) * C / 32 >= 2048 units (2 * 3 * 32 * 32 = 6144; H = 35 =
# 16 + 16 + 3 makes the last strip overlap the one before).  Their reference and comparison run on the GPU in float64.
DW_CASES = [
    # kernel instance, shape, plane sink only
    ("pixel", (1, 9, 11, 100), False),
    ("rows<8>", (1, 11, 9, 64), False),
    ("rows<16>", (2, 51, 250, 1024), False),
    ("dma<17>", (2, 51, 250, 1024), True),
    ("dma<16>", (2, 35, 250, 1024), True),
]
DW_IDS = [c[0].replace("<", "").replace(">", "") for c in DW_CASES]


def require_instance(want: str, shape, planes_only: bool, dev):
    got = dwconv_instance(shape, planes_only, dev)
    assert got == want, (f"shape {shape} ({'planes only' if planes_only else 'fp32 rows'}) selects dwconv kernel {got} on this device "
                         f"({torch.cuda.get_device_properties(dev).multi_processor_count} CUs), not {want}: this case would test something else")


assert_planes_split_of = R.assert_planes_split_of


def run_dwconv(hip, x, w, b, planes_only: bool, what: str):
    """-> the fp32 rows [N,H,W,C] of the kernel under test; with ``planes_only`` the LDS-DMA kernel runs too and its planes must be
    the exact split of those rows (the two kernels promise the same arithmetic in the same order)."""
    n, h, wd, c = x.shape
    wt = hip.pack_dw_weight(w)
    of = torch.full((n, h, wd, c), 9.0, device=x.device)
    hip.dwconv_gelu(x, of, wt, b)
    if planes_only:
        p = hip_ops.Planes.alloc(n * h * wd, c, x.device)
        hip.dwconv_gelu(x, None, wt, b, planes=p)
        torch.cuda.synchronize()
        assert_planes_split_of(p, of.reshape(-1, c), what)
    return of


@pytest.mark.parametrize("case", DW_CASES, ids=DW_IDS)
def test_gelu_alone_through_every_dwconv_kernel(case, hip, dev, record_property):
    """Weights 1 on the centre tap, 0 elsewhere, bias 0: the accumulator is the input exactly, the output gelu_erf2(x) alone, held to
    ``gelu_bound`` over the whole GELU sweep (both joints of erf_2range to 4096 ulps, subnormals, +-1e30, 2^22 points on [-8, 8])."""
    want, shape, planes_only = case
    require_instance(want, shape, planes_only, dev)
    if planes_only:
        require_instance("rows<16>" if shape[1] == 51 else "rows<8>", shape, False, dev)
    n, h, wd, c = shape
    numel = n * h * wd * c
    sweep = R.gelu_sweep().to(dev)
    w, b = (t.to(dev) for t in R.centre_tap_params(c))
    if numel >= sweep.numel():
        x = R.tile_to(sweep, numel).reshape(shape)
        got = run_dwconv(hip, x, w, b, planes_only, want)
    else:                               # a small map: the sweep goes through in as many launches as it takes
        k = (sweep.numel() + numel - 1) // numel
        x = R.tile_to(sweep, k * numel).reshape(k, *shape)
        got = torch.full_like(x, 9.0)
        wt = hip.pack_dw_weight(w)
        for i in range(k):
            hip.dwconv_gelu(x[i], got[i], wt, b)
    torch.cuda.synchronize()
    ratio = R.worst_ratio(got, R.gelu64(x), R.gelu_bound(x))
    report(record_property, f"GELU alone through {want}", ratio)
    assert ratio <= 1.0, f"{want}: gelu_erf2 exceeds gelu_bound, worst err/bound {ratio:.3f}"


@pytest.mark.parametrize("scale", R.DWCONV_SCALES)
@pytest.mark.parametrize("case", DW_CASES, ids=DW_IDS)
def test_dwconv_gelu_general_weights(case, scale, hip, dev, record_property):
    want, shape, planes_only = case
    require_instance(want, shape, planes_only, dev)
    n, h, wd, c = shape
    numel = n * h * wd * c
    if numel <= 1 << 20:
        x = R.dwconv_input(shape, scale).to(dev)
    else:                               # any tiled random input will do (an odd period, so that no two channels see the same map)
        x = R.tile_to(R.dwconv_input((1000003,), scale).to(dev), numel).reshape(shape)
    w, b = (t.to(dev) for t in R.dwconv_params(c))
    got = run_dwconv(hip, x, w, b, planes_only, want)
    torch.cuda.synchronize()
    ref, bound = R.dwconv_gelu64(x, w, b)
    ratio = R.worst_ratio(got, ref, bound)
    report(record_property, f"dwconv + GELU {want} scale {scale}", ratio)
    assert ratio <= 1.0, f"{want} scale {scale}: worst err/bound {ratio:.3f}"


@pytest.mark.parametrize("case", DW_CASES[:2], ids=DW_IDS[:2])
def test_dwconv_gelu_channel_slice_of_a_wider_map(case, hip, dev, record_property):
    """Input and output are channel slices (row pitch > C); the channels beside the output slice stay untouched."""
    want, shape, _ = case
    require_instance(want, shape, False, dev)
    n, h, wd, c = shape
    x = R.dwconv_input(shape, 2.0).to(dev)
    w, b = (t.to(dev) for t in R.dwconv_params(c))
    wide_in = torch.full((n, h, wd, c + 64), 7.0, device=dev)
    wide_in[..., 64:] = x
    wide_out = torch.full((n, h, wd, c + 32), 9.0, device=dev)
    hip.dwconv_gelu(wide_in[..., 64:], wide_out[..., 16:16 + c], hip.pack_dw_weight(w), b)
    torch.cuda.synchronize()
    ref, bound = R.dwconv_gelu64(x, w, b)
    ratio = R.worst_ratio(wide_out[..., 16:16 + c], ref, bound)
    report(record_property, f"dwconv + GELU {want} on a channel slice", ratio)
    assert ratio <= 1.0, f"{want}: worst err/bound {ratio:.3f}"
    assert (wide_out[..., :16] == 9.0).all() and (wide_out[..., 16 + c:] == 9.0).all()


# ------------------------------------------------------------------ LayerNorm
@pytest.fixture(scope="module")
def ln_cases(dev):
    """Per channel width: the seven hostile families stacked (7 x 64 rows), the float64 reference and its bound -- computed once."""
    out = {}
    for c in R.LN_WIDTHS:
        x, gamma, beta = R.layernorm_inputs(c)
        y, bound = R.layernorm64(x, gamma, beta)
        out[c] = tuple(t.to(dev) for t in (x, gamma, beta, y, bound))
    return out


@pytest.mark.parametrize("mode", ["plain", "window_map", "groups", "rows_and_planes"])
@pytest.mark.parametrize("c", R.LN_WIDTHS)
def test_layernorm_hostile_rows(c, mode, ln_cases, hip, dev, record_property):
    """C = 224: one partial vector per lane; 448: the second vector (has1) on 48 of 64 lanes; 512: both vectors full; 672: the loop
    path.  Families: plain; mean 1000 sigma 1; mean 100 sigma 0.01; sigma 1e-4 (variance far below eps); constant rows; one 1e4 outlier;
    scale 1e12."""
    x, gamma, beta, y, bound = ln_cases[c]
    rows = x.shape[0]
    assert rows == 448
    src_of_row = torch.arange(rows, device=dev)
    planes = None
    if mode == "plain":
        out = torch.full((rows, c), 9.0, device=dev)
        hip.layernorm(x, out, gamma, beta)
    elif mode == "window_map":                 # gathered into window order; zero-padded tokens (negative entries) are beta exactly
        geo = windows.build_window_geometry(2, 14, 16, 4, 2)
        assert geo.row_map.numel() == 512 and (geo.row_map < 0).any() and int(geo.row_map.max()) == rows - 1
        src_of_row = geo.row_map.to(dev).long()
        out = torch.full((512, c), 9.0, device=dev)
        hip.layernorm(x, out, gamma, beta, geo.row_map.to(dev))
    elif mode == "groups":                     # a group-strided [G, R, C] view: two channel slices of one wider token matrix
        buf = torch.full((224, 8 + 2 * c), 7.0, device=dev)
        view = buf[:, 8:].unflatten(1, (2, c)).permute(1, 0, 2)
        view.copy_(x.reshape(2, 224, c))
        out = torch.full((rows, c), 9.0, device=dev)
        hip.layernorm(view, out, gamma, beta)
    else:                                      # fp32 rows and the plane sink together
        out = torch.full((rows, c), 9.0, device=dev)
        planes = hip_ops.Planes.alloc(rows, c, dev)
        hip.layernorm(x, out, gamma, beta, planes=planes)
    torch.cuda.synchronize()
    live = src_of_row >= 0
    assert torch.equal(out[~live], beta[None].expand(int((~live).sum()), c)), "a zero-padded token is not beta bit for bit"
    got, src = out[live], src_of_row[live]
    ref, bnd = y[src], bound[src]
    worst = {}
    for k, fam in enumerate(R.LN_FAMILIES):
        sel = (src >= k * R.LN_ROWS) & (src < (k + 1) * R.LN_ROWS)
        assert int(sel.sum()) == R.LN_ROWS
        worst[fam] = round(R.worst_ratio(got[sel], ref[sel], bnd[sel]), 3)
    ratio = max(worst.values())
    report(record_property, f"LayerNorm C={c} {mode}", ratio, per_family=str(worst))
    assert ratio <= 1.0, f"LayerNorm C={c} {mode}: worst err/bound per family {worst}"
    if planes is not None:
        M.assert_split_of(planes, out, f"LayerNorm C={c} plane sink")


# ------------------------------------------------------------------ residual sigmoid sites
RES_B, RES_H, RES_W = 2, 97, 120          # 3 channels x 23280 pixels >= the 69640 arguments of the sweep


@pytest.fixture(scope="module")
def residual_case(dev):
    """r and it as planar [B,3,H,W] fp32, the float64 reference of it + tanh(r / 2) and its bound."""
    r, it = R.residual_inputs(RES_B * 3 * RES_H * RES_W)
    assert r.numel() >= R.sigmoid_sweep().numel() and torch.isinf(r).sum() >= 2
    r, it = (t.reshape(RES_B, 3, RES_H, RES_W).to(dev) for t in (r, it))
    v, bound = R.residual_sigmoid64(it, r)
    return r, it, v, bound


def check_residual(what, it_sum, it_clamped, case, record_property):
    _, _, v, bound = case
    assert not torch.isnan(it_sum).any() and not torch.isnan(it_clamped).any(), f"{what}: NaN in the output"
    ratio = R.worst_ratio(it_sum, v, bound)
    report(record_property, what, ratio)
    assert ratio <= 1.0, f"{what}: worst err/bound {ratio:.3f}"
    assert torch.equal(it_clamped, it_sum.clamp(0.0, 1.0)), f"{what}: it_clamped is not clamp(it_sum, 0, 1) bit for bit"


def test_final_residual_saturating_arguments(residual_case, hip, dev, record_property):
    r, it = residual_case[:2]
    buf = torch.full((RES_B, RES_H, RES_W, 8), 7.0, device=dev)           # r is channels 4..6 of an NHWC map
    buf[..., 4:7] = r.permute(0, 2, 3, 1)
    s, c = torch.full_like(it, 9.0), torch.full_like(it, 9.0)
    hip.final_residual(it, buf[..., 4:7], s, c)
    torch.cuda.synchronize()
    check_residual("final_residual", s, c, residual_case, record_property)


def test_refine_tail_saturating_arguments(residual_case, hip, dev, record_property):
    """r on the centre-tap planes of ``contrib`` (tap 4: planes 12..14), zeros on the other 24 planes, bias 0 and PReLU slope 1: the
    kernel's sum is r exactly.  Without slope / bias arrays PReLU must be the identity: the same bits."""
    r, it = residual_case[:2]
    px = RES_B * RES_H * RES_W
    contrib = torch.zeros(27, px, device=dev)
    contrib[12:15] = r.permute(1, 0, 2, 3).reshape(3, px)
    s, c = torch.full_like(it, 9.0), torch.full_like(it, 9.0)
    hip.refine_tail(contrib, torch.zeros(3, device=dev), torch.ones(3, device=dev), it, s, c)
    torch.cuda.synchronize()
    check_residual("refine_tail", s, c, residual_case, record_property)
    s2, c2 = torch.full_like(it, 9.0), torch.full_like(it, 9.0)
    hip.refine_tail(contrib, None, None, it, s2, c2)
    torch.cuda.synchronize()
    assert torch.equal(s2, s) and torch.equal(c2, c), "refine_tail without slope / bias arrays differs from slope 1, bias 0"


@pytest.mark.parametrize("width", [40, 38], ids=["W40_tiled", "W38_direct"])
def test_warp_blend_masks_saturating_arguments(width, hip, dev, record_property):
    """Zero flows, per-channel constant images: mask1 = sigmoid(r), mask2 = 1 - mask1 of the kernel's own mask1 bit for bit,
    it = s c0 + (1 - s) c1 to 12 U.  W = 40 takes the LDS-tiled kernel, W = 38 (W % 4 != 0) the direct one."""
    b = 2
    h = (R.sigmoid_sweep().numel() + b * width - 1) // (b * width)
    r, _ = R.residual_inputs(b * h * width)
    r = r.reshape(b, h, width).to(dev)
    c0, c1 = torch.tensor([0.9, 0.25, 0.0], device=dev), torch.tensor([0.1, 0.75, 1.0], device=dev)
    im0 = c0[None, :, None, None].expand(b, 3, h, width).contiguous()
    im1 = c1[None, :, None, None].expand(b, 3, h, width).contiguous()
    assert hip._tiled_warp_ok(width, im0, im1) == (width == 40), "the launch would not take the kernel this case is for"
    buf = torch.zeros(b, h, width, 8, device=dev)                       # motion = channels 3..7: four zero flow components, r
    buf[..., 7] = r
    outs = [torch.full((b, 3, h, width), 9.0, device=dev) for _ in range(3)] + [torch.full((b, 2, h, width), 9.0, device=dev) for _ in range(2)] \
        + [torch.full((b, 1, h, width), 9.0, device=dev) for _ in range(2)]
    hip.warp_blend(im0, im1, buf[..., 3:8], *outs)
    torch.cuda.synchronize()
    i0w, i1w, it, f0, f1, m1, m2 = outs
    assert not any(torch.isnan(t).any() for t in outs), "NaN in an output"
    assert (f0 == 0).all() and (f1 == 0).all()
    assert torch.equal(m2, 1.0 - m1), "mask2 is not 1 - mask1 bit for bit"
    s, sbound = R.sigmoid_mask64(r)
    mratio = R.worst_ratio(m1[:, 0], s, sbound)
    # the two samples of the constant planes: 6 U c each (pointwise_ref.blend_const64)
    sratio = max(R.worst_ratio(i0w, im0.double(), 6 * R.U * im0.double()), R.worst_ratio(i1w, im1.double(), 6 * R.U * im1.double()))
    ref, bound = R.blend_const64(r, c0, c1)
    bratio = R.worst_ratio(it, ref, bound)
    report(record_property, f"warp_blend W={width}", max(mratio, sratio, bratio), mask1=round(mratio, 3), samples=round(sratio, 3), it=round(bratio, 3))
    assert mratio <= 1.0 and sratio <= 1.0 and bratio <= 1.0, f"warp_blend W={width}: worst err/bound mask1 {mratio:.3f}, samples {sratio:.3f}, it {bratio:.3f}"


# ------------------------------------------------------------------ motion head
@pytest.mark.parametrize("scale", [3.0, 50.0])
def test_motion_head_fp64(scale, hip, dev, record_property):
    """The geometry of test_gpu_ops.py::test_motion_head (a window row map with negative entries, a [2, B*h*w, 2] view of a wider
    matrix), fp32 view and plane sink together."""
    frames, h, w, ws, shift = 4, 6, 10, 4, 2
    geo = windows.build_window_geometry(frames, h, w, ws, shift)
    assert (geo.row_map < 0).any()
    rows, px = geo.row_map.numel(), (frames // 2) * h * w
    mo, w0, b0, w1, b1 = R.motion_head_inputs(rows, scale)
    y, bound = R.motion_head64(mo, w0, b0, w1, b1)
    keep = geo.row_map >= 0
    want = torch.full((2 * px, 2), 7.0, dtype=torch.float64)
    wbound = torch.zeros(2 * px, 2, dtype=torch.float64)
    want[geo.row_map[keep].long()] = y[keep]
    wbound[geo.row_map[keep].long()] = bound[keep]
    dg = torch.full((px, 24), 7.0, device=dev)
    view = dg[:, 4:8].unflatten(1, (2, 2)).permute(1, 0, 2)
    sink = hip_ops.Planes.alloc(px, 40, dev)
    hip.motion_head(*(t.to(dev) for t in (mo, geo.row_map, w0, b0, w1, b1)), view, planes=sink, planes_c0=4, planes_gc=2)
    torch.cuda.synchronize()
    got = view.reshape(2 * px, 2).cpu()
    ratio = R.worst_ratio(got, want, wbound)
    report(record_property, f"motion head scale {scale}", ratio)
    assert ratio <= 1.0, f"motion head scale {scale}: worst err/bound {ratio:.3f}"
    rest = dg.clone()
    rest[:, 4:8] = 7.0
    assert (rest == 7.0).all()
    assert int(keep.sum()) == 2 * px, "every output row is written in this geometry"
    M.assert_split_of(sink, dg[:, 4:8], "motion head plane sink", c0=4)
