"""CPU only: the fp64 references and derived bounds of tests/pointwise_ref.py have teeth.

* the references agree with the existing fp32 double (tests/cpu_ops.py) on the benign inputs of tests/test_gpu_ops.py;
* well-behaved fp32 arithmetic -- plain fp32 torch, and for GELU a numpy emulation of common.h's erf_2range built from the coefficients
  parsed out of the header -- stays inside every bound (worst ratio <= 1) on the hostile input families of
  tests/test_gpu_pointwise_fp64.py at their small shapes;
* each mutant (what a subtly wrong kernel would compute) exceeds the bound on at least one element of the same inputs;
* the GELU sweep contains what it claims.

"fp32 torch" for GELU is the kernel's own formula 0.5 x (1 + erf(x * 0.70710678f)) written out with torch.erf: torch's fused
``F.gelu`` takes a vectorised erf on the CPU that is ~1.1e-6 off around x = -3.5 (ratio 3.7 against ``gelu_bound``; its scalar path,
taken for a handful of elements, stays at 0.1), so it is no fp32 yardstick at this level -- one more reason the HIP kernels are
judged against float64 here and not against tests/cpu_ops.py.
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R
from cpu_ops import CpuOps

windows = importlib.import_module("atm-vfi_amd.windows")

RSQRT2_F32 = torch.tensor(0.70710678118654752440, dtype=torch.float32)


def gelu_f32(x: torch.Tensor) -> torch.Tensor:
    x = x.float()
    return 0.5 * x * (1.0 + torch.erf(x * RSQRT2_F32))


def rnd(gen, *shape, scale=1.0):
    return (torch.rand(*shape, generator=gen) * 2 - 1) * scale


@pytest.fixture(scope="module")
def sweep():
    x = R.gelu_sweep()
    return x, R.gelu64(x), R.gelu_bound(x)


@pytest.fixture(scope="module")
def coef():
    return R.parse_erf_2range()


# ------------------------------------------------------------------ agreement with the existing double, at its own tolerances
def test_references_agree_with_cpu_ops_on_benign_inputs():
    cpu = CpuOps()
    g = torch.Generator().manual_seed(5)
    frames, h, w, ws, shift, C = 2, 5, 6, 4, 2, 224                       # test_layernorm_gather_groups
    geo = windows.build_window_geometry(frames, h, w, ws, shift)
    src = rnd(g, frames * h * w, C, scale=3.0)
    gamma, beta = 1 + rnd(g, C, scale=0.2), rnd(g, C, scale=0.2)
    out = torch.empty(geo.row_map.numel(), C)
    cpu.layernorm(src, out, gamma, beta, geo.row_map)
    y, _ = R.layernorm64(src, gamma, beta)
    idx = geo.row_map.long()
    ref = torch.where((idx >= 0)[:, None], y[idx.clamp_min(0)], beta.double()[None])
    assert (out.double() - ref).abs().max().item() <= 2e-5
    for shape in ((2, 7, 9, 448), (2, 5, 6, 100)):                         # test_dwconv_gelu
        n, hh, ww, c = shape
        g = torch.Generator().manual_seed(6 + c)
        x, wt, b = rnd(g, n, hh, ww, c, scale=2.0), rnd(g, c, 1, 3, 3, scale=0.5), rnd(g, c, scale=0.3)
        oc = torch.empty(n, hh, ww, c)
        cpu.dwconv_gelu(x, oc, wt, b)
        assert (oc.double() - R.dwconv_gelu64(x, wt, b)[0]).abs().max().item() <= 2e-5
    g = torch.Generator().manual_seed(8)                                   # test_motion_head
    geo = windows.build_window_geometry(4, 6, 10, 4, 2)
    rows = geo.row_map.numel()
    mo = rnd(g, rows, 8, 2, scale=3.0)
    w0, b0, w1, b1 = rnd(g, 4, 8), rnd(g, 4), rnd(g, 1, 4), rnd(g, 1)
    dc = torch.full((2, 120, 2), 7.0)                                     # [frame of the pair, B * h * w, 2]
    cpu.motion_head(mo, geo.row_map, w0, b0, w1, b1, dc)
    y, _ = R.motion_head64(mo, w0, b0, w1, b1)
    keep = geo.row_map >= 0
    want = torch.full((240, 2), 7.0, dtype=torch.float64)
    want[geo.row_map[keep].long()] = y[keep]
    assert (dc.reshape(240, 2).double() - want).abs().max().item() <= 2e-5
    g = torch.Generator().manual_seed(13)                                  # test_pack_final_l1
    im0 = torch.rand(2, 3, 10, 14, generator=g)
    r = rnd(g, 2, 10, 14, 4, scale=3.0)
    sc, cc = torch.empty(2, 3, 10, 14), torch.empty(2, 3, 10, 14)
    cpu.final_residual(im0, r[..., :3], sc, cc)
    v, _ = R.residual_sigmoid64(im0, r[..., :3].permute(0, 3, 1, 2))
    assert (sc.double() - v).abs().max().item() <= 2e-6 and (cc.double() - v.clamp(0, 1)).abs().max().item() <= 2e-6


# ------------------------------------------------------------------ well-behaved fp32 stays inside
def test_gelu_fp32_torch_and_emulated_kernel_stay_inside(sweep, coef):
    x, ref, bound = sweep
    r_torch = R.worst_ratio(gelu_f32(x), ref, bound)
    r_emul = R.worst_ratio(torch.from_numpy(R.gelu_erf2_emulated(x, coef)), ref, bound)
    print(f"GELU worst ratio: fp32 torch {r_torch:.3f}, emulated erf_2range {r_emul:.3f}")
    assert r_torch <= 1.0 and r_emul <= 1.0, (r_torch, r_emul)


@pytest.mark.parametrize("scale", R.DWCONV_SCALES)
@pytest.mark.parametrize("shape", R.DWCONV_SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv_fp32_torch_stays_inside(shape, scale):
    x = R.dwconv_input(shape, scale)
    w, b = R.dwconv_params(shape[3])
    got = gelu_f32(F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1, groups=shape[3])).permute(0, 2, 3, 1)
    ref, bound = R.dwconv_gelu64(x, w, b)
    ratio = R.worst_ratio(got, ref, bound)
    print(f"dwconv {shape} scale {scale}: worst ratio {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("c", R.LN_WIDTHS)
def test_layernorm_fp32_torch_stays_inside_and_one_pass_does_not(c):
    x, gamma, beta = R.layernorm_inputs(c)
    ref, bound = R.layernorm64(x, gamma, beta)
    worst = {}
    for k, fam in enumerate(R.LN_FAMILIES):
        rows = slice(k * R.LN_ROWS, (k + 1) * R.LN_ROWS)
        two = R.worst_ratio(R.layernorm_two_pass_f32(x[rows], gamma, beta), ref[rows], bound[rows])
        lib = R.worst_ratio(F.layer_norm(x[rows], (c,), gamma, beta, R.LN_EPS), ref[rows], bound[rows])
        one = R.worst_ratio(R.layernorm_one_pass_f32(x[rows], gamma, beta), ref[rows], bound[rows])
        worst[fam] = (two, lib, one)
    print(f"LayerNorm C={c}: worst ratio (two-pass fp32, F.layer_norm, one-pass MUTANT) per family: {worst}")
    assert all(v[0] <= 1.0 and v[1] <= 1.0 for v in worst.values()), worst
    # the mutant cancels on the rows with an offset mean
    assert worst["mean1000"][2] > 1.0 and worst["mean100_sigma0.01"][2] > 1.0, worst


def test_residual_sigmoid_fp32_torch_stays_inside_and_fp16_does_not():
    r, it = R.residual_inputs(R.sigmoid_sweep().numel())
    assert torch.isinf(r).sum() == 2
    v, bound = R.residual_sigmoid64(it, r)
    got = it + (2.0 * torch.sigmoid(r) - 1.0)
    ratio = R.worst_ratio(got, v, bound)
    assert not torch.isnan(got).any()
    s, sbound = R.sigmoid_mask64(r)
    mratio = R.worst_ratio(torch.sigmoid(r), s, sbound)
    c0, c1 = torch.tensor([0.9, 0.25, 0.0]), torch.tensor([0.1, 0.75, 1.0])
    m1 = torch.sigmoid(r)
    blend, bbound = R.blend_const64(r.reshape(1, 1, -1), c0, c1)
    got_b = m1[None, None, None] * c0[None, :, None, None] + (1.0 - m1)[None, None, None] * c1[None, :, None, None]
    bratio = R.worst_ratio(got_b, blend, bbound)
    print(f"sigmoid sites, fp32 torch: residual {ratio:.3f}, mask {mratio:.3f}, blend {bratio:.3f}")
    assert ratio <= 1.0 and mratio <= 1.0 and bratio <= 1.0, (ratio, mratio, bratio)
    mutant = it + (2.0 * R.sigmoid_f16(r) - 1.0)
    assert R.worst_ratio(mutant, v, bound) > 1.0
    assert R.worst_ratio(R.sigmoid_f16(r), s, sbound) > 1.0


@pytest.mark.parametrize("scale", [3.0, 50.0])
def test_motion_head_fp32_torch_stays_inside(scale):
    mo, w0, b0, w1, b1 = R.motion_head_inputs(480, scale)
    ref, bound = R.motion_head64(mo, w0, b0, w1, b1)
    got = F.linear(gelu_f32(F.linear(mo.permute(0, 2, 1), w0, b0)), w1, b1)[..., 0]
    seq = torch.zeros(480, 2)                      # and the kernel's own order: sequential sums, products rounded separately
    for k in range(2):
        o = b1[0].expand(480).clone()
        for j in range(4):
            a = b0[j].expand(480).clone()
            for hh in range(8):
                a = a + w0[j, hh] * mo[:, hh, k]
            o = o + w1[0, j] * gelu_f32(a)
        seq[:, k] = o
    r1, r2 = R.worst_ratio(got, ref, bound), R.worst_ratio(seq, ref, bound)
    print(f"motion head scale {scale}: worst ratio F.linear {r1:.3f}, sequential {r2:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    assert R.worst_ratio(F.linear(F.gelu(F.linear(mo.permute(0, 2, 1), w0, b0), approximate="tanh"), w1, b1)[..., 0], ref, bound) > 1.0


# ------------------------------------------------------------------ mutants violate the GELU bound
def test_gelu_mutant_tanh_form(sweep):
    x, ref, bound = sweep
    assert R.worst_ratio(R.gelu_tanh64(x), ref, bound) > 1.0


def test_gelu_mutant_select_threshold_0p9(sweep, coef):
    x, ref, bound = sweep
    assert R.worst_ratio(torch.from_numpy(R.gelu_erf2_emulated(x, coef, select=0.9)), ref, bound) > 1.0


def test_gelu_mutant_last_range_b_coefficient_shifted(sweep, coef):
    x, ref, bound = sweep
    assert R.worst_ratio(torch.from_numpy(R.gelu_erf2_emulated(x, coef, b_last_shift=4e-6)), ref, bound) > 1.0


def test_gelu_mutant_clamp_at_3p5(sweep, coef):
    x, ref, bound = sweep
    assert R.worst_ratio(torch.from_numpy(R.gelu_erf2_emulated(x, coef, clamp=3.5)), ref, bound) > 1.0


def test_dwconv_mutant_tanh_gelu_violates_the_dwconv_bound():
    shape = R.DWCONV_SMALL_SHAPES[1]
    x = R.dwconv_input(shape, 2.0)
    w, b = R.dwconv_params(shape[3])
    ref, bound = R.dwconv_gelu64(x, w, b)
    got = F.gelu(F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1, groups=shape[3]), approximate="tanh").permute(0, 2, 3, 1)
    assert R.worst_ratio(got, ref, bound) > 1.0


# ------------------------------------------------------------------ the sweep is what it claims
def test_gelu_sweep_contents():
    x = R.gelu_sweep()
    assert x.dtype == torch.float32 and torch.isfinite(x).all() and x.abs().max().item() <= float(np.float32(1e30))
    v = x.numpy()
    bits = set(v.view(np.int32).tolist())
    for centre in (np.float32(R.SQRT2), np.float32(4.0 * R.SQRT2)):
        for sign in (1.0, -1.0):
            c = int(np.array([sign * centre], dtype=np.float32).view(np.int32)[0])
            assert all(c + d in bits for d in range(-4096, 4097)), (centre, sign)
    # the joints themselves: z = x * 0.70710678f crosses 1 and 4 inside the neighbourhoods
    z = (v.astype(np.float64) * np.float64(np.float32(0.70710678118654752440))).astype(np.float32)
    for joint in (1.0, 4.0):
        for sign in (1.0, -1.0):
            near = z[np.abs(z - sign * joint) < 1e-3] * sign
            assert (near < joint).any() and (near >= joint).any()
    for s in R.GELU_SPECIALS:
        for sign in (1.0, -1.0):
            want = np.array([sign * s], dtype=np.float32).view(np.int32)[0]
            assert int(want) in bits, (s, sign)
    assert np.float32(2.0 ** -149) > 0 and int(np.array([0.0], dtype=np.float32).view(np.int32)[0]) in bits
    grid = np.linspace(-8.0, 8.0, 2 ** 22).astype(np.float32)
    assert v.size >= 2 ** 22 + 4 * 8193 + 16 and np.array_equal(v[-grid.size:], grid)


def test_sigmoid_sweep_contents():
    r = R.sigmoid_sweep()
    assert r.numel() == 2 ** 16 + 2 ** 12 + 8 and not torch.isnan(r).any()
    assert r.min().item() == -float("inf") and r.max().item() == float("inf")
    fin = r[torch.isfinite(r)]
    assert fin.min().item() == -110.0 and fin.max().item() == 110.0
    for s in (88.8, 103.9):
        assert (r == torch.tensor(s, dtype=torch.float32)).any() and (r == torch.tensor(-s, dtype=torch.float32)).any()
    assert (torch.signbit(r) & (r == 0)).any() and (~torch.signbit(r) & (r == 0)).any()
    assert ((r.abs() <= 1e-3) & (r != 0)).sum() >= 2 ** 12 - 2
