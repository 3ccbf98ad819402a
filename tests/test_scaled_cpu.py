"""Half-resolution motion on the host: the twins of atm-vfi_amd/scaled.py against the torch composition that defines the mode, the x2 rule
against F.interpolate, frame_half's contract, the fp64 bound of the synthesis (tests/scaled_ref.py) with the kernel's fp32 emulation
inside it and every mutant outside, the ABI's host checks, and the loops on a CPU model."""
import ctypes
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scaled_ref as SR
import warp_ref as WR

scaled = importlib.import_module("atm-vfi_amd.scaled")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
F32 = np.float32
U = SR.U
SHAPES = ((1, 1, 1), (2, 5, 7), (1, 16, 24))           # (B, h, w) half sizes


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ------------------------------------------------------------------------------------------------------------------------ frame_half
def test_frame_half_twin_is_the_stated_expression_bit_for_bit():
    rng = np.random.default_rng(1)
    x = (rng.normal(0, 1, (2, 3, 10, 14)) * 10.0 ** rng.integers(-3, 4, (2, 3, 10, 14))).astype(F32)
    got = scaled.frame_half_numpy(x)
    assert got.dtype == F32 and got.shape == (2, 3, 5, 7)
    for y in range(5):
        for xx in range(7):
            a, b, c, d = x[..., 2 * y, 2 * xx], x[..., 2 * y, 2 * xx + 1], x[..., 2 * y + 1, 2 * xx], x[..., 2 * y + 1, 2 * xx + 1]
            want = (F32(a + b) + F32(c + d)) * F32(0.25)
            assert np.array_equal(got[..., y, xx], want.astype(F32))
    # the definition's F.avg_pool2d is the same average up to its summation order: three roundings of sums of four terms
    ref = F.avg_pool2d(_t64(x), 2).numpy()
    mag = F.avg_pool2d(_t64(np.abs(x)), 2).numpy()
    assert np.all(np.abs(got - ref) <= SR.g(3) * mag)
    for bad in ((3, 4), (4, 3), (0, 4)):
        with pytest.raises(ValueError):
            scaled.frame_half_numpy(np.zeros(bad, F32))


def test_frame_half_commutes_with_rot180():
    x = np.random.default_rng(2).normal(0, 3, (3, 12, 18)).astype(F32)
    rot = lambda a: a[..., ::-1, ::-1]
    assert np.array_equal(scaled.frame_half_numpy(np.ascontiguousarray(rot(x))), rot(scaled.frame_half_numpy(x)))


# ------------------------------------------------------------------------------------------------------------------------- the x2 rule
@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (5, 7), (16, 24)])
def test_up2_rule_is_f_interpolate(h, w):
    for mine, theirs in zip(scaled.up2_taps(h) + scaled.up2_taps(w), SR.taps(h) + SR.taps(w)):      # the package's table against the rule restated
        assert np.array_equal(mine, theirs)
    rng = np.random.default_rng([h, w])
    # integer-valued maps: every product and sum is exact in fp32, so any evaluation order gives the same bits -- max difference 0
    t = rng.integers(-2048, 2049, (2, 3, h, w)).astype(F32)
    ref = F.interpolate(torch.from_numpy(t), scale_factor=2, mode="bilinear", align_corners=False).numpy()
    assert np.array_equal(scaled.up2_numpy(t), ref)
    assert torch.equal(scaled.up2_torch(torch.from_numpy(t)), torch.from_numpy(ref))
    # real-valued maps: in float64 the rule and F.interpolate agree to float64's roundings; the fp32 twin stays within its four roundings
    t = rng.normal(0, 3, (2, 3, h, w)).astype(F32)
    ref = F.interpolate(_t64(t), scale_factor=2, mode="bilinear", align_corners=False).numpy()
    v, bound = SR.up2_64(t.astype(np.float64))
    assert np.all(np.abs(v - ref) <= 8 * 2.0 ** -53 * np.abs(ref) + 1e-300)
    assert np.all(np.abs(scaled.up2_numpy(t) - ref) <= bound)
    assert np.array_equal(scaled.up2_torch(torch.from_numpy(t)).numpy(), scaled.up2_numpy(t))
    # the weights are 0.25 / 0.75 and a constant map stays constant bit for bit (so a constant flow doubles exactly)
    c = np.full((1, 1, h, w), F32(1.1))
    assert np.all(scaled.up2_numpy(c) == F32(1.1))


# ------------------------------------------------------------------------------------------------- reference, bound, twin, emulation
def _double_composition(case):
    """The definition's last five lines by torch in float64 (F.interpolate, grid_sample): independent of scaled_ref's gathers."""
    h = case["half"]
    o = {"im_t_list": [_t64(h["it_sum"])], **{k: _t64(h[k]) for k in ("I_t_0", "I_t_1", "opt_flow_0", "opt_flow_1", "occ_mask1")}}
    return scaled.synth_torch(_t64(case["store0"]), _t64(case["store1"]), o)


@pytest.mark.parametrize("b,h,w", SHAPES)
@pytest.mark.parametrize("flow", ("gauss", "const_int", "blocks"))
def test_fp64_reference_is_the_torch_composition_in_double(b, h, w, flow):
    case = SR.make_case(b, h, w, flow=flow)
    ref = SR.synth64(case["half"], case["store0"], case["store1"])
    comp = _double_composition(case)
    for k in ("I_t", "opt_flow_0", "opt_flow_1", "occ_mask1"):
        # taps that sit exactly on a pixel (const_int, blocks) are decided by float64 roundings of grid_sample's own normalisation:
        # the bilinear function is continuous, so the two differ by float64 roundings times the slopes, far below the fp32 bound
        err = np.abs(comp[k].numpy() - ref[k][0])
        assert err.max() <= 1e-9, (k, err.max())


@pytest.mark.parametrize("b,h,w", SHAPES)
@pytest.mark.parametrize("flow", SR.FLOW_FAMILIES)
@pytest.mark.parametrize("mask", SR.MASK_FAMILIES)
def test_emulation_and_twin_stay_inside_the_bound(b, h, w, flow, mask):
    case = SR.make_case(b, h, w, flow=flow, mask=mask)
    ref = SR.synth64(case["half"], case["store0"], case["store1"])
    emu = SR.synth32(case["half"], case["store0"], case["store1"])
    ratios = SR.worst(emu, ref)
    assert max(ratios.values()) <= 1.0, ratios
    twin = scaled.synth_up2_numpy(SR.as_forward_dict(case["half"]), case["store0"], case["store1"])
    for k, v in emu.items():
        assert np.array_equal(twin[k], v, equal_nan=True), k          # the package's twin and the emulation built on warp_ref: the same bits
    if flow == "wild" and h * w >= 35:
        assert ref["dead"].any() and not ref["dead"].all()
    assert not np.isnan(emu["I_t"]).any()


def test_slot_lists_permute_and_repeat_store_frames():
    case = SR.make_case(3, 5, 7, stores=4)
    s0, s1 = [3, 0, 3], [1, 1, 2]
    ref = SR.synth64(case["half"], case["store0"], case["store1"], s0, s1)
    twin = scaled.synth_up2_numpy(SR.as_forward_dict(case["half"]), case["store0"], case["store1"], s0, s1)
    assert max(SR.worst(twin, ref).values()) <= 1.0
    plain = scaled.synth_up2_numpy(SR.as_forward_dict(case["half"]), case["store0"][s0], case["store1"][s1])
    assert np.array_equal(twin["I_t"], plain["I_t"])


@pytest.mark.parametrize("mutant", SR.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    worst = 0.0
    for flow in SR.FINITE_FAMILIES:
        for mask in ("rand", "binary"):
            case = SR.make_case(2, 5, 7, flow=flow, mask=mask)
            ref = SR.synth64(case["half"], case["store0"], case["store1"])
            worst = max(worst, max(SR.worst(SR.synth32(case["half"], case["store0"], case["store1"], mutant=mutant), ref).values()))
    assert worst > 1.0, f"{mutant}: worst error / bound = {worst}"


def test_u8_rule_and_ties():
    ties = SR.tie_pixels()
    assert len(ties) >= 200
    k = np.rint(ties.astype(np.float64) * 255.0 - 0.5).astype(np.int64)
    assert np.all((ties * F32(255.0)).astype(F32) == (k + 0.5).astype(F32))
    x = np.zeros((1, 3, 2, len(ties)), F32)
    x[:] = ties
    q = scaled.to_u8_numpy(x)
    assert np.array_equal(q[0, 0, :, 0], k + (k & 1))                       # half to even
    y = np.random.default_rng(3).uniform(-0.5, 1.5, (2, 3, 6, 8)).astype(F32)
    full, win = scaled.to_u8_numpy(y), scaled.to_u8_numpy(y, (1, 2, 4, 5), bgr=True)
    assert np.array_equal(win, full[:, 1:5, 2:7, ::-1])
    assert full.min() == 0 and full.max() == 255


# --------------------------------------------------------------------------------------------------------------------------------- ABI
P = 0x10000        # a fake, 16-byte aligned device address: every call below is refused before it would be touched


def _params(**kw):
    p = hip_ops.SynthUp2Params()
    h, w = 4, 6
    step = 1 << 20
    names = ("it_sum", "it0", "it1", "flow0", "flow1", "m1", "store0", "store1", "dst_f32")
    for i, n in enumerate(names):
        setattr(p, n, P + i * step)
    p.B, p.h, p.w, p.S0, p.S1 = 2, h, w, 2, 2
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_abi_version_symbols_and_refusals():
    lib = hip_ops.load_library()
    assert (lib.atmvfi_version() >> 8) & 255 >= 26
    for name in ("atmvfi_frame_half", "atmvfi_synth_up2", "atmvfi_synth_up2_workspace_floats"):
        assert hasattr(lib, name) and name in hip_ops.SIGNATURES
    err = lambda: lib.atmvfi_last_error()
    half = lib.atmvfi_frame_half
    for args, word in (((None, P + 4096, 1, 4, 4), b"null"), ((P, None, 1, 4, 4), b"null"), ((P, P + 4096, 1, 3, 4), b"even"),
                       ((P, P + 4096, 1, 4, 5), b"even"), ((P, P + 4096, 0, 4, 4), b"planes"), ((P, P + 4096, 1, 0, 4), b"even"),
                       ((P, P, 1, 4, 4), b"overlap"), ((P, P + 60, 1, 4, 4), b"overlap"), ((P + 8, P, 1, 4, 4), b"overlap")):
        assert half(*args, None) == -1 and word in err(), (args, err())
    assert lib.atmvfi_synth_up2_workspace_floats(2, 4, 6) == 0                    # this implementation needs no scratch
    assert lib.atmvfi_synth_up2_workspace_floats(17, 4, 6) < 0 and lib.atmvfi_synth_up2_workspace_floats(1, 0, 6) < 0
    synth = lambda p: lib.atmvfi_synth_up2(ctypes.cast(ctypes.pointer(p), ctypes.c_void_p), None)
    assert lib.atmvfi_synth_up2(None, None) == -1
    full = 2 * 3 * 8 * 12 * 4
    bad_slots = (ctypes.c_int32 * 2)(0, 2)
    cases = [(dict(it0=None), b"null input"), (dict(store1=None), b"null input"), (dict(B=17), b"16"), (dict(B=0), b"shape"), (dict(h=0), b"shape"),
             (dict(S0=0), b"store"), (dict(dst_f32=None), b"no output"), (dict(f0_out=P + (20 << 20)), b"pairs"),
             (dict(slots0=ctypes.cast(bad_slots, ctypes.c_void_p)), b"outside the stores"),
             (dict(S1=1), b"outside the stores"),
             (dict(dst_u8=P + (30 << 20), pad_top=1, pad_left=0, hh=8, ww=12), b"window"),
             (dict(dst_u8=P + (30 << 20), pad_top=0, pad_left=0, hh=0, ww=12), b"window"),
             (dict(path=3), b"path"), (dict(path=2, w=5), b"staged"), (dict(path=2, store0=P + (6 << 20) + 4), b"staged"),
             (dict(dst_f32=P + (6 << 20) + full - 4), b"overlaps store0"), (dict(dst_f32=P), b"overlaps it_sum"),
             (dict(m_out=P + (5 << 20)), b"m_out overlaps m1"),
             (dict(dst_u8=P + (8 << 20) + 16, pad_top=0, pad_left=0, hh=8, ww=12), b"dst_u8 overlaps dst_f32")]
    for kw, word in cases:
        assert synth(_params(**kw)) == -1 and word in err(), (kw, err())


def test_hipops_wrappers_refuse_on_the_host():
    ops = hip_ops.HipOps.__new__(hip_ops.HipOps)          # no device: every refusal below comes before the library is touched
    ops.recording = None
    with pytest.raises(ValueError):
        ops.frame_half(torch.zeros(3, 4, 4), torch.zeros(3, 2, 2))             # CPU tensors
    with pytest.raises(ValueError):
        ops.synth_up2({}, None, want=("I_t",))
    with pytest.raises(ValueError):
        ops.synth_up2({}, None, path="fast")


# ------------------------------------------------------------------------------------------------------- the loops on a CPU model
host_io = importlib.import_module("atm-vfi_amd.host_io")
mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
yuv = importlib.import_module("atm-vfi_amd.yuv")


class Toy(torch.nn.Module):
    """A CPU model without the HIP backend that returns ``forward``'s whole dict: smooth flows of a pixel or two, a mask, the two frames as
    the warped frames and a residual -- and records the frame sizes it is asked for."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.shapes = []

    def forward(self, a, b):
        self.shapes.append(tuple(a.shape))
        g = a.mean(1, keepdim=True) - b.mean(1, keepdim=True)
        m = (0.25 + 0.5 * a.mean(1, keepdim=True)).clamp(0, 1)
        f0 = torch.cat([0.75 + g, -0.5 * g], 1)
        f1 = torch.cat([-0.75 - g, 0.5 + g], 1)
        s = m * a + (1 - m) * b + 0.1 * (a - b)
        return {"I_t": s.clamp(0, 1), "im_t_list": [s], "I_t_0": a, "I_t_1": b, "opt_flow_0": f0, "opt_flow_1": f1, "occ_mask1": m, "occ_mask2": 1 - m}


LH, LW, LDIV = 24, 40, 8               # frames; the canvas of divisor 16 is 32 x 48, the network's 16 x 24


def _video(n, seed=3):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (LH + 8, LW + 8, 3)).astype(np.uint8)
    return [np.ascontiguousarray(base[k:k + LH, 2 * k:2 * k + LW]) for k in range(n)]


def _canvas(frame, bgr):
    t = torch.tensor(np.ascontiguousarray((frame[:, :, ::-1] if bgr else frame).transpose(2, 0, 1))) / 255.
    return host_io.InputPadder((1, 3, LH, LW), divisor=2 * LDIV).pad(t.unsqueeze(0), t.unsqueeze(0))[0]


def _twin(model, a, b):
    return scaled.forward_scaled_host(model.forward, a, b)["I_t"]


def _u8(canvas, bgr):
    left, _, top, _ = host_io.InputPadder((1, 3, LH, LW), divisor=2 * LDIV)._pad
    return scaled.to_u8_numpy(canvas, (top, left, LH, LW), bgr=bgr)[0]


@pytest.mark.parametrize("bgr", (False, True))
def test_nx_4x_on_a_cpu_model_is_the_chain_of_the_twin(bgr):
    video, model = _video(3), Toy()
    got = list(mf.interpolate_video_nx(iter(video), model, factor=4, divisor=LDIV, isBGR=bgr, motion_scale=2))
    assert len(got) == 9 and all(got[4 * k] is video[k] for k in range(3))
    assert model.shapes and all(s[-2:] == (16, 24) for s in model.shapes)           # the forwards ran at half size
    hand = Toy()
    for seg in range(2):
        c0, c4 = _canvas(video[seg], bgr), _canvas(video[seg + 1], bgr)
        p2 = _twin(hand, c0, c4)
        p1, p3 = _twin(hand, c0, p2), _twin(hand, p2, c4)                             # the unrounded full-size prediction feeds level 2
        for k, p in ((1, p1), (2, p2), (3, p3)):
            assert np.array_equal(got[4 * seg + k], _u8(p, bgr)), (seg, k)
    assert mf.inference_nx(video[0], video[1], Toy(), factor=4, isBGR=bgr, divisor=LDIV, motion_scale=2)[1].tobytes() == got[2].tobytes()
    one = host_io.inference_2frame(video[0], video[1], Toy(), isBGR=bgr, divisor=LDIV, motion_scale=2)
    assert np.array_equal(one, got[2])


def test_tta_and_the_retimed_loop_on_a_cpu_model():
    video = _video(3)
    got = list(mf.interpolate_video_nx(iter(video), Toy(), factor=2, divisor=LDIV, isBGR=False, tta=True, motion_scale=2))
    hand = Toy()
    c0, c1 = _canvas(video[0], False), _canvas(video[1], False)
    rot = lambda t: t.flip(2).flip(3).contiguous()
    avg = (_twin(hand, c0, c1) + rot(_twin(hand, rot(c0), rot(c1)))) / 2              # rotated at full size
    left, _, top, _ = host_io.InputPadder((1, 3, LH, LW), divisor=2 * LDIV)._pad
    want = np.round(avg[0, :, top:top + LH, left:left + LW].numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
    assert np.array_equal(got[1], want)
    plain = list(mf.interpolate_video_nx(iter(video), Toy(), factor=2, divisor=LDIV, isBGR=False, motion_scale=2))
    model = Toy()
    re = list(rt.interpolate_video_retimed(iter(video), model, 30, 60, levels=1, divisor=LDIV, isBGR=False, motion_scale=2))
    assert len(re) == len(plain) == 5 and all(np.array_equal(a, b) for a, b in zip(re, plain))
    assert all(s[-2:] == (16, 24) for s in model.shapes)


def test_motion_scale_1_is_the_earlier_loop_and_calls_nothing_new(monkeypatch):
    video = _video(3)
    before = list(mf.interpolate_video_nx(iter(video), Toy(), factor=4, divisor=LDIV))
    re_before = list(rt.interpolate_video_retimed(iter(video), Toy(), 24, 60, levels=2, divisor=LDIV))
    one_before = host_io.inference_2frame(video[0], video[1], Toy(), divisor=LDIV)

    def boom(*a, **k):
        raise AssertionError("motion_scale=1 reached the half-resolution code")
    for name in ("forward_scaled_host", "frame_half_numpy", "synth_up2_numpy", "up2_numpy"):
        monkeypatch.setattr(scaled, name, boom)
    model = Toy()
    after = list(mf.interpolate_video_nx(iter(video), model, factor=4, divisor=LDIV, motion_scale=1))
    assert len(after) == len(before) == 9 and all(np.array_equal(a, b) for a, b in zip(after, before))
    assert all(s[-2:] == (24, 40) for s in model.shapes)                               # divisor 8: the frames as they are
    re_after = list(rt.interpolate_video_retimed(iter(video), Toy(), 24, 60, levels=2, divisor=LDIV, motion_scale=1))
    assert len(re_after) == len(re_before) and all(np.array_equal(a, b) for a, b in zip(re_after, re_before))
    assert np.array_equal(host_io.inference_2frame(video[0], video[1], Toy(), divisor=LDIV, motion_scale=1), one_before)
    # ... and the frames are those of the commit before the mode existed: sha256 of the frames' bytes, recorded by running that commit's
    # loops on this video and this model (uint8 frames of elementwise fp32 arithmetic: the same on every machine)
    import hashlib
    sha = lambda frames: hashlib.sha256(b"".join(np.ascontiguousarray(f).tobytes() for f in frames)).hexdigest()
    assert sha(after) == "20eeaa8eb05e1e3579fe24f7eff8390a73c1f04857903e5954b45c604608d0a4"
    assert sha(re_after) == "582b978d5ad7beae42b95601440ce6bd5caf506efb90ecbdb1b469db245c07da"
    assert sha([one_before]) == "007b98b2f69f52acdb1d165f3590d38950f226c661f35a3c4cbc0142dcae636f"


def test_loop_refusals(tmp_path):
    video = _video(2)
    for bad in (0, 3, 4, 2.5, True, "2"):
        with pytest.raises(ValueError, match="motion_scale"):
            list(mf.interpolate_video_nx(iter(video), Toy(), motion_scale=bad))
        with pytest.raises(ValueError, match="motion_scale"):
            rt.interpolate_video_retimed(iter(video), Toy(), 24, 60, motion_scale=bad)
        with pytest.raises(ValueError, match="motion_scale"):
            host_io.inference_2frame(video[0], video[1], Toy(), motion_scale=bad)
    with pytest.raises(ValueError, match="shutter"):
        rt.interpolate_video_retimed(iter(video), Toy(), 24, 60, shutter=180, motion_scale=2)
    with pytest.raises(ValueError, match="shutter"):
        yuv.interpolate_y4m(str(tmp_path / "none.y4m"), str(tmp_path / "out.y4m"), Toy(), fps_out=60, shutter=180, motion_scale=2)
    with pytest.raises(ValueError, match="motion_scale"):
        yuv.interpolate_raw(str(tmp_path / "none.yuv"), str(tmp_path / "out.yuv"), Toy(), yuv.Format(16, 16), 24, motion_scale=3)
    with pytest.raises(ValueError, match="even"):                                     # no divisor: odd sides cannot be halved
        list(mf.interpolate_video_nx(iter([f[:23] for f in video]), Toy(), divisor=None, motion_scale=2))


def test_y4m_helper_hands_motion_scale_on(tmp_path):
    fmt = yuv.Format(32, 48)
    rng = np.random.default_rng(5)
    frames = [yuv.encode_numpy(rng.integers(0, 256, (32, 48, 3)).astype(np.uint8), fmt) for _ in range(2)]
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    with yuv.Y4MWriter(src, fmt, 24) as wr:
        for f in frames:
            wr.write(f)
    model = Toy()
    info = yuv.interpolate_y4m(src, dst, model, factor=2, divisor=8, motion_scale=2)
    assert info["frames_out"] == 3 and model.shapes and all(s[-2:] == (16, 24) for s in model.shapes)
    want = list(mf.interpolate_video_nx(iter(frames), Toy(), factor=2, divisor=8, pixfmt=fmt, motion_scale=2))
    got = list(yuv.Y4MReader(dst))
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name,variant,h,w,glob,seed", [("lite_128x192", "lite", 128, 192, False, 7), ("base_128x128_global", "base", 128, 128, True, 11)])
def test_golden_is_the_twin_on_the_oracle(name, variant, h, w, glob, seed):
    """tests/golden/scaled_ref.npz (the reference's forward through the torch composition) against the numpy twins around the CPU oracle's
    forward, within the oracle's own tolerance against the reference (tests/test_oracle_golden.py: ORACLE_TOL = 2e-5), on every output."""
    import os
    import pairs
    from oracle import atmvfi_oracle as O
    pkg = importlib.import_module("atm-vfi_amd")
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaled_ref.npz"))
    sd = pkg.synthetic_state_dict(variant, seed=1)
    im0, im1 = pairs.smooth_pair(1, h, w, seed=seed)
    assert np.allclose(gold[f"{name}.in_sums"], [im0.double().sum().item(), im1.double().sum().item()])
    out = scaled.forward_scaled_host(lambda a, b: O.forward(sd, a, b, global_motion=glob), im0, im1, want=scaled.WANT_KEYS)
    err = {"I_t": np.abs(out["I_t"].numpy() - gold[f"{name}.I_t"]).max()}
    for k, short in (("opt_flow_0", "f0"), ("opt_flow_1", "f1"), ("occ_mask1", "m")):
        err[short] = np.abs(out[k].numpy()[..., ::2, ::2] - gold[f"{name}.{short}"]).max()
    print("twin on the oracle against the golden:", {k: float(v) for k, v in err.items()})
    assert max(err.values()) <= 2e-5, err
