"""GPU: the synthetic shutter on the device (csrc/shutter.hip atmvfi_shutter_accumulate / atmvfi_shutter_resolve; atm-vfi_amd/shutter.py):
the kernels against the loop model of tests/cpu_shutter.py bit for bit, and ``interpolate_video_retimed(shutter=)`` on the HIP path
against ``blend_numpy`` of the frames the N-x run yields at every output's samples -- pooled and plain, TTA, dropped duplicates, a
scene cut, I420 frames."""
import importlib

import numpy as np
import pytest
import torch

import cpu_framediff as D
import cpu_scene as C
import cpu_shutter as S
import pairs

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scene = importlib.import_module("atm-vfi_amd.scene")
rt = importlib.import_module("atm-vfi_amd.retime")
sh = importlib.import_module("atm-vfi_amd.shutter")
yuv = importlib.import_module("atm-vfi_amd.yuv")

LIGHTS = ("code", "linear")
POISON = -0x12345678


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    torch.set_grad_enabled(False)
    out = {}
    for v, cls in (("lite", pkg.NetworkLite), ("base", pkg.NetworkBase)):
        net = cls()
        net.load_state_dict(pkg.synthetic_state_dict(v, seed=1), strict=True)
        out[v] = net.to(dev).eval()
    return out


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


# ------------------------------------------------------------------------------------------------ the kernels
CASES = [            # h, w, Hp, Wp, pad_top, pad_left, fp32 offset in floats, uint8 offset in bytes
    (1, 1, 1, 1, 0, 0, 0, 0),
    (3, 5, 3, 5, 0, 0, 0, 0),                    # general path
    (8, 16, 8, 16, 0, 0, 0, 0),                  # aligned path
    (40, 1100, 40, 1100, 0, 0, 0, 0),            # 43 workgroups, rows that end inside a wave
    (24, 40, 32, 64, 5, 4, 0, 0),                # inside a padded canvas, aligned
    (24, 40, 32, 64, 5, 3, 0, 0),                # pad_left 3: general path
    (8, 16, 8, 16, 0, 0, 1, 0),                  # the fp32 source offset by 4 bytes
    (8, 16, 8, 16, 0, 0, 0, 1),                  # the uint8 source offset by 1 byte
]


def canvas_of(h, w, Hp, Wp, seed):
    """fp32 [3,Hp,Wp]: values a little outside [0, 1], every tenth an exact .5 tie of x * 255, some far outside"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.05, 1.05, (3, Hp, Wp)).astype(np.float32)
    flat = c.reshape(-1)
    ties = (rng.integers(0, 255, flat[::10].shape).astype(np.float32) + np.float32(0.5)) / np.float32(255)
    keep = (ties * np.float32(255)) % 1 == np.float32(0.5)         # the ones that survive the fp32 product as ties
    flat[::10] = np.where(keep, ties, flat[::10])
    flat[3::17] = rng.choice(np.array([-3.0, 7.5, 1.0, 0.0, 1e30, -1e30], np.float32), flat[3::17].shape)
    return c


def offset_copy(arr, dev, elems):
    """the same values behind a pointer offset by ``elems`` elements from a fresh allocation"""
    t = torch.from_numpy(arr)
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=dev)
    s = buf[elems:].view(t.shape)
    s.copy_(t)
    return s


@pytest.fixture(scope="module")
def models():
    """Per case and light: the inputs and the loop model's accumulators and pixels.  Computed once."""
    out = {}
    for case in CASES:
        h, w, Hp, Wp, pt, pl = case[:6]
        rng = np.random.default_rng(h * w + pl)
        canvas = canvas_of(h, w, Hp, Wp, seed=h + w + pl)
        frame = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        q = S.pixels_of_canvas(canvas, pt, pl, h, w)
        for light in LIGHTS:
            lut = S.derived_table(light)
            a1 = S.accumulate_model(None, q, 3, lut, True)                            # fp32 source, weight 3, first
            a2 = S.accumulate_model(a1, frame[:, :, ::-1], 1, lut, False)             # uint8 source read as B, G, R, weight 1
            out[case, light] = (canvas, frame, q, a1, a2, S.resolve_model(a2, h, w, 4, lut))
    return out


@pytest.mark.parametrize("light", LIGHTS)
@pytest.mark.parametrize("case", CASES, ids=lambda v: "x".join(str(k) for k in v))
def test_the_kernels_are_the_loop_model(ops, dev, models, case, light):
    h, w, Hp, Wp, pt, pl, f_off, b_off = case
    canvas, frame, q, a1, a2, pixels = models[case, light]
    src, u8 = offset_copy(canvas, dev, f_off), offset_copy(frame, dev, b_off)
    assert src.data_ptr() % 16 == 4 * f_off and u8.data_ptr() % 4 == b_off
    acc = torch.full((3, h, w), POISON, dtype=torch.int32, device=dev)              # poisoned: `first` writes without reading
    ops.shutter_accumulate(acc, src=src, weight=3, light=light, first=True, pad_top=pt, pad_left=pl)
    got = acc.cpu().numpy().reshape(-1)
    assert np.array_equal(got, np.array(a1, np.int64)), np.flatnonzero(got != np.array(a1))[:8]
    ops.shutter_accumulate(acc, src_u8=u8, weight=1, light=light, bgr=True)
    got = acc.cpu().numpy().reshape(-1)
    assert np.array_equal(got, np.array(a2, np.int64)), np.flatnonzero(got != np.array(a2))[:8]
    for bgr in (False, True):
        dst = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device=dev)
        ops.shutter_resolve(acc, 4, dst, light=light, bgr=bgr)
        want = pixels[:, :, ::-1] if bgr else pixels
        assert np.array_equal(dst.cpu().numpy(), want), np.argwhere(dst.cpu().numpy() != want)[:4]
    # the host twin saw the same
    assert np.array_equal(pixels, sh.blend_numpy([q, q, q, np.ascontiguousarray(frame[:, :, ::-1])], [1, 1, 1, 1], light))
    # a single accumulated frame resolves to itself, in either channel order, with any weight
    for weight in (1, 3):
        ops.shutter_accumulate(acc, src_u8=u8, weight=weight, light=light, first=True, bgr=True)
        back = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
        ops.shutter_resolve(acc, weight, back, light=light, bgr=True)
        assert np.array_equal(back.cpu().numpy(), frame)
    ops.shutter_accumulate(acc, src=src, weight=2, light=light, first=True, pad_top=pt, pad_left=pl)
    back = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    ops.shutter_resolve(acc, 2, back, light=light)
    assert np.array_equal(back.cpu().numpy(), q)


def test_fp32_ties_and_values_outside_the_unit_interval(ops, dev):
    """x * 255 at exact .5 ties rounds half to even; values outside [0, 1] clamp: frame_f32_to_u8's pixel"""
    vals = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 126.5 / 255, 127.5 / 255, 253.5 / 255, 254.5 / 255, -0.2, -1e-9, 1.0, 1.002, 1.5, 300.0, -7.0, 0.0, 0.999],
                    np.float32)
    ties = (vals[:7] * np.float32(255)) % 1 == np.float32(0.5)
    assert ties.sum() >= 4                                            # (not every k + .5 survives the division by 255 as a tie)
    canvas = np.stack([np.tile(vals, (8, 1))] * 3).astype(np.float32)           # [3,8,16]
    want = S.pixels_of_canvas(canvas, 0, 0, 8, 16)
    assert want[0, 7, 0] == 0 and want[0, 9, 0] == 255 and want[0, 12, 0] == 255 and want[0, 13, 0] == 0
    src = torch.from_numpy(canvas).to(dev)
    ref = torch.empty(8, 16, 3, dtype=torch.uint8, device=dev)
    ops.frame_f32_to_u8(src, ref, 0, 0, False)
    assert np.array_equal(ref.cpu().numpy(), want)
    acc = torch.empty(3, 8, 16, dtype=torch.int32, device=dev)
    out = torch.empty(8, 16, 3, dtype=torch.uint8, device=dev)
    for light in LIGHTS:
        ops.shutter_accumulate(acc, src=src, light=light, first=True)
        ops.shutter_resolve(acc, 1, out, light=light)
        assert np.array_equal(out.cpu().numpy(), want), light


@pytest.mark.parametrize("light", LIGHTS)
def test_twenty_accumulations_and_the_largest_weight(ops, dev, light):
    rng = np.random.default_rng(20)
    h, w = 12, 20
    frames = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(20)]
    weights = [int(v) for v in rng.integers(1, 4, 20)]
    acc = torch.full((3, h, w), POISON, dtype=torch.int32, device=dev)
    for k, (f, wt) in enumerate(zip(frames, weights)):
        ops.shutter_accumulate(acc, src_u8=torch.from_numpy(f).to(dev), weight=wt, light=light, first=k == 0)
    out = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    ops.shutter_resolve(acc, sum(weights), out, light=light)
    assert np.array_equal(out.cpu().numpy(), S.blend_model(frames, weights, light))
    # Wt = 32767 with all-ones sources: 65535 Wt stays inside int32
    white = torch.full((h, w, 3), 255, dtype=torch.uint8, device=dev)
    ones = torch.ones(3, h, w, dtype=torch.float32, device=dev)
    for k in range(7):                                                # 7 x 4681 = 32767
        ops.shutter_accumulate(acc, src=ones if k % 2 else None, src_u8=None if k % 2 else white, weight=4681, light=light, first=k == 0)
    assert (acc.cpu().numpy() == 65535 * 32767).all()
    ops.shutter_resolve(acc, 32767, out, light=light)
    assert (out.cpu().numpy() == 255).all()
    # every total weight's rounding division, on the values around each multiple: (acc + (Wt >> 1)) // Wt
    for total in (1, 2, 3, 7, 255, 4681, 32766, 32767):
        v = rng.integers(0, 65536, 3 * h * w)
        v[:4] = [0, 1, 65534, 65535]
        a = v * total + rng.integers(-(total // 2) - 1, total // 2 + 2, v.shape)
        a = np.clip(a, 0, 65535 * total).astype(np.int64)
        acc.copy_(torch.from_numpy(a.astype(np.int32).reshape(3, h, w)))
        ops.shutter_resolve(acc, total, out, light=light)
        want = S.resolve_model(a.tolist(), h, w, total, S.derived_table(light))
        assert np.array_equal(out.cpu().numpy(), want), total


@pytest.mark.parametrize("light", LIGHTS)
def test_the_inverse_of_every_value(ops, dev, light):
    """Every v in 0..65535 (Wt = 1, and as the rounded mean at Wt = 3) through the kernel's inverse: the count of thresholds.  The kernel
    does not bisect the 255 thresholds in eight steps: it reads the count for v & ~255 from a 256-entry bucket table and searches the at
    most 15 thresholds of that bucket in four steps (a static_assert in csrc/shutter.hip holds the tables to that bound).  This is the
    test that the substitution gives the definition's value everywhere."""
    inv = np.array(S.inverse_table(S.derived_table(light)), np.uint8)
    h, w = 128, 176                                                   # 3 h w = 67584 >= 65536 values
    v = (np.arange(3 * h * w) % 65536).astype(np.int32)
    out = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    for total in (1, 3):
        acc = torch.from_numpy((v * total + (total // 2)).reshape(3, h, w)).to(dev)
        ops.shutter_resolve(acc, total, out, light=light)
        got = out.cpu().numpy().transpose(2, 0, 1).reshape(-1)
        assert np.array_equal(got, inv[v]), np.flatnonzero(got != inv[v])[:8]


def test_a_frame_that_crosses_the_grid_stride(ops, dev):
    """2160 x 4096: 2 211 840 groups of four pixels on 8192 x 256 lanes; against the host twin (the loop model holds it on the CPU)"""
    h, w = 2160, 4096
    rng = np.random.default_rng(4)
    a, b = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2))
    acc = torch.empty(3, h, w, dtype=torch.int32, device=dev)
    ops.shutter_accumulate(acc, src_u8=torch.from_numpy(a).to(dev), weight=2, first=True)
    ops.shutter_accumulate(acc, src_u8=torch.from_numpy(b).to(dev), weight=1)
    out = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    ops.shutter_resolve(acc, 3, out)
    assert np.array_equal(out.cpu().numpy(), sh.blend_numpy([a, b], [2, 1], "linear"))


def test_wrapper_refusals_and_the_table(ops, dev):
    for light in LIGHTS:
        assert ops.shutter_table(light) == tuple(sh.SHUTTER_TABLES[light])
    acc = torch.zeros(3, 8, 16, dtype=torch.int32, device=dev)
    u8 = torch.zeros(8, 16, 3, dtype=torch.uint8, device=dev)
    f32 = torch.zeros(3, 8, 16, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        ops.shutter_accumulate(acc)
    with pytest.raises(ValueError):
        ops.shutter_accumulate(acc, src=f32, src_u8=u8)
    with pytest.raises(ValueError):
        ops.shutter_accumulate(acc.float(), src_u8=u8)
    with pytest.raises(ValueError):
        ops.shutter_accumulate(acc, src_u8=u8[:4].contiguous())
    with pytest.raises(ValueError):
        ops.shutter_accumulate(acc, src_u8=u8, light="gamma")
    with pytest.raises(ValueError):
        ops.shutter_table("gamma")
    with pytest.raises(RuntimeError, match="window outside the canvas"):
        ops.shutter_accumulate(acc, src=f32, pad_left=1)
    with pytest.raises(RuntimeError, match="weight 0"):
        ops.shutter_accumulate(acc, src_u8=u8, weight=0)
    with pytest.raises(RuntimeError, match="total_weight 40000"):
        ops.shutter_resolve(acc, 40000, u8)
    with pytest.raises(ValueError):
        ops.shutter_resolve(acc, 1, u8[:, :8].contiguous())
    # never part of a launch plan
    plan = ops.begin_plan([f32])
    try:
        ops.shutter_accumulate(acc, src=f32, first=True)
        ops.shutter_resolve(acc, 1, u8)
        assert plan.ops_list == []
    finally:
        ops.abort_plan()


# ------------------------------------------------------------------------------------------------ the loop
H, W = 64, 96
KW = dict(isBGR=True, divisor=32, max_batch=1)


def count_forwards(monkeypatch, net):
    """Counting wrappers around ``forward`` / ``forward_pooled`` of the model's class."""
    calls = {"forward": 0, "forward_pooled": 0}
    for name in calls:
        klass = next(k for k in type(net).__mro__ if name in k.__dict__)

        def wrapper(self, *a, _orig=klass.__dict__[name], _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(klass, name, wrapper)
    return calls


def lite(nets):
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    return net


def retimed(net, frames, fi, fo, **kw):
    return list(host_io.interpolate_video_retimed(iter(frames), net, fi, fo, **dict(KW, **kw)))


def check(got, outs, sample_frame, light="linear", encode=None, originals=None):
    """every multi-sample output is blend_numpy of the frames at its samples, a single-sample one is that frame"""
    assert len(got) == len(outs), (len(got), len(outs))
    for g, (m, pos, samples) in zip(got, outs):
        frames = [sample_frame(j, p) for j, p, _ in samples]
        if len(samples) == 1:
            want = frames[0]
        else:
            want = sh.blend_numpy(frames, [w for _, _, w in samples], light)
            want = encode(want) if encode else want
        assert g.dtype == want.dtype and g.shape == want.shape, m
        if not np.array_equal(g, want):
            at = np.argwhere(g != want)[0]
            raise AssertionError(f"output {m} {samples}: first difference at {tuple(at)}: {g[tuple(at)]} != {want[tuple(at)]} "
                                 f"({np.count_nonzero(g != want)} elements)")


@pytest.fixture(scope="module")
def video():
    return pairs.uint8_video(5, H, W, seed=5)


@pytest.fixture(scope="module")
def full8(nets, video):
    """the 8x run of the video, one pair per forward, no pool: frame 8 j + p is sample (j, p).  Computed once."""
    return retimed(lite(nets), video, 1, 8, levels=3, pool=False)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("light", LIGHTS)
def test_60_to_60_at_180_degrees(nets, video, full8, monkeypatch, pool, light):
    net = lite(nets)
    keep = net.max_workspaces
    calls = count_forwards(monkeypatch, net)
    report = {}
    got = retimed(net, video, 60, 60, levels=3, pool=pool, shutter=sh.Shutter(180, light), report=report)
    assert net.max_workspaces == keep
    outs = list(sh.shutter_slots(range(5), 60, 60, 3, 180))
    check(got, outs, lambda j, p: full8[8 * j + p], light)
    assert report == {"outputs": 5, "interpolated": 0, "forwards": 5 * 4, "blended": 5, "samples": 17}       # 5 per segment
    assert calls["forward_pooled" if pool else "forward"] == 20 and (pool or calls["forward_pooled"] == 0)


def test_a_small_angle_is_the_unblurred_conversion(nets, video):
    net = lite(nets)
    for fi, fo in ((24, 60), (60, 60)):
        plain = retimed(net, video, fi, fo, levels=3, pool=True)
        report = {}
        got = retimed(net, video, fi, fo, levels=3, pool=True, shutter=sh.Shutter(45), report=report)
        assert len(got) == len(plain) and all(np.array_equal(g, p) for g, p in zip(got, plain)) and report["blended"] == 0
        for g, (j, p) in zip(got, rt.retime_slots(range(5), fi, fo, 3)):
            assert p != 0 or g is video[j]                            # originals: the caller's own arrays


def test_60_to_24_and_24_to_60(nets, video, full8):
    net = lite(nets)
    full4 = retimed(net, video, 1, 4, levels=2, pool=False)
    report = {}
    got = retimed(net, video, 60, 24, levels=2, pool=True, shutter=sh.Shutter(180), report=report)
    outs = list(sh.shutter_slots(range(5), 60, 24, 2, 180))
    check(got, outs, lambda j, p: full4[4 * j + p])
    assert report["outputs"] == 2 and report["blended"] == 2 and report["samples"] == 8 and report["forwards"] == 5
    # upwards: singles (the unblurred frames) and pairs in one run; a crop
    got = retimed(net, video, 24, 60, levels=3, pool=True, shutter=sh.Shutter(180), crop=(32, 64))
    y0, x0, h, w = mf.centre_window(H, W, (32, 64))
    cropped = retimed(net, video, 1, 8, levels=3, pool=False, crop=(32, 64))
    check(got, list(sh.shutter_slots(range(5), 24, 60, 3, 180)), lambda j, p: cropped[8 * j + p])


def test_tta_once(nets, video):
    net = lite(nets)
    full = retimed(net, video[:3], 1, 4, levels=2, pool=True, tta=True)
    got = retimed(net, video[:3], 60, 60, levels=2, pool=True, tta=True, shutter=sh.Shutter(360))
    check(got, list(sh.shutter_slots(range(3), 60, 60, 2, 360)), lambda j, p: full[4 * j + p])


def test_dropped_duplicates(nets):
    net = lite(nets)
    A, B, Cc = (C.shot(1, H, W, seed=30 + k, tone=tone)[0] for k, tone in enumerate((60, 120, 180)))
    video = [A, D.primed(A, 1), B, Cc]
    dd = rt.Duplicates()
    got = retimed(net, video, 24, 24, levels=2, pool=True, dedup=dd, shutter=sh.Shutter(360))
    assert dd.dropped == [1]
    outs = list(sh.shutter_slots([0, 2, 3], 24, 24, 2, 360))
    assert outs[2][2] == [(0, 3, 2), (1, 0, 1), (1, 1, 1)]             # the widened segment's samples count double
    full = retimed(net, [A, B, Cc], 1, 4, levels=2, pool=False)
    check(got, outs, lambda j, p: full[4 * j + p])
    assert got[0] is A


@pytest.mark.parametrize("fi,fo,levels,angle,dups,kept", [
    (24, 60, 2, 180, (1, 0), [0, 2, 3]), (24, 60, 3, 180, (3, 0, 3), [0, 4, 5, 9]), (24, 60, 3, 45, (3, 0, 3), [0, 4, 5, 9]),
    (60, 60, 1, 180, (2, 0), [0, 3, 4]),
], ids=lambda v: str(v).replace(" ", "")[:12])
@pytest.mark.parametrize("pool", [False, True])
def test_a_widened_segment_shows_one_position_in_two_outputs(nets, pool, fi, fo, levels, angle, dups, kept):
    """Dropped frames stretch a segment's positions further apart than the outputs: two outputs have one nearest position, one through its
    window and the other as the position of an empty window, or both.  The prediction is accumulated into each."""
    net = lite(nets)
    n = 1 << levels
    pictures = [C.shot(1, H, W, seed=40 + k, tone=tone)[0] for k, tone in enumerate((40, 100, 160, 220))][:len(dups) + 1]
    video = []
    for k, f in enumerate(pictures):
        video += [f] + [D.primed(f, 10 * k + r + 1) for r in range(dups[k] if k < len(dups) else 0)]
    outs = list(sh.shutter_slots(kept, fi, fo, levels, angle))
    shown = [(j, p) for _, _, s in outs for j, p, _ in s if 0 < p < n]
    assert len(shown) > len(set(shown))                               # the case this test is about
    dd = rt.Duplicates()
    got = retimed(net, video, fi, fo, levels=levels, pool=pool, dedup=dd, shutter=sh.Shutter(angle))
    assert [i for i in range(len(video)) if i not in dd.dropped] == kept
    full = retimed(net, pictures, 1, n, levels=levels, pool=False)
    check(got, outs, lambda j, p: full[n * j + p])
    if angle == 45:                                                   # all single: the unblurred conversion, frame for frame
        plain = retimed(net, video, fi, fo, levels=levels, pool=pool, dedup=rt.Duplicates())
        assert len(plain) == len(got) and all(np.array_equal(g, p) for g, p in zip(got, plain))


def test_no_output_mixes_the_two_shots_of_a_cut(nets, monkeypatch):
    net = lite(nets)
    shots = C.shot(3, H, W, seed=11, tone=60) + C.shot(3, H, W, seed=12, tone=190)
    full = retimed(net, shots, 1, 4, levels=2, pool=True, scene=scene.SceneCuts())
    calls = count_forwards(monkeypatch, net)
    sc = scene.SceneCuts()
    got = retimed(net, shots, 24, 24, levels=2, pool=True, scene=sc, shutter=sh.Shutter(360))
    assert sc.cuts == [2] and sum(calls.values()) == 3 * 4                # the cut segment runs no forward
    outs = list(sh.shutter_slots(range(6), 24, 24, 2, 360, cuts=[2]))
    check(got, outs, lambda j, p: full[4 * j + p])
    first = lambda j, p: j < 2 or (j == 2 and p <= 2)
    assert all(len({first(j, p) for j, p, _ in s}) == 1 for _, _, s in outs)
    assert any(j == 2 and 0 < p < 4 for _, _, s in outs for j, p, _ in s)


def test_i420_frames(nets, video):
    net = lite(nets)
    fmt = yuv.Format(H, W)
    frames = [yuv.encode_numpy(f, fmt) for f in video[:4]]
    kw = dict(divisor=32, pool=False, max_batch=1)
    got = list(host_io.interpolate_video_retimed(iter(frames), net, 60, 60, levels=2, pixfmt=fmt, shutter=sh.Shutter(360), **kw))
    rgb = [yuv.decode_numpy(v, fmt) for v in frames]
    full = list(host_io.interpolate_video_retimed(iter(rgb), net, 1, 4, levels=2, isBGR=False, **kw))
    outs = list(sh.shutter_slots(range(4), 60, 60, 2, 360))
    assert all(len(s) > 1 for _, _, s in outs) and all(g.dtype == np.uint8 and g.shape == (fmt.frame_bytes,) for g in got)
    check(got, outs, lambda j, p: full[4 * j + p], encode=lambda f: yuv.encode_numpy(f, fmt))
    # a small angle: the caller's own bytes
    got = list(host_io.interpolate_video_retimed(iter(frames), net, 60, 60, levels=2, pixfmt=fmt, shutter=sh.Shutter(45), **kw))
    assert all(g is f for g, f in zip(got, frames))
    # upwards at a small angle: a produced single-sample output goes accumulate, resolve, rgb_to_yuv420(src_u8=) where the unblurred loop
    # encodes the fp32 prediction -- the same bytes
    report = {}
    got = list(host_io.interpolate_video_retimed(iter(frames), net, 24, 60, levels=3, pixfmt=fmt, shutter=sh.Shutter(45), report=report, **kw))
    plain = list(host_io.interpolate_video_retimed(iter(frames), net, 24, 60, levels=3, pixfmt=fmt, **kw))
    assert report["blended"] == 0 and report["interpolated"] == 6 and len(got) == len(plain) == 8
    assert all(g.dtype == p.dtype and np.array_equal(g, p) for g, p in zip(got, plain))
    assert all(g is frames[j] for g, (j, p) in zip(got, rt.retime_slots(range(4), 24, 60, 3)) if p == 0)
    with pytest.raises(ValueError, match="10-bit"):
        host_io.interpolate_video_retimed(iter(frames), net, 60, 60, pixfmt=yuv.Format(H, W, depth=10), keep_depth=True, shutter=180)


def test_network_base_once(nets):
    net = nets["base"]
    net.global_motion, net.ensemble_global_motion = True, False
    frames = pairs.uint8_video(3, 128, 192, seed=9)
    kw = dict(isBGR=True, divisor=64, pool=True, max_batch=1)
    full = list(host_io.interpolate_video_retimed(iter(frames), net, 1, 4, levels=2, **kw))
    got = list(host_io.interpolate_video_retimed(iter(frames), net, 60, 60, levels=2, shutter=sh.Shutter(180, "linear"), **kw))
    check(got, list(sh.shutter_slots(range(3), 60, 60, 2, 180)), lambda j, p: full[4 * j + p])
