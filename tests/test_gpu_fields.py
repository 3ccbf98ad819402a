"""GPU: interlaced input on the device (csrc/fields.hip atmvfi_field_bob / atmvfi_field_rows; atm-vfi_amd/fields.py deinterlace_video).
Both kernels bit for bit against the per-pixel loop models of tests/cpu_fields.py -- the 16-byte and the scalar instances, reached by
shape and by pointer offsets, strips of every length class, NaN-filled destinations and source padding, guard bytes around every row
-- the model's mutants, the HIP loop against frames made by hand from single launches, pool against plain forwards, the launch plans of
the steady state, the command-line tool, and parity of the forwards on bobbed canvases with the reference (tests/golden/fields_ref.npz,
tools/gen_fields_golden.py).

At 2176 x 4096 and 2160 x 4096 the expected bits come from the numpy twins (tests/test_fields_cpu.py pins those to the loop models on
every small shape): a Python loop over 27 M elements would take minutes.

Launch plans: ``Network._planned`` runs a key's first two calls with direct launches, records on the third (direct launches plus
one verifying replay of the new plan; ``plan_stats`` bin "recorded") and replays from the fourth.  A steady-state call is one with a
single stale slot; the test holds the third to "recorded" and every later one to "replayed", in both stages.

Measured on one MI355X (``test_forwards_on_bobbed_canvases_match_the_reference`` prints them): see README, "Interlaced input"."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cpu_fields as M

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")
fields = importlib.import_module("atm-vfi_amd.fields")
segments = importlib.import_module("atm-vfi_amd.segments")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
STRIP = hip_ops.FIELD_BOB_STRIP
TOL = 1e-3                                                            # the project's one-forward budget against the reference


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


def make_net(dev, kind):
    torch.set_grad_enabled(False)
    n = pkg.NetworkLite() if kind == "lite" else pkg.Network()
    n.load_state_dict(pkg.synthetic_state_dict(kind, seed=1), strict=True)
    n = n.to(dev).eval()
    n.global_motion, n.ensemble_global_motion = True, False
    return n


@pytest.fixture(scope="module")
def net(dev):
    return make_net(dev, "lite")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ field_bob
def woven_canvas(planes, hp, wp, top, left, h, w, seed):
    """a canvas whose padding is NaN and whose picture is hostile: (canvas, picture)"""
    S = M.hostile((planes, h, w), seed)
    C = np.full((planes, hp, wp), np.nan, F32)
    C[:, top:top + h, left:left + w] = S
    return C, S


def run_bob(ops, dev, C, top, left, h, w, which="both", offset=0):
    """``ops.field_bob`` with every tensor ``offset`` floats into its allocation and NaN-filled destinations -> (even, odd) or None"""
    n = C.size

    def at(fill):
        t = torch.full((n + offset,), float("nan"), dtype=torch.float32, device=dev)
        v = t[offset:].view(*C.shape)
        if fill is not None:
            v.copy_(torch.from_numpy(fill))
        return v
    src = at(C)
    even = at(None) if which in ("both", "even") else None
    odd = at(None) if which in ("both", "odd") else None
    ops.field_bob(src, even, odd, top, left, h, w)
    torch.cuda.synchronize()
    assert np.array_equal(bits(src.cpu().numpy()), bits(C))                                  # the source is untouched
    return tuple(None if t is None else t.cpu().numpy() for t in (even, odd))


def check_bob(ops, dev, planes, hp, wp, top, left, h, w, which="both", offset=0, expect=None):
    C, S = woven_canvas(planes, hp, wp, top, left, h, w, seed=h * 131 + w)
    got = run_bob(ops, dev, C, top, left, h, w, which, offset)
    for p, g in enumerate(got):
        if g is None:
            continue
        want = expect(S, p) if expect else M.canvas_model(S, p, top, left, hp, wp)
        assert not np.isnan(g).any(), "an element was not written, or the source's padding was read"
        assert np.array_equal(bits(g), bits(want)), (planes, hp, wp, top, left, h, w, which, offset, p)


@pytest.mark.parametrize("h,w", ((2, 1), (3, 5), (21, 37)))
def test_field_bob_scalar_instance_is_the_model(ops, dev, h, w):
    check_bob(ops, dev, 3, 32, 48, 3, 5, h, w)


@pytest.mark.parametrize("offset", (0, 1), ids=("16-byte", "scalar by a pointer offset"))
def test_field_bob_both_instances_give_the_model(ops, dev, offset):
    check_bob(ops, dev, 3, 24, 40, 3, 4, 16, 32, offset=offset)
    for which in ("even", "odd"):
        check_bob(ops, dev, 2, 24, 40, 3, 4, 16, 32, which=which, offset=offset)


@pytest.mark.parametrize("h", (STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1))
def test_field_bob_strip_boundaries(ops, dev, h):
    for offset in (0, 1):
        check_bob(ops, dev, 1, h + 5, 16, 2, 4, h, 8, offset=offset)
    check_bob(ops, dev, 1, h + 5, 13, 2, 3, h, 7)                      # a canvas width that is no multiple of a lane's four columns


def test_field_bob_at_4k(ops, dev):
    twin = lambda S, p: fields.bob_numpy(S, p, canvas=(8, 0, 2176, 4096))
    check_bob(ops, dev, 3, 2176, 4096, 8, 0, 2160, 4096, expect=twin)


def test_field_bob_wrapper_refusals(ops, dev):
    a = torch.zeros(3, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match="no two fields"):
        ops.field_bob(a, torch.zeros_like(a), None, 0, 0, 1, 8)
    with pytest.raises(RuntimeError, match="overlaps the source"):
        ops.field_bob(a, a, None)
    with pytest.raises(ValueError, match="one shape"):
        ops.field_bob(a, torch.zeros(3, 8, 12, device=dev))


# ------------------------------------------------------------------------------------------------ field_rows
POISON = 0xA5


def check_rows(ops, dev, dst_bytes, src_bytes, geometry, seed=0, base=0, expect=None):
    """both parities: a poisoned destination (every byte outside the moved rows is a guard) against the byte model"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, src_bytes, dtype=np.uint8)
    src[src == POISON] = 0
    d_src = torch.zeros(src_bytes + base + 16, dtype=torch.uint8, device=dev)[base:base + src_bytes].copy_(torch.from_numpy(src))
    for p in (0, 1):
        dst = np.full(dst_bytes, POISON, np.uint8)
        d_dst = torch.zeros(dst_bytes + base + 16, dtype=torch.uint8, device=dev)[base:base + dst_bytes].copy_(torch.from_numpy(dst))
        ops.field_rows(d_dst, d_src, geometry, p)
        torch.cuda.synchronize()
        want = (expect or M.rows_bytes_model)(dst, src, geometry, p)
        assert np.array_equal(d_dst.cpu().numpy(), want), (geometry, p, base)
        assert np.array_equal(d_src.cpu().numpy(), src)
        moved = sum(rb * ((rows - p + 1) // 2) for _, _, _, _, rb, rows in geometry)
        assert int((want != POISON).sum()) == moved                     # (the source holds no poison byte)


@pytest.mark.parametrize("W", (5, 32))
def test_field_rows_one_rgb_plane(ops, dev, W):
    check_rows(ops, dev, 7 * 3 * W, 7 * 3 * W, fields.plane_geometry(None, None, 7, W), seed=W)


@pytest.mark.parametrize("rb", (1, 15, 16, 17))
@pytest.mark.parametrize("base", (0, 3), ids=("aligned", "misaligned"))
def test_field_rows_row_bytes_and_guards(ops, dev, rb, base):
    check_rows(ops, dev, 32 + 6 * 48, 16 + 6 * 64, [(32, 16, 48, 64, rb, 6)], seed=rb, base=base)
    check_rows(ops, dev, 5 + 5 * 33, 7 + 5 * 19, [(5, 7, 33, 19, rb, 5)], seed=rb + 1, base=base)      # misaligned offsets and pitches


def test_field_rows_three_planes_with_unequal_pitches_and_offsets(ops, dev):
    g = [(0, 16, 64, 80, 48, 9), (1024, 2048, 32, 48, 32, 9), (1024 + 9 * 32 + 5, 2048 + 9 * 48 + 3, 40, 36, 24, 8)]
    check_rows(ops, dev, 2048, 4096, g, seed=11)
    check_rows(ops, dev, 2048, 4096, g[:2], seed=12)
    check_rows(ops, dev, 64, 64, [(0, 0, 16, 16, 16, 1)], seed=13)     # one row: the odd parity moves nothing


def test_field_rows_a_4k_422_10bit_frame(ops, dev):
    fmt = yuv.Format(2160, 4096, "bt709", False, "left", 10, "422")

    def sliced(dst, src, geometry, p):
        out = dst.copy()
        for doff, soff, dp, sp, rb, rows in geometry:
            assert dp == sp == rb                                       # tight planes: a row is a slice
            out[doff:doff + rows * dp].reshape(rows, dp)[p::2] = src[soff:soff + rows * sp].reshape(rows, sp)[p::2]
        return out
    check_rows(ops, dev, fmt.frame_bytes, fmt.frame_bytes, fields.plane_geometry(fmt, fmt), seed=5, expect=sliced)


def test_field_rows_wrapper_refusals(ops, dev):
    a, b = torch.zeros(256, dtype=torch.uint8, device=dev), torch.zeros(256, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="does not lie inside"):
        ops.field_rows(a, b, [(0, 0, 64, 64, 64, 5)], 0)
    with pytest.raises(RuntimeError, match="above a pitch"):
        ops.field_rows(a, b, [(0, 0, 16, 64, 32, 4)], 0)
    with pytest.raises(RuntimeError, match="overlap the rows read"):
        ops.field_rows(a, a, [(0, 0, 64, 64, 64, 4)], 0)
    with pytest.raises(RuntimeError, match="parity"):
        ops.field_rows(a, b, [(0, 0, 64, 64, 64, 4)], 2)


# ------------------------------------------------------------------------------------------------ the model's mutants
def test_every_mutant_of_the_model_fails_on_these_inputs():
    """The comparisons above have teeth: each deliberate mistake changes what the model gives on the inputs they use."""
    top, left, hp, wp = 3, 5, 32, 48
    for h, w in ((3, 5), (21, 37)):
        _, S = woven_canvas(3, hp, wp, top, left, h, w, seed=h * 131 + w)
        for p in (0, 1):
            good = M.canvas_model(S, p, top, left, hp, wp)
            for mutant in ("parity", "edge", "padding"):
                if mutant == "edge" and p == 0 and h % 2 == 1:
                    continue                                            # the first and the last row are both real: no edge row is filled
                assert not np.array_equal(bits(M.canvas_model(S, p, top, left, hp, wp, mutant=mutant)), bits(good)), (h, w, p, mutant)
    rng = np.random.default_rng(1)
    src, dst = rng.integers(0, 200, (7, 15), dtype=np.uint8), np.full((7, 15), POISON, np.uint8)
    assert not np.array_equal(M.rows_model(dst, src, 0, mutant="parity"), M.rows_model(dst, src, 0))
    pics = [M.hostile((3, 6, 8), seed=s) for s in range(3)]
    mean = lambda a, b: ((torch.from_numpy(a) + torch.from_numpy(b)) / 2).numpy()
    good = M.predictions_model(pics, "bff", "mc", mean, (1, 2, 8, 12))
    for mutant in ("order", "k2"):
        bad = M.predictions_model(pics, "bff", "mc", mean, (1, 2, 8, 12), mutant=mutant)
        assert any(not np.array_equal(bits(a[0]), bits(b[0])) for a, b in zip(good, bad)), mutant
    assert [p for _, p, _ in good] != [p for _, p, _ in M.predictions_model(pics, "bff", "mc", mean, (1, 2, 8, 12), mutant="order")]


# ------------------------------------------------------------------------------------------------ the loop
H, W = 64, 96


def stream_of(kind, rgb):
    """-> (pixfmt, frames, keywords of the loop)"""
    enc = lambda fmt: [yuv.encode_numpy(f.astype(F32) / F32(255) if fmt.depth == 10 else f, fmt) for f in rgb]
    if kind == "bgr":
        return None, [np.ascontiguousarray(f[:, :, ::-1]) for f in rgb], {}
    if kind == "i422":
        fmt = yuv.Format(H, W, "bt601", False, "left", 8, "422")
        return fmt, enc(fmt), {}
    layout, depth = {"uyvy": ("uyvy", 8), "v210": ("v210", 10)}[kind]
    k = yuv.Packed(yuv.Format(H, W, "bt709", False, "left", depth, "422"), layout)
    return k, [yuv.pack_numpy(f, k) for f in enc(k.planar)], (dict(keep_depth=True) if depth == 10 else {})


def by_hand(ops, dev, model, frames, pixfmt, order="tff", bgr=True, cuts=(), divisor=64):
    """Every output from single launches: the existing convert, ``ops.field_bob``, ``model.forward``, the loop's own encoder,
    ``ops.field_rows`` (and, packed, ``ops.yuv_unpack`` / ``ops.yuv_pack`` around them)."""
    packed = pixfmt if isinstance(pixfmt, yuv.Packed) else None
    planar = pixfmt.planar if packed is not None else pixfmt
    deep = planar is not None and planar.depth == 10
    h, w = frames[0].shape[:2] if pixfmt is None else (pixfmt.height, pixfmt.width)
    top, left, hp, wp = segments._canvas(h, w, divisor)
    B, stored, n = {}, [], len(frames)
    for j, f in enumerate(frames):
        d = torch.from_numpy(np.ascontiguousarray(f).view(np.uint8).reshape(f.shape if pixfmt is None else -1)).to(dev)
        if packed is not None:
            d = ops.yuv_unpack(d, packed)
        stored.append(d)
        C = torch.empty(3, hp, wp, device=dev)
        if pixfmt is None:
            ops.frame_u8_to_f32(d, C, top, left, bgr)
        elif deep:
            ops.yuv_decode(d, planar, dst=C, pad_top=top, pad_left=left, keep_depth=True)
        else:
            rgb = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
            ops.yuv_decode(d, planar, dst_u8=rgb)
            ops.frame_u8_to_f32(rgb, C, top, left, False)
        even, odd = torch.empty_like(C), torch.empty_like(C)
        ops.field_bob(C, even, odd, top, left, h, w)
        for k in (2 * j, 2 * j + 1):
            B[k] = odd if M.parity_model(k, order) else even
    out_fmt = None if pixfmt is None else yuv.out_format(planar, deep)
    geometry = fields.plane_geometry(out_fmt, planar, h, w)
    outs = []
    for k in range(2 * n):
        j = k // 2
        bob = k in (0, 2 * n - 1) or (k & 1 and j in cuts) or (not k & 1 and (j - 1) in cuts)
        P = B[k] if bob else model.forward(B[k - 1].unsqueeze(0), B[k + 1].unsqueeze(0))["I_t"][0]
        if pixfmt is None:
            buf = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
            ops.frame_f32_to_u8(P, buf, top, left, bgr)
            ops.field_rows(buf.view(-1), stored[j].view(-1), geometry, M.parity_model(k, order))
            outs.append(buf.cpu().numpy())
            continue
        buf = torch.empty(out_fmt.frame_bytes, dtype=torch.uint8, device=dev)
        ops.yuv_encode(buf, out_fmt, src=P, pad_top=top, pad_left=left)
        ops.field_rows(buf, stored[j], geometry, M.parity_model(k, order))
        if packed is not None:
            buf = ops.yuv_pack(buf, packed.tight())
        a = buf.cpu().numpy()
        outs.append(a.view(np.uint16) if (packed or out_fmt).dtype == np.uint16 else a)
    return outs


def same(got, want):
    return len(got) == len(want) and all(g.dtype == w_.dtype and np.array_equal(g, w_) for g, w_ in zip(got, want))


def test_the_loop_pool_plain_and_by_hand_and_its_launch_plans(ops, dev):
    net = make_net(dev, "lite")                                         # a fresh model: no plan has been recorded for it
    frames = M.interlaced_video(5, H, W)
    calls, inner = [], net.forward_pooled

    def counted(pool, left, right, **kw):
        stale = sum(pool.keys[s] is None for s in set(left + right))
        before = net.plan_stats()
        out = inner(pool, left, right, **kw)
        after = net.plan_stats()
        calls.append((stale, {kind: [b for b in c if after[kind][b] != before[kind][b]] for kind, c in after.items() if kind != "forward"}))
        return out
    net.forward_pooled = counted
    pooled = list(host_io.deinterlace_video(iter(frames), net, mode="mc"))
    del net.forward_pooled
    assert len(pooled) == 10 and len(calls) == 8 and [s for s, _ in calls] == [2, 2, 1, 1, 1, 1, 1, 1]
    steady = [bins for s, bins in calls if s == 1]
    assert steady[2] == {"pooled_frame": ["recorded"], "pooled_pair": ["replayed"]}      # (the pair key has run since the first call)
    assert all(bins == {"pooled_frame": ["replayed"], "pooled_pair": ["replayed"]} for bins in steady[3:]), steady
    plain = list(host_io.deinterlace_video(iter(frames), net, mode="mc", pool=False))
    assert same(pooled, plain)
    assert same(pooled, by_hand(ops, dev, net, frames, None))
    for k, g in enumerate(pooled):                                      # the real rows are the source's bytes
        p = M.parity_model(k, "tff")
        assert np.array_equal(g[p::2], frames[k // 2][p::2])
    bob = list(host_io.deinterlace_video(iter(frames), net, mode="bob"))
    pics = [(torch.tensor(np.ascontiguousarray(f[:, :, ::-1].transpose(2, 0, 1))) / 255.).numpy() for f in frames]
    top, left, _, _ = canvas = segments._canvas(H, W, 64)
    for k, g in enumerate(bob):
        P = fields.bob_numpy(pics[k // 2], M.parity_model(k, "tff"), canvas)[:, top:top + H, left:left + W]
        u8 = np.round(P.transpose(1, 2, 0) * 255).astype(np.uint8)[:, :, ::-1]
        assert np.array_equal(g, fields.weave_numpy(frames[k // 2], None, M.parity_model(k, "tff"), u8)), k


@pytest.mark.parametrize("kind,order", (("i422", "bff"), ("uyvy", "tff"), ("v210", "bff"), ("bgr", "bff")))
def test_the_loop_on_every_kind_of_stream(ops, dev, net, kind, order):
    pixfmt, frames, kw = stream_of(kind, M.interlaced_video(3, H, W, seed=8))
    got = list(host_io.deinterlace_video(iter(frames), net, order=order, pixfmt=pixfmt, **kw))
    assert same(got, by_hand(ops, dev, net, frames, pixfmt, order=order))
    assert same(got, list(host_io.deinterlace_video(iter(frames), net, order=order, pixfmt=pixfmt, pool=False, **kw)))


def test_the_loop_with_a_scene_cut(ops, dev, net):
    A, B = M.interlaced_video(3, H, W, seed=5, tone=70), M.interlaced_video(2, H, W, seed=9, tone=190)
    cuts = host_io.SceneCuts()
    got = list(host_io.deinterlace_video(A + B, net, scene=cuts))
    one = lambda v: list(host_io.deinterlace_video(v, net))
    assert cuts.cuts == [len(A) - 1] and same(got, one(A) + one(B))
    assert same(got, by_hand(ops, dev, net, A + B, None, cuts=(len(A) - 1,)))


def test_the_loop_on_network_base(ops, dev):
    base = make_net(dev, "base")
    frames = M.interlaced_video(3, 192, 320, seed=4)
    got = list(host_io.deinterlace_video(frames, base, isBGR=False))
    assert same(got, by_hand(ops, dev, base, frames, None, bgr=False))


def test_the_command_line_tool_deinterlaces_a_uyvy_file(tmp_path, dev, net):
    k, frames, _ = stream_of("uyvy", M.interlaced_video(3, H, W, seed=8))
    src, dst = tmp_path / "in.uyvy", tmp_path / "out.uyvy"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "interp_raw.py"), str(src), str(dst), "--pix-fmt", "uyvy422", "--size", f"{W}x{H}",
                        "--fps", "25", "--matrix", "bt709", "--model", "lite", "--interlaced", "tff", "--deint-only"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "'frames_out': 6" in r.stdout and "'fps_out': '50'" in r.stdout
    got = list(yuv.RawReader(str(dst), k, 50))
    assert same(got, list(host_io.deinterlace_video(frames, net, pixfmt=k)))


# ------------------------------------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize("case", M.REF_CASES, ids=lambda c: c[0])
def test_forwards_on_bobbed_canvases_match_the_reference(case, ops, dev):
    name, v = case
    gold = np.load(M.FIELDS_REF)
    model = make_net(dev, v)
    top, left, hp, wp = segments._canvas(M.REF_H, M.REF_W, M.REF_DIVISOR)
    B = {}
    for j, f in enumerate(M.reference_video()):
        C, even, odd = (torch.empty(3, hp, wp, device=dev) for _ in range(3))
        ops.frame_u8_to_f32(torch.from_numpy(f).to(dev), C, top, left, False)
        ops.field_bob(C, even, odd, top, left, M.REF_H, M.REF_W)
        B[2 * j], B[2 * j + 1] = even, odd                              # tff
    sums = np.array([B[i].double().sum().item() for i in range(2 * M.REF_N)])
    assert np.all(np.abs(sums - gold["in_sums"]) <= 1e-6 * np.abs(gold["in_sums"]))
    worst = 0.0
    for k in range(1, 2 * M.REF_N - 1):
        it = model.forward(B[k - 1].unsqueeze(0), B[k + 1].unsqueeze(0))["I_t"][0]
        d = float(np.abs(it[:, ::M.REF_STEP, ::M.REF_STEP].cpu().numpy() - gold[f"{name}.it.{k}"]).max())
        print(f"{name} field {k}: max|d| = {d:.3e}")
        worst = max(worst, d)
        assert d <= TOL, (name, k, d)
    print(f"{name}: worst max|d| over the interior fields = {worst:.3e}")
