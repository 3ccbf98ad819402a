"""GPU: half-resolution motion (csrc/warp.hip atmvfi_frame_half / atmvfi_synth_up2, ``Network.forward_scaled``, ``motion_scale=2`` of the
video loops).  frame_half bit for bit against its twin; synth_up2 against the fp64 reference and elementwise bound of
tests/scaled_ref.py on the hostile families, the staged and the direct path to each other's bits, the uint8 output against
``frame_f32_to_u8`` of the same launch's fp32 output; ``forward_scaled`` against its own composition and the golden of the reference."""
import importlib
import os

import numpy as np
import pytest
import torch

import pairs
import scaled_ref as SR
import warp_ref as WR

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
scaled = importlib.import_module("atm-vfi_amd.scaled")

F32 = np.float32
GUARD = 256                       # bytes on each side of an output (a multiple of 16: the view keeps the allocation's alignment)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaled_ref.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


def poisoned(nbytes, dev, poison=0xA5, offset=0):
    buf = torch.full((GUARD + offset + nbytes + GUARD,), poison, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD + offset:GUARD + offset + nbytes]


def guards_intact(buf, view, poison=0xA5):
    lo = view.data_ptr() - buf.data_ptr()
    return bool((buf[:lo] == poison).all()) and bool((buf[lo + view.numel():] == poison).all())


# ------------------------------------------------------------------------------------------------------------------------ frame_half
def _half_on(ops, dev, x, src_offset=0, dst_offset=0):
    raw = torch.from_numpy(x.reshape(-1).view(np.uint8))
    sbuf = torch.empty(raw.numel() + src_offset, dtype=torch.uint8, device=dev)
    sbuf[src_offset:].copy_(raw)
    src = sbuf[src_offset:].view(torch.float32).view(x.shape)
    oshape = x.shape[:-2] + (x.shape[-2] // 2, x.shape[-1] // 2)
    buf, view = poisoned(4 * int(np.prod(oshape)), dev, offset=dst_offset)
    dst = view.view(torch.float32).view(oshape)
    ops.frame_half(src, dst)
    torch.cuda.synchronize()
    assert guards_intact(buf, view)
    return dst.cpu().numpy()


@pytest.mark.parametrize("planes,h,w,so,do", [(3, 2, 2, 0, 0), (3, 10, 14, 0, 0), (2, 34, 70, 0, 0),      # W % 8 != 0: the scalar path
                                              (3, 16, 32, 0, 0), (2, 6, 520, 0, 0),                       # the 16-byte path, more than one block
                                              (3, 16, 32, 4, 0), (3, 16, 32, 0, 4), (1, 8, 24, 4, 4)])    # pointers offset by one float
def test_frame_half_bit_for_bit(ops, dev, planes, h, w, so, do):
    rng = np.random.default_rng([planes, h, w])
    x = (rng.normal(0, 1, (planes, h, w)) * 10.0 ** rng.integers(-3, 4, (planes, h, w))).astype(F32)
    assert np.array_equal(_half_on(ops, dev, x, so, do), scaled.frame_half_numpy(x))


def test_frame_half_at_2176x4096(ops, dev):
    x = torch.rand(3, 2176, 4096, device=dev)
    buf, view = poisoned(4 * 3 * 1088 * 2048, dev)
    dst = view.view(torch.float32).view(3, 1088, 2048)
    ops.frame_half(x, dst)
    want = ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])) * 0.25      # the stated expression, elementwise fp32
    assert torch.equal(dst, want) and guards_intact(buf, view)
    rot = torch.empty_like(x)
    ops.frame_rot180(x, rot)
    dst2 = torch.empty_like(dst)
    ops.frame_half(rot, dst2)
    assert torch.equal(dst2, dst.flip(-2).flip(-1))


# ------------------------------------------------------------------------------------------------------------------------- synth_up2
def _synth_on(ops, dev, case, slots0=None, slots1=None, path="auto", window=None, bgr=False, f32=True, u8=True, want=SR.scaled.WANT_KEYS, poison=0xA5):
    """One launch on poisoned outputs between guards -> dict of numpy arrays ("I_t", "I_t_u8", the wanted maps)."""
    t = lambda a: torch.from_numpy(a).to(dev)
    half = {k: (t(v[0]),) if isinstance(v, list) else t(v) for k, v in SR.as_forward_dict(case["half"]).items()}
    half["im_t_list"] = list(half["im_t_list"])
    b, _, h, w = case["half"]["it_sum"].shape
    fb = fv = ub = uv = None
    if f32:
        fb, fv = poisoned(4 * b * 3 * 2 * h * 2 * w, dev, poison)
        fv = fv.view(torch.float32).view(b, 3, 2 * h, 2 * w)
    if u8:
        _, _, hh, ww = window or (0, 0, 2 * h, 2 * w)
        ub, uv = poisoned(b * hh * ww * 3, dev, poison)
        uv = uv.view(b, hh, ww, 3)
    out = ops.synth_up2(half, t(case["store0"]), t(case["store1"]), slots0, slots1, dst=fv, dst_u8=uv, window=window, bgr=bgr, want=want, path=path)
    torch.cuda.synchronize()
    assert fb is None or guards_intact(fb, fv.view(-1).view(torch.uint8), poison)
    assert ub is None or guards_intact(ub, uv.view(-1), poison)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _u8_of(ops, dev, it, window, bgr):
    """``frame_f32_to_u8`` of every frame of the fp32 result [B,3,H,W] -> uint8 [B,hh,ww,3]"""
    pt, pl, hh, ww = window
    src = torch.from_numpy(it).to(dev)
    out = torch.empty(it.shape[0], hh, ww, 3, dtype=torch.uint8, device=dev)
    for i in range(it.shape[0]):
        ops.frame_f32_to_u8(src[i], out[i], pt, pl, bgr)
    return out.cpu().numpy()


# (B, h, w, stores, slots0, slots1, window (pad_top, pad_left, hh, ww) of the 2h x 2w canvas)
GEOMETRIES = [
    (1, 1, 1, 1, None, None, (0, 1, 2, 1)),
    (2, 5, 7, 3, [2, 0], [1, 1], (1, 3, 8, 9)),                 # 2w = 14: the direct path only
    (1, 9, 10, 1, None, None, (0, 0, 18, 20)),                  # 2w % 4 == 0, one partial tile
    (1, 16, 24, 2, [1], [0], (3, 8, 26, 33)),                   # several tiles, unequal pads
    (2, 20, 36, 3, [1, 1], [2, 0], (5, 2, 30, 69)),             # crosses output tiles in both directions, B = 2, repeated store frames
]
# (flow0 family, flow1 family, mask family)
INPUTS = [("gauss", None, "rand"), ("const_int", None, "binary"), ("const_ulp", None, "ones"), ("blocks", None, "rand"), ("outside", "gauss", "zeros"),
          ("wild", None, "rand"), ("far", None, "rand"), ("far", "gauss", "binary")]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"B{g[0]}_{g[1]}x{g[2]}")
@pytest.mark.parametrize("inp", INPUTS, ids=lambda i: "-".join(str(x) for x in i))
def test_synth_up2_against_fp64_bound(ops, dev, geo, inp):
    b, h, w, stores, s0, s1, window = geo
    case = SR.make_case(b, h, w, flow=inp[0], flow1=inp[1], mask=inp[2], stores=stores)
    ref = SR.synth64(case["half"], case["store0"], case["store1"], s0, s1)
    bgr = (h + w) % 2 == 1
    direct = _synth_on(ops, dev, case, s0, s1, "direct", window, bgr)
    ratios = SR.worst(direct, ref)
    print(f"synth_up2 B{b} {h}x{w} {inp}: worst error / bound {ratios}")
    assert max(ratios.values()) <= 1.0, ratios
    assert not np.isnan(direct["I_t"]).any()
    assert np.array_equal(direct["I_t_u8"], _u8_of(ops, dev, direct["I_t"], window, bgr))
    if inp[0] == "wild":       # a non-finite flow: that source's sample is 0.0 exactly -- with m at 0 / 1 and no residual the pixel is 0.0
        z = {k: v.copy() for k, v in case["half"].items()}
        z["occ_mask1"][:] = 1.0
        z["it_sum"] = z["I_t_0"].copy()
        got = _synth_on(ops, dev, dict(case, half=z), s0, s1, "direct", window, bgr)
        dead0 = ~np.isfinite(got["opt_flow_0"]).all(axis=1)
        assert (dead0.any() or h * w < 35) and np.all(got["I_t"][np.broadcast_to(dead0[:, None], got["I_t"].shape)] == 0.0)
    if (2 * w) % 4 == 0:
        staged = _synth_on(ops, dev, case, s0, s1, "staged", window, bgr)
        for k in direct:
            assert np.array_equal(staged[k], direct[k], equal_nan=True), f"staged and direct differ in {k}"
        auto = _synth_on(ops, dev, case, s0, s1, "auto", window, bgr, poison=0x00)          # another poison: nothing of the outputs is read
        assert np.array_equal(auto["I_t"], direct["I_t"]) and np.array_equal(auto["I_t_u8"], direct["I_t_u8"])
        if inp[0] == "far" and h * w >= 16 * 24:
            f0, f1 = direct["opt_flow_0"], direct["opt_flow_1"]
            st0 = {v["state"] for v in WR.staged_boxes(f0).values()}
            st1 = {v["state"] for v in WR.staged_boxes(f1).values()}
            assert "falls back" in st0 and ("fits" in st0 or "fits" in st1), (st0, st1)     # tiles beyond the box, alone and beside staged ones
    else:
        with pytest.raises(RuntimeError, match="staged"):
            _synth_on(ops, dev, case, s0, s1, "staged", window, bgr)


def test_synth_up2_ties_and_either_output_alone(ops, dev):
    """Exact .5 ties of the uint8 rule.  Zero frames and zero half-size warps leave the output = the up-sampled residual = it_sum, and a
    map that is constant on 3 x 3 half-size blocks up-samples to exactly that constant at each block's four centre pixels: there the
    fp32 output is a value x with fl(x * 255) = k + 0.5, bit for bit."""
    ties = SR.tie_pixels()
    by, bx = 8, 32
    assert by * bx >= len(ties)
    h, w = 3 * by, 3 * bx
    case = SR.make_case(1, h, w)
    blocks = np.resize(ties, (3, by, bx))
    case["half"]["it_sum"] = np.repeat(np.repeat(blocks, 3, axis=1), 3, axis=2)[None].astype(F32)
    for k in ("I_t_0", "I_t_1"):
        case["half"][k][:] = 0
    case["store0"][:] = 0
    case["store1"][:] = 0
    cy, cx = (6 * np.arange(by)[:, None] + np.array([2, 3])).reshape(-1), (6 * np.arange(bx)[:, None] + np.array([2, 3])).reshape(-1)
    for window, bgr in (((0, 0, 2 * h, 2 * w), False), ((1, 5, 2 * h - 4, 2 * w - 9), True)):
        both = _synth_on(ops, dev, case, path="staged", window=window, bgr=bgr)
        centre = both["I_t"][0][:, cy][:, :, cx]
        assert np.array_equal(centre, np.repeat(np.repeat(blocks, 2, axis=1), 2, axis=2))
        kk = np.rint(centre.astype(np.float64) * 255.0 - 0.5).astype(np.int64)
        assert np.all((centre * F32(255.0)).astype(F32) == (kk + 0.5).astype(F32))
        full = scaled.to_u8_numpy(both["I_t"])                      # rint of the same fp32 product, half to even
        assert np.array_equal(np.moveaxis(full[0][cy][:, cx], -1, 0), kk + (kk & 1))
        pt, pl, hh, ww = window
        want = full[:, pt:pt + hh, pl:pl + ww]
        assert np.array_equal(both["I_t_u8"], want[..., ::-1] if bgr else want)
        assert np.array_equal(both["I_t_u8"], _u8_of(ops, dev, both["I_t"], window, bgr))
        only_f = _synth_on(ops, dev, case, path="direct", window=window, bgr=bgr, u8=False, want=())
        only_u = _synth_on(ops, dev, case, path="direct", window=window, bgr=bgr, f32=False, want=())
        assert "I_t_u8" not in only_f and np.array_equal(only_f["I_t"], both["I_t"])
        assert "I_t" not in only_u and np.array_equal(only_u["I_t_u8"], both["I_t_u8"])


def test_synth_up2_refusals(ops, dev):
    case = SR.make_case(2, 4, 6)
    t = lambda a: torch.from_numpy(a).to(dev)
    half = {k: [t(v[0])] if isinstance(v, list) else t(v) for k, v in SR.as_forward_dict(case["half"]).items()}
    st = t(case["store0"])
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.synth_up2(half, st, st, dst=st)
    with pytest.raises(ValueError):
        ops.synth_up2(half, st, st, slots0=[0, 2])
    with pytest.raises(ValueError):
        ops.synth_up2(half, st[:, :, :6], st)
    big = {k: [v[0].repeat(9, 1, 1, 1)] if isinstance(v, list) else v.repeat(9, 1, 1, 1) for k, v in half.items()}
    with pytest.raises(ValueError, match="16"):
        ops.synth_up2(big, st, st, slots0=[0] * 18, slots1=[0] * 18)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.frame_half(st, st.view(-1)[:st.numel() // 4].view(2, 3, 4, 6))


# -------------------------------------------------------------------------------------------------------------------- forward_scaled
def _net(dev, variant, glob):
    torch.set_grad_enabled(False)
    n = (pkg.NetworkLite if variant == "lite" else pkg.NetworkBase)()
    n.load_state_dict(pkg.synthetic_state_dict(variant, seed=1), strict=True)
    n = n.to(dev).eval()
    n.global_motion, n.ensemble_global_motion = glob, False
    return n


@pytest.fixture(scope="module")
def net(dev):
    return _net(dev, "lite", False)


GOLDEN_CASES = {"lite": ("lite_128x192", 128, 192, False, 7), "base": ("base_128x128_global", 128, 128, True, 11)}


@pytest.mark.parametrize("variant", ("lite", "base"))
def test_forward_scaled_is_its_composition_and_meets_the_golden(ops, dev, net, variant):
    name, h, w, glob, seed = GOLDEN_CASES[variant]
    model = net if variant == "lite" else _net(dev, "base", glob)
    im0, im1 = (x.to(dev) for x in pairs.smooth_pair(1, h, w, seed=seed))
    gold = np.load(GOLDEN)
    assert np.allclose(gold[f"{name}.in_sums"], [im0.double().sum().item(), im1.double().sum().item()])
    out = model.forward_scaled(im0, im1, want=scaled.WANT_KEYS)
    assert set(out) == {"I_t", "half"} | set(scaled.WANT_KEYS) and out["half"]["I_t"].shape == (1, 3, h // 2, w // 2)
    # the composition by hand: synth_up2 of forward(frame_half(.))
    mops = model._ops(dev)
    h0, h1 = torch.empty(1, 3, h // 2, w // 2, device=dev), torch.empty(1, 3, h // 2, w // 2, device=dev)
    mops.frame_half(im0, h0)
    mops.frame_half(im1, h1)
    o = model.forward(h0, h1)
    assert torch.equal(o["I_t"], o["im_t_list"][0].clamp(0, 1))
    hand = mops.synth_up2(o, im0, im1, want=scaled.WANT_KEYS)
    for k in ("I_t",) + scaled.WANT_KEYS:
        assert torch.equal(out[k], hand[k]), k
    again = model.forward_scaled(im0, im1)                   # (plans replay from the third forward of a shape on)
    assert torch.equal(again["I_t"], out["I_t"]) and set(again) == {"I_t", "half"}
    step = 2
    errs = {"I_t": np.abs(out["I_t"].cpu().numpy() - gold[f"{name}.I_t"]).max()}
    for k, short in (("opt_flow_0", "f0"), ("opt_flow_1", "f1"), ("occ_mask1", "m")):
        errs[short] = np.abs(out[k].cpu().numpy()[..., ::step, ::step] - gold[f"{name}.{short}"]).max()
    print(f"forward_scaled {name} against the golden of the reference: max |d| = " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["I_t"] <= 1e-3, errs
    for bad in (1, 4, 0.5, True):
        with pytest.raises(ValueError):
            model.forward_scaled(im0, im1, scale=bad)
    with pytest.raises(ValueError):
        model.forward_scaled(im0[..., :-1], im1[..., :-1])


# ----------------------------------------------------------------------------------------------------------------------------- the loops
import cpu_scene as CS  # noqa: E402

host_io = importlib.import_module("atm-vfi_amd.host_io")
mf = importlib.import_module("atm-vfi_amd.multiframe")
rt = importlib.import_module("atm-vfi_amd.retime")
yuv = importlib.import_module("atm-vfi_amd.yuv")
scene = importlib.import_module("atm-vfi_amd.scene")

LH, LW, LDIV = 128, 192, 16            # frames; motion_scale=2 pads under 32: the canvas is 128 x 192, the network's 64 x 96


def _dev_bytes(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev)


class Hand:
    """The loops' frames made by hand: ``load`` a source frame into the canvas of ``divisor * 2`` with the loop's own decoder, the
    recursion composed here from ``net.forward_scaled``'s fp32 ``I_t`` in the loop's batch composition (the unrounded full-size
    prediction feeds the next level), ``store`` through the loop's own encoder.  ``kind``: "u8" (RGB or BGR), "i420" or "deep"."""

    def __init__(self, net, ops, dev, kind="u8", fmt=None, window=None, bgr=False, compose=False):
        self.net, self.ops, self.dev, self.kind, self.fmt, self.bgr, self.compose = net, ops, dev, kind, fmt, bgr, compose
        self.window = y0, x0, h, w = window or (0, 0, LH, LW)
        self.pl, pr, self.pt, pb = host_io.InputPadder((1, 3, h, w), divisor=2 * LDIV)._pad
        self.hp, self.wp = h + self.pt + pb, w + self.pl + pr
        self.sizes = []

    def load(self, frame):
        y0, x0, h, w = self.window
        t = torch.empty(1, 3, self.hp, self.wp, dtype=torch.float32, device=self.dev)
        if self.kind == "deep":
            self.ops.yuv_decode(_dev_bytes(frame, self.dev), self.fmt, dst=t[0], window=self.window, pad_top=self.pt, pad_left=self.pl, keep_depth=True)
            return t
        if self.kind == "i420":
            rgb = torch.empty(LH, LW, 3, dtype=torch.uint8, device=self.dev)
            self.ops.yuv_decode(_dev_bytes(frame, self.dev), self.fmt, dst_u8=rgb)
        else:
            rgb = torch.from_numpy(np.ascontiguousarray(frame)).to(self.dev)
        if (y0, x0, h, w) == (0, 0, LH, LW):
            self.ops.frame_u8_to_f32(rgb, t[0], self.pt, self.pl, self.bgr)
        else:
            self.ops.frame_u8_window(rgb, 0, y0, x0, h, w, dst=t[0], pad_top=self.pt, pad_left=self.pl, bgr=self.bgr)
        return t

    def store(self, pred, flip=None, border=None):
        y0, x0, h, w = self.window
        if self.kind == "u8":
            out = torch.empty(h, w, 3, dtype=torch.uint8, device=self.dev)
            if flip is not None:
                self.ops.tta_merge(pred, flip, out_u8=out, pad_top=self.pt, pad_left=self.pl, bgr=self.bgr)
            else:
                self.ops.frame_f32_to_u8(pred, out, self.pt, self.pl, self.bgr)
            if self.compose:
                full = torch.empty(LH, LW, 3, dtype=torch.uint8, device=self.dev)
                self.ops.frame_compose(full, torch.from_numpy(border).to(self.dev), self.window, src=pred, pad_top=self.pt, pad_left=self.pl, bgr=self.bgr)
                return full.cpu().numpy()
            return out.cpu().numpy()
        out_fmt = self.fmt.cropped(h, w)
        buf = torch.empty(out_fmt.frame_bytes, dtype=torch.uint8, device=self.dev)
        self.ops.yuv_encode(buf, out_fmt, src=pred.contiguous(), pad_top=self.pt, pad_left=self.pl)
        raw = buf.cpu().numpy()
        return raw.view(np.uint16) if self.kind == "deep" else raw

    def segment(self, a, b, factor, tta=False, levels=None, emit=None, max_batch=4):
        fr = {0: self.load(a), factor: self.load(b)}
        shown = {}
        rot = lambda t: t.flip(2).flip(3).contiguous()
        for level in (mf.nx_levels(factor) if levels is None else levels):
            for i in range(0, len(level), max_batch):
                chunk = level[i:i + max_batch]
                l = torch.cat([fr[x] for x, _, _ in chunk], 0).contiguous()
                r = torch.cat([fr[y] for _, y, _ in chunk], 0).contiguous()
                out = self.net.forward_scaled(l, r)
                self.sizes.append(tuple(out["half"]["I_t"].shape[-2:]))
                pred = out["I_t"].clone()
                flip = self.net.forward_scaled(rot(l), rot(r))["I_t"].clone() if tta else None
                for j, (_, _, pos) in enumerate(chunk):
                    fr[pos], shown[pos] = pred[j:j + 1], (pred[j], None if flip is None else flip[j])
        return [self.store(*shown[pos], border=a if pos <= factor // 2 else b) for pos in (range(1, factor) if emit is None else emit)]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _half_sizes(monkeypatch, net):
    """the frame sizes ``forward`` / ``forward_pooled`` are asked for while the loop runs"""
    seen = []
    klass = next(k for k in type(net).__mro__ if "forward" in k.__dict__)
    monkeypatch.setattr(klass, "forward", lambda self, a, b, *x, _o=klass.__dict__["forward"], **kw: (seen.append(tuple(a.shape[-2:])), _o(self, a, b, *x, **kw))[1])
    klass = next(k for k in type(net).__mro__ if "forward_pooled" in k.__dict__)
    monkeypatch.setattr(klass, "forward_pooled",
                        lambda self, pool, *x, _o=klass.__dict__["forward_pooled"], **kw: (seen.append((pool.hp, pool.wp)), _o(self, pool, *x, **kw))[1])
    return seen


def _check_nx(got, hand, video, factor, tta=False, cuts=(), original=lambda f: f):
    assert len(got) == factor * (len(video) - 1) + 1
    for seg in range(len(video) - 1):
        assert _same(np.asarray(got[seg * factor]), np.asarray(original(video[seg])))
        if seg in cuts:
            for pos in range(1, factor):
                assert _same(np.asarray(got[seg * factor + pos]), np.asarray(original(video[seg + (pos > factor // 2)])))
            continue
        want = hand.segment(video[seg], video[seg + 1], factor, tta)
        for pos in range(1, factor):
            g = got[seg * factor + pos]
            assert _same(g, want[pos - 1]), (seg, pos, int((g != want[pos - 1]).sum()) if g.shape == want[pos - 1].shape else (g.shape, want[pos - 1].shape))
    assert hand.sizes and all(s == (hand.hp // 2, hand.wp // 2) for s in hand.sizes)


NX_LOOPS = [      # factor, tta, crop, bgr
    (4, False, None, True),
    (8, False, None, False),
    (4, True, None, False),
    (4, False, (96, 160), True),
]


@pytest.mark.parametrize("factor,tta,crop,bgr", NX_LOOPS, ids=lambda v: str(v).replace(" ", ""))
def test_nx_loop_at_motion_scale_2(net, ops, dev, monkeypatch, factor, tta, crop, bgr):
    video = CS.shot(3, LH, LW, seed=21, tone=110)
    window = mf.centre_window(LH, LW, crop)
    kw = dict(factor=factor, divisor=LDIV, tta=tta, crop=crop, isBGR=bgr, max_batch=4)
    seen = _half_sizes(monkeypatch, net)
    got = list(mf.interpolate_video_nx(iter(video), net, motion_scale=2, **kw))
    hand = Hand(net, ops, dev, window=window, bgr=bgr)
    assert seen and all(s == (hand.hp // 2, hand.wp // 2) for s in seen)                 # the loop's forwards ran at half size
    y0, x0, h, w = window
    _check_nx(got, hand, video, factor, tta, original=lambda f: f[y0:y0 + h, x0:x0 + w])
    plain = list(mf.interpolate_video_nx(iter(video), net, motion_scale=2, pool=False, **kw))       # pooled and plain are equal
    assert len(plain) == len(got) and all(_same(a, b) for a, b in zip(plain, got))
    if factor == 4 and not tta and crop is None:
        one = list(mf.interpolate_video_nx(iter(video), net, motion_scale=1, **kw))               # motion_scale=1 is today's loop
        base = list(mf.interpolate_video_nx(iter(video), net, **kw))
        assert len(one) == len(base) and all(np.array_equal(a, b) for a, b in zip(one, base))
        mid = host_io.inference_2frame(video[0], video[1], net, isBGR=bgr, divisor=LDIV, motion_scale=2)
        assert _same(mid, got[2])                                                                  # the kernel's own uint8 output
        assert np.array_equal(host_io.inference_2frame(video[0], video[1], net, isBGR=bgr, divisor=LDIV, motion_scale=1),
                              host_io.inference_2frame(video[0], video[1], net, isBGR=bgr, divisor=LDIV))


def test_nx_loop_on_i420_and_deep_rgb(net, ops, dev):
    rgb = CS.shot(2, LH, LW, seed=22, tone=120)
    fmt = yuv.Format(LH, LW)
    video = [yuv.encode_numpy(f, fmt) for f in rgb]
    got = list(mf.interpolate_video_nx(iter(video), net, factor=4, divisor=LDIV, pixfmt=fmt, motion_scale=2))
    _check_nx(got, Hand(net, ops, dev, "i420", fmt), video, 4)
    deep = yuv.surface_of("gbrp10le", LH, LW)
    rng = np.random.default_rng(4)
    video = [np.clip(f.astype(np.int64).transpose(2, 0, 1)[[1, 2, 0]] * 4 + rng.integers(0, 4, (3, LH, LW)), 0, 1023).astype(np.uint16) for f in rgb]
    got = list(mf.interpolate_video_nx(iter(video), net, factor=4, divisor=LDIV, pixfmt=deep, keep_depth=True, motion_scale=2))
    assert all(g.dtype == np.uint16 for g in got[1:4])
    _check_nx([np.asarray(g).reshape(-1) for g in got], Hand(net, ops, dev, "deep", deep), video, 4, original=lambda f: f.reshape(-1))


def test_scene_cut_and_active_picture(net, ops, dev):
    video = CS.shot(2, LH, LW, seed=23, tone=60) + CS.shot(2, LH, LW, seed=24, tone=190)
    cuts = scene.SceneCuts()
    got = list(mf.interpolate_video_nx(iter(video), net, factor=4, divisor=LDIV, isBGR=False, scene=cuts, motion_scale=2))
    assert cuts.cuts == [1]
    _check_nx(got, Hand(net, ops, dev), video, 4, cuts={1})
    win = (32, 0, 64, 192)
    boxed = []
    for f in CS.shot(3, LH, LW, seed=25, tone=120):
        g = np.zeros_like(f)
        g[32:96] = f[32:96]
        boxed.append(g)
    got = list(mf.interpolate_video_nx(iter(boxed), net, factor=4, divisor=LDIV, isBGR=False, active=win, motion_scale=2))
    hand = Hand(net, ops, dev, window=win, compose=True)
    assert (hand.hp, hand.wp) == (64, 192)
    _check_nx(got, hand, boxed, 4)


def test_retimed_24_to_60(net, ops, dev):
    video, L = CS.shot(4, LH, LW, seed=26, tone=100), 2
    got = list(rt.interpolate_video_retimed(iter(video), net, 24, 60, levels=L, divisor=LDIV, isBGR=False, motion_scale=2))
    slots = list(rt.retime_slots(range(len(video)), 24, 60, L))
    assert len(got) == len(slots)
    hand, n, made = Hand(net, ops, dev), 1 << L, {}
    for j in sorted({j for j, _ in slots}):
        interior = sorted({p for jj, p in slots if jj == j and 0 < p < n})
        if interior:
            frames = hand.segment(video[j], video[j + 1], n, levels=rt.sparse_levels(interior, L), emit=interior)
            made.update({(j, p): f for p, f in zip(interior, frames)})
    assert made and all(s == (64, 96) for s in hand.sizes)
    for g, (j, p) in zip(got, slots):
        if p in (0, n):
            assert g is video[j + (p == n)]
        else:
            assert _same(g, made[j, p]), (j, p)
    base = list(rt.interpolate_video_retimed(iter(video), net, 24, 60, levels=L, divisor=LDIV, isBGR=False))
    one = list(rt.interpolate_video_retimed(iter(video), net, 24, 60, levels=L, divisor=LDIV, isBGR=False, motion_scale=1))
    assert len(one) == len(base) and all(np.array_equal(a, b) for a, b in zip(one, base))
    with pytest.raises(ValueError, match="shutter"):
        rt.interpolate_video_retimed(iter(video), net, 24, 60, shutter=180, motion_scale=2)
