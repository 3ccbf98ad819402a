"""GPU: the single-pass fp16 mode ("f16": Network.set_precision, HipOps.plane_terms = 1, ATMVFI_PREC_F16, terms = 1 of
atmvfi_conv3p and its read-out with terms = 1) against the exact fp64 model of tests/f16_model.py.

Exact family: the configurations, engines and tile widths of tests/test_gpu_f16x3_contract.py; the kernel must equal the hi-only model
up to the epilogue's final roundings.  tests/test_f16_mode_cpu.py shows that the three-term result misses that bound by more than
10x on every configuration (and the other way round): a launch that ran the other mode fails here.  Statistical families, plane sinks,
the fused read-out, the forward (mode switches leave nothing stale; plans, pool, replicas, the N-x loop) and the reference goldens."""
import importlib
import zlib

import numpy as np
import pytest
import torch

import f16_model as F16
import f16x3_model as M
import golden_util as G
import pairs

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
host_io = importlib.import_module("atm-vfi_amd.host_io")
mf = importlib.import_module("atm-vfi_amd.multiframe")
Network = pkg.Network
GEMM_CONV, GEMM_LINEAR, GEMM_DECONV = 0, 1, 2
# plane-input engines with a single-term instance: -3 gemm_pp, -2 / -4 gemm_duo 128 / 64 columns, 0 auto
ENGINES = [-3, -2, -4, 0]
ENGINE_IDS = ["pp", "duo", "duo64", "auto"]
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def f16_ops(dev, engine=0):
    h = hip_ops.HipOps(dev)
    h.plane_terms = 1
    h.gemm_tile_wn = engine
    return h


def r4(c):
    return (c + 3) // 4 * 4


def padded_nhwc(x, dev):
    c = x.shape[-1]
    buf = torch.zeros(*x.shape[:-1], r4(c), device=dev)
    buf[..., :c] = x.to(dev)
    return buf[..., :c]


def out_view(shape, dev, fill=7.0):
    c = shape[-1]
    return torch.full((*shape[:-1], r4(c)), fill, device=dev)[..., :c]


def planes_of(x2d, hip, dev):
    m, c = x2d.shape
    p = hip_ops.Planes.alloc(m, c, dev)
    hip.split_planes(padded_nhwc(x2d, dev), p)
    return p


def poisoned_sink(rows, c, dev):
    """A plane sink whose every half is NaN before the launch: what the launch does not write shows."""
    p = hip_ops.Planes.alloc(rows, c, dev)
    p.t.fill_(NAN)
    return p


def check_exact(got, res: M.Result, what, splitk=False):
    got = got.detach().double().cpu()
    tol = res.splitk_tol() if splitk else res.exact_tol()
    err = (got - res.y).abs()
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off the f16 model, worst {float((err / tol.clamp_min(1e-300)).max()):.2f}x the bound"


def check_stat(got, y_model, abs_xw, cpu32_err, what):
    got = got.detach().double().cpu()
    bound = M.stat_bound(abs_xw, cpu32_err)
    err = (got - y_model).abs()
    assert torch.isfinite(got).all(), what
    assert (err <= bound).all(), f"{what}: worst {float((err / bound).max()):.2f}x the statistical bound"


# ------------------------------------------------------------------ exact family: plane-input GEMM engines
@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("cfg", M.CASES_PLANES, ids=lambda c: c["id"])
def test_exact_gemm_planes_f16(cfg, engine, dev):
    hip = f16_ops(dev, engine)
    x, w, res = F16.build_case(cfg)
    p = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in cfg["dev_args"](x, w).items()}
    kind = cfg["kind"]
    pw = hip.pack_weight({"linear": GEMM_LINEAR, "conv": GEMM_CONV, "deconv": GEMM_DECONV}[kind], w.to(dev))
    variants = [(None, False)]
    if engine == 0 and cfg.get("splitk"):
        variants.append(("ws", True))
    for ws, splitk in variants:
        used = []

        def scratch(n):
            used.append(n)
            return torch.empty(n, device=dev)
        hip.gemm_workspace = scratch if ws else None
        if kind == "linear":
            out = out_view((cfg["rows_out"], w.shape[0]), dev)
            hip.linear(planes_of(x, hip, dev), pw, out, bias=p.get("bias"), residual=p.get("residual"), out_row_map=p.get("row_map"))
            torch.cuda.synchronize()
            got = M.gather_rows(out.cpu(), cfg.get("row_map_cpu"))
        elif kind == "conv":
            n, h, wd, cin = x.shape
            rows = x.reshape(-1, cin)
            out = out_view(tuple(res.y.shape), dev)
            kw = dict(out=out, stride=cfg["stride"], pad=cfg["pad"], dil=cfg["dil"], bias=p.get("bias"), prelu=p.get("slope"))
            if cfg.get("two_sources"):
                c1 = 32 * cfg["two_sources"]
                hip.conv_planes(planes_of(rows[:, :c1], hip, dev), n, h, wd, pw, x2=planes_of(rows[:, c1:], hip, dev),
                                split_chunks=cfg["two_sources"], **kw)
            else:
                hip.conv_planes(planes_of(rows, hip, dev), n, h, wd, pw, **kw)
            torch.cuda.synchronize()
            got = out
        else:
            n, h, wd, cin = x.shape
            out = out_view(tuple(res.y.shape), dev)
            hip.deconv(None, pw, out, bias=p.get("bias"), prelu=p.get("slope"), planes=planes_of(x.reshape(-1, cin), hip, dev),
                       in_shape=(n, h, wd, cin))
            torch.cuda.synchronize()
            got = out
        if splitk:
            assert used, f"{cfg['id']}: the launcher did not ask for split-K scratch: the case tests nothing"
        check_exact(got, res, f"{cfg['id']} engine={engine} splitk={splitk}", splitk=splitk)


# ------------------------------------------------------------------ exact family: the 3x3 plane kernel
@pytest.mark.parametrize("cfg", M.CASES_CONV3, ids=lambda c: c["id"])
def test_exact_conv3x3_planes_f16(cfg, dev):
    """Every tile width, fp32 rows + both sinks; the split-K launch where the case is meant for it."""
    hip = f16_ops(dev)
    x, w, res = F16.build_case(cfg)
    p = {k: v.to(dev) for k, v in cfg["dev_args"](x, w).items()}
    pw = hip.pack_weight(GEMM_CONV, w.to(dev))
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    xp = planes_of(x.reshape(-1, cin), hip, dev)
    for wn in range(1, 9):
        out = out_view(tuple(res.y.shape), dev)
        s1, s2 = poisoned_sink(n * h * wd, cout, dev), poisoned_sink(n * h * wd, cout, dev)
        hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=p.get("bias"), prelu=p.get("slope"), planes=s1, planes2=s2, wn=wn)
        torch.cuda.synchronize()
        check_exact(out, res, f"{cfg['id']} wn={wn}")
        M.assert_split_of(s1, out, f"{cfg['id']} wn={wn} sink")
        M.assert_split_of(s2, out, f"{cfg['id']} wn={wn} sink2")
    if cfg.get("kparts"):
        nws = hip.conv3x3_workspace_floats(n, h, wd, cin, cout)
        assert nws > 0, f"{cfg['id']}: meant for split-K but the launcher would not split it"
        out = out_view(tuple(res.y.shape), dev)
        s1 = poisoned_sink(n * h * wd, cout, dev)
        hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=p.get("bias"), prelu=p.get("slope"), planes=s1, workspace=torch.empty(nws, device=dev))
        torch.cuda.synchronize()
        check_exact(out, res, f"{cfg['id']} split-K", splitk=True)
        M.assert_split_of(s1, out, f"{cfg['id']} split-K sink")


def test_exact_conv3x3_planes_f16_persistent_grid(dev):
    cfg = M.CASE_CONV3_PERSISTENT
    hip = f16_ops(dev)
    x, w, res = F16.build_case(cfg)
    p = {k: v.to(dev) for k, v in cfg["dev_args"](x, w).items()}
    pw = hip.pack_weight(GEMM_CONV, w.to(dev))
    n, h, wd, cin = x.shape
    xp = planes_of(x.reshape(-1, cin), hip, dev)
    for wn in (0, 2):
        out = out_view(tuple(res.y.shape), dev)
        hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=p["bias"], prelu=p["slope"], wn=wn)
        torch.cuda.synchronize()
        check_exact(out, res, f"persistent wn={wn}")


# ------------------------------------------------------------------ wide / edge / cancel families
@pytest.mark.parametrize("family", ["wide", "edge", "cancel"])
@pytest.mark.parametrize("path", ["linear_planes", "deconv_planes", "conv_s2_planes", "conv3x3_planes"])
def test_statistical_families_f16(path, family, dev):
    """Finite, and within the statistical rule of the hi-only model: 8 x max(error of plain fp32 on the CPU against fp64 on the SAME hi
    operands, 2^-24 sum |hi(x)| |hi(w)|)."""
    hip = f16_ops(dev)
    g = torch.Generator().manual_seed(zlib.crc32(f"f16/{path}/{family}".encode()))
    gen = {"wide": M.wide, "edge": M.edge, "cancel": M.wide}[family]
    F = torch.nn.functional
    if path.startswith("conv"):
        n, h, wd, cin, cout = 2, 13, 19, 64, 40
        x = gen(g, n, h, wd, cin)
        w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (9 * cin) ** 0.5
        if family == "wide":
            w = M.wide(g, cout, cin, 3, 3, lo=-20.0, hi=2.0)
        if family == "cancel":
            x, w = M.cancel(g, x, w, 3, 1)
        b = (torch.rand(cout, generator=g) * 2 - 1) * 0.2
        stride = 2 if path == "conv_s2_planes" else 1
        res = F16.conv(x, w, b, None, stride=stride)
        cpu32 = F.conv2d(F16.hi(x).permute(0, 3, 1, 2), F16.hi(w), b, stride=stride, padding=1).permute(0, 2, 3, 1)
        pw = hip.pack_weight(GEMM_CONV, w.to(dev))
        out = out_view(tuple(res.y.shape), dev)
        xp = planes_of(x.reshape(-1, cin), hip, dev)
        if path == "conv3x3_planes":
            hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=b.to(dev))
        else:
            hip.conv_planes(xp, n, h, wd, pw, out=out, stride=2, pad=1, dil=1, bias=b.to(dev))
    elif path == "linear_planes":
        m, k, nout = 1000, 200, 96
        x = gen(g, m, k)
        w = (torch.rand(nout, k, generator=g) * 2 - 1) / k ** 0.5
        if family == "wide":
            w = M.wide(g, nout, k, lo=-20.0, hi=2.0)
        if family == "cancel":
            x, w = M.cancel(g, x, w, 1, 1)
        b = (torch.rand(nout, generator=g) * 2 - 1) * 0.2
        res = F16.linear(x, w, b)
        cpu32 = F16.hi(x) @ F16.hi(w).t() + b
        pw = hip.pack_weight(GEMM_LINEAR, w.to(dev))
        out = out_view((m, nout), dev)
        hip.linear(planes_of(x, hip, dev), pw, out, bias=b.to(dev))
    else:
        n, h, wd, cin, cout = 2, 9, 14, 96, 40
        x = gen(g, n, h, wd, cin)
        w = (torch.rand(cin, cout, 2, 2, generator=g) * 2 - 1) / cin ** 0.5
        if family == "wide":
            w = M.wide(g, cin, cout, 2, 2, lo=-20.0, hi=2.0)
        if family == "cancel":
            x, w = M.cancel(g, x, w, 3, 0)
        b = (torch.rand(cout, generator=g) * 2 - 1) * 0.2
        res = F16.deconv2x2(x, w, b)
        cpu32 = F.conv_transpose2d(F16.hi(x).permute(0, 3, 1, 2), F16.hi(w), b, stride=2).permute(0, 2, 3, 1)
        pw = hip.pack_weight(GEMM_DECONV, w.to(dev))
        out = out_view(tuple(res.y.shape), dev)
        hip.deconv(None, pw, out, bias=b.to(dev), planes=planes_of(x.reshape(-1, cin), hip, dev), in_shape=(n, h, wd, cin))
    torch.cuda.synchronize()
    check_stat(out, res.y, res.abs_xw, (cpu32.double() - res.y).abs().max().item(), f"{path} {family}")


# ------------------------------------------------------------------ plane sinks: both planes, the split of the launch's own fp32 result
def test_plane_sinks_in_f16_mode(dev):
    """The mode drops lo' from the PRODUCTS only: every sink still writes hi and lo' of its launch's own fp32 result, bit for bit
    (the stem, attention, pointwise kernels and the default mode read lo').  Destinations are NaN beforehand."""
    hip = f16_ops(dev)
    g = torch.Generator().manual_seed(4242)
    # 3x3: first sink through planes_prelu, raw second sink at a channel offset
    n, h, wd, cin, cout = 2, 19, 21, 37, 52
    x3 = torch.rand(n, h, wd, cin, generator=g) * 2 - 1
    w3 = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (9 * cin) ** 0.5
    b3 = ((torch.rand(cout, generator=g) * 2 - 1) * 0.3).to(dev)
    pw = hip.pack_weight(GEMM_CONV, w3.to(dev))
    out = out_view((n, h, wd, cout), dev)
    s1, s2 = poisoned_sink(n * h * wd, cout, dev), poisoned_sink(n * h * wd, 8 + cout, dev)
    hip.conv3x3_planes(planes_of(x3.reshape(-1, cin), hip, dev), n, h, wd, pw, out=out, bias=b3, planes=s1,
                       planes_prelu=hip.pad_channels(torch.full((cout,), 0.5, device=dev)), planes2=s2, planes2_c0=8)
    torch.cuda.synchronize()
    o = out.reshape(-1, cout).cpu()
    assert torch.isfinite(o).all() and (o < 0).any() and (o > 0).any()
    M.assert_split_of(s1, torch.where(o > 0, o, o * 0.5), "3x3 f16 first sink (planes_prelu)")
    M.assert_split_of(s2, o, "3x3 f16 second sink (raw, offset 8)", c0=8)
    lo = s2.to_rows().cpu()[1, :o.shape[0], 8:8 + cout]
    assert (lo != 0).float().mean().item() > 0.9, "the lo' plane of an f16 launch is (almost) all zero: the sink dropped it"
    # deconv sink and strided-conv sink, every engine that has the instance
    nd, hd_, wd_, cid, cod = 1, 15, 22, 101, 44
    xd = torch.rand(nd * hd_ * wd_, cid, generator=g) * 2 - 1
    wdc = (torch.rand(cid, cod, 2, 2, generator=g) * 2 - 1) / cid ** 0.5
    bd = ((torch.rand(cod, generator=g) * 2 - 1) * 0.3).to(dev)
    ns, hs, ws_, cis, cos = 2, 24, 40, 48, 56
    xs = torch.rand(ns * hs * ws_, cis, generator=g) * 2 - 1
    wsc = (torch.rand(cos, cis, 3, 3, generator=g) * 2 - 1) / (9 * cis) ** 0.5
    bs = ((torch.rand(cos, generator=g) * 2 - 1) * 0.3).to(dev)
    for engine in ENGINES:
        hip = f16_ops(dev, engine)
        pwd = hip.pack_weight(GEMM_DECONV, wdc.to(dev))
        sink = poisoned_sink(nd * 4 * hd_ * wd_, 4 + cod, dev)
        out = out_view((nd, 2 * hd_, 2 * wd_, cod), dev)
        hip.deconv(None, pwd, out, bias=bd, planes=planes_of(xd, hip, dev), sink=sink, sink_c0=4, in_shape=(nd, hd_, wd_, cid))
        torch.cuda.synchronize()
        M.assert_split_of(sink, out.reshape(-1, cod), f"deconv f16 sink engine={engine}", c0=4)
        pws = hip.pack_weight(GEMM_CONV, wsc.to(dev))
        sink = poisoned_sink(ns * (hs // 2) * (ws_ // 2), 8 + cos, dev)
        out = out_view((ns, hs // 2, ws_ // 2, cos), dev)
        hip.conv_planes(planes_of(xs, hip, dev), ns, hs, ws_, pws, out=out, stride=2, pad=1, dil=1, bias=bs, sink=sink, sink_c0=8)
        torch.cuda.synchronize()
        M.assert_split_of(sink, out.reshape(-1, cos), f"strided conv f16 sink engine={engine}", c0=8)


# ------------------------------------------------------------------ the fused read-out: main product hi-only, W2 three-term
@pytest.mark.parametrize("case", [(128, 64, 1, 40, 72), (64, 32, 2, 21, 35)], ids=lambda c: f"cin{c[0]}_c{c[1]}_n{c[2]}_{c[3]}x{c[4]}")
def test_readout_f16(case, dev):
    """atmvfi_conv3p's read-out (terms = 1) + atmvfi_refine_tail against the chain in fp64 with the MAIN product on hi(x), hi(w)
    and everything behind it (the W2 product on the activated tile, the tail) on full values: the existing read-out test's shapes and
    its tolerance -- what is left beside the model is the same fp32 accumulation and the same three-term W2 product."""
    cin, c, n, h, w = case
    g = torch.Generator().manual_seed(9100 + cin + h + w)
    rnd = lambda *s, scale=1.0: (torch.rand(*s, generator=g) * 2 - 1) * scale        # noqa: E731
    hip = f16_ops(dev)
    xp = hip_ops.Planes.alloc(n * h * w, cin, dev)
    hip.split_planes(rnd(n * h * w, cin, scale=1.5).to(dev), xp)
    xh = xp.to_rows().cpu()[0, :n * h * w, :cin].double().reshape(n, h, w, cin).permute(0, 3, 1, 2)       # the hi plane the kernel reads
    xfull = xp.to_float().cpu().double().reshape(n, h, w, cin).permute(0, 3, 1, 2)
    wa, ba, pa = rnd(c, cin, 3, 3, scale=1.0 / np.sqrt(9 * cin)), rnd(c, scale=0.2), 0.25 + rnd(c, scale=0.2)
    wb, bb, pb = rnd(3, c, 3, 3, scale=2.0 / np.sqrt(9 * c)), rnd(3, scale=0.2), 0.25 + rnd(3, scale=0.2)
    it = torch.rand(n, 3, h, w, generator=g)
    F = torch.nn.functional

    def chain(xin, wmain):
        r1 = F.prelu(F.conv2d(xin, wmain, ba.double(), padding=1), pa.double())
        r = F.prelu(F.conv2d(r1, wb.double(), bb.double(), padding=1), pb.double())
        return it.double() + (2.0 * torch.sigmoid(r) - 1.0)
    want = chain(xh, F16.hi(wa).double())
    want_x3 = chain(xfull, wa.double())
    pw = hip.pack_weight(GEMM_CONV, wa.to(dev))
    w2 = hip.pack_readout(wb.to(dev))
    contrib = torch.full((27, n * h * w), NAN, device=dev)
    hip.conv3x3_planes_readout(xp, n, h, w, pw, ba.to(dev), pa.to(dev), w2, contrib)
    s, cl = torch.full((n, 3, h, w), 7.0, device=dev), torch.full((n, 3, h, w), 7.0, device=dev)
    hip.refine_tail(contrib, bb.to(dev), pb.to(dev), it.to(dev), s, cl)
    torch.cuda.synchronize()
    assert not torch.isnan(contrib).any(), "a tap contribution was never written"
    err = (s.cpu().double() - want).abs().max().item()
    print(f"read-out f16 {case}: max|d| vs hi-only chain {err:.3e}; the two chains differ by {(want - want_x3).abs().max().item():.3e}")
    assert err <= 3e-5, f"max|d| {err:.3e}"
    assert torch.equal(cl, s.clamp(0, 1))
    # the unfused f16 launch of the same layer: same main product; the W2 product through the three-term fp32-input kernel
    r1g = torch.empty(n, h, w, c, device=dev)
    hip.conv3x3_planes(xp, n, h, w, pw, out=r1g, bias=ba.to(dev), prelu=pa.to(dev))
    rg = torch.empty(n, h, w, 4, device=dev)
    hip.conv(r1g, hip.pack_weight(GEMM_CONV, wb.to(dev)), rg[..., :3], 1, 1, 1, bb.to(dev), pb.to(dev))
    s2, cl2 = torch.empty_like(s), torch.empty_like(s)
    hip.final_residual(it.to(dev), rg[..., :3], s2, cl2)
    torch.cuda.synchronize()
    assert (s - s2).abs().max().item() <= 2e-5


# ------------------------------------------------------------------ the forward
def make_net(variant, dev, **kw):
    net = (pkg.NetworkLite if variant == "lite" else pkg.NetworkBase)(**kw)
    net.load_state_dict(pkg.synthetic_state_dict(variant, seed=1), strict=True)
    return net.to(dev).eval()


def same(x, y, what):
    assert set(x) == set(y) and len(x) == 10
    for k in x:
        assert Network._same_results(x[k], y[k]), f"{what}: {k} differs"


def keep(out):
    return {k: ([t.clone() for t in v] if isinstance(v, (list, tuple)) else v.clone()) for k, v in out.items()}


@pytest.mark.parametrize("variant,h,w", [("lite", 64, 96), ("base", 128, 192)])
def test_mode_reaches_the_forward_and_leaves_nothing_stale(variant, h, w, dev):
    torch.set_grad_enabled(False)
    net = make_net(variant, dev)
    a, b = (t.to(dev) for t in pairs.smooth_pair(1, h, w, seed=71))
    outs = []
    for mode in ("f16x3", "f16", "f16x3"):
        net.set_precision(mode)
        outs.append(keep(net(a, b)))
    torch.cuda.synchronize()
    same(outs[0], outs[2], f"{variant}: f16x3 before and after f16")
    assert not torch.equal(outs[0]["I_t"], outs[1]["I_t"]), "the f16 forward equals the f16x3 one: the mode did not reach the kernels"
    assert not torch.equal(outs[0]["opt_flow_0"], outs[1]["opt_flow_0"])
    assert all(torch.isfinite(outs[1][k]).all() for k in ("I_t", "opt_flow_0", "opt_flow_1", "occ_mask1"))
    d = (outs[0]["I_t"] - outs[1]["I_t"]).abs().max().item()
    print(f"{variant} {h}x{w}: max|I_t(f16) - I_t(f16x3)| = {d:.3e}")
    assert d < 0.1


def test_plans_pool_replicas_and_nx_in_f16(dev):
    torch.set_grad_enabled(False)
    h, w = 64, 96
    net = make_net("lite", dev)
    eager = make_net("lite", dev, selections={"use_plans": False})
    for m in (net, eager):
        m.set_precision("f16")
    a, b = (t.to(dev) for t in pairs.smooth_pair(1, h, w, seed=72))
    ref = keep(eager(a, b))
    net(*(t.to(dev) for t in pairs.smooth_pair(1, 64, 64, seed=73)))       # another shape first: the model's weights are packed
    net.enable_plans(True)                                                  # (and the counts start at zero)
    for call in range(1, 5):
        same(ref, net(a, b), f"forward {call}")
        st = net.plan_stats()["forward"]
        if call == 3:
            # the third forward of a shape is recorded, which includes one replay of the plan (into poisoned outputs) that has to
            # equal the direct launches bit for bit before the recording counts
            assert st == {"eager": 2, "recorded": 1, "replayed": 0, "refused": 0}, st
    assert net.plan_stats()["forward"] == {"eager": 2, "recorded": 1, "replayed": 1, "refused": 0}, net.plan_stats()
    assert all(sum(c.values()) == c["eager"] for c in eager.plan_stats().values())
    # the pooled forward, on a batch of two, against forward on the same batch; tokens of the other mode are stale
    fr = []
    for k in range(2):
        p0, p1 = pairs.smooth_pair(1, h, w, 60 + k)
        fr += [p0[0], p1[0]]
    frames = torch.stack(fr, 0).to(dev)
    pool = mf.FramePool(net, h, w, 4)
    for s in range(4):
        pool.put(s, frames[s])
    left, right = [0, 2], [1, 3]
    want = keep(net(frames[left].contiguous(), frames[right].contiguous()))
    for call in range(4):
        same(want, net.forward_pooled(pool, left, right), f"forward_pooled call {call}")
    net.set_precision("f16x3")
    want3 = keep(net(frames[left].contiguous(), frames[right].contiguous()))
    assert not torch.equal(want3["I_t"], want["I_t"])
    same(want3, net.forward_pooled(pool, left, right), "forward_pooled after the switch to f16x3 (nothing invalidated by hand)")
    net.set_precision("f16")
    same(want, net.forward_pooled(pool, left, right), "forward_pooled back in f16")
    pool.release()
    # a replica inherits the mode
    rep = net.replica()
    same(ref, rep(a, b), "replica")
    assert rep._ops_obj.plane_terms == 1
    # the N-x loop with and without the pool
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (h + 16, w + 16, 3), dtype=np.uint8)
    vid = [np.ascontiguousarray(base[k:k + h, 2 * k:2 * k + w]) for k in range(3)]
    runs = {p: list(host_io.interpolate_video_nx(iter(vid), net, factor=4, divisor=32, pool=p)) for p in (True, False)}
    assert len(runs[True]) == 2 * 4 + 1 == len(runs[False])
    for i, (x, y) in enumerate(zip(runs[True], runs[False])):
        assert np.array_equal(x, y), f"N-x frame {i}: pool=True and pool=False differ in f16"
    net.set_precision("f16x3")
    x3 = list(host_io.interpolate_video_nx(iter(vid), net, factor=4, divisor=32, pool=True))
    assert any(not np.array_equal(x, y) for x, y in zip(runs[True], x3)), "the N-x loop ignores the mode"
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end against the reference goldens
E2E_FIXTURES = ["base_64x64_g", "base_128x192_g", "base_160x96_nog_b2", "lite_64x64_g", "lite_128x192_g_b2", "lite_96x160_g_rand"]
E2E_KEYS = ("I_t", "opt_flow_0", "opt_flow_1", "occ_mask1")
# max|d| against the reference goldens in "f16" mode, measured on the MI355X (stress weights of the fixtures):
E2E_MEASURED = {
    # fixture:              (I_t,     opt_flow_0, opt_flow_1, occ_mask1)
    "base_64x64_g":         (2.69e-3, 2.58e-3, 2.36e-3, 4.15e-4),
    "base_128x192_g":       (3.03e-3, 2.69e-3, 2.56e-3, 4.08e-4),
    "base_160x96_nog_b2":   (1.56e-3, 3.02e-3, 2.69e-3, 4.53e-4),
    "lite_64x64_g":         (4.21e-3, 3.03e-3, 2.80e-3, 2.32e-4),
    "lite_128x192_g_b2":    (4.88e-3, 3.35e-3, 3.22e-3, 2.53e-4),
    "lite_96x160_g_rand":   (7.16e-3, 3.45e-3, 3.13e-3, 2.66e-4),
}
E2E_WORST = {"I_t": 7.159e-3, "opt_flow_0": 3.452e-3, "opt_flow_1": 3.219e-3, "occ_mask1": 4.531e-4}
# the asserted budget per output: 2x the largest value measured over the six fixtures (the kernels are deterministic: the factor is
# room for later changes of tile and split-K choices, not for noise)
E2E_BUDGET = {k: 2.0 * v for k, v in E2E_WORST.items()}
TOL, TOL_FLOW = 1e-3, 2e-3        # the default mode's budget (tests/test_gpu_e2e.py)


def test_f16_vs_reference_goldens(dev, weights):
    """max|d| of I_t, opt_flow_0/1 and occ_mask1 against the reference goldens, measured on the MI355X in "f16" mode:

    | fixture | I_t | opt_flow_0 (px) | opt_flow_1 (px) | occ_mask1 |
    |---|---|---|---|---|
    | base_64x64_g | 2.69e-3 | 2.58e-3 | 2.36e-3 | 4.15e-4 |
    | base_128x192_g | 3.03e-3 | 2.69e-3 | 2.56e-3 | 4.08e-4 |
    | base_160x96_nog_b2 | 1.56e-3 | 3.02e-3 | 2.69e-3 | 4.53e-4 |
    | lite_64x64_g | 4.21e-3 | 3.03e-3 | 2.80e-3 | 2.32e-4 |
    | lite_128x192_g_b2 | 4.88e-3 | 3.35e-3 | 3.22e-3 | 2.53e-4 |
    | lite_96x160_g_rand | 7.16e-3 | 3.45e-3 | 3.13e-3 | 2.66e-4 |
    | largest | 7.159e-3 | 3.452e-3 | 3.219e-3 | 4.531e-4 |
    | asserted budget (2x the largest) | 1.432e-2 | 6.90e-3 | 6.44e-3 | 9.06e-4 |

    (E2E_MEASURED / E2E_WORST above; README "Precision modes".  No value is above twice its row of the CPU estimate the mode was
    proposed with, which rounded more layers than the mode covers.)

    The f16x3 run of the same fixtures stays within the default 1e-3 (flows 2e-3)."""
    torch.set_grad_enabled(False)
    cases = {c["name"]: c for c in G.e2e_cases()}
    nets = {}
    worst = {k: 0.0 for k in E2E_KEYS}
    for name in E2E_FIXTURES:
        case = cases[name]
        assert case.get("motion_gain", 1.0) == 1.0
        gold = G.load_npz(name)
        im0, im1 = G.case_inputs(case)
        G.check_inputs_match(case, gold, im0, im1)
        v = case["variant"]
        if v not in nets:
            nets[v] = make_net(v, dev)
        net = nets[v]
        net.global_motion, net.ensemble_global_motion = case["global"], case["ensemble"]
        net.set_precision("f16x3")
        out = net(im0.to(dev), im1.to(dev))
        torch.cuda.synchronize()
        G.compare_e2e(out, gold, case["step"], TOL, TOL_FLOW)
        net.set_precision("f16")
        out = net(im0.to(dev), im1.to(dev))
        torch.cuda.synchronize()
        errs = G.compare_e2e(out, gold, case["step"], float("inf"), float("inf"))
        print(f"f16 e2e {name}: " + "  ".join(f"{k} {errs[k]:.2e}" for k in E2E_KEYS))
        for k in E2E_KEYS:
            assert np.isfinite(errs[k])
            worst[k] = max(worst[k], errs[k])
    print("f16 e2e worst: " + "  ".join(f"{k} {worst[k]:.2e}" for k in E2E_KEYS))
    for k in E2E_KEYS:
        assert worst[k] <= E2E_BUDGET[k], f"{k}: max|d| {worst[k]:.3e} over the fixtures > budget {E2E_BUDGET[k]:.3e}"
