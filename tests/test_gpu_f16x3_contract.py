"""GPU: every f16x3 contraction engine held to its ~22-bit contract against the exact fp64 model of tests/f16x3_model.py.

Exact family: operands on a dyadic grid where no fp32 accumulation can round (the certificate is checked on the CPU, see
test_f16x3_model_cpu.py, for every configuration below), so the kernel must equal the model up to the epilogue's final roundings.
An engine that kept 4 bits of lo', dropped a cross term or dropped lo' on its last k-chunk misses that bound by more than 10x.
Wide / edge / cancel families: the statistical rule 8 x max(fp32-on-CPU error, 2^-24 sum |x||w|) against the model, which
saturates like the library.  Plane sinks: bit for bit the split of their own fp32 result, driven to the fp16 boundaries.
Checked build: the range counter fires exactly for |x| > 65488."""
import importlib
import os
import zlib

import numpy as np
import pytest
import torch

import f16x3_model as M

pytestmark = pytest.mark.gpu

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
windows = importlib.import_module("atm-vfi_amd.windows")
GEMM_CONV, GEMM_LINEAR, GEMM_DECONV = 0, 1, 2
REF_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lib", "libatmvfi_hip_ref.so")
# plane-input engines: -1 reference schedule (gemm_split.hip, diagnostic library), -3 gemm_pp, -2 / -4 gemm_duo 128 / 64 columns, 0 auto
ENGINES = [-1, -3, -2, -4, 0]
ENGINE_IDS = ["split", "pp", "duo", "duo64", "auto"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def ops_for(dev, engine=0):
    h = hip_ops.HipOps(dev, lib_path=REF_LIB) if engine == -1 else hip_ops.HipOps(dev)
    h.gemm_tile_wn = engine
    return h


def r4(c):
    return (c + 3) // 4 * 4


def padded_nhwc(x, dev):
    """[N,H,W,C] fp32 on the device as a channel view of a buffer whose pixel stride is a multiple of 4."""
    c = x.shape[-1]
    buf = torch.zeros(*x.shape[:-1], r4(c), device=dev)
    buf[..., :c] = x.to(dev)
    return buf[..., :c]


def out_view(shape, dev, fill=7.0):
    c = shape[-1]
    return torch.full((*shape[:-1], r4(c)), fill, device=dev)[..., :c]


def check_exact(got, res: M.Result, what, splitk=False):
    got = got.detach().double().cpu()
    tol = res.splitk_tol() if splitk else res.exact_tol()
    err = (got - res.y).abs()
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off the exact model, worst {float((err / tol.clamp_min(1e-300)).max()):.2f}x the bound"


def check_stat(got, y_model, abs_xw, cpu32_err, what):
    got = got.detach().double().cpu()
    bound = M.stat_bound(abs_xw, cpu32_err)
    err = (got - y_model).abs()
    assert torch.isfinite(got).all(), what
    assert (err <= bound).all(), f"{what}: worst {float((err / bound).max()):.2f}x the statistical bound"


def planes_of(x2d, hip, dev):
    """fp32 rows [M, C] -> Planes (split on the device by atmvfi_split_planes: tested bit for bit below)."""
    m, c = x2d.shape
    p = hip_ops.Planes.alloc(m, c, dev)
    hip.split_planes(padded_nhwc(x2d, dev), p)
    return p


# ------------------------------------------------------------------ exact family: fp32-input f16x3 GEMM (gemm_f16x3.hip)
@pytest.mark.parametrize("cfg", M.CASES_GEMM32, ids=lambda c: c["id"])
def test_exact_gemm_fp32_input(cfg, dev):
    hip = hip_ops.HipOps(dev)
    x, w, res = M.build_case(cfg)
    p = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in cfg["dev_args"](x, w).items()}
    for wn in cfg.get("wns", [0]):
        hip.gemm_tile_wn = wn
        kind = cfg["kind"]
        pw = hip.pack_weight({"linear": GEMM_LINEAR, "conv": GEMM_CONV, "deconv": GEMM_DECONV}[kind], w.to(dev))
        if kind == "linear":
            out = out_view((cfg["rows_out"], w.shape[0]), dev)
            hip.linear(padded_nhwc(x, dev), pw, out, bias=p.get("bias"), residual=p.get("residual"), out_row_map=p.get("row_map"))
            torch.cuda.synchronize()
            got = M.gather_rows(out.cpu(), cfg.get("row_map_cpu"))
        elif kind == "conv":
            out = out_view(tuple(res.y.shape), dev)
            hip.conv(padded_nhwc(x, dev), pw, out, cfg["stride"], cfg["pad"], cfg["dil"], p.get("bias"), p.get("slope"),
                     hip.pad_channels(p["in_prelu"]) if "in_prelu" in p else None)
            torch.cuda.synchronize()
            got = out
        else:
            out = out_view(tuple(res.y.shape), dev)
            hip.deconv(padded_nhwc(x, dev), pw, out, bias=p.get("bias"), prelu=p.get("slope"),
                       in_prelu=hip.pad_channels(p["in_prelu"]) if "in_prelu" in p else None)
            torch.cuda.synchronize()
            got = out
        check_exact(got, res, f"{cfg['id']} wn={wn}")


# ------------------------------------------------------------------ exact family: plane-input engines (gemm_split / pp / duo)
@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("cfg", M.CASES_PLANES, ids=lambda c: c["id"])
def test_exact_gemm_planes(cfg, engine, dev):
    hip = ops_for(dev, engine)
    x, w, res = M.build_case(cfg)
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
            xp = planes_of(x, hip, dev)
            out = out_view((cfg["rows_out"], w.shape[0]), dev)
            hip.linear(xp, pw, out, bias=p.get("bias"), residual=p.get("residual"), out_row_map=p.get("row_map"))
            torch.cuda.synchronize()
            got = M.gather_rows(out.cpu(), cfg.get("row_map_cpu"))
        elif kind == "conv":
            n, h, wd, cin = x.shape
            rows = x.reshape(-1, cin)
            if cfg.get("two_sources"):
                c1 = 32 * cfg["two_sources"]
                xa, xb = planes_of(rows[:, :c1], hip, dev), planes_of(rows[:, c1:], hip, dev)
                out = out_view(tuple(res.y.shape), dev)
                hip.conv_planes(xa, n, h, wd, pw, out=out, stride=cfg["stride"], pad=cfg["pad"], dil=cfg["dil"], bias=p.get("bias"),
                                prelu=p.get("slope"), x2=xb, split_chunks=cfg["two_sources"])
            else:
                xp = planes_of(rows, hip, dev)
                out = out_view(tuple(res.y.shape), dev)
                hip.conv_planes(xp, n, h, wd, pw, out=out, stride=cfg["stride"], pad=cfg["pad"], dil=cfg["dil"], bias=p.get("bias"),
                                prelu=p.get("slope"))
            torch.cuda.synchronize()
            got = out
        else:
            n, h, wd, cin = x.shape
            xp = planes_of(x.reshape(-1, cin), hip, dev)
            out = out_view(tuple(res.y.shape), dev)
            hip.deconv(None, pw, out, bias=p.get("bias"), prelu=p.get("slope"), planes=xp, in_shape=(n, h, wd, cin))
            torch.cuda.synchronize()
            got = out
        if splitk:
            assert used, f"{cfg['id']}: the launcher did not ask for split-K scratch: the case tests nothing"
        check_exact(got, res, f"{cfg['id']} engine={engine} splitk={splitk}", splitk=splitk)


# ------------------------------------------------------------------ exact family: the 3x3 kernels
@pytest.mark.parametrize("schedule", [0, 1], ids=["row", "half"])
@pytest.mark.parametrize("cfg", M.CASES_CONV3, ids=lambda c: c["id"])
def test_exact_conv3x3_f16x3(cfg, schedule, dev):
    hip = hip_ops.HipOps(dev)
    x, w, res = M.build_case(cfg)
    p = {k: v.to(dev) for k, v in cfg["dev_args"](x, w).items()}
    pw = hip.pack_weight(GEMM_CONV, w.to(dev))
    xg = padded_nhwc(x, dev)
    for wn in range(1, 9):
        hip.conv3_instance = (schedule, wn)
        out = out_view(tuple(res.y.shape), dev)
        hip.conv(xg, pw, out, 1, 1, 1, p.get("bias"), p.get("slope"))
        torch.cuda.synchronize()
        check_exact(out, res, f"{cfg['id']} schedule={schedule} wn={wn}")


@pytest.mark.parametrize("cfg", M.CASES_CONV3, ids=lambda c: c["id"])
def test_exact_conv3x3_planes(cfg, dev):
    """conv3x3_planes (fp32 out + plane sink), planes2 (second raw sink) and planes3 (split-K workspace) for every tile width."""
    hip = hip_ops.HipOps(dev)
    x, w, res = M.build_case(cfg)
    p = {k: v.to(dev) for k, v in cfg["dev_args"](x, w).items()}
    pw = hip.pack_weight(GEMM_CONV, w.to(dev))
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    xp = planes_of(x.reshape(-1, cin), hip, dev)
    for wn in range(1, 9):
        out = out_view(tuple(res.y.shape), dev)
        s1, s2 = hip_ops.Planes.alloc(n * h * wd, cout, dev), hip_ops.Planes.alloc(n * h * wd, cout, dev)
        hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=p.get("bias"), prelu=p.get("slope"), planes=s1, planes2=s2, wn=wn)
        torch.cuda.synchronize()
        check_exact(out, res, f"{cfg['id']} wn={wn}")
        M.assert_split_of(s1, out, f"{cfg['id']} wn={wn} sink")
        M.assert_split_of(s2, out, f"{cfg['id']} wn={wn} sink2")
    if cfg.get("kparts"):
        nws = hip.conv3x3_workspace_floats(n, h, wd, cin, cout)
        assert nws > 0, f"{cfg['id']}: meant for split-K but the launcher would not split it"
        out = out_view(tuple(res.y.shape), dev)
        s1 = hip_ops.Planes.alloc(n * h * wd, cout, dev)
        hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=p.get("bias"), prelu=p.get("slope"), planes=s1,
                           workspace=torch.empty(nws, device=dev))
        torch.cuda.synchronize()
        check_exact(out, res, f"{cfg['id']} split-K", splitk=True)
        M.assert_split_of(s1, out, f"{cfg['id']} split-K sink")


def test_exact_conv3x3_planes_persistent_grid(dev):
    """More than 256 output tiles of 16 x 16 pixels: the persistent grid walks several tiles per workgroup."""
    cfg = M.CASE_CONV3_PERSISTENT
    hip = hip_ops.HipOps(dev)
    x, w, res = M.build_case(cfg)
    p = {k: v.to(dev) for k, v in cfg["dev_args"](x, w).items()}
    pw = hip.pack_weight(GEMM_CONV, w.to(dev))
    n, h, wd, cin = x.shape
    xp = planes_of(x.reshape(-1, cin), hip, dev)
    for wn in (0, 2):
        out = out_view(tuple(res.y.shape), dev)
        hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=p["bias"], prelu=p["slope"], wn=wn)
        torch.cuda.synchronize()
        check_exact(out, res, f"persistent wn={wn}")
    out = out_view(tuple(res.y.shape), dev)
    hip.conv(padded_nhwc(x, dev), pw, out, 1, 1, 1, p["bias"], p["slope"])
    torch.cuda.synchronize()
    check_exact(out, res, "persistent conv3x3_f16x3")


# ------------------------------------------------------------------ head1x1_planes (fp32 FMAs on the split activations)
@pytest.mark.parametrize("family", ["exact", "wide", "edge"])
def test_head1x1_planes_model(family, dev):
    hip = hip_ops.HipOps(dev)
    g = torch.Generator().manual_seed(515)
    n, h, wd, cin, cout = 1, 17, 23, 576, 5
    x = {"exact": M.exact, "wide": M.wide, "edge": M.edge}[family](g, n * h * wd, cin)
    w = M.exact(g, cout, cin, 1, 1) if family == "exact" else (torch.rand(cout, cin, 1, 1, generator=g) * 2 - 1) / cin ** 0.5
    b = M.exact_bias(g, cout)
    pw = hip.pack_weight(GEMM_CONV, w.to(dev))
    xp = planes_of(x, hip, dev)
    out = torch.full((n, h, wd, 8), 3.0, device=dev)
    hip.head1x1_planes(xp, n, h, wd, pw, out[..., :cout], bias=b.to(dev))
    torch.cuda.synchronize()
    y = M.head1x1(x, w.reshape(cout, cin), b).reshape(n, h, wd, cout)
    xd = M.dequant(x)
    cpu32 = (xd.float() @ w.reshape(cout, cin).t() + b).double().reshape(n, h, wd, cout)
    absxw = (xd.abs() @ w.reshape(cout, cin).double().abs().t()).reshape(n, h, wd, cout)
    # not certifiable: the product of the fp32 weight and the 21-bit activation is rounded by every FMA; statistical rule
    check_stat(out[..., :cout], y, absxw, (cpu32 - y).abs().max().item(), f"head1x1 {family}")
    assert torch.all(out[..., cout:] == 3.0)


# ------------------------------------------------------------------ wide / edge / cancel families
@pytest.mark.parametrize("family", ["wide", "edge", "cancel"])
@pytest.mark.parametrize("path", ["conv3x3_f16x3", "conv3x3_planes", "conv_gemm32", "linear32", "linear_planes", "deconv_planes"])
def test_statistical_families(path, family, dev):
    hip = hip_ops.HipOps(dev)
    g = torch.Generator().manual_seed(zlib.crc32(f"{path}/{family}".encode()))
    gen = {"wide": M.wide, "edge": M.edge, "cancel": M.wide}[family]
    if path.startswith("conv"):
        n, h, wd, cin, cout = 2, 13, 19, 64, 40
        x = gen(g, n, h, wd, cin)
        w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (9 * cin) ** 0.5
        if family == "wide":
            w = M.wide(g, cout, cin, 3, 3, lo=-20.0, hi=2.0)
        if family == "cancel":
            x, w = M.cancel(g, x, w, 3, 1)
        b = (torch.rand(cout, generator=g) * 2 - 1) * 0.2
        stride = 2 if path == "conv_gemm32" else 1
        res = M.conv(x, w, b, None, stride=stride)
        xd, wdq = M.dequant(x), M.dequant(w)
        cpu32 = torch.nn.functional.conv2d(xd.float().permute(0, 3, 1, 2), wdq.float(), b, stride=stride, padding=1).permute(0, 2, 3, 1)
        pw = hip.pack_weight(GEMM_CONV, w.to(dev))
        out = out_view(tuple(res.y.shape), dev)
        if path == "conv3x3_planes":
            hip.conv3x3_planes(planes_of(x.reshape(-1, cin), hip, dev), n, h, wd, pw, out=out, bias=b.to(dev))
        else:
            hip.conv(padded_nhwc(x, dev), pw, out, stride, 1, 1, b.to(dev), None)
    elif path.startswith("linear"):
        m, k, nout = 1000, 200, 96
        x = gen(g, m, k)
        w = (torch.rand(nout, k, generator=g) * 2 - 1) / k ** 0.5
        if family == "wide":
            w = M.wide(g, nout, k, lo=-20.0, hi=2.0)
        if family == "cancel":
            x, w = M.cancel(g, x, w, 1, 1)
        b = (torch.rand(nout, generator=g) * 2 - 1) * 0.2
        res = M.linear(x, w, b)
        cpu32 = M.dequant(x).float() @ M.dequant(w).float().t() + b
        pw = hip.pack_weight(GEMM_LINEAR, w.to(dev))
        out = out_view((m, nout), dev)
        hip.linear(planes_of(x, hip, dev) if path == "linear_planes" else padded_nhwc(x, dev), pw, out, bias=b.to(dev))
    else:
        n, h, wd, cin, cout = 2, 9, 14, 96, 40
        x = gen(g, n, h, wd, cin)
        w = (torch.rand(cin, cout, 2, 2, generator=g) * 2 - 1) / cin ** 0.5
        if family == "wide":
            w = M.wide(g, cin, cout, 2, 2, lo=-20.0, hi=2.0)
        if family == "cancel":
            x, w = M.cancel(g, x, w, 3, 0)
        b = (torch.rand(cout, generator=g) * 2 - 1) * 0.2
        res = M.deconv2x2(x, w, b)
        cpu32 = torch.nn.functional.conv_transpose2d(M.dequant(x).float().permute(0, 3, 1, 2), M.dequant(w).float(), b, stride=2).permute(0, 2, 3, 1)
        pw = hip.pack_weight(GEMM_DECONV, w.to(dev))
        out = out_view(tuple(res.y.shape), dev)
        hip.deconv(None, pw, out, bias=b.to(dev), planes=planes_of(x.reshape(-1, cin), hip, dev), in_shape=(n, h, wd, cin))
    torch.cuda.synchronize()
    check_stat(out, res.y, res.abs_xw, (cpu32.double() - res.y).abs().max().item(), f"{path} {family}")


ATTN_CASES = [
    # ws, hd, frames, h, w, shift, cross, logit scale
    (8, 48, 2, 12, 20, 4, True, 60.0),       # padded + shifted windows with region labels, cross-frame
    (8, 32, 2, 16, 16, 0, False, 60.0),
    (12, 44, 4, 4, 4, 6, True, 20.0),        # 4x4 maps padded to one 12x12 window
    (7, 16, 2, 14, 14, 3, True, 60.0),
]


@pytest.mark.parametrize("family", ["wide", "edge"])
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: f"ws{c[0]}_hd{c[1]}_{c[3]}x{c[4]}_s{c[5]}")
def test_window_attention_f16x3_model(case, family, dev):
    """window_attention_f16x3 against the model (Q, K, P and V split where attention.hip splits them) with logits up to +-60, and no
    worse than 4x the exact-fp32 kernel against fp64 on the same inputs."""
    ws, hd, frames, h, w, shift, cross, lscale = case
    heads = 8
    c = heads * hd
    g = torch.Generator().manual_seed(ws * 1000 + hd + (family == "edge"))
    geo = windows.build_window_geometry(frames, h, w, ws, shift)
    bw, n = frames * geo.n_windows, ws * ws
    qkv = (torch.rand(bw * n, 3 * c, generator=g) * 2 - 1)
    # q . k / sqrt(hd) reaches ~ +-lscale: q, k of magnitude sqrt(lscale) (1/sqrt(hd) and the sum over hd cancel on average)
    qkv[:, :2 * c] *= (lscale * 3.0 / hd ** 0.5) ** 0.5
    if family == "wide":
        qkv[:, 2 * c:] = M.wide(g, bw * n, c, lo=-20.0, hi=8.0)
    else:
        qkv[:, 2 * c:] = M.edge(g, bw * n, c, frac=0.1)
    kv_shift = bw // 2 if cross else 0
    lab = None if geo.labels is None else geo.labels
    outs = {}
    for eng in ("f16x3", "f32"):
        hip = hip_ops.HipOps(dev)
        hip.attention_f16x3 = eng == "f16x3"
        o = torch.full((bw * n, c), 9.0, device=dev)
        hip.window_attention(qkv.to(dev), o, None, None if lab is None else lab.to(dev), bw, geo.n_windows, ws, heads, hd, kv_shift)
        torch.cuda.synchronize()
        outs[eng] = o.cpu().double()
    y, _, absr = M.attention(qkv, lab, bw, geo.n_windows, ws, heads, hd, kv_shift)
    # fp64 reference on the fp32 inputs (no split) for the comparison with the exact-fp32 kernel
    t = qkv.double().reshape(bw, n, 3, heads, hd)
    src = (torch.arange(bw) + kv_shift) % bw
    q, k, v = t[:, :, 0].permute(0, 2, 1, 3), t[src, :, 1].permute(0, 2, 1, 3), t[src, :, 2].permute(0, 2, 1, 3)
    s = (q @ k.transpose(-2, -1)) / hd ** 0.5
    if lab is not None:
        mask = (lab[:, :, None] != lab[:, None, :]).double() * -100.0
        s = (s.reshape(bw // geo.n_windows, geo.n_windows, heads, n, n) + mask[None, :, None]).reshape(bw, heads, n, n)
    assert s.abs().max().item() > 0.5 * lscale, "the logits do not reach the intended range"
    ref = (s.softmax(-1) @ v).transpose(1, 2).reshape(bw * n, c)
    assert torch.isfinite(outs["f16x3"]).all()
    err16 = (outs["f16x3"] - y).abs()
    bound = 8 * torch.clamp(M.EPS32 * absr, min=(outs["f32"] - ref).abs().max().item())
    assert (err16 <= bound).all(), f"f16x3 attention vs model: worst {float((err16 / bound).max()):.2f}x"
    if family == "wide":
        # (the edge family's V saturates beyond 65504 by contract: there only the model, which saturates too, is the yardstick)
        e16, e32 = (outs["f16x3"] - ref).abs().max().item(), (outs["f32"] - ref).abs().max().item()
        assert e16 <= 4 * e32, (e16, e32)


# ------------------------------------------------------------------ plane sinks: bit for bit the split of their own fp32 result
SINK_SCALES = [65488.0, 65487.99, 65504.0, 65519.99, 65520.0, 7e4, 2.0 ** -14, 2.0 ** -20]


def sink_bias(g, cout, target):
    """Bias that drives every output near +-target (random sign) on top of O(1) sums; a few channels right at it."""
    s = torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1
    return (s * target).float()


@pytest.mark.parametrize("target", SINK_SCALES)
def test_plane_sinks_at_fp16_edges(target, dev):
    """Every producer's plane sink equals split() of its own fp32 output bit for bit with outputs at the fp16 boundaries: the
    gemm_split / pp / duo sinks (and the split-K reduce's), both conv3x3 sinks (and the split-K reduce's), layernorm, split_planes
    (with its PReLU form) and split_planes_at."""
    g = torch.Generator().manual_seed(int(target * 7) % 9973)
    small = target < 1
    xs = 1e-3 * target if small else 1.0
    # GEMM engines on plane input: linear with a plane sink at a channel offset
    m, k, nout = 700, 96, 72
    x = (torch.rand(m, k, generator=g) * 2 - 1) * xs
    w = (torch.rand(nout, k, generator=g) * 2 - 1) / k ** 0.5
    b = sink_bias(g, nout, target)
    for engine in ENGINES:
        hip = ops_for(dev, engine)
        pw = hip.pack_weight(GEMM_LINEAR, w.to(dev))
        out = out_view((m, nout), dev)
        sink = hip_ops.Planes.alloc(m, 8 + nout, dev)
        hip.linear(planes_of(x, hip, dev), pw, out, bias=b.to(dev), sink=sink, sink_c0=8)
        torch.cuda.synchronize()
        M.assert_split_of(sink, out, f"linear sink engine={engine} target={target}", c0=8)
    # split-K reduce's sink (deconv, long K)
    hip = hip_ops.HipOps(dev)
    hip.gemm_workspace = lambda n: torch.empty(n, device=dev)
    n_, h_, w_, cin, cout = 1, 32, 32, 1024, 61
    xd = (torch.rand(n_ * h_ * w_, cin, generator=g) * 2 - 1) * xs
    wdc = (torch.rand(cin, cout, 2, 2, generator=g) * 2 - 1) / cin ** 0.5
    pw = hip.pack_weight(GEMM_DECONV, wdc.to(dev))
    sink = hip_ops.Planes.alloc(n_ * 4 * h_ * w_, cout, dev)
    out = out_view((n_, 2 * h_, 2 * w_, cout), dev)
    hip.deconv(None, pw, out, bias=sink_bias(g, cout, target).to(dev), planes=planes_of(xd, hip, dev), sink=sink, in_shape=(n_, h_, w_, cin))
    torch.cuda.synchronize()
    M.assert_split_of(sink, out.reshape(-1, cout), f"deconv split-K sink target={target}")
    # the two 3x3 kernels' sinks, the split-K reduce's, with the plane PReLU of the fp32-input kernel
    hip = hip_ops.HipOps(dev)
    n, h, wd, cin, cout = 1, 16, 16, 712, 48
    x3 = (torch.rand(n, h, wd, cin, generator=g) * 2 - 1) * xs
    w3 = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (9 * cin) ** 0.5
    b3 = sink_bias(g, cout, target).to(dev)
    pw = hip.pack_weight(GEMM_CONV, w3.to(dev))
    out = out_view((n, h, wd, cout), dev)
    sink = hip_ops.Planes.alloc(n * h * wd, cout, dev)
    pp = hip.pad_channels(torch.full((cout,), 0.5, device=dev))
    hip.conv(padded_nhwc(x3, dev), pw, out, 1, 1, 1, b3, None, planes=sink, planes_prelu=pp)
    torch.cuda.synchronize()
    o = out.reshape(-1, cout).cpu()
    M.assert_split_of(sink, torch.where(o > 0, o, o * 0.5), f"conv3x3_f16x3 sink target={target}")
    xp = planes_of(x3.reshape(-1, cin), hip, dev)
    nws = hip.conv3x3_workspace_floats(n, h, wd, cin, cout)
    assert nws > 0
    for ws in (None, torch.empty(nws, device=dev)):
        out = out_view((n, h, wd, cout), dev)
        s1, s2 = hip_ops.Planes.alloc(n * h * wd, 8 + cout, dev), hip_ops.Planes.alloc(n * h * wd, cout, dev)
        hip.conv3x3_planes(xp, n, h, wd, pw, out=out, bias=b3, planes=s1, planes_c0=8, planes2=s2, workspace=ws)
        torch.cuda.synchronize()
        M.assert_split_of(s1, out.reshape(-1, cout), f"conv3x3_planes sink split-K={ws is not None} target={target}", c0=8)
        M.assert_split_of(s2, out.reshape(-1, cout), f"conv3x3_planes sink2 split-K={ws is not None} target={target}")
    # layernorm: beta at the target
    C = 96
    src = (torch.rand(300, C, generator=g) * 2 - 1).to(dev)
    gamma = (torch.rand(C, generator=g) * 0.01).to(dev)
    beta = sink_bias(g, C, target).to(dev)
    of = torch.empty(300, C, device=dev)
    pl = hip_ops.Planes.alloc(300, C, dev)
    hip.layernorm(src, of, gamma, beta, planes=pl)
    torch.cuda.synchronize()
    M.assert_split_of(pl, of, f"layernorm sink target={target}")
    # split_planes (PReLU form) and split_planes_at
    v = ((torch.rand(200, 40, generator=g) * 2 - 1) * 0.01 + sink_bias(g, 40, target)).to(dev)
    sl = torch.full((40,), -1.0, device=dev)        # PReLU with slope -1: |x|
    pl = hip_ops.Planes.alloc(200, 40, dev)
    hip.split_planes(padded_nhwc(v, dev), pl, prelu=sl)
    pa = hip_ops.Planes.alloc(200, 8 + 40, dev)
    hip.split_planes(padded_nhwc(v, dev), pa, c0=8)
    torch.cuda.synchronize()
    M.assert_split_of(pl, v.abs().cpu(), f"split_planes prelu target={target}")
    M.assert_split_of(pa, v.cpu(), f"split_planes_at target={target}", c0=8)


# ------------------------------------------------------------------ checked build: the counter fires exactly for |x| > 65488
@pytest.mark.parametrize("value,fires", [(65504.0, True), (65488.01, True), (7e4, True), (65488.0, False), (65487.99, False),
                                         (-65488.0, False), (-65504.0, True)])
def test_checked_build_threshold(value, fires, dev):
    hip = hip_ops.HipOps(dev, checked=True)
    word = hip.range_word

    def count(fn):
        word.zero_()
        hip.begin_forward()
        fn()
        torch.cuda.synchronize()
        return int(word.item())
    x = torch.zeros(64, 64)
    x[5, 7] = value
    xg = x.to(dev)
    sites = {}
    # atmvfi_split_planes
    sites["split_planes"] = count(lambda: hip.split_planes(xg, hip_ops.Planes.alloc(64, 64, dev)))
    # in-kernel operand split of the fp32-input GEMM and of the fp32-input 3x3 kernel
    wl = hip.pack_weight(GEMM_LINEAR, torch.full((32, 64), 2.0 ** -10, device=dev))
    sites["gemm_f16x3"] = count(lambda: hip.linear(xg, wl, torch.empty(64, 32, device=dev)))
    w3 = hip.pack_weight(GEMM_CONV, torch.full((32, 64, 3, 3), 2.0 ** -12, device=dev))
    x4 = xg.reshape(1, 8, 8, 64)
    sites["conv3x3_f16x3"] = count(lambda: hip.conv(x4, w3, torch.empty(1, 8, 8, 32, device=dev), 1, 1, 1, None, None))
    # plane sinks: the output itself at the value (bias), zero input
    zero = hip_ops.Planes.alloc(64, 64, dev)
    bias = torch.zeros(32, device=dev)
    bias[3] = value
    sites["gemm_sink"] = count(lambda: hip.linear(zero, wl, torch.empty(64, 32, device=dev), bias=bias,
                                                  sink=hip_ops.Planes.alloc(64, 32, dev)))
    sites["conv3x3_planes_sink"] = count(lambda: hip.conv3x3_planes(zero, 1, 8, 8, w3, out=torch.empty(1, 8, 8, 32, device=dev), bias=bias,
                                                                    planes=hip_ops.Planes.alloc(64, 32, dev)))
    beta = torch.zeros(64, device=dev)
    beta[9] = value
    sites["layernorm_sink"] = count(lambda: hip.layernorm(xg * 0, None, torch.ones(64, device=dev), beta, planes=hip_ops.Planes.alloc(64, 64, dev)))
    for site, n in sites.items():
        assert (n > 0) == fires, f"{site}: count {n} for an activation at {value}"
