"""CPU: the single-pass fp16 mode ("f16") -- the teeth of its GPU tests (the exact family separates the two modes both ways), the
ABI additions (the library loads without a GPU; every refusal happens before a launch) and the host logic that keys on the mode."""
import ctypes
import importlib
import os

import pytest
import torch

import f16_model as F16
import f16x3_model as M

pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")

SEPARATION_CASES = M.CASES_PLANES + M.CASES_CONV3 + [M.CASE_CONV3_PERSISTENT]


def _widest_tol(cfg, res):
    """The widest bound a GPU test applies to a launch of this configuration: the split-K one where the case is also run split."""
    return res.splitk_tol() if (cfg.get("splitk") or cfg.get("kparts")) else res.exact_tol()


@pytest.mark.parametrize("cfg", SEPARATION_CASES, ids=lambda c: c["id"] + f"_{c['seed']}")
def test_exact_family_separates_the_two_modes(cfg):
    """A kernel that silently ran the other mode cannot pass either GPU test: on every exact-family configuration the three-term model
    lies more than 10x outside the f16 model's bound somewhere, and the f16 model more than 10x outside the f16x3 bound."""
    o = M.case_operands(cfg)
    x3 = M.case_model(cfg, o)
    f16 = F16.case_model(cfg, o)
    dev = (x3.y - f16.y).abs()
    for name, res in (("f16", f16), ("f16x3", x3)):
        for tol_name, tol in (("exact", res.exact_tol()), ("widest", _widest_tol(cfg, res))):
            worst = (dev / tol.clamp_min(1e-300)).max().item()
            assert worst > 10, f"{cfg['id']}: the other mode is only {worst:.1f}x outside the {name} {tol_name} bound"


def test_f16_model_is_the_hi_only_product():
    """The helper against a naive fp64 sum of hi * hi, and its statistical operand: |hi(x)| |hi(w)|."""
    g = torch.Generator().manual_seed(11)
    x, w = M.wide(g, 5, 40, lo=-10.0, hi=5.0), M.edge(g, 6, 40)
    b = torch.randn(6, generator=g)
    xh, wh = M.split(x)[0].double(), M.split(w)[0].double()
    res = F16.linear(x, w, b)
    assert torch.equal(res.acc, xh @ wh.t()) and float(res.cor.abs().max()) == 0.0
    assert torch.equal(res.y, xh @ wh.t() + b.double())
    assert torch.equal(res.abs_xw, xh.abs() @ wh.abs().t())
    assert torch.equal(F16.hi(torch.tensor([7e4, -7e4, 1.0 + 2.0 ** -11, 2.0 ** -25])), torch.tensor([65504.0, -65504.0, 1.0, 0.0]))


# ------------------------------------------------------------------ ABI
P = 0x10000        # a fake, 16-byte aligned device address: every call below is refused before it would be touched


def _err(lib):
    return lib.atmvfi_last_error()


def test_abi_version_and_symbols():
    lib = hip_ops.load_library()
    assert (lib.atmvfi_version() >> 8) & 255 >= 24
    name = "atmvfi_conv3p"                                            # the 3x3 plane kernel and its read-out: `terms` of the block
    assert hasattr(lib, name) and name in hip_ops.SIGNATURES
    assert lib.atmvfi_plan_fn_id(name.encode()) >= 0                  # a launch entry point: a plan can hold it
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atmvfi.h")).read()
    assert "#define ATMVFI_PREC_F16   2" in hdr


def _gemm(**kw):
    p = hip_ops.GemmParams(mode=1, in_=P, in_ld=64, N=1, H=1, W=1, Cin=64, in_gstride=0, in_rpg=0, weight=P, Cout=32, kh=1, kw=1, stride=1,
                           pad=0, dil=1, Ho=1, Wo=1, M=128, out=P, out_ld=32, out_gstride=0, out_rpg=0, out_row_map=None, bias=None,
                           prelu=None, in_prelu=None, residual=None, res_ld=0)
    p.precision, p.weight_hi, p.weight_lo = 2, P, P
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _conv3p(**kw):
    """A valid plain block on fake addresses (1x16x16, Cin = Cout = 32, fp32 output); ``kw`` overrides fields."""
    p = hip_ops.Conv3pParams(in_hi=P, in_lo=P, in_rows=300, N=1, H=16, W=16, Cin=32, w_hi=P, w_lo=P, Cout=32, out=P, out_ld=32, terms=3)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _readout(**kw):
    """The same as a read-out block: no fp32 output, the W2 operand and 27 planes of 256 pixels."""
    return _conv3p(**{"out": None, "out_ld": 0, "readout_w": P, "readout": P, "readout_plane": 256, **kw})


def test_abi_refuses_f16_without_plane_input_and_bad_term_counts():
    lib = hip_ops.load_library()
    # ATMVFI_PREC_F16 on fp32 input: no such engine
    for fn in (lib.atmvfi_gemm, lib.atmvfi_linear):
        assert fn(ctypes.byref(_gemm()), None) == -1 and b"split-plane input" in _err(lib)
    # ... and on the reference schedule, which has no single-term instance
    assert lib.atmvfi_gemm(ctypes.byref(_gemm(in_=None, in_hi=P, in_lo=P, in_ld=128, tile_wn=-1)), None) == -1 and b"tile_wn = -1" in _err(lib)
    # an unknown precision value
    assert lib.atmvfi_gemm(ctypes.byref(_gemm(precision=3)), None) == -1 and b"bad precision" in _err(lib)
    # the 3x3 kernel and its read-out: a term count other than 3 or 1 (0, the value of a zeroed block, included)
    for terms in (2, 0, 4, -1):
        rc = lib.atmvfi_conv3p(ctypes.byref(_conv3p(terms=terms)), None)
        assert rc == -1 and b"conv3x3_planes: terms must be 3" in _err(lib), terms
        rc = lib.atmvfi_conv3p(ctypes.byref(_readout(terms=terms)), None)
        assert rc == -1 and b"conv3x3_planes_readout: terms must be 3" in _err(lib), terms
    # both term counts pass that check and reach the next one (still before any launch: in_rows must exceed N*H*W)
    for terms in (3, 1):
        rc = lib.atmvfi_conv3p(ctypes.byref(_conv3p(terms=terms, in_rows=256)), None)
        assert rc == -1 and b"in_rows" in _err(lib), terms


@pytest.mark.parametrize("block,wrong,text", [
    (_conv3p, dict(in_hi=None), b"conv3x3_planes: null pointer"),
    (_conv3p, dict(out_hi=P, out_lo=P, plane_rows=256, out_c0=4), b"multiple of 8"),
    (_conv3p, dict(wn=9), b"wn 0 (auto)"),
    (_conv3p, dict(out_hi2=P, out_lo2=P, plane_rows2=256), b"needs the first one"),
    (_readout, dict(out=P, out_ld=32), b"out, both plane sinks, workspace and wn must be unset"),
    (_readout, dict(readout_plane=255), b"contrib_plane"),
], ids=["first_pointer", "out_c0", "wn", "second_sink_alone", "readout_with_out", "readout_plane"])
def test_conv3p_block_layout_matches_the_header(block, wrong, text):
    """hip_ops.Conv3pParams against the C struct: one wrong field at a time on an otherwise valid block, each refused (before any launch)
    with the message of exactly that field -- a ctypes field that sits elsewhere than its C counterpart makes the launcher read another
    value there and report something else (or nothing)."""
    lib = hip_ops.load_library()
    rc = lib.atmvfi_conv3p(ctypes.byref(block(**wrong)), None)
    assert rc == -1 and text in _err(lib), _err(lib)


# ------------------------------------------------------------------ host logic
class _Ops:
    """What Network reads of an op backend when it builds its keys."""
    precision = "f16x3"
    plane_terms = 3
    attention_f16x3 = True
    warp_tiles = True
    conv3_instance = None
    gemm_tile_wn = 0


def test_set_precision_accepts_f16_and_rejects_unknown_names():
    net = pkg.NetworkLite()
    assert net._precision == "f16x3"
    for name in ("f16", "f32", "f16x3", "f16"):
        net.set_precision(name)
        assert net._precision == name and not net._checked
    for bad in ("fp16", "f16-checked", "bf16", "", "F16"):
        with pytest.raises(ValueError):
            net.set_precision(bad)
    assert net._precision == "f16"
    with pytest.raises(RuntimeError):
        net.range_violations()                     # no checked twin: as in "f16x3"


def test_mode_reaches_the_backend_and_the_keys():
    net = pkg.NetworkLite()
    ops = _Ops()
    net._ops_obj = ops
    keys = {}
    for name in ("f16x3", "f16", "f32"):
        net.set_precision(name)
        assert ops.precision == ("f32" if name == "f32" else "f16x3")          # the plane path (split-plane engines, layouts) stays on in "f16"
        assert ops.plane_terms == (1 if name == "f16" else 3)
        keys[name] = (net._mode_fields(ops), net._pool_validity_key(ops, True, None))
    assert len({k[0] for k in keys.values()}) == 3 and len({k[1] for k in keys.values()}) == 3
    net.set_precision("f16x3")
    assert (net._mode_fields(ops), net._pool_validity_key(ops, True, None)) == keys["f16x3"]


def test_replica_carries_the_mode():
    net = pkg.NetworkLite()
    net.set_precision("f16")
    rep = net.replica()
    assert rep._precision == "f16" and rep._ops_obj is None
    ops = _Ops()
    rep._apply_precision(ops)
    assert ops.precision == "f16x3" and ops.plane_terms == 1
    net.set_precision("f16x3")
    assert rep._precision == "f16"                 # a replica owns its mode from then on, like its plans


def test_hip_ops_refuses_unknown_term_counts():
    class Fake(hip_ops.HipOps):
        def __init__(self):
            self.plane_terms = 2
    p = _gemm(precision=1, in_hi=P, in_lo=P)
    with pytest.raises(ValueError):
        Fake()._plane_prec(p)
    f = Fake()
    f.plane_terms = 1
    f._plane_prec(p)
    assert p.precision == 2
    q = _gemm(precision=1)                          # fp32 input: stays f16x3 (the fp32-input engines have no single-pass instance)
    f._plane_prec(q)
    assert q.precision == 1
