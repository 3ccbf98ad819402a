"""Exact fp64 model of the single-pass fp16 mode ("f16": Network.set_precision, ATMVFI_PREC_F16, terms = 1 of
atmvfi_conv3p with terms = 1) -- CPU only, test infrastructure only.

A product of the mode is hi(x) * hi(w) alone, hi = the high half of the library's split (fp16, round to nearest even, saturating),
accumulated in fp32 into the one accumulator ``acc``; the epilogue (bias, PReLU, residual, split-K fold and reduce) is the f16x3
kernels' own.  That IS the f16x3 model (tests/f16x3_model.py) applied to operands whose lo' half is zero, so nothing is restated
here: ``hi()`` replaces both operands by their high halves as fp32 values, and ``M.linear`` / ``M.conv`` / ``M.deconv2x2`` /
``M.case_model`` give ``acc`` (their ``cor`` is exactly 0), ``kparts`` and the epilogue.  The bounds are the model's own:
``exact_tol()`` / ``splitk_tol()`` of that result for the exact family, ``M.stat_bound`` with ``abs_xw`` over the hi operands for the
wide / edge / cancel families.
"""
from __future__ import annotations

import torch

import f16x3_model as M


def hi(x) -> torch.Tensor:
    """The high half of the split of fp32 values, as fp32: what the mode contracts with."""
    return M.split(x)[0].float()


def hi_operands(o: dict) -> dict:
    """The operands of an exact-family configuration (``M.case_operands``) with x and w replaced by their high halves."""
    o2 = dict(o)
    o2["x"], o2["w"] = hi(o["x"]), hi(o["w"])
    return o2


def case_model(cfg, o: dict) -> M.Result:
    """The f16 model of a configuration on its ORIGINAL operands ``o``."""
    res = M.case_model(cfg, hi_operands(o))
    assert float(res.cor.abs().max()) == 0.0
    return res


def linear(x, w, bias=None, residual=None, kparts=False) -> M.Result:
    return M.linear(hi(x), hi(w), bias, residual, kparts=kparts)


def conv(x, w, bias=None, slope=None, stride=1, pad=1, dil=1, kparts=False) -> M.Result:
    return M.conv(hi(x), hi(w), bias, slope, stride, pad, dil, kparts=kparts)


def deconv2x2(x, w, bias=None, slope=None, kparts=False) -> M.Result:
    return M.deconv2x2(hi(x), hi(w), bias, slope, kparts=kparts)


_CACHE = {}


def build_case(cfg):
    """(x, w, f16 model Result) of a configuration -- x and w are the operands the f16x3 tests use, unchanged: the kernels drop lo'
    themselves.  Cached per process; fills cfg["dev_args"] / cfg["row_map_cpu"] / cfg["rows_out"] like ``M.build_case``."""
    key = cfg["id"] + cfg["kind"] + str(cfg["seed"])
    if key not in _CACHE:
        o = M.case_operands(cfg)
        _CACHE[key] = (o, case_model(cfg, o))
    o, res = _CACHE[key]
    cfg["dev_args"] = lambda x, w: {k: v for k, v in o.items() if k not in ("x", "w")}
    cfg["row_map_cpu"] = o.get("row_map")
    if cfg["kind"] == "linear":
        cfg["rows_out"] = cfg["M"]
    return o["x"], o["w"], res
