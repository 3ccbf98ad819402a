"""CPU: the C ABI of the image-geometry family (atm-vfi_amd/csrc/warp.hip: the warps, the fused warp + blend, the align_corners resize,
the image pyramid, the frame pack): every entry point is declared, exported, typed and plannable, and every host-side refusal of its
launchers comes back with its return code and its text, the entry point's own name in front.  No pointer below is ever dereferenced:
each call fails its checks before a launch."""
import ctypes
import importlib
import os
import re

import cpu_scene as CS

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")

ENTRIES = ("atmvfi_flow_warp", "atmvfi_flow_warp_ex", "atmvfi_flow_warp_tiled", "atmvfi_flow_warp_up2", "atmvfi_flow_warp_up2_tiled",
           "atmvfi_flow_warp_nhwc", "atmvfi_warp_blend", "atmvfi_warp_blend_planes", "atmvfi_warp_blend_tiled", "atmvfi_resize_bilinear_ac",
           "atmvfi_image_pyramid", "atmvfi_image_pyramid_pack", "atmvfi_pack_frames")
P = 0x10000                   # 16-byte aligned, never dereferenced
EINVAL, EALIGN = -1, -2
HUGE = dict(B=1 << 20, H=1 << 14, W=1 << 15)          # 2^41 tiles of 32 x 8


def test_warp_abi_is_declared_exported_and_built_from_warp_hip():
    hdr = open(os.path.join(CS.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    assert len(set(ENTRIES)) == 13
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in hip_ops.SIGNATURES and hasattr(lib, name), name
        assert lib.atmvfi_plan_fn_id(name.encode()) >= 0, name
    mk = open(os.path.join(CS.ROOT, "atm-vfi_amd", "csrc", "Makefile")).read()
    assert " warp.hip" in mk and " pointwise.hip" in mk


def _refusals(lib):
    """-> refused(rc, who, fragment, got): asserts one refusal."""
    err = lib.atmvfi_last_error
    err.restype = ctypes.c_char_p

    def refused(got, rc, who, fragment):
        text = err()
        assert got == rc, (who, fragment, got, text)
        assert text.startswith(who.encode() + b": "), (who, text)
        assert fragment.encode() in text, (who, fragment, text)
    return refused


def test_the_flow_warp_launchers_refuse_on_the_host_under_their_own_names():
    lib = hip_ops.load_library()
    refused = _refusals(lib)

    def planar(fn, src=P, flow=P, dst=P, B=1, C=3, H=16, W=32):
        return getattr(lib, "atmvfi_" + fn)(src, flow, 2 * H * W, 1, H * W, dst, B, C, H, W, None)

    def up2(fn, src=P, flow=P, dst=P, up=P, B=1, C=3, H=16, W=32):
        return getattr(lib, "atmvfi_" + fn)(src, flow, dst, up, B, C, H, W, None)

    def ex(src=P, flow=P, dst=P, mask=P, B=1, C=3, H=16, W=32, mode=0):
        return lib.atmvfi_flow_warp_ex(src, flow, dst, mask, B, C, H, W, mode, None)

    for fn in ("flow_warp", "flow_warp_tiled"):
        for null in ("src", "flow", "dst"):
            refused(planar(fn, **{null: None}), EINVAL, fn, "null pointer")
        for bad in (dict(H=1), dict(W=1), dict(B=0), dict(C=0)):
            refused(planar(fn, **bad), EINVAL, fn, "bad shape (H, W must be > 1)")
    for fn in ("flow_warp_up2", "flow_warp_up2_tiled"):
        for null in ("src", "flow", "dst", "up"):
            refused(up2(fn, **{null: None}), EINVAL, fn, "null pointer")
        for bad in (dict(H=1), dict(W=1), dict(B=0), dict(C=0)):
            refused(up2(fn, **bad), EINVAL, fn, "bad shape (H, W must be > 1)")
    for null in ("src", "flow", "dst"):
        refused(ex(**{null: None}), EINVAL, "flow_warp_ex", "null pointer")
    for bad in (dict(H=1), dict(W=1), dict(B=0), dict(C=0)):
        refused(ex(**bad), EINVAL, "flow_warp_ex", "bad shape (H, W must be > 1)")
    refused(ex(mode=3), EINVAL, "flow_warp_ex", "padding_mode must be 0 (zeros), 1 (border) or 2 (reflection), got 3")
    refused(ex(mode=-1), EINVAL, "flow_warp_ex", "padding_mode must be 0")
    # the tiled forms: rows by 16-byte loads, one workgroup per tile
    for call, fn in ((planar, "flow_warp_tiled"), (up2, "flow_warp_up2_tiled")):
        refused(call(fn, W=30), EINVAL, fn, "W must be a multiple of 4 and src 16-byte aligned (got W = 30)")
        refused(call(fn, src=P + 4), EINVAL, fn, "W must be a multiple of 4 and src 16-byte aligned (got W = 32)")
        refused(call(fn, **HUGE), EINVAL, fn, "grid too large")


def test_flow_warp_nhwc_refuses_on_the_host():
    lib = hip_ops.load_library()
    refused = _refusals(lib)

    def nhwc(src=P, src_ld=64, src_bs=64 * 512, flow=P, dst=P, dst_ld=64, dst_bs=64 * 512, B=1, C=64, H=16, W=32):
        return lib.atmvfi_flow_warp_nhwc(src, src_ld, src_bs, flow, 2 * H * W, 1, H * W, dst, dst_ld, dst_bs, B, C, H, W, None)

    for null in ("src", "flow", "dst"):
        refused(nhwc(**{null: None}), EINVAL, "flow_warp_nhwc", "null pointer")
    for bad in (dict(C=6), dict(C=0), dict(B=0), dict(H=1), dict(W=1)):
        refused(nhwc(**bad), EINVAL, "flow_warp_nhwc", "bad shape")
    for bad in (dict(src_ld=66), dict(dst_ld=66), dict(src_bs=2), dict(dst_bs=2), dict(src=P + 4), dict(dst=P + 8)):
        refused(nhwc(**bad), EALIGN, "flow_warp_nhwc", "views must be 16-byte aligned")


def test_the_warp_blend_launchers_refuse_on_the_host_under_their_own_names():
    lib = hip_ops.load_library()
    refused = _refusals(lib)
    B, H, W = 1, 16, 32
    base = dict(im0=P, im1=P, motion=P, mld=5, i0w=P, i1w=P, it=P, f0=None, f1=None, m1=None, m2=None, o0=None, o1=None, pack15=None, pack_ld=0,
                hi=None, lo=None, rows=0, c0=0, B=B, H=H, W=W)

    def blend(fn, **kw):
        a = dict(base, **kw)
        head = (a["im0"], a["im1"], a["motion"], a["mld"], a["mld"] * a["H"] * a["W"], a["i0w"], a["i1w"], a["it"], a["f0"], a["f1"], a["m1"],
                a["m2"], a["o0"], a["o1"], a["pack15"], a["pack_ld"])
        sink = () if fn == "warp_blend" else (a["hi"], a["lo"], a["rows"], a["c0"])
        return getattr(lib, "atmvfi_" + fn)(*head, *sink, a["B"], a["H"], a["W"], None)

    # atmvfi_warp_blend and atmvfi_warp_blend_planes both report as warp_blend
    for fn, who in (("warp_blend", "warp_blend"), ("warp_blend_planes", "warp_blend"), ("warp_blend_tiled", "warp_blend_tiled")):
        for null in ("im0", "im1", "motion", "i0w", "i1w", "it"):
            refused(blend(fn, **{null: None}), EINVAL, who, "null pointer")
        for bad in (dict(H=1), dict(W=1), dict(B=0), dict(mld=4)):
            refused(blend(fn, **bad), EINVAL, who, "bad shape")
        refused(blend(fn, f0=P), EINVAL, who, "flow/mask outputs come in pairs")
        refused(blend(fn, f1=P), EINVAL, who, "flow/mask outputs come in pairs")
        refused(blend(fn, m1=P), EINVAL, who, "flow/mask outputs come in pairs")
        refused(blend(fn, m2=P), EINVAL, who, "flow/mask outputs come in pairs")
        refused(blend(fn, pack15=P, pack_ld=16), EINVAL, who, "pack15 needs orig0/orig1 and ld >= 15")
        refused(blend(fn, pack15=P, pack_ld=16, o0=P), EINVAL, who, "pack15 needs orig0/orig1 and ld >= 15")
        refused(blend(fn, pack15=P, pack_ld=14, o0=P, o1=P), EINVAL, who, "pack15 needs orig0/orig1 and ld >= 15")
        if fn == "warp_blend":
            continue
        ok = dict(hi=P, lo=P, rows=B * H * W, c0=8, o0=P, o1=P)
        text = "plane sink needs orig0/orig1, rows >= B*H*W, a channel offset that is a multiple of 4, aligned planes"
        refused(blend(fn, **dict(ok, lo=None)), EINVAL, who, "the plane sink needs both planes")
        refused(blend(fn, **dict(ok, hi=None)), EINVAL, who, "the plane sink needs both planes")
        refused(blend(fn, **dict(ok, hi=P + 8)), EINVAL, who, text)
        refused(blend(fn, **dict(ok, lo=P + 2)), EINVAL, who, text)
        refused(blend(fn, **dict(ok, c0=2)), EINVAL, who, text)
        refused(blend(fn, **dict(ok, c0=-4)), EINVAL, who, text)
        refused(blend(fn, **dict(ok, rows=B * H * W - 1)), EINVAL, who, text)
        refused(blend(fn, **dict(ok, o1=None)), EINVAL, who, text)
    refused(blend("warp_blend_tiled", W=30), EINVAL, "warp_blend_tiled", "W must be a multiple of 4 and the images 16-byte aligned (got W = 30)")
    refused(blend("warp_blend_tiled", im0=P + 4), EINVAL, "warp_blend_tiled", "W must be a multiple of 4 and the images 16-byte aligned (got W = 32)")
    refused(blend("warp_blend_tiled", im1=P + 8), EINVAL, "warp_blend_tiled", "W must be a multiple of 4 and the images 16-byte aligned (got W = 32)")
    refused(blend("warp_blend_tiled", **HUGE), EINVAL, "warp_blend_tiled", "grid too large")
    # the order of the checks: the tiled form names its alignment before the pairs
    refused(blend("warp_blend_tiled", W=30, f0=P), EINVAL, "warp_blend_tiled", "W must be a multiple of 4")


def test_resize_pyramid_and_pack_refuse_on_the_host():
    lib = hip_ops.load_library()
    refused = _refusals(lib)

    def resize(src=P, dst=P, B=1, C=2, Hi=8, Wi=8, Ho=16, Wo=16):
        return lib.atmvfi_resize_bilinear_ac(src, C * Hi * Wi, Hi * Wi, Wi, 1, dst, B, C, Hi, Wi, Ho, Wo, 2.0, None)

    def pyramid(im0=P, im1=P, l1=P, l2=P, l3=P, pack=None, B=1, H=64, W=64):
        return lib.atmvfi_image_pyramid_pack(im0, im1, l1, l2, l3, pack, B, H, W, None)

    for null in ("src", "dst"):
        refused(resize(**{null: None}), EINVAL, "resize_bilinear_ac", "null pointer")
    for bad in ("B", "C", "Hi", "Wi", "Ho", "Wo"):
        refused(resize(**{bad: 0}), EINVAL, "resize_bilinear_ac", "bad shape")
    for null in ("im0", "im1", "l1", "l2", "l3"):
        refused(pyramid(**{null: None}), EINVAL, "image_pyramid", "null pointer")
        refused(lib.atmvfi_image_pyramid(*[None if k == null else P for k in ("im0", "im1", "l1", "l2", "l3")], 1, 64, 64, None), EINVAL,
                "image_pyramid", "null pointer")
    refused(pyramid(H=7), EINVAL, "image_pyramid", "H, W must be at least 8 (got 7x64)")
    refused(pyramid(W=4), EINVAL, "image_pyramid", "H, W must be at least 8 (got 64x4)")
    refused(pyramid(B=0), EINVAL, "image_pyramid", "H, W must be at least 8")
    refused(pyramid(pack=P + 4), EALIGN, "image_pyramid", "pack must be 16-byte aligned")
    for bad in (dict(im0=None), dict(im1=None), dict(dst=None), dict(B=0), dict(H=0), dict(W=0)):
        a = dict(dict(im0=P, im1=P, dst=P, B=1, H=8, W=8), **bad)
        refused(lib.atmvfi_pack_frames(a["im0"], a["im1"], a["dst"], a["B"], a["H"], a["W"], None), EINVAL, "pack_frames", "bad arguments")
    refused(lib.atmvfi_pack_frames(P, P, P + 4, 1, 8, 8, None), EALIGN, "pack_frames", "dst must be 16-byte aligned")
