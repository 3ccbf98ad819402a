"""ctypes binding of ``libatmvfi_hip.so`` (C ABI in ``include/atmvfi.h``).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic
operation of the hot path is a hand-written HIP kernel reached through this module.
There is NO fallback: if the shared library is missing, or a tensor is not a CUDA
(= HIP) fp32 tensor, the call raises.

Tensors are passed as strided *views*: a channel slice ``buf[..., a:b]`` of an NHWC
buffer is a view with ``ld = buf.stride(-2)``; a frame-stacked token matrix is a 3-D
view ``[groups, rows, C]``.  The helpers below turn such views into the raw
(pointer, ld, group stride) triples of the C ABI and validate them on the host.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import List, Optional

import torch

from .pixfmt import DeepRGB, Packed, Surface, YuvDesc, _not_420, _origin_error, as_surface

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libatmvfi_hip.so")
CHECKED_LIB_PATH = os.path.join(_HERE, "libatmvfi_hip_checked.so")     # the same sources with -DATMVFI_RANGE_CHECK (csrc/Makefile)

GEMM_CONV, GEMM_LINEAR, GEMM_DECONV = 0, 1, 2

c_f = ctypes.c_void_p      # device pointers travel as void*
c_i = ctypes.c_int
C_SLOTS = ctypes.POINTER(ctypes.c_int32)      # a HOST int32 list read at launch time (atmvfi_pool_blocks' slots)
c_l = ctypes.c_int64


class HipLibraryMissing(RuntimeError):
    pass


class GemmParams(ctypes.Structure):
    _fields_ = [
        ("mode", ctypes.c_int32),
        ("in_", c_f), ("in_ld", ctypes.c_int32), ("N", ctypes.c_int32), ("H", ctypes.c_int32),
        ("W", ctypes.c_int32), ("Cin", ctypes.c_int32),
        ("in_gstride", ctypes.c_int64), ("in_rpg", ctypes.c_int32),
        ("weight", c_f),
        ("Cout", ctypes.c_int32), ("kh", ctypes.c_int32), ("kw", ctypes.c_int32), ("stride", ctypes.c_int32),
        ("pad", ctypes.c_int32), ("dil", ctypes.c_int32),
        ("Ho", ctypes.c_int32), ("Wo", ctypes.c_int32),
        ("M", ctypes.c_int64),
        ("out", c_f), ("out_ld", ctypes.c_int32),
        ("out_gstride", ctypes.c_int64), ("out_rpg", ctypes.c_int32),
        ("out_row_map", c_f),
        ("bias", c_f), ("prelu", c_f), ("in_prelu", c_f), ("residual", c_f),
        ("res_ld", ctypes.c_int32),
        ("precision", ctypes.c_int32), ("weight_hi", c_f), ("weight_lo", c_f),
        ("in_hi", c_f), ("in_lo", c_f),
        ("out_hi", c_f), ("out_lo", c_f), ("out_plane_rows", ctypes.c_int64), ("out_plane_c0", ctypes.c_int32),
        ("out_plane_gc", ctypes.c_int32), ("tile_wn", ctypes.c_int32),
        ("in_hi2", c_f), ("in_lo2", c_f), ("in_ld2", ctypes.c_int32), ("in_split_chunks", ctypes.c_int32),
        ("workspace", c_f), ("workspace_floats", ctypes.c_int64),
    ]


class Conv3pParams(ctypes.Structure):
    """``atmvfi_conv3p_params`` (include/atmvfi.h).  Pointer fields are ``c_f``: ``LaunchPlan.add_op`` scans them."""
    _fields_ = [
        ("in_hi", c_f), ("in_lo", c_f), ("in_rows", ctypes.c_int64),
        ("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("Cin", ctypes.c_int32),
        ("w_hi", c_f), ("w_lo", c_f), ("Cout", ctypes.c_int32),
        ("bias", c_f), ("prelu", c_f),
        ("out", c_f), ("out_ld", ctypes.c_int32), ("out_cmin", ctypes.c_int32),
        ("out_hi", c_f), ("out_lo", c_f), ("plane_rows", ctypes.c_int64), ("out_c0", ctypes.c_int32), ("plane_prelu", c_f),
        ("out_hi2", c_f), ("out_lo2", c_f), ("plane_rows2", ctypes.c_int64), ("out_c02", ctypes.c_int32),
        ("wn", ctypes.c_int32), ("workspace", c_f), ("workspace_floats", ctypes.c_int64),
        ("readout_w", c_f), ("readout", c_f), ("readout_plane", ctypes.c_int64),
        ("terms", ctypes.c_int32),
    ]


class PlanArg(ctypes.Union):
    _fields_ = [("u", ctypes.c_uint64), ("i", ctypes.c_int64), ("f", ctypes.c_double)]


PLAN_MAX_ARGS = 28


class PlanOp(ctypes.Structure):
    _fields_ = [("fn", ctypes.c_int32), ("nargs", ctypes.c_int32), ("a", PlanArg * PLAN_MAX_ARGS)]


class PlanPatch(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("arg", ctypes.c_int32), ("slot", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("offset", ctypes.c_int64)]


# name -> (restype, argtypes); also the list of symbols the header declares (checked by the CPU tests)
SIGNATURES = {
    "atmvfi_version": (c_i, []),
    "atmvfi_last_error": (ctypes.c_char_p, []),
    "atmvfi_source_digest": (ctypes.c_char_p, []),
    "atmvfi_range_word_set": (c_i, [c_f, c_f]),
    "atmvfi_range_checked": (c_i, []),
    "atmvfi_gemm": (c_i, [ctypes.POINTER(GemmParams), c_f]),
    "atmvfi_gemm_workspace_floats": (c_l, [c_l, c_i, c_i]),
    "atmvfi_split_planes": (c_i, [c_f, c_i, c_l, c_i, c_f, c_f, c_f, c_i, c_f]),
    "atmvfi_split_planes_at": (c_i, [c_f, c_i, c_l, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_conv2d": (c_i, [ctypes.POINTER(GemmParams), c_f]),
    "atmvfi_linear": (c_i, [ctypes.POINTER(GemmParams), c_f]),
    "atmvfi_deconv2x2": (c_i, [ctypes.POINTER(GemmParams), c_f]),
    "atmvfi_packed_weight_floats": (c_l, [c_i, c_i, c_i, c_i, c_i]),
    "atmvfi_pack_weight": (c_i, [c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_split_weight_halves": (c_l, [c_i, c_i, c_i, c_i, c_i]),
    "atmvfi_pack_weight_split": (c_i, [c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_conv3x3_weight_halves": (c_l, [c_i, c_i]),
    "atmvfi_pack_weight_conv3x3": (c_i, [c_f, c_f, c_f, c_i, c_i, c_f]),
    "atmvfi_conv3x3_f16x3": (c_i, [c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_i, c_f, c_i, c_f, c_f, c_f, c_f, c_l, c_f, c_i, c_i, c_f]),
    "atmvfi_conv3p": (c_i, [ctypes.POINTER(Conv3pParams), c_f]),
    "atmvfi_flow_warp_up2": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_flow_warp_up2_tiled": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_image_pyramid": (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_image_pyramid_pack": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_head1x1_planes": (c_i, [c_f, c_f, c_l, c_l, c_i, c_f, c_f, c_i, c_f, c_i, c_f]),
    "atmvfi_conv3x3_planes_workspace_floats": (c_l, [c_i, c_i, c_i, c_i, c_i]),
    "atmvfi_refine_tail": (c_i, [c_f, c_l, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_layernorm": (c_i, [c_f, c_i, c_l, c_i, c_f, c_f, c_i, c_f, c_f, c_l, c_i, c_f, c_f, c_i, c_f]),
    "atmvfi_dwconv3x3_gelu": (c_i, [c_f, c_i, c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_f, c_i, c_f]),
    "atmvfi_pack_dw_weight": (c_i, [c_f, c_f, c_i, c_f]),
    "atmvfi_window_attention": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_i, c_f]),
    "atmvfi_window_attention_f16x3": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_i, c_f]),
    "atmvfi_window_attn_cross_motion": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_window_attn_self": (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_motion_head": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_l, c_i, c_l, c_i, c_f]),
    "atmvfi_motion_head_planes": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_l, c_i, c_l, c_i, c_f, c_f, c_l, c_i, c_i, c_f]),
    "atmvfi_flow_warp": (c_i, [c_f, c_f, c_l, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_flow_warp_tiled": (c_i, [c_f, c_f, c_l, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_flow_warp_ex": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_flow_warp_nhwc": (c_i, [c_f, c_i, c_l, c_f, c_l, c_i, c_i, c_f, c_i, c_l, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_warp_blend": (c_i, [c_f, c_f, c_f, c_i, c_l, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i,
                                c_i, c_i, c_i, c_f]),
    "atmvfi_warp_blend_planes": (c_i, [c_f, c_f, c_f, c_i, c_l, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i,
                                       c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_warp_blend_tiled": (c_i, [c_f, c_f, c_f, c_i, c_l, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i,
                                      c_f, c_f, c_l, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_resize_bilinear_ac": (c_i, [c_f, c_l, c_l, c_l, c_l, c_f, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_float, c_f]),
    "atmvfi_frame_u8_to_f32": (c_i, [c_f, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_frame_u8_window": (c_i, [c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_f]),
    "atmvfi_frame_f32_to_u8": (c_i, [c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_pool_blocks": (c_i, [c_f, c_l, c_i, C_SLOTS, c_i, c_l, c_f, c_i, c_f]),
    "atmvfi_tta_merge": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_frame_rot180": (c_i, [c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_frame_signature_workspace_ints": (c_l, [c_i, c_i]),
    "atmvfi_frame_signature": (c_i, [c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_l, c_f]),
    "atmvfi_frame_difference_workspace_ints": (c_l, [c_i, c_i]),
    "atmvfi_frame_difference": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_l, c_f]),
    "atmvfi_frame_borders_workspace_ints": (c_l, [c_i, c_i]),
    "atmvfi_frame_borders": (c_i, [c_f, c_i, c_i, c_i, c_f, c_f, c_l, c_f]),
    "atmvfi_frame_compose": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_f]),
    "atmvfi_yuv_borders_workspace_ints": (c_l, [c_i, c_i]),
    "atmvfi_yuv_borders": (c_i, [ctypes.POINTER(YuvDesc), c_f, c_f, c_f, c_l, c_f]),
    "atmvfi_yuv_compose": (c_i, [ctypes.POINTER(YuvDesc), c_f, c_f] + [c_i] * 4 + [c_f] + [c_i] * 4 + [c_f, c_f]),
    "atmvfi_shutter_accumulate": (c_i, [c_f, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_shutter_resolve": (c_i, [c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_f]),
    "atmvfi_shutter_table": (c_i, [c_i, ctypes.POINTER(ctypes.c_uint16)]),
    "atmvfi_yuv_decode": (c_i, [ctypes.POINTER(YuvDesc), c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_yuv_encode": (c_i, [ctypes.POINTER(YuvDesc), c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_f]),
    "atmvfi_yuv_unpack": (c_i, [c_f, c_i, c_i, c_i, c_l, c_f, c_f]),
    "atmvfi_yuv_pack": (c_i, [c_f, c_i, c_i, c_i, c_f, c_f]),
    "atmvfi_rgb16_decode": (c_i, [c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_f]),
    "atmvfi_rgb16_encode": (c_i, [c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_frame_half": (c_i, [c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_field_bob": (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f]),
    "atmvfi_field_rows": (c_i, [c_f, c_f, c_i, ctypes.POINTER(ctypes.c_int64), c_i, c_f]),
    "atmvfi_synth_up2": (c_i, [c_f, c_f]),
    "atmvfi_synth_up2_workspace_floats": (c_l, [c_i, c_i, c_i]),
    "atmvfi_pack_frames": (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_final_residual": (c_i, [c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_f]),
    "atmvfi_l1_mean": (c_i, [c_f, c_f, c_f, c_i, c_l, c_f, c_l, c_f]),
    "atmvfi_l1_mean_workspace_floats": (c_l, [c_i, c_l]),
    "atmvfi_ssim_psnr": (c_i, [c_f, c_l, c_l, c_l, c_l, c_f, c_l, c_l, c_l, c_l, c_i, c_i, c_i, ctypes.c_float, c_i, c_f, c_f, c_l, c_f]),
    "atmvfi_ssim_psnr_workspace_floats": (c_l, [c_i, c_i, c_i]),
    "atmvfi_ensemble_select": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_l, c_f]),
    "atmvfi_stem_fused": (c_i, [c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_l, c_f]),
    "atmvfi_plan_fn_id": (c_i, [ctypes.c_char_p]),
    "atmvfi_plan_run": (c_i, [ctypes.POINTER(PlanOp), c_i, ctypes.POINTER(PlanPatch), c_i, ctypes.POINTER(ctypes.c_uint64), c_i,
                              ctypes.POINTER(c_i), c_f]),
}
FIELD_BOB_STRIP = 16          # include/atmvfi.h ATMVFI_FIELD_BOB_STRIP: the picture rows a lane of atmvfi_field_bob walks
SSIM_X_U8, SSIM_X_BGR, SSIM_ROUND_Y, SSIM_ACCUMULATE, SSIM_MSE_F32 = 1, 2, 4, 8, 16     # include/atmvfi.h ATMVFI_SSIM_*


class SynthUp2Params(ctypes.Structure):
    """``atmvfi_synth_up2_params`` of include/atmvfi.h."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ("it_sum", "it0", "it1", "flow0", "flow1", "m1", "store0", "store1", "slots0", "slots1", "dst_f32",
                                                 "dst_u8", "f0_out", "f1_out", "m_out", "workspace")]
                + [(n, ctypes.c_int32) for n in ("B", "h", "w", "S0", "S1", "pad_top", "pad_left", "hh", "ww", "bgr", "path", "reserved")])


def load_library(path: str = LIB_PATH, optional=()) -> ctypes.CDLL:
    """``optional``: symbols that may be missing (an older build of the ABI loaded beside this one for a same-process A/B)."""
    if not os.path.exists(path):
        raise HipLibraryMissing(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if name in optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


@dataclass
class PackedWeight:
    mode: int
    cout: int
    cin: int
    kh: int
    kw: int
    orig: torch.Tensor                 # the parameter (OIHW / [out,in] / IOHW)
    packed: Optional[torch.Tensor]     # GEMM layout on the device (None only for test doubles)
    hi: Optional[torch.Tensor] = None  # split-precision planes (fp16), k-step major, of the two GEMM engines (gemm_f16x3 / gemm_split)
    lo: Optional[torch.Tensor] = None
    hi3: Optional[torch.Tensor] = None  # 3x3 weights again in the conv3x3_f16x3 layout (k-step major, tap-packed channel tail)
    lo3: Optional[torch.Tensor] = None


@dataclass
class StemWeights:
    """Operands of ``atmvfi_stem_fused`` (HipOps.pack_stem)."""
    c0: int
    c1: int
    w1h: torch.Tensor
    w1l: torch.Tensor
    b1: torch.Tensor
    p1: torch.Tensor
    w2h: torch.Tensor
    w2l: torch.Tensor
    b2: torch.Tensor
    p2: torch.Tensor
    w3h: torch.Tensor
    w3l: torch.Tensor
    b3: torch.Tensor
    p3: torch.Tensor


class Planes:
    """Split-plane activation rows: one fp16 tensor [2, chunks, rows, 32] -- plane 0 = hi, plane 1 = lo' = (x - hi) * 1024, CHUNK
    MAJOR (channel c of row r at [c // 32, r, c % 32]) -- holding ``c`` real channels per row; the pad channels of the last chunk
    are finite (zero).  Producers write it in their epilogue; the split GEMM reads it by LDS-DMA, 16 rows x 64 bytes = one
    contiguous KiB per instruction."""

    def __init__(self, t: torch.Tensor, c: int, rows: Optional[int] = None):
        if t.dtype != torch.float16 or t.dim() != 4 or t.shape[0] != 2 or t.shape[3] != 32 or not t.is_contiguous() or c > t.shape[1] * 32 \
                or c <= (t.shape[1] - 1) * 32:
            raise ValueError(f"Planes: expected contiguous fp16 [2, ceil(C/32), rows, 32], got {tuple(t.shape)} {t.dtype} C={c}")
        if not t.is_cuda:
            raise TypeError("Planes: tensor must live on the GPU")
        if rows is not None and not 0 < rows <= t.shape[2]:
            raise ValueError(f"Planes: {rows} valid rows do not fit the {t.shape[2]} allocated ones")
        self.t, self.c = t, c
        self._rows = t.shape[2] if rows is None else rows

    @property
    def rows(self):
        """Rows that hold data.  ``ld_rows`` (>= rows) is the allocated row count = the chunk stride every kernel is given; rows past
        ``rows`` are never written and stay zero (the 3x3 kernel on plane input reads row ``rows`` for pixels outside the image)."""
        return self._rows

    @property
    def ld_rows(self):
        return self.t.shape[2]

    @property
    def chunks(self):
        return self.t.shape[1]

    def to_rows(self) -> torch.Tensor:
        """[2, rows, chunks*32] row-major copy (tests / debugging)."""
        return self.t[:, :, :self.rows].permute(0, 2, 1, 3).reshape(2, self.rows, self.chunks * 32)

    def to_float(self) -> torch.Tensor:
        """[rows, C] fp32 value hi + lo' / 1024 (tests / debugging)."""
        r = self.to_rows().float()
        return (r[0] + r[1] / 1024.0)[:, :self.c]

    @staticmethod
    def alloc(rows: int, c: int, device) -> "Planes":
        """Zero-initialised planes with one spare (zero) row behind the data."""
        return Planes(torch.zeros(2, (c + 31) // 32, rows + 1, 32, dtype=torch.float16, device=device), c, rows)


class TPtr(ctypes.c_void_p):
    """A device pointer that remembers the tensor it was derived from (``src``).  Launch plans classify pointer arguments by that tensor
    -- per-call memory or workspace -- never by what allocation the raw address happens to fall into: a biased or one-past-the-end
    pointer lies inside a NEIGHBOURING allocation."""
    __slots__ = ("src",)


def _ptr(t: Optional[torch.Tensor], byte_offset: int = 0):
    """-> ``TPtr`` of ``t.data_ptr() + byte_offset`` (None for a missing optional tensor)."""
    if t is None:
        return None
    p = TPtr(t.data_ptr() + byte_offset)
    p.src = t
    return p


def _chk(t: torch.Tensor, what: str):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f"{what}: expected a CUDA/HIP float32 tensor, got "
                        f"{getattr(t, 'device', None)} {getattr(t, 'dtype', None)}")


def nhwc_view(t: torch.Tensor, what: str):
    """-> (ld, N, H, W, C) of an NHWC view (channel slice of a contiguous NHWC buffer)."""
    _chk(t, what)
    if t.dim() != 4:
        raise ValueError(f"{what}: expected [N,H,W,C], got {tuple(t.shape)}")
    n, h, w, c = t.shape
    ld = t.stride(2)
    if (c > 1 and t.stride(3) != 1) or (h > 1 and t.stride(1) != w * ld) or (n > 1 and t.stride(0) != h * w * ld):
        raise ValueError(f"{what}: not an NHWC pixel-contiguous view: shape {tuple(t.shape)} strides {t.stride()}")
    return ld, n, h, w, c


def rows_view(t: torch.Tensor, what: str):
    """-> (ld, M, C, gstride, rpg) of a token matrix [M,C] or a grouped one [G,R,C]."""
    _chk(t, what)
    if t.dim() == 2:
        if t.stride(1) != 1:
            raise ValueError(f"{what}: rows must be channel-contiguous")
        return t.stride(0), t.shape[0], t.shape[1], 0, 0
    if t.dim() == 3:
        if t.stride(2) != 1:
            raise ValueError(f"{what}: rows must be channel-contiguous")
        g, r, c = t.shape
        return t.stride(1), g * r, c, t.stride(0), r
    raise ValueError(f"{what}: expected [M,C] or [G,R,C], got {tuple(t.shape)}")


def flow_view(flow: torch.Tensor, h: int, w: int, what: str):
    """[B,2,H,W] view (planar, or a permuted channel pair of an NHWC map) -> (bstride, pstride, cstride)."""
    _chk(flow, what)
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[2] != h or flow.shape[3] != w:
        raise ValueError(f"{what}: expected [B,2,{h},{w}], got {tuple(flow.shape)}")
    ps = flow.stride(3)
    if flow.stride(2) != w * ps:
        raise ValueError(f"{what}: rows of the flow view must be pixel-contiguous")
    return flow.stride(0), ps, flow.stride(1)


def _planar(t: torch.Tensor, c: int, what: str):
    _chk(t, what)
    if t.dim() != 4 or t.shape[1] != c or not t.is_contiguous():
        raise ValueError(f"{what}: expected contiguous [B,{c},H,W], got {tuple(t.shape)} strides {t.stride()}")


def _is_u8_frame(t, hw=None) -> bool:
    return (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous() and t.is_cuda
            and (hw is None or t.shape[:2] == tuple(hw)))


def _u8_frame(t, what: str, hw=None, which: str = ""):
    """``t`` is a packed uint8 frame [H,W,3] on the device (of exactly ``hw`` = (h, w) when given), or ``ValueError`` naming it
    ``what + which``."""
    if not _is_u8_frame(t, hw):
        raise ValueError(f"{what}{which} must be a contiguous CUDA uint8 [{'H,W' if hw is None else f'{hw[0]},{hw[1]}'},3] tensor")


def _f32_canvas(t, what: str, which: str = ""):
    """``t`` is a planar fp32 frame [3,Hp,Wp] on the device, or ``ValueError`` naming it ``what + which``."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != 3 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{what}{which} must be a contiguous CUDA fp32 [3,Hp,Wp] tensor")


def _yuv_buf(t, desc, who: str, role: str):
    """``t`` is one frame of ``desc`` (a ``pixfmt.Format`` or ``Surface``) as bytes on the device, or ``ValueError``.  -> its byte count"""
    n = desc.frame_bytes
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
        layout = f"{desc.chroma} surface, pitch {desc.pitch}" if isinstance(desc, Surface) else "packed planar"
        raise ValueError(f"{who}: {role} buf must be a contiguous CUDA uint8 tensor of {n} bytes ({desc.height} x {desc.width} "
                         f"{desc.subsampling}, depth {desc.depth}, {layout})")
    return n


def _window(who: str, desc, window):
    """``window`` (y0, x0, h, w) of a frame of ``desc`` as ints, or ``ValueError`` where it does not lie in the frame."""
    y0, x0, wh, ww = map(int, window)
    if y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > desc.height or x0 + ww > desc.width:
        raise ValueError(f"{who}: window {wh} x {ww} at ({y0}, {x0}) outside the {desc.height} x {desc.width} frame")
    return y0, x0, wh, ww


_SAMPLES_PER_PIXEL = {"420": 1.5, "422": 2.0, "444": 3.0}          # 1 + 2 / (sy * sx) of the subsampling steps


class PlanUnsupported(Exception):
    """Raised while recording when a forward cannot be expressed as a launch plan (the caller falls back to direct launches)."""


class LaunchPlan:
    """One forward of the hot path recorded as an array of ``atmvfi_plan_op`` (include/atmvfi.h, "Launch plans") and replayed by ONE
    ``atmvfi_plan_run`` call: per-call memory -- the caller's input tensors (the two frames of ``forward``, the three pool tensors of
    ``forward_pooled``; any number) and the output tensors, fresh on every call -- enters through a slot table that the library
    patches into the recorded arguments.  A plan may have no outputs at all (``finish(None)``: it only writes into its inputs).

    Recording (``HipOps.begin_plan`` ... ``end_plan``): every launch of ``HipOps._run`` is executed as usual AND appended; every
    ``HipOps.empty`` becomes an output slot; pointer arguments (by the entry point's declared types) that fall inside a slot's
    memory become patches.  A pointer field of a GEMM parameter block inside per-call memory cannot be patched: PlanUnsupported.

    Host integer lists (the slot list of ``atmvfi_pool_blocks``, declared ``POINTER(c_int32)``): the library reads such an array at
    launch time (include/atmvfi.h, "Launch plans"), so the op records the ctypes array's ADDRESS, the plan keeps the array alive and
    registers it under the ROLE its caller gave it (``HipOps.pool_blocks(..., role=)``); ``run(..., lists={role: values})`` overwrites
    every registered array before the replay.  The length of a role is fixed by the recording; no replay ever sees stale values."""

    debug = False      # diagnostic: replay one op per call, synchronised, announced on stderr first (finds the op that faults)

    def __init__(self, lib, inputs):
        self.lib = lib
        self.ops_list = []                 # (fn id, [values], [is_float])
        self.keep = []                     # parameter blocks referenced by address
        self.lists = {}                    # role -> [host int32 arrays referenced by address]: rewritten from run(lists=) per replay
        self.slots = []                    # (base, bytes): inputs first, then outputs
        self._slot_store = []              # per slot: address of the storage the slot's tensor lives in
        for t in inputs:
            self._add_slot(t)
        for i in range(len(self.slots)):
            for j in range(i):
                (bi, ni), (bj, nj) = self.slots[i], self.slots[j]
                if bi < bj + nj and bj < bi + ni:
                    raise PlanUnsupported("the input tensors overlap in memory: a pointer into one could not be told from a pointer into the other")
        self.n_inputs = len(inputs)
        self.align = tuple(t.data_ptr() & 15 for t in inputs)      # kernel choices (16-byte row loads) were made for this alignment
        self.out_meta = []                 # (shape, dtype) per output slot, allocation order
        self.out_tensors = []              # the recording call's own outputs (kept alive until end_plan)
        self.patches = []
        self.template = None               # result structure with ("slot", k) leaves
        self.c_ops = self.c_patches = self.c_slots = None
        self._fn_ids = {}
        self.by_tensor = self.by_address = 0      # pointer arguments classified per-call by their tensor / refused by raw address

    # ---- recording ----
    def _add_slot(self, t: torch.Tensor):
        self.slots.append((t.data_ptr(), t.numel() * t.element_size()))
        self._slot_store.append(t.untyped_storage().data_ptr())

    def _slot_of(self, ptr: int):
        """The slot whose byte range holds the raw address ``ptr`` (assertions and untyped parameter-block fields only)."""
        for k, (base, nb) in enumerate(self.slots):
            if base <= ptr < base + nb:
                return k, ptr - base
        return None

    def _slot_of_tensor(self, t: torch.Tensor):
        """The slot a tensor belongs to: same storage AND the tensor starts inside the slot's bytes (two inputs may be slices of one
        stacked tensor).  None: the tensor is workspace / parameter memory, whatever its neighbours in the address space are."""
        st = t.untyped_storage().data_ptr()
        p = t.data_ptr()
        for k, (base, nb) in enumerate(self.slots):
            if self._slot_store[k] == st and base <= p < base + max(nb, 1):
                return k
        return None

    def add_output(self, t: torch.Tensor):
        self._add_slot(t)
        self.out_meta.append((tuple(t.shape), t.dtype))
        self.out_tensors.append(t)

    def add_op(self, fn, args):
        """Pointer arguments are ``TPtr`` (hip_ops._ptr): the tensor they were derived from decides whether they are per-call
        pointers (patched on replay, offset relative to the slot's base -- it may be negative or past the end) or fixed ones.  A
        pointer WITHOUT a tensor (a raw integer) must not lie in per-call memory: the plan refuses it rather than guess."""
        name = fn.__name__
        fid = self._fn_ids.get(name)
        if fid is None:
            fid = self.lib.atmvfi_plan_fn_id(name.encode())
            if fid < 0:
                raise PlanUnsupported(f"{name} is not a launch entry point")
            self._fn_ids[name] = fid
        types = SIGNATURES[name][1]
        args = args[:-1]                   # the stream is the plan's
        if len(args) > PLAN_MAX_ARGS:
            raise PlanUnsupported(f"{name}: {len(args)} arguments")
        vals = []
        k = len(self.ops_list)
        for j, (v, ty) in enumerate(zip(args, types)):
            if isinstance(v, float):
                vals.append(("f", v))
                continue
            if hasattr(v, "_obj"):         # ctypes.byref(parameter block): referenced by address, kept alive with the plan
                blk = v._obj
                for t in getattr(blk, "_srcs", ()):                 # the tensors its pointer fields were taken from (by tensor first)
                    if isinstance(t, torch.Tensor) and self._slot_of_tensor(t) is not None:
                        raise PlanUnsupported(f"{name}: a parameter-block operand lives in per-call memory")
                for fname, ftype in blk._fields_:
                    if ftype is c_f and getattr(blk, fname) and self._slot_of(getattr(blk, fname)) is not None:
                        raise PlanUnsupported(f"{name}: parameter block field {fname} points into per-call memory")
                self.keep.append(blk)
                vals.append(("u", ctypes.addressof(blk)))
                continue
            if ty is C_SLOTS:              # a host integer list, read by the library at launch time: by address, under its role
                role = getattr(v, "role", None)
                if not isinstance(v, ctypes.Array) or v._type_ is not ctypes.c_int32 or role is None:
                    raise PlanUnsupported(f"{name}: argument {j} is a host integer list without a role")
                known = self.lists.setdefault(role, [])
                if known and len(known[0]) != len(v):
                    raise PlanUnsupported(f"{name}: role {role!r} names lists of {len(known[0])} and of {len(v)} entries")
                known.append(v)
                vals.append(("u", ctypes.addressof(v)))
                continue
            src = getattr(v, "src", None) if isinstance(v, TPtr) else None
            if isinstance(v, ctypes.c_void_p):
                v = v.value
            v = 0 if v is None else int(v)
            if ty is c_f and v:
                if src is not None:
                    slot = self._slot_of_tensor(src)
                    if slot is not None:
                        self.patches.append((k, j, slot, v - self.slots[slot][0]))
                        self.by_tensor += 1
                elif self._slot_of(v) is not None:
                    self.by_address += 1
                    raise PlanUnsupported(f"{name}: argument {j} is a raw address inside per-call memory with no tensor to attribute it to")
            vals.append(("u" if v >= 0 else "i", v))
        self.ops_list.append((fid, vals))

    def finish(self, result):
        """Freeze the plan; ``result`` is what the recorded forward returned (tensors must be whole output slots)."""
        by_ptr = {base: k for k, (base, _) in enumerate(self.slots) if k >= self.n_inputs}

        def walk(x):
            if isinstance(x, torch.Tensor):
                k = by_ptr.get(x.data_ptr())
                if k is None or tuple(x.shape) != self.out_meta[k - self.n_inputs][0]:
                    raise PlanUnsupported("a returned tensor is not a whole per-call output")
                return ("slot", k)
            if isinstance(x, dict):
                return {kk: walk(v) for kk, v in x.items()}
            if isinstance(x, (list, tuple)):
                return [walk(v) for v in x]
            return x
        self.template = walk(result)
        n = len(self.ops_list)
        self.c_ops = (PlanOp * n)()
        for i, (fid, vals) in enumerate(self.ops_list):
            op = self.c_ops[i]
            op.fn, op.nargs = fid, len(vals)
            for j, (kind, v) in enumerate(vals):
                setattr(op.a[j], kind, v)
        self.c_patches = (PlanPatch * max(1, len(self.patches)))()
        for i, (k, j, slot, off) in enumerate(self.patches):
            pp = self.c_patches[i]
            pp.op, pp.arg, pp.slot, pp.offset = k, j, slot, off
        self.c_slots = (ctypes.c_uint64 * len(self.slots))()
        self.failed = c_i(-1)
        self.out_tensors = []
        return self

    # ---- replay ----
    def _rewrite_lists(self, lists):
        if set(lists or ()) != set(self.lists):
            raise ValueError(f"LaunchPlan.run: the plan's host lists are {sorted(self.lists)}, given {sorted(lists or ())}")
        new = {role: [int(x) for x in lists[role]] for role in self.lists}
        for role, arrays in self.lists.items():
            if len(new[role]) != len(arrays[0]):
                raise ValueError(f"LaunchPlan.run: list {role!r} was recorded with {len(arrays[0])} entries, given {len(new[role])}")
        for role, arrays in self.lists.items():              # (only now: a refused call leaves the arrays as they were)
            for arr in arrays:
                arr[:] = new[role]

    def run(self, inputs, device, stream, poison: bool = False, lists=None):
        """``poison``: fill the fresh outputs with NaN first (the record-time self-check: an element the replay does not write, or
        writes somewhere else, then differs from the recording forward's result).  ``lists``: {role: sequence of ints} for every host
        integer list of the plan -- all of them, each of its recorded length, else ``ValueError`` before anything is launched (a plan
        without such lists takes None).  Returns the recorded result structure over fresh tensors (None for a plan without outputs)."""
        if len(inputs) != self.n_inputs:
            raise ValueError(f"LaunchPlan.run: {len(inputs)} inputs, recorded with {self.n_inputs}")
        if self.lists or lists:
            self._rewrite_lists(lists)
        outs = [torch.empty(shape, dtype=dt, device=device) for shape, dt in self.out_meta]
        if poison:
            for t in outs:
                t.fill_(float("nan"))
        sl = self.c_slots
        for k, t in enumerate(inputs):
            sl[k] = t.data_ptr()
        base = self.n_inputs
        for k, t in enumerate(outs):
            sl[base + k] = t.data_ptr()
        if LaunchPlan.debug:          # diagnostic (set LaunchPlan.debug = True): one op per call, synchronised, announced on stderr first
            import sys
            names = {v: k for k, v in self._fn_ids.items()}
            for k, j, slot, off in self.patches:
                self.c_ops[k].a[j].u = sl[slot] + off
            rc = 0
            for i in range(len(self.ops_list)):
                print(f"plan op {i} {names.get(self.c_ops[i].fn)} args " + " ".join(hex(self.c_ops[i].a[j].u) for j in range(self.c_ops[i].nargs)),
                      file=sys.stderr, flush=True)
                one = ctypes.cast(ctypes.byref(self.c_ops[i]), ctypes.POINTER(PlanOp))
                rc = self.lib.atmvfi_plan_run(one, 1, None, 0, None, 0, ctypes.byref(self.failed), stream)
                torch.cuda.synchronize()
                if rc:
                    break
        else:
            rc = self.lib.atmvfi_plan_run(self.c_ops, len(self.ops_list), self.c_patches, len(self.patches), sl, len(self.slots),
                                          ctypes.byref(self.failed), stream)
        if rc != 0:
            raise RuntimeError(f"plan_run failed ({rc}) at op {self.failed.value}: {self.lib.atmvfi_last_error().decode()}")

        def build(x):
            if isinstance(x, tuple) and len(x) == 2 and x[0] == "slot":
                return outs[x[1] - base]
            if isinstance(x, dict):
                return {kk: build(v) for kk, v in x.items()}
            if isinstance(x, list):
                return [build(v) for v in x]
            return x
        return build(self.template)


class HipOps:
    """The op vocabulary of the hot path, each a single HIP kernel launch."""

    def __init__(self, device: torch.device, checked: bool = False, lib_path: Optional[str] = None, lib_optional=()):
        # checked: the build that counts operands beyond the f16x3 engines' fp16 range (libatmvfi_hip_checked.so, include/atmvfi.h
        # atmvfi_range_word_set).  One device word per HipOps; attached at the top of every forward (begin_forward): the library has
        # one attachment per device, so one checked model runs at a time on a device.
        self.checked = bool(checked)
        # lib_path: another build of the same ABI (tests and tools: the diagnostic libraries under tools/lib/)
        self.lib = load_library(lib_path, lib_optional) if lib_path else load_library(CHECKED_LIB_PATH) if self.checked else load_library()
        self.device = device
        self.range_word: Optional[torch.Tensor] = None
        if self.checked:
            if self.lib.atmvfi_range_checked() != 1:
                raise HipLibraryMissing(f"{CHECKED_LIB_PATH} is not a checked build (make -C atm-vfi_amd/csrc checked)")
            self.range_word = torch.zeros(1, dtype=torch.int32, device=device)
        self.profile: Optional[List] = None      # when a list: (name, meta, start_evt, end_evt) per launch
        # "f16x3": 3x3/s1 convs run split-precision on the 16-bit MFMA (hi*hi + hi*lo + lo*hi, fp32 accumulate);
        # "f32": everything on the exact-fp32 MFMA.
        self.precision = "f16x3"
        # Terms of a product in the PLANE kernels (conv3x3_planes, conv3x3_planes_readout, every GEMM on split-plane input), under
        # precision "f16x3": 3 = hi*hi + hi*lo' + lo'*hi (the default), 1 = hi*hi alone (Network.set_precision("f16"): one MFMA per
        # product, ~11 significand bits per operand).  Layouts, sinks, tile and split-K choices do not depend on it.
        self.plane_terms = 3
        self.attention_f16x3 = True        # window attention on the f16x3 MFMA path too (False: the exact-fp32 kernel)
        # per-call kernel-instance overrides (parity tests, sweeps): (schedule, wn) of the fp32-input 3x3 kernel, tile width of the
        # fp32-input f16x3 GEMM; None / 0 = the library's cost model
        self.conv3_instance = None
        self.gemm_tile_wn = 0
        self.warp_tiles = True             # planar warps with LDS-staged source tiles (False: the direct gathers; bit-identical)
        self.recording: Optional[LaunchPlan] = None     # when set: every launch is also appended to this plan
        # split-K scratch for the plane-input GEMM: a callable floats -> fp32 tensor (Network hands out workspace memory); None: never split
        self.gemm_workspace = None

    # ------------------------------------------------------------------ launch plans
    def begin_plan(self, inputs) -> LaunchPlan:
        if self.profile is not None:
            raise PlanUnsupported("per-launch profiling is on")
        self.recording = LaunchPlan(self.lib, inputs)
        return self.recording

    def end_plan(self, result) -> LaunchPlan:
        plan, self.recording = self.recording, None
        return plan.finish(result)

    def abort_plan(self):
        self.recording = None

    # ------------------------------------------------------------------ utils
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def begin_forward(self):
        """Called by Network at the top of every forward: attaches the range word of the checked build."""
        if self.checked:
            self._check(self.lib.atmvfi_range_word_set(self.range_word.data_ptr(), self._stream()), "range_word_set")

    def _check(self, rc: int, name: str):
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc}): {self.lib.atmvfi_last_error().decode()}")

    def _run(self, name: str, meta: dict, fn, *args):
        if self.recording is not None:
            self.recording.add_op(fn, args)
        if self.profile is None:
            self._check(fn(*args), name)
            return
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        st = torch.cuda.current_stream(self.device)
        s.record(st)
        self._check(fn(*args), name)
        e.record(st)
        self.profile.append((name, meta, s, e))

    def empty(self, *shape) -> torch.Tensor:
        t = torch.empty(*shape, dtype=torch.float32, device=self.device)
        if self.recording is not None:
            self.recording.add_output(t)
        return t

    def to_device_int(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    # ---------------------------------------------------------------- weights
    def pack_weight(self, mode: int, w: torch.Tensor) -> PackedWeight:
        _chk(w, "pack_weight")
        w = w.detach().contiguous()
        if mode == GEMM_DECONV:
            cin, cout, kh, kw = w.shape
        elif mode == GEMM_LINEAR:
            cout, cin = w.shape[0], w.shape[1]
            kh = kw = 1
        else:
            cout, cin, kh, kw = w.shape
        n = self.lib.atmvfi_packed_weight_floats(mode, cout, cin, kh, kw)
        dst = self.empty(n)
        self._check(self.lib.atmvfi_pack_weight(mode, _ptr(w), _ptr(dst), cout, cin, kh, kw, self._stream()), "pack_weight")
        pw = PackedWeight(mode, cout, cin, kh, kw, w, dst)
        if cin >= 16:       # split-precision planes for the f16x3 engines (tiny-K layers stay on the fp32 MFMA)
            nh = self.lib.atmvfi_split_weight_halves(mode, cout, cin, kh, kw)
            pw.hi = torch.empty(nh, dtype=torch.float16, device=self.device)
            pw.lo = torch.empty(nh, dtype=torch.float16, device=self.device)
            self._check(self.lib.atmvfi_pack_weight_split(mode, _ptr(w), _ptr(pw.hi), _ptr(pw.lo), cout, cin, kh, kw, self._stream()),
                        "pack_weight_split")
            if mode == GEMM_CONV and kh == 3 and kw == 3:
                n3 = self.lib.atmvfi_conv3x3_weight_halves(cout, cin)
                pw.hi3 = torch.empty(n3, dtype=torch.float16, device=self.device)
                pw.lo3 = torch.empty(n3, dtype=torch.float16, device=self.device)
                self._check(self.lib.atmvfi_pack_weight_conv3x3(_ptr(w), _ptr(pw.hi3), _ptr(pw.lo3), cout, cin, self._stream()),
                            "pack_weight_conv3x3")
        return pw

    def pack_dw_weight(self, w: torch.Tensor) -> torch.Tensor:
        _chk(w, "pack_dw_weight")
        w = w.detach().contiguous()
        c = w.shape[0]
        dst = self.empty(9 * c)
        self._check(self.lib.atmvfi_pack_dw_weight(_ptr(w), _ptr(dst), c, self._stream()), "pack_dw_weight")
        return dst

    def _plane_prec(self, p: "GemmParams"):
        """The precision field of a launch on split-plane input under ``plane_terms``: ATMVFI_PREC_F16 (2) for single-term products."""
        if self.plane_terms not in (1, 3):
            raise ValueError(f"plane_terms must be 3 (f16x3) or 1 (f16), got {self.plane_terms!r}")
        if self.plane_terms == 1 and p.precision == 1 and p.in_hi:
            p.precision = 2

    def _prec(self, w: PackedWeight):
        """(precision, hi, lo) fields of GemmParams for this weight under the current precision mode."""
        if self.precision == "f16x3" and w.hi is not None:
            return 1, w.hi.data_ptr(), w.lo.data_ptr()
        return 0, None, None

    def pad_channels(self, v: torch.Tensor, mult: int = 32) -> torch.Tensor:
        """Per-channel vector padded with zeros to a multiple of ``mult`` (in_prelu contract)."""
        c = v.shape[0]
        out = torch.zeros((c + mult - 1) // mult * mult, dtype=torch.float32, device=self.device)
        out[:c] = v.detach()
        return out

    # ------------------------------------------------------------------ GEMMs
    @staticmethod
    def _gemm_sink(p: "GemmParams", sink: Optional[Planes], rows: int, cout: int, c0: int, gc: int, groups: int, what: str):
        """Fill the plane-sink fields of ``p``: ``rows`` output rows (per group) x ``cout`` channels at channel offset ``c0``
        (+ ``gc`` per row group) of ``sink``."""
        if sink is None:
            return
        if p.precision != 1:
            raise ValueError(f"{what}: a plane sink needs the f16x3 engine")
        top = c0 + (groups - 1) * gc + cout
        if sink.rows != rows or c0 % 4 or gc % 4 or top > sink.chunks * 32:
            raise ValueError(f"{what}: plane sink [{sink.rows},{sink.c}] cannot take {rows} rows x {cout} channels at offset {c0} (+{gc} per group)")
        p.out_hi, p.out_lo = sink.t[0].data_ptr(), sink.t[1].data_ptr()
        p.out_plane_rows, p.out_plane_c0, p.out_plane_gc = sink.ld_rows, c0, gc

    def conv(self, x, w: PackedWeight, out, stride=1, pad=1, dil=1, bias=None, prelu=None, in_prelu=None,
             planes: Optional[Planes] = None, planes_prelu=None, planes_c0: int = 0, out_shape=None):
        """``planes``: also write the result as split planes, at channel offset ``planes_c0``; through ``planes_prelu`` (3x3 / stride 1
        f16x3 kernel only).  ``out`` may be None (planes only; generic GEMM path) when ``out_shape`` = (N, Ho, Wo, Cout) is given."""
        ld, n, h, wd, cin = nhwc_view(x, "conv.in")
        if out is None:
            if planes is None or out_shape is None:
                raise ValueError("conv: no output")
            old, (on, oh, ow, cout) = 0, out_shape
        else:
            old, on, oh, ow, cout = nhwc_view(out, "conv.out")
        if cin != w.cin or cout != w.cout or on != n or w.mode != GEMM_CONV:
            raise ValueError(f"conv: shape mismatch in {tuple(x.shape)} w ({w.cout},{w.cin},{w.kh},{w.kw}) out {(on, oh, ow, cout)}")
        meta = {"flops": 2.0 * n * oh * ow * cout * cin * w.kh * w.kw,
                "bytes": 4.0 * (n * h * wd * cin + n * oh * ow * cout + cout * cin * w.kh * w.kw),
                "shape": f"M{n * oh * ow} N{cout} K{cin * w.kh * w.kw}"}
        if (self.precision == "f16x3" and w.hi3 is not None and w.kh == 3 and stride == 1 and pad == 1 and dil == 1
                and in_prelu is None and out is not None and planes_c0 == 0):
            if planes is not None and (planes.rows < n * h * wd or planes.c != cout):
                raise ValueError(f"conv: plane sink [{planes.rows},{planes.c}] does not match {n * h * wd} pixels x {cout} channels")
            if planes is not None and planes_prelu is not None and planes_prelu.numel() < (cout + 31) // 32 * 32:
                raise ValueError("conv: planes_prelu must be padded to a multiple of 32 channels")
            self._run("conv3x3_f16x3", meta, self.lib.atmvfi_conv3x3_f16x3, _ptr(x), ld, n, h, wd, cin, _ptr(w.hi3), _ptr(w.lo3),
                      cout, _ptr(out), old, _ptr(bias), _ptr(prelu),
                      _ptr(planes.t[0]) if planes is not None else None, _ptr(planes.t[1]) if planes is not None else None,
                      planes.ld_rows if planes is not None else 0, _ptr(planes_prelu) if planes is not None else None,
                      *(self.conv3_instance or (-1, 0)), self._stream())
            return
        if planes is not None and planes_prelu is not None:
            raise ValueError("conv: planes_prelu needs the 3x3 / stride-1 f16x3 kernel")
        p = GemmParams(mode=GEMM_CONV, in_=x.data_ptr(), in_ld=ld, N=n, H=h, W=wd, Cin=cin, in_gstride=0, in_rpg=0,
                       weight=w.packed.data_ptr(), Cout=cout, kh=w.kh, kw=w.kw, stride=stride, pad=pad, dil=dil,
                       Ho=oh, Wo=ow, M=n * oh * ow, out=None if out is None else out.data_ptr(), out_ld=old, out_gstride=0, out_rpg=0,
                       out_row_map=None, bias=_ptr(bias), prelu=_ptr(prelu), in_prelu=_ptr(in_prelu), residual=None, res_ld=0)
        p.precision, p.weight_hi, p.weight_lo = self._prec(w)
        p.tile_wn = self.gemm_tile_wn
        self._gemm_sink(p, planes, n * oh * ow, cout, planes_c0, 0, 1, "conv")
        p._srcs = (x, out, bias, prelu, in_prelu)
        self._run("conv2d_f16x3" if p.precision else "conv2d", meta, self.lib.atmvfi_conv2d, ctypes.byref(p), self._stream())

    def _gemm_splitk(self, p: "GemmParams", m: int, ngemm: int, ksteps: int):
        """Give the launch split-K scratch when the launcher would use it (under-filled grid, long K); returns the tensor (kept alive by
        the caller's workspace) or None."""
        if self.gemm_workspace is None or p.precision != 1 or not p.in_hi or p.tile_wn != 0:
            return None
        need = int(self.lib.atmvfi_gemm_workspace_floats(m, ngemm, ksteps))
        if not need:
            return None
        ws = self.gemm_workspace(need)
        if ws is None:
            return None
        p.workspace, p.workspace_floats = ws.data_ptr(), ws.numel()
        return ws

    def pack_stem(self, w1, b1, p1, w2, b2, p2, w3, b3, p3) -> "StemWeights":
        """The operand layouts of ``atmvfi_stem_fused`` (include/atmvfi.h) from the nine parameters of feat_extracts.0.0 / 0.1 / 1.0
        (weight, bias, PReLU slope each): fp16 hi / lo' planes [k-step][cout][32] with k = (ky * 3 + kx) * Cin + c (layer 1: one
        k-step of 27 values).  Host-side torch ops, once per parameter version (like the q / kv stacking in ``_prepare``)."""
        c0, c1 = w2.shape[0], w3.shape[0]
        if tuple(w1.shape) != (c0, 3, 3, 3) or tuple(w2.shape) != (c0, c0, 3, 3) or tuple(w3.shape) != (c1, c0, 3, 3):
            raise ValueError("pack_stem: expected 3 -> C0 -> C0 -> C1 3x3 weights")
        ns = (9 * c0 + 31) // 32

        def planes_of(w, rows):
            k = w.detach().float().permute(0, 2, 3, 1).reshape(w.shape[0], 9 * c0)          # [cout][(ky, kx, c)]
            full = torch.zeros(rows, ns * 32, dtype=torch.float32, device=self.device)
            full[:w.shape[0], :9 * c0] = k
            full = full.reshape(rows, ns, 32).permute(1, 0, 2).contiguous()                  # [k-step][cout][32]
            hi = full.half()
            lo = ((full - hi.float()) * 1024.0).half()
            return hi, lo

        def padded(v, rows, fill):
            out = torch.full((rows,), fill, dtype=torch.float32, device=self.device)
            out[:v.shape[0]] = v.detach().float()
            return out
        r2 = (c0 + 15) // 16 * 16
        w2h, w2l = planes_of(w2, r2)
        w3h, w3l = planes_of(w3, c1)
        k1 = torch.zeros(r2, 32, dtype=torch.float32, device=self.device)                   # [cout][(ky, kx, ci)], 27 values
        k1[:c0, :27] = w1.detach().float().permute(0, 2, 3, 1).reshape(c0, 27)
        w1h = k1.half()
        w1l = ((k1 - w1h.float()) * 1024.0).half()
        return StemWeights(c0, c1, w1h, w1l, padded(b1, r2, 0.0), padded(p1, r2, 1.0), w2h, w2l, padded(b2, r2, 0.0), padded(p2, r2, 1.0),
                           w3h, w3l, b3.detach().float().contiguous(), p3.detach().float().contiguous())

    def stem_fused(self, x, w: "StemWeights", out: Planes):
        """feat_extracts.0.0 -> 0.1 -> 1.0 (network_base.py:99-110) in one launch: NHWC4 frames [F,H,W,4] -> split planes of the
        half-resolution C1-channel map (rows = pixels (f, y, x))."""
        _chk(x, "stem_fused.x")
        if x.dim() != 4 or x.shape[3] != 4 or not x.is_contiguous():
            raise ValueError(f"stem_fused: expected contiguous NHWC4 frames [F,H,W,4], got {tuple(x.shape)}")
        f, h, wd, _ = x.shape
        if h % 2 or wd % 2 or out.rows != f * (h // 2) * (wd // 2) or out.c != w.c1:
            raise ValueError(f"stem_fused: planes [{out.rows},{out.c}] do not hold {f}x{h // 2}x{wd // 2} pixels x {w.c1} channels")
        if self.precision != "f16x3":
            raise ValueError("stem_fused: needs the f16x3 engine")
        flops = 2.0 * f * h * wd * (27 * w.c0 + 9 * w.c0 * w.c0) + 2.0 * f * (h // 2) * (wd // 2) * 9 * w.c0 * w.c1
        meta = {"flops": flops, "bytes": 16.0 * f * h * wd + 4.0 * out.rows * out.chunks * 32, "shape": f"{f}x{h}x{wd} 3>{w.c0}>{w.c0}>{w.c1}s2"}
        self._run("stem_fused", meta, self.lib.atmvfi_stem_fused, _ptr(x), f, h, wd, w.c0, w.c1, _ptr(w.w1h), _ptr(w.w1l), _ptr(w.b1), _ptr(w.p1),
                  _ptr(w.w2h), _ptr(w.w2l), _ptr(w.b2), _ptr(w.p2), _ptr(w.w3h), _ptr(w.w3l), _ptr(w.b3), _ptr(w.p3),
                  _ptr(out.t[0]), _ptr(out.t[1]), out.ld_rows, self._stream())

    def conv3x3_planes(self, x: Planes, n: int, h: int, wd: int, w: PackedWeight, out=None, bias=None, prelu=None,
                       planes: Optional[Planes] = None, planes_c0: int = 0, planes_prelu=None, in_chunk0: int = 0, cin: Optional[int] = None,
                       wn: int = 0, out_cmin: int = 0, planes2: Optional[Planes] = None, planes2_c0: int = 0,
                       workspace: Optional[torch.Tensor] = None):
        """3x3 / stride 1 / pad 1 conv (+bias, PReLU) on split-plane input ``x`` (rows = pixels of an [n,h,wd] map; channels
        ``32*in_chunk0 .. +cin``).  ``out``: fp32 NHWC view or None; ``planes``: plane sink written at channel offset ``planes_c0``
        (its own ``planes_prelu`` applied to that copy only); ``planes2``: a second, raw plane sink.  ``out_cmin``: only channels >= it are stored in ``out``.  Needs the spare
        zero row of ``Planes.alloc``.  ``workspace``: fp32 scratch of at least ``conv3x3_workspace_floats(...)`` elements: lets the launcher
        split K over idle CUs on under-filled grids (split-K with a fixed-order reduce; small frames)."""
        cin = (x.c - 32 * in_chunk0) if cin is None else cin
        if self.precision != "f16x3" or w.hi3 is None:
            raise ValueError("conv3x3_planes: needs the f16x3 engine and the conv3x3 weight planes")
        if w.mode != GEMM_CONV or w.kh != 3 or w.kw != 3 or w.cin != cin:
            raise ValueError(f"conv3x3_planes: weight ({w.cout},{w.cin},{w.kh},{w.kw}) does not match Cin {cin}")
        if x.rows != n * h * wd or x.ld_rows <= x.rows or 32 * in_chunk0 + cin > x.chunks * 32:
            raise ValueError(f"conv3x3_planes: input planes [{x.rows} (+{x.ld_rows - x.rows} spare), {x.c}] do not fit {n}x{h}x{wd} pixels x {cin} channels "
                             "(one spare zero row is required)")
        cout = w.cout
        old = out_addr = 0
        if out is not None:
            old, on, oh, ow, oc = nhwc_view(out, "conv3x3_planes.out")
            # the block takes the address of the first STORED channel: the start of a compact buffer of just the channels [out_cmin, cout),
            # column out_cmin of a full-width view (out_cmin % 4 == 0 keeps the 16-byte alignment)
            if (on, oh, ow) == (n, h, wd) and oc == cout - out_cmin and out_cmin > 0:
                out_addr = out.data_ptr()
            elif (on, oh, ow, oc) == (n, h, wd, cout):
                out_addr = out.data_ptr() + 4 * out_cmin
            else:
                raise ValueError(f"conv3x3_planes: out {tuple(out.shape)} != [{n},{h},{wd},{cout}] (or {cout - out_cmin} channels: compact)")
        elif planes is None:
            raise ValueError("conv3x3_planes: no output")
        if planes is not None:
            if planes.rows != n * h * wd or planes_c0 % 8 or planes_c0 + cout > planes.chunks * 32:
                raise ValueError(f"conv3x3_planes: plane sink [{planes.rows},{planes.c}] cannot take {cout} channels at offset {planes_c0}")
            if planes_prelu is not None and planes_prelu.numel() < (cout + 31) // 32 * 32:
                raise ValueError("conv3x3_planes: planes_prelu must be padded to a multiple of 32 channels")
        if planes2 is not None and (planes is None or planes2.rows != n * h * wd or planes2_c0 % 8 or planes2_c0 + cout > planes2.chunks * 32):
            raise ValueError(f"conv3x3_planes: second plane sink [{planes2.rows},{planes2.c}] needs the first one and room for {cout} channels at {planes2_c0}")
        meta = {"flops": 2.0 * n * h * wd * cout * cin * 9, "bytes": 4.0 * (n * h * wd * (cin + cout) + cout * cin * 9),
                "shape": f"M{n * h * wd} N{cout} K{cin * 9}"}
        coff = in_chunk0 * x.ld_rows * 32 * 2       # bytes
        if workspace is not None and (workspace.dtype != torch.float32 or not workspace.is_cuda or not workspace.is_contiguous()):
            raise ValueError("conv3x3_planes: the split-K workspace must be a contiguous CUDA fp32 tensor")
        if self.plane_terms not in (1, 3):
            raise ValueError(f"plane_terms must be 3 (f16x3) or 1 (f16), got {self.plane_terms!r}")
        p = Conv3pParams(in_hi=x.t[0].data_ptr() + coff, in_lo=x.t[1].data_ptr() + coff, in_rows=x.ld_rows, N=n, H=h, W=wd, Cin=cin,
                         w_hi=w.hi3.data_ptr(), w_lo=w.lo3.data_ptr(), Cout=cout, bias=_ptr(bias), prelu=_ptr(prelu),
                         out=out_addr or None, out_ld=old, out_cmin=out_cmin, out_c0=planes_c0, out_c02=planes2_c0, wn=wn,
                         workspace=_ptr(workspace), workspace_floats=workspace.numel() if workspace is not None else 0, terms=self.plane_terms)
        if planes is not None:
            p.out_hi, p.out_lo, p.plane_rows, p.plane_prelu = planes.t[0].data_ptr(), planes.t[1].data_ptr(), planes.ld_rows, _ptr(planes_prelu)
        if planes2 is not None:
            p.out_hi2, p.out_lo2, p.plane_rows2 = planes2.t[0].data_ptr(), planes2.t[1].data_ptr(), planes2.ld_rows
        p._srcs = (x.t, w.hi3, w.lo3, out, bias, prelu, planes.t if planes is not None else None, planes_prelu,
                   planes2.t if planes2 is not None else None, workspace)
        self._run("conv3x3_planes", meta, self.lib.atmvfi_conv3p, ctypes.byref(p), self._stream())

    def pack_readout(self, w: torch.Tensor) -> torch.Tensor:
        """The ``readout_w`` operand of ``atmvfi_conv3p``: refine_head.1's weight [3, C, 3, 3] (C = 32 or 64) as the 27 x C matrix
        W2[(tap, o)][c], hi / lo' split, in the producing kernel's register order: fp16 [plane][row tile 2][k-step C / 32][lane][8] with
        lane = 16 g + r -> row 16 t + r, and the lane's eight k values = its four channels of n-tile 2 kk and of n-tile 2 kk + 1
        (channels 32 kk + cb(g) + e and 32 kk + 16 + cb(g) + e, cb = {0, 8, 4, 12}[g]).  Host-side torch ops, once per parameter version."""
        o3, c, kh, kw = w.shape
        if (o3, kh, kw) != (3, 3, 3) or c not in (32, 64):
            raise ValueError(f"pack_readout: expected a [3, 32 | 64, 3, 3] weight, got {tuple(w.shape)}")
        w2 = torch.zeros(32, c, dtype=torch.float32, device=self.device)
        w2[:27] = w.detach().float().permute(2, 3, 0, 1).reshape(27, c)            # row = (ky * 3 + kx) * 3 + o
        kk_n = c // 32
        lane = torch.arange(64, device=self.device)
        r, g = lane & 15, lane >> 4
        cb = 8 * (g & 1) + 4 * (g >> 1)
        e = torch.arange(8, device=self.device)
        ch = cb[:, None] + torch.where(e < 4, e, 16 + e - 4)[None, :]            # [lane, 8] channel inside a 32-channel k-step
        full = torch.empty(2, kk_n, 64, 8, dtype=torch.float32, device=self.device)
        for t in range(2):
            for kk in range(kk_n):
                full[t, kk] = w2[(16 * t + r)[:, None].expand(64, 8), 32 * kk + ch]
        hi = full.half()
        lo = ((full - hi.float()) * 1024.0).half()
        return torch.stack([hi, lo], 0).contiguous()

    def conv3x3_planes_readout(self, x: Planes, n: int, h: int, wd: int, w: PackedWeight, bias, prelu, w2: torch.Tensor, contrib: torch.Tensor):
        """refine_head.0 (3x3 conv + PReLU on split-plane input, Cout 32 or 64) with refine_head.1's 27 tap contributions per pixel
        computed in its epilogue: contrib [27, n*h*wd] planar fp32 (include/atmvfi.h)."""
        if self.precision != "f16x3" or w.hi3 is None or w.kh != 3 or w.cin > x.chunks * 32 or x.rows != n * h * wd or x.ld_rows <= x.rows:
            raise ValueError("conv3x3_planes_readout: needs the f16x3 engine, conv3x3 weight planes and input planes with a spare zero row")
        if w.cout not in (32, 64) or tuple(w2.shape) != (2, 2, w.cout // 32, 64, 8) or w2.dtype != torch.float16:
            raise ValueError("conv3x3_planes_readout: Cout must be 32 or 64 and w2 the pack_readout() operand of that width")
        if contrib.dtype != torch.float32 or contrib.dim() != 2 or contrib.shape[0] != 27 or contrib.shape[1] < n * h * wd or not contrib.is_contiguous():
            raise ValueError("conv3x3_planes_readout: contrib must be contiguous fp32 [27, >= N*H*W]")
        meta = {"flops": 2.0 * n * h * wd * w.cout * (w.cin * 9 + 27), "bytes": 4.0 * n * h * wd * (w.cin + 27), "shape": f"M{n * h * wd} N{w.cout} K{w.cin * 9} +27"}
        if self.plane_terms not in (1, 3):
            raise ValueError(f"plane_terms must be 3 (f16x3) or 1 (f16), got {self.plane_terms!r}")
        p = Conv3pParams(in_hi=x.t[0].data_ptr(), in_lo=x.t[1].data_ptr(), in_rows=x.ld_rows, N=n, H=h, W=wd, Cin=w.cin,
                         w_hi=w.hi3.data_ptr(), w_lo=w.lo3.data_ptr(), Cout=w.cout, bias=_ptr(bias), prelu=_ptr(prelu),
                         readout_w=w2.data_ptr(), readout=contrib.data_ptr(), readout_plane=contrib.shape[1], terms=self.plane_terms)
        p._srcs = (x.t, w.hi3, w.lo3, bias, prelu, w2, contrib)
        self._run("conv3x3_planes", meta, self.lib.atmvfi_conv3p, ctypes.byref(p), self._stream())

    def refine_tail(self, contrib, bias, slope, it, it_sum, it_clamped):
        """out = clamp(it + 2 * sigmoid(PReLU(bias + sum of the nine shifted tap contributions)) - 1): refine_head.1 + the residual."""
        _planar(it, 3, "refine_tail.it"); _planar(it_sum, 3, "refine_tail.sum"); _planar(it_clamped, 3, "refine_tail.clamped")
        b, _, h, w = it.shape
        if contrib.dim() != 2 or contrib.shape[0] != 27 or contrib.shape[1] < b * h * w or not contrib.is_contiguous():
            raise ValueError("refine_tail: contrib must be contiguous fp32 [27, >= B*H*W]")
        self._run("refine_tail", {"bytes": 4.0 * b * h * w * (27 + 9)}, self.lib.atmvfi_refine_tail, _ptr(contrib), contrib.shape[1], _ptr(bias),
                  _ptr(slope), _ptr(it), _ptr(it_sum), _ptr(it_clamped), b, h, w, self._stream())

    def conv3x3_workspace_floats(self, n: int, h: int, wd: int, cin: int, cout: int) -> int:
        """fp32 elements of split-K scratch ``conv3x3_planes`` wants for this shape on this device (0: it would not split)."""
        return int(self.lib.atmvfi_conv3x3_planes_workspace_floats(n, h, wd, cin, cout))

    def head1x1_planes(self, x: Planes, n: int, h: int, wd: int, w: PackedWeight, out, bias=None):
        """nn.Conv2d(Cin, Cout <= 8, 1) on split-plane input (the 5-channel read-out of a motion MLP): one lane per pixel row, fp32 FMAs."""
        old, on, oh, ow, oc = nhwc_view(out, "head1x1_planes.out")
        if w.mode != GEMM_CONV or w.kh != 1 or w.cout > 8 or (on, oh, ow, oc) != (n, h, wd, w.cout) or x.rows != n * h * wd or w.cin > x.chunks * 32:
            raise ValueError(f"head1x1_planes: weight ({w.cout},{w.cin},{w.kh},{w.kw}) / out {tuple(out.shape)} / planes [{x.rows},{x.c}] mismatch")
        wt = w.orig.detach()
        if not wt.is_contiguous():
            wt = wt.contiguous()
        meta = {"flops": 2.0 * n * h * wd * w.cout * w.cin, "bytes": 4.0 * n * h * wd * (w.cin + w.cout), "shape": f"M{n * h * wd} N{w.cout} K{w.cin}"}
        self._run("head1x1_planes", meta, self.lib.atmvfi_head1x1_planes, _ptr(x.t[0]), _ptr(x.t[1]), x.ld_rows, n * h * wd, w.cin,
                  _ptr(wt), _ptr(bias), w.cout, _ptr(out), old, self._stream())

    def conv_planes(self, x: Planes, n: int, h: int, wd: int, w: PackedWeight, out=None, stride=1, pad=1, dil=1, bias=None, prelu=None,
                    sink: Optional[Planes] = None, sink_c0: int = 0, in_chunk0: int = 0, x2: Optional[Planes] = None, x2_chunk0: int = 0,
                    split_chunks: int = 0):
        """Conv2d (k 1 or 3, any stride / dilation; + bias, PReLU) on split-plane input through the LDS-DMA GEMM's CONV mode: rows of
        ``x`` = pixels of an [n,h,wd] map, channels from 32-channel chunk ``in_chunk0`` on.  With ``x2`` the first ``split_chunks``
        chunks come from ``x`` and the rest from ``x2`` (chunk ``x2_chunk0`` on): a channel concat that never materialises.
        ``out``: fp32 NHWC view or None; ``sink``: plane sink at channel ``sink_c0``.  Needs the spare zero row of ``Planes.alloc``."""
        if self.precision != "f16x3" or w.hi is None or w.mode != GEMM_CONV:
            raise ValueError("conv_planes: needs the f16x3 engine and split conv weights")
        cin, cout = w.cin, w.cout
        oh = (h + 2 * pad - dil * (w.kh - 1) - 1) // stride + 1
        ow = (wd + 2 * pad - dil * (w.kw - 1) - 1) // stride + 1
        c1 = 32 * split_chunks if x2 is not None else cin
        for t, c0, cc, what in ((x, in_chunk0, c1, "x"),) + (((x2, x2_chunk0, cin - c1, "x2"),) if x2 is not None else ()):
            if t.rows != n * h * wd or t.ld_rows <= t.rows or 32 * c0 + cc > t.chunks * 32:
                raise ValueError(f"conv_planes: {what} [{t.rows} (+{t.ld_rows - t.rows} spare), {t.c}] does not hold {n}x{h}x{wd} pixels x "
                                 f"{cc} channels from chunk {c0} (one spare zero row is required)")
        if x2 is not None and not 0 < 32 * split_chunks < cin:
            raise ValueError("conv_planes: split_chunks must cut the input channels at a 32-channel boundary inside (0, Cin)")
        old = 0
        if out is not None:
            old, on, ooh, oow, oc = nhwc_view(out, "conv_planes.out")
            if (on, ooh, oow, oc) != (n, oh, ow, cout):
                raise ValueError(f"conv_planes: out {tuple(out.shape)} != [{n},{oh},{ow},{cout}]")
        elif sink is None:
            raise ValueError("conv_planes: no output")
        p = GemmParams(mode=GEMM_CONV, in_=None, in_ld=x.ld_rows, N=n, H=h, W=wd, Cin=cin, in_gstride=0, in_rpg=0,
                       weight=w.packed.data_ptr(), Cout=cout, kh=w.kh, kw=w.kw, stride=stride, pad=pad, dil=dil,
                       Ho=oh, Wo=ow, M=n * oh * ow, out=None if out is None else out.data_ptr(), out_ld=old, out_gstride=0, out_rpg=0,
                       out_row_map=None, bias=_ptr(bias), prelu=_ptr(prelu), in_prelu=None, residual=None, res_ld=0)
        p.precision, p.weight_hi, p.weight_lo = 1, w.hi.data_ptr(), w.lo.data_ptr()
        off = in_chunk0 * x.ld_rows * 64
        p.in_hi, p.in_lo = x.t[0].data_ptr() + off, x.t[1].data_ptr() + off
        if x2 is not None:
            off2 = x2_chunk0 * x2.ld_rows * 64
            p.in_hi2, p.in_lo2, p.in_ld2, p.in_split_chunks = x2.t[0].data_ptr() + off2, x2.t[1].data_ptr() + off2, x2.ld_rows, split_chunks
        p.tile_wn = self.gemm_tile_wn if self.gemm_tile_wn < 0 else 0        # -1: the reference schedule (gemm_split.hip)
        self._gemm_sink(p, sink, n * oh * ow, cout, sink_c0, 0, 1, "conv_planes")
        meta = {"flops": 2.0 * n * oh * ow * cout * cin * w.kh * w.kw, "bytes": 4.0 * (n * h * wd * cin + n * oh * ow * cout + cout * cin * w.kh * w.kw),
                "shape": f"M{n * oh * ow} N{cout} K{cin * w.kh * w.kw}"}
        ws = self._gemm_splitk(p, n * oh * ow, cout, w.kh * w.kw * ((cin + 31) // 32))
        p._srcs = (out, bias, prelu, ws)
        self._plane_prec(p)
        self._run("conv2d_split", meta, self.lib.atmvfi_conv2d, ctypes.byref(p), self._stream())

    def deconv(self, x, w: PackedWeight, out, bias=None, prelu=None, in_prelu=None, planes: Optional[Planes] = None,
               sink: Optional[Planes] = None, sink_c0: int = 0, in_shape=None):
        """``planes``: the input rows [N*H*W, Cin] again in split-plane form (already through in_prelu): the LDS-DMA GEMM
        then replaces the fp32-input engine (``x`` may then be None with ``in_shape`` = (N, H, W, Cin)).  ``sink``: also write the
        result as split planes at channel offset ``sink_c0`` (``out`` may then be None)."""
        if x is None:
            if planes is None or in_shape is None:
                raise ValueError("deconv: no input")
            ld, (n, h, wd, cin) = 0, in_shape
        else:
            ld, n, h, wd, cin = nhwc_view(x, "deconv.in")
        cout = w.cout
        if out is None:
            if sink is None:
                raise ValueError("deconv: no output")
            old, on, oh, ow = 0, n, 2 * h, 2 * wd
        else:
            old, on, oh, ow, oc = nhwc_view(out, "deconv.out")
            if oc != cout:
                raise ValueError(f"deconv: out has {oc} channels, weight {cout}")
        if cin != w.cin or on != n or w.mode != GEMM_DECONV or oh != 2 * h or ow != 2 * wd:
            raise ValueError(f"deconv: shape mismatch in {(n, h, wd, cin)} w ({w.cin},{w.cout}) out {(on, oh, ow, cout)}")
        p = GemmParams(mode=GEMM_DECONV, in_=None if x is None else x.data_ptr(), in_ld=ld, N=n, H=h, W=wd, Cin=cin, in_gstride=0, in_rpg=0,
                       weight=w.packed.data_ptr(), Cout=cout, kh=2, kw=2, stride=2, pad=0, dil=1, Ho=oh, Wo=ow,
                       M=n * h * wd, out=None if out is None else out.data_ptr(), out_ld=old, out_gstride=0, out_rpg=0, out_row_map=None,
                       bias=_ptr(bias), prelu=_ptr(prelu), in_prelu=_ptr(in_prelu), residual=None, res_ld=0)
        p.precision, p.weight_hi, p.weight_lo = self._prec(w)
        p.tile_wn = self.gemm_tile_wn
        self._gemm_sink(p, sink, n * oh * ow, cout, sink_c0, 0, 1, "deconv")
        use_planes = planes is not None and p.precision == 1
        if x is None and not use_planes:
            raise ValueError("deconv: plane input needs the f16x3 engine")
        if use_planes:
            if planes.rows < n * h * wd or planes.c != cin:
                raise ValueError("deconv: planes do not match the input rows")
            p.in_, p.in_ld, p.in_prelu = None, planes.ld_rows, None
            p.in_hi, p.in_lo = planes.t[0].data_ptr(), planes.t[1].data_ptr()
        meta = {"flops": 2.0 * n * h * wd * 4 * cout * cin, "bytes": 4.0 * (n * h * wd * cin + n * oh * ow * cout + 4 * cout * cin),
                "shape": f"M{n * h * wd} N{4 * cout} K{cin}"}
        ws = self._gemm_splitk(p, n * h * wd, 4 * ((cout + 3) // 4 * 4), (cin + 31) // 32) if use_planes else None
        p._srcs = (x, out, bias, prelu, in_prelu, ws)
        self._plane_prec(p)
        self._run("deconv2x2_split" if use_planes else "deconv2x2_f16x3" if p.precision else "deconv2x2", meta, self.lib.atmvfi_deconv2x2,
                  ctypes.byref(p), self._stream())

    split_planes_ok = True        # this backend has the split-plane sinks and the LDS-DMA GEMM
    pyramid_packs = True          # image_pyramid(pack=...) does pack_frames' work in the same launch

    def split_planes(self, x, out: Planes, prelu=None, c0: Optional[int] = None):
        """fp32 rows -> split planes, optionally through a per-channel PReLU first.  ``c0``: write the channels at this offset
        (multiple of 8) of wider planes and leave everything else alone (zero fill only up to the next multiple of 8)."""
        ld, m, c, gs, _ = rows_view(x, "split_planes.in")
        if gs != 0 or m != out.rows or (c0 is None and c != out.c) or (c0 is not None and (c0 % 8 or c0 + c > out.chunks * 32)):
            raise ValueError("split_planes: expected a plain [rows,C] view matching the planes")
        if prelu is not None and prelu.numel() < c:
            raise ValueError("split_planes: prelu needs one slope per channel")
        meta = {"bytes": 4.0 * m * c + 4.0 * m * ((c + 31) // 32 * 32 if c0 is None else (c + 7) // 8 * 8)}
        if c0 is None:
            self._run("split_planes", meta, self.lib.atmvfi_split_planes, _ptr(x), ld, m, c, _ptr(prelu), _ptr(out.t[0]),
                      _ptr(out.t[1]), out.ld_rows, self._stream())
        else:
            self._run("split_planes", meta, self.lib.atmvfi_split_planes_at, _ptr(x), ld, m, c, _ptr(prelu), _ptr(out.t[0]),
                      _ptr(out.t[1]), out.ld_rows, c0, 8, self._stream())

    def linear(self, x, w: PackedWeight, out, bias=None, residual=None, out_row_map=None, sink: Optional[Planes] = None,
               sink_c0: int = 0, sink_gc: int = 0):
        """``sink``: also write the result as split planes: output row r (after ``out_row_map``; of its row group when ``out`` is a
        grouped [G,R,C] view) at channel ``sink_c0`` (+ ``sink_gc`` per group)."""
        planes = x if isinstance(x, Planes) else None
        if planes is not None:
            if self.precision != "f16x3" or w.hi is None:
                raise ValueError("linear: split-plane input needs the f16x3 engine and split weights")
            ld, m, cin, gs, rpg = planes.ld_rows, planes.rows, planes.c, 0, 0
        else:
            ld, m, cin, gs, rpg = rows_view(x, "linear.in")
        old, mo, cout, ogs, orpg = rows_view(out, "linear.out")
        if cin != w.cin or cout != w.cout or w.kh != 1 or w.mode == GEMM_DECONV:
            raise ValueError(f"linear: shape mismatch in {tuple(x.shape)} w ({w.cout},{w.cin}) out {tuple(out.shape)}")
        if out_row_map is None and mo != m:
            raise ValueError("linear: row count mismatch")
        if out_row_map is not None and (out_row_map.numel() != m or out_row_map.dtype != torch.int32 or not out_row_map.is_cuda):
            raise ValueError("linear: out_row_map must be a CUDA int32 tensor with one entry per GEMM row")
        res_ld = 0
        if residual is not None:
            res_ld, rm, rc, rgs, _ = rows_view(residual, "linear.residual")
            if rm != m or rc != cout or rgs != 0:
                raise ValueError("linear: residual must be a plain [M,Cout] view")
        p = GemmParams(mode=GEMM_LINEAR, in_=None if planes is not None else x.data_ptr(), in_ld=ld, N=1, H=1, W=1, Cin=cin, in_gstride=gs, in_rpg=rpg,
                       weight=w.packed.data_ptr(), Cout=cout, kh=1, kw=1, stride=1, pad=0, dil=1, Ho=1, Wo=1, M=m,
                       out=out.data_ptr(), out_ld=old, out_gstride=ogs, out_rpg=orpg, out_row_map=_ptr(out_row_map),
                       bias=_ptr(bias), prelu=None, in_prelu=None, residual=_ptr(residual), res_ld=res_ld)
        p.precision, p.weight_hi, p.weight_lo = self._prec(w)
        p.tile_wn = self.gemm_tile_wn
        if planes is not None:
            p.in_hi, p.in_lo = planes.t[0].data_ptr(), planes.t[1].data_ptr()
        if sink is not None:
            self._gemm_sink(p, sink, orpg if orpg else mo, cout, sink_c0, sink_gc, (mo // orpg) if orpg else 1, "linear")
        meta = {"flops": 2.0 * m * cout * cin, "bytes": 4.0 * (m * cin + m * cout + cout * cin), "shape": f"M{m} N{cout} K{cin}"}
        ws = self._gemm_splitk(p, m, cout, (cin + 31) // 32) if planes is not None else None
        p._srcs = (None if planes is not None else x, out, bias, residual, out_row_map, ws)
        self._plane_prec(p)
        self._run("linear_split" if planes is not None else "linear_f16x3" if p.precision else "linear", meta, self.lib.atmvfi_linear, ctypes.byref(p), self._stream())

    # ------------------------------------------------------------- transformer
    @staticmethod
    def _sink(planes: Optional[Planes], rows: int, c: int, what: str):
        """(hi, lo, ld) arguments of a kernel's split-plane sink (all null when the caller wants fp32 only)."""
        if planes is None:
            return None, None, 0
        if planes.rows != rows or planes.c != c:
            raise ValueError(f"{what}: planes hold {planes.rows} x {planes.c}, kernel writes {rows} x {c}")
        return _ptr(planes.t[0]), _ptr(planes.t[1]), planes.ld_rows

    def layernorm(self, x, out, gamma, beta, src_row_map=None, planes: Optional[Planes] = None):
        """``out`` (fp32 rows) may be None when only the split planes are wanted."""
        ld, m, c, gs, rpg = rows_view(x, "layernorm.in")
        if out is None:
            if planes is None:
                raise ValueError("layernorm: no output")
            old, mo, co, ogs = 0, planes.rows, planes.c, 0
        else:
            old, mo, co, ogs, _ = rows_view(out, "layernorm.out")
        if co != c or ogs != 0:
            raise ValueError("layernorm: output must be a plain [rows,C] view")
        if src_row_map is None and mo != m:
            raise ValueError("layernorm: row count mismatch")
        if src_row_map is not None and src_row_map.numel() != mo:
            raise ValueError("layernorm: src_row_map needs one entry per output row")
        hi, lo, pld = self._sink(planes, mo, c, "layernorm")
        meta = {"bytes": 4.0 * mo * c * (1 + (out is not None) + (planes is not None))}
        self._run("layernorm", meta, self.lib.atmvfi_layernorm, _ptr(x), ld, gs, rpg, _ptr(src_row_map), _ptr(out), old,
                  _ptr(gamma), _ptr(beta), mo, c, hi, lo, pld, self._stream())

    def dwconv_gelu(self, x, out, w9, bias, planes: Optional[Planes] = None):
        ld, n, h, w, c = nhwc_view(x, "dwconv.in")
        old = 0
        if out is not None:
            old, on, oh, ow, oc = nhwc_view(out, "dwconv.out")
            if (on, oh, ow, oc) != (n, h, w, c):
                raise ValueError("dwconv: shape mismatch")
        elif planes is None:
            raise ValueError("dwconv: no output")
        hi, lo, pld = self._sink(planes, n * h * w, c, "dwconv")
        meta = {"bytes": 4.0 * n * h * w * c * (1 + (out is not None) + (planes is not None))}
        self._run("dwconv3x3_gelu", meta, self.lib.atmvfi_dwconv3x3_gelu, _ptr(x), ld, _ptr(out), old, _ptr(w9), _ptr(bias),
                  n, h, w, c, hi, lo, pld, self._stream())

    def window_attention(self, qkv, out, motion, labels, bw, nw, ws, heads, hd, kv_shift, planes: Optional[Planes] = None):
        _chk(qkv, "attn.qkv")
        n = ws * ws
        c = heads * hd
        if out is None and planes is None:
            raise ValueError("window_attention: no output")
        if out is not None:
            _chk(out, "attn.out")
        if tuple(qkv.shape) != (bw * n, 3 * c) or not qkv.is_contiguous() or (
                out is not None and (tuple(out.shape) != (bw * n, c) or not out.is_contiguous())):
            raise ValueError(f"window_attention: qkv {tuple(qkv.shape)} / out do not match Bw {bw} N {n} C {c}")
        if motion is not None and (tuple(motion.shape) != (bw * n, heads, 2) or not motion.is_contiguous()):
            raise ValueError("window_attention: motion must be contiguous [Bw*N, heads, 2]")
        if labels is not None and (tuple(labels.shape) != (nw, n) or labels.dtype != torch.int32 or not labels.is_cuda):
            raise ValueError("window_attention: labels must be CUDA int32 [nW, N]")
        meta = {"flops": 4.0 * bw * heads * n * n * hd, "bytes": 4.0 * bw * n * 4 * c}
        hi, lo, pld = self._sink(planes, bw * n, c, "window_attention")
        fn = self.lib.atmvfi_window_attention_f16x3 if self.precision == "f16x3" and self.attention_f16x3 else self.lib.atmvfi_window_attention
        self._run("window_attention", meta, fn, _ptr(qkv), _ptr(out), _ptr(motion), _ptr(labels),
                  bw, nw, ws, heads, hd, kv_shift, hi, lo, pld, self._stream())

    def motion_head(self, motion, row_map, w0, b0, w1, b1, out, planes: Optional[Planes] = None, planes_c0: int = 0, planes_gc: int = 0):
        """``planes``: also write the two values as split planes -- channel ``planes_c0`` (+ ``planes_gc`` per row group of ``out``),
        plane row = the row inside its group."""
        old, mo, co, ogs, orpg = rows_view(out, "motion_head.out")
        rows = motion.shape[0]
        if co != 2:
            raise ValueError("motion_head: output view must have 2 channels")
        if planes is not None:
            groups = (mo // orpg) if orpg else 1
            if planes.rows != (orpg if orpg else mo) or planes_c0 % 2 or planes_gc % 2 or planes_c0 + (groups - 1) * planes_gc + 2 > planes.chunks * 32:
                raise ValueError("motion_head: the plane sink must hold one row per row of a group and even channel offsets inside its chunks")
        self._run("motion_head", {"bytes": 4.0 * rows * 18}, self.lib.atmvfi_motion_head_planes, _ptr(motion), _ptr(row_map), _ptr(w0),
                  _ptr(b0), _ptr(w1), _ptr(b1), _ptr(out), old, ogs, orpg, rows, motion.shape[1],
                  _ptr(planes.t[0]) if planes is not None else None, _ptr(planes.t[1]) if planes is not None else None,
                  planes.ld_rows if planes is not None else 0, planes_c0, planes_gc, self._stream())

    # ------------------------------------------------------------------ warps
    def _tiled_warp_ok(self, w, *planes) -> bool:
        """The LDS-staged warps (csrc/warp.hip: `atmvfi_flow_warp_tiled`, `atmvfi_flow_warp_up2_tiled`, `atmvfi_warp_blend_tiled`; they share
        the direct ones' taps, sampling and blend, so they are bit-identical to them) take rows by
        16-byte loads: W a multiple of 4, planes 16-byte aligned.  ``warp_tiles = False`` is the A/B switch."""
        return self.warp_tiles and w % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in planes)

    def flow_warp(self, src, flow, dst):
        _chk(src, "flow_warp.src"); _chk(dst, "flow_warp.dst")
        b, c, h, w = src.shape
        if not src.is_contiguous() or not dst.is_contiguous() or tuple(dst.shape) != (b, c, h, w):
            raise ValueError("flow_warp: src/dst must be contiguous NCHW of equal shape")
        bs, ps, cs = flow_view(flow, h, w, "flow_warp.flow")
        meta = {"bytes": 4.0 * b * h * w * (2 * c + 2)}
        fn = self.lib.atmvfi_flow_warp_tiled if self._tiled_warp_ok(w, src) else self.lib.atmvfi_flow_warp
        self._run("flow_warp", meta, fn, _ptr(src), _ptr(flow), bs, ps, cs, _ptr(dst), b, c, h, w, self._stream())

    PADDING_MODES = {"zeros": 0, "border": 1, "reflection": 2}

    def flow_warp_ex(self, src, flow, dst, mask=None, padding_mode="zeros"):
        """flow_warp(feature, flow, mask=..., padding_mode=...) of the reference in its non-default forms (flow_warp.py:50-60):
        contiguous planar src / dst [B,C,H,W], flow [B,2,H,W]; ``mask``: a [B,H,W] bool / uint8 tensor to fill, or None."""
        _chk(src, "flow_warp_ex.src"); _chk(dst, "flow_warp_ex.dst"); _chk(flow, "flow_warp_ex.flow")
        b, c, h, w = src.shape
        if padding_mode not in self.PADDING_MODES:
            raise ValueError(f"flow_warp: padding_mode must be one of {sorted(self.PADDING_MODES)}, got {padding_mode!r}")
        if (not all(t.is_contiguous() for t in (src, flow, dst)) or tuple(dst.shape) != (b, c, h, w) or tuple(flow.shape) != (b, 2, h, w)):
            raise ValueError("flow_warp_ex: contiguous src/dst [B,C,H,W] and flow [B,2,H,W] expected")
        if mask is not None and (mask.device != src.device or not mask.is_contiguous() or tuple(mask.shape) != (b, h, w) or mask.element_size() != 1):
            raise ValueError("flow_warp_ex: mask must be a contiguous [B,H,W] bool / uint8 tensor on the source's device")
        meta = {"bytes": 4.0 * b * h * w * (2 * c + 2)}
        self._run("flow_warp_ex", meta, self.lib.atmvfi_flow_warp_ex, _ptr(src), _ptr(flow), _ptr(dst), 0 if mask is None else mask.data_ptr(),
                  b, c, h, w, self.PADDING_MODES[padding_mode], self._stream())

    def flow_warp_up2(self, src, flow, dst, flow_up):
        """flow_warp(src, flow) -> dst and the flow up-sampled x2 (values doubled) -> flow_up, one launch; all contiguous planar."""
        b, c, h, w = src.shape
        if (not all(t.is_contiguous() for t in (src, flow, dst, flow_up)) or tuple(dst.shape) != (b, c, h, w) or tuple(flow.shape) != (b, 2, h, w)
                or tuple(flow_up.shape) != (b, 2, 2 * h, 2 * w)):
            raise ValueError("flow_warp_up2: contiguous src/dst [B,C,H,W], flow [B,2,H,W], flow_up [B,2,2H,2W] expected")
        meta = {"bytes": 4.0 * b * h * w * (2 * c + 2 + 8)}
        fn = self.lib.atmvfi_flow_warp_up2_tiled if self._tiled_warp_ok(w, src) else self.lib.atmvfi_flow_warp_up2
        self._run("flow_warp_up2", meta, fn, _ptr(src), _ptr(flow), _ptr(dst), _ptr(flow_up), b, c, h, w, self._stream())

    def flow_warp_nhwc(self, src, flow, dst):
        ld, b, h, w, c = nhwc_view(src, "flow_warp_nhwc.src")
        old, ob, oh, ow, oc = nhwc_view(dst, "flow_warp_nhwc.dst")
        if (ob, oh, ow, oc) != (b, h, w, c):
            raise ValueError("flow_warp_nhwc: shape mismatch")
        bs, ps, cs = flow_view(flow, h, w, "flow_warp_nhwc.flow")
        meta = {"bytes": 4.0 * b * h * w * (2 * c + 2)}
        self._run("flow_warp_nhwc", meta, self.lib.atmvfi_flow_warp_nhwc, _ptr(src), ld, src.stride(0), _ptr(flow), bs, ps, cs,
                  _ptr(dst), old, dst.stride(0), b, c, h, w, self._stream())

    def warp_blend(self, im0, im1, motion, i0w, i1w, it, flow0=None, flow1=None, mask1=None, mask2=None,
                   orig0=None, orig1=None, pack15=None, pack_planes: Optional[Planes] = None, pack_c0: int = 0):
        _planar(im0, 3, "warp_blend.im0"); _planar(im1, 3, "warp_blend.im1")
        b, _, h, w = im0.shape
        mld, mb, mh, mw, mc = nhwc_view(motion, "warp_blend.motion")
        if (mb, mh, mw, mc) != (b, h, w, 5):
            raise ValueError(f"warp_blend: motion view {tuple(motion.shape)} != [{b},{h},{w},5]")
        for t in (i0w, i1w, it):
            _planar(t, 3, "warp_blend.out")
        pld = 0
        if pack15 is not None:
            pld, pb, ph, pw, pc = nhwc_view(pack15, "warp_blend.pack15")
            if (pb, ph, pw, pc) != (b, h, w, 15):
                raise ValueError("warp_blend: pack15 view must be [B,H,W,15]")
            _planar(orig0, 3, "warp_blend.orig0"); _planar(orig1, 3, "warp_blend.orig1")
        # algorithmic bytes per pixel: two 3-channel sources + 5 motion channels read, three 3-channel frames written; the finest
        # level also writes the two flows and two masks (6 floats) and -- for the refiner -- reads the two original frames (6) and
        # writes the 15-channel pack (fp32 NHWC, or 16 channels of split planes at the same 4 bytes per element)
        per_px = 6 + 5 + 9 + (6 if flow0 is not None else 0) + ((6 + 15) if pack15 is not None else 0) + ((6 + 16) if pack_planes is not None else 0)
        meta = {"bytes": 4.0 * b * h * w * per_px}
        if pack_planes is not None:
            if pack_planes.rows != b * h * w or pack_c0 % 4 or pack_c0 + 16 > pack_planes.chunks * 32:
                raise ValueError("warp_blend: the plane sink must hold B*H*W rows and 16 channels at the offset")
            _planar(orig0, 3, "warp_blend.orig0"); _planar(orig1, 3, "warp_blend.orig1")
        fn = self.lib.atmvfi_warp_blend_tiled if self._tiled_warp_ok(w, im0, im1) else self.lib.atmvfi_warp_blend_planes
        self._run("warp_blend", meta, fn, _ptr(im0), _ptr(im1), _ptr(motion), mld, motion.stride(0),
                  _ptr(i0w), _ptr(i1w), _ptr(it), _ptr(flow0), _ptr(flow1), _ptr(mask1), _ptr(mask2), _ptr(orig0), _ptr(orig1),
                  _ptr(pack15), pld, _ptr(pack_planes.t[0]) if pack_planes is not None else None,
                  _ptr(pack_planes.t[1]) if pack_planes is not None else None,
                  pack_planes.ld_rows if pack_planes is not None else 0, pack_c0, b, h, w, self._stream())

    def resize(self, src, dst, value_scale=1.0):
        """src: any [B,C,Hi,Wi] strided view; dst: contiguous planar [B,C,Ho,Wo]."""
        _chk(src, "resize.src"); _chk(dst, "resize.dst")
        b, c, hi, wi = src.shape
        if not dst.is_contiguous() or dst.shape[0] != b or dst.shape[1] != c:
            raise ValueError("resize: dst must be contiguous [B,C,Ho,Wo]")
        meta = {"bytes": 4.0 * b * c * (hi * wi + dst.shape[2] * dst.shape[3])}
        self._run("resize_bilinear_ac", meta, self.lib.atmvfi_resize_bilinear_ac, _ptr(src), src.stride(0), src.stride(1),
                  src.stride(2), src.stride(3), _ptr(dst), b, c, hi, wi, dst.shape[2], dst.shape[3], float(value_scale), self._stream())

    def image_pyramid(self, im0, im1, l1, l2, l3, pack=None):
        """The x0.5 pyramid levels 1..3 of both frames in one launch: im0 / im1 contiguous [B,3,H,W]; l1..l3 contiguous [2B,3,H>>l,W>>l].
        ``pack``: also write torch.cat([im0, im1], 0) as NHWC4 [2B,H,W,4] (``pack_frames``' output) in the same launch."""
        b, c, h, w = im0.shape
        if pack is not None and (tuple(pack.shape) != (2 * b, h, w, 4) or not pack.is_contiguous()):
            raise ValueError("image_pyramid: pack must be contiguous [2B,H,W,4]")
        for t, l in ((l1, 1), (l2, 2), (l3, 3)):
            if not t.is_contiguous() or tuple(t.shape) != (2 * b, 3, h >> l, w >> l):
                raise ValueError(f"image_pyramid: level {l} must be contiguous [{2 * b},3,{h >> l},{w >> l}], got {tuple(t.shape)}")
        if c != 3 or im1.shape != im0.shape or not im0.is_contiguous() or not im1.is_contiguous():
            raise ValueError("image_pyramid: frames must be contiguous [B,3,H,W]")
        meta = {"bytes": 4.0 * 2 * b * 3 * h * w * (1 + 0.25 + 0.0625 + 0.015625) + (4.0 * 2 * b * h * w * 7 if pack is not None else 0.0)}
        self._run("image_pyramid", meta, self.lib.atmvfi_image_pyramid_pack, _ptr(im0), _ptr(im1), _ptr(l1), _ptr(l2), _ptr(l3), _ptr(pack),
                  b, h, w, self._stream())

    def frame_u8_to_f32(self, src_u8, dst, pad_top: int, pad_left: int, bgr: bool):
        """uint8 [H,W,3] device tensor -> fp32 planar [3,Hp,Wp] (x / 255, replicate padding, optional BGR -> RGB)."""
        _u8_frame(src_u8, "frame_u8_to_f32: source")
        _f32_canvas(dst, "frame_u8_to_f32: destination")
        h, w = src_u8.shape[:2]
        self._run("frame_u8_to_f32", {"bytes": 3.0 * h * w + 12.0 * dst.shape[1] * dst.shape[2]}, self.lib.atmvfi_frame_u8_to_f32,
                  _ptr(src_u8), h, w, int(bgr), _ptr(dst), dst.shape[1], dst.shape[2], pad_top, pad_left, self._stream())

    def frame_u8_window(self, src_u8, mode: int, y0: int, x0: int, h: int, w: int, dst=None, dst_u8=None, pad_top: int = 0,
                        pad_left: int = 0, bgr: bool = False):
        """One resident uint8 [H,W,3] frame -> the h x w window at (y0, x0) (``mode`` 0) or the 2x area reduction of the 2h x 2w window
        there (``mode`` 1: (a + b + c + d + 2) >> 2, cv2.INTER_AREA at scale 2), as ``dst`` fp32 planar [3,Hp,Wp] (q / 255, replicate
        padding, the window at (pad_top, pad_left)) and / or ``dst_u8`` uint8 [h,w,3] RGB (include/atmvfi.h atmvfi_frame_u8_window)."""
        _u8_frame(src_u8, "frame_u8_window: source")
        if dst is None and dst_u8 is None:
            raise ValueError("frame_u8_window: give dst, dst_u8 or both")
        if dst is not None:
            _f32_canvas(dst, "frame_u8_window: dst")
        if dst_u8 is not None:
            _u8_frame(dst_u8, "frame_u8_window: dst_u8", (h, w))
        sh, sw = src_u8.shape[:2]
        hp, wp = (dst.shape[1], dst.shape[2]) if dst is not None else (h + pad_top, w + pad_left)
        scale = 2 if mode == 1 else 1
        meta = {"bytes": 3.0 * scale * scale * h * w + (12.0 * hp * wp if dst is not None else 0.0) + (3.0 * h * w if dst_u8 is not None else 0.0)}
        self._run("frame_u8_window", meta, self.lib.atmvfi_frame_u8_window, _ptr(src_u8), sh, sw, int(bgr), int(mode), int(y0), int(x0),
                  int(h), int(w), _ptr(dst), hp, wp, int(pad_top), int(pad_left), _ptr(dst_u8), self._stream())

    def frame_signature_workspace(self, h: int, w: int):
        """A fresh int32 scratch tensor for ``frame_signature`` on an h x w window (one per stream that computes signatures)."""
        n = self.lib.atmvfi_frame_signature_workspace_ints(int(h), int(w))
        if n < 0:
            raise ValueError(f"frame_signature: {self.lib.atmvfi_last_error().decode()}")
        return torch.empty(n, dtype=torch.int32, device=self.device)

    def frame_signature(self, src_u8, y0: int = 0, x0: int = 0, h: Optional[int] = None, w: Optional[int] = None, bgr: bool = False,
                        out=None, workspace=None):
        """The scene-cut signature of the h x w window at (y0, x0) (default: the whole frame) of a resident uint8 [H,W,3] frame: int32
        [288] on the device = 16 x 16 luma cell sums + 32 luma bins (include/atmvfi.h atmvfi_frame_signature; the bits of
        ``scene.signature_numpy``).  ``out`` is written completely (a new tensor when None).  ``workspace``: the call's scratch
        (``frame_signature_workspace``); None: one kept per (window size, stream) by this object.  Not part of a forward: never recorded
        into a launch plan."""
        _u8_frame(src_u8, "frame_signature: source")
        sh, sw = src_u8.shape[:2]
        h = sh - int(y0) if h is None else int(h)
        w = sw - int(x0) if w is None else int(w)
        if out is None:
            out = torch.empty(288, dtype=torch.int32, device=src_u8.device)
        elif out.dtype != torch.int32 or out.numel() != 288 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("frame_signature: out must be a contiguous CUDA int32 tensor of 288 words")
        if workspace is None:
            cache = self.__dict__.setdefault("_signature_workspaces", {})
            key = (h, w, torch.cuda.current_stream(self.device).cuda_stream)
            workspace = cache.get(key)
            if workspace is None:
                workspace = cache[key] = self.frame_signature_workspace(h, w)
        elif workspace.dtype != torch.int32 or not workspace.is_contiguous() or not workspace.is_cuda:
            raise ValueError("frame_signature: workspace must be a contiguous CUDA int32 tensor")
        self._check(self.lib.atmvfi_frame_signature(_ptr(src_u8), sh, sw, int(bool(bgr)), int(y0), int(x0), h, w, _ptr(out), _ptr(workspace),
                                                    workspace.numel(), self._stream()), "frame_signature")
        return out

    def frame_difference_workspace(self, h: int, w: int):
        """A fresh int32 scratch tensor for ``frame_difference`` on an h x w window (one per stream that computes differences)."""
        n = self.lib.atmvfi_frame_difference_workspace_ints(int(h), int(w))
        if n < 0:
            raise ValueError(f"frame_difference: {self.lib.atmvfi_last_error().decode()}")
        return torch.empty(n, dtype=torch.int32, device=self.device)

    def frame_difference(self, a, b, y0: int = 0, x0: int = 0, h: Optional[int] = None, w: Optional[int] = None, bgr: bool = True,
                         out=None, workspace=None):
        """The luma difference of the h x w window at (y0, x0) (default: the whole frame) of two resident uint8 [H,W,3] frames of one
        size: int32 [258] on the device = 16 x 16 cell sums of |Ya - Yb|, the peak, the number of differing pixels (include/atmvfi.h
        atmvfi_frame_difference; the bits of ``retime.difference_numpy``).  ``out`` is written completely (a new tensor when None).
        ``workspace``: the call's scratch (``frame_difference_workspace``); None: one kept per (window size, stream) by this object.
        Not part of a forward: never recorded into a launch plan."""
        if not (_is_u8_frame(a) and _is_u8_frame(b)):
            raise ValueError("frame_difference: sources must be contiguous CUDA uint8 [H,W,3] tensors")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError(f"frame_difference: two frames of one size on one device expected, got {tuple(a.shape)} and {tuple(b.shape)}")
        sh, sw = a.shape[:2]
        h = sh - int(y0) if h is None else int(h)
        w = sw - int(x0) if w is None else int(w)
        if out is None:
            out = torch.empty(258, dtype=torch.int32, device=a.device)
        elif out.dtype != torch.int32 or out.numel() != 258 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("frame_difference: out must be a contiguous CUDA int32 tensor of 258 words")
        if workspace is None:
            cache = self.__dict__.setdefault("_difference_workspaces", {})
            key = (h, w, torch.cuda.current_stream(self.device).cuda_stream)
            workspace = cache.get(key)
            if workspace is None:
                workspace = cache[key] = self.frame_difference_workspace(h, w)
        elif workspace.dtype != torch.int32 or not workspace.is_contiguous() or not workspace.is_cuda:
            raise ValueError("frame_difference: workspace must be a contiguous CUDA int32 tensor")
        self._check(self.lib.atmvfi_frame_difference(_ptr(a), _ptr(b), sh, sw, int(bool(bgr)), int(y0), int(x0), h, w, _ptr(out),
                                                     _ptr(workspace), workspace.numel(), self._stream()), "frame_difference")
        return out

    def frame_borders_workspace(self, h: int, w: int):
        """A fresh int32 scratch tensor for ``frame_borders`` on an h x w frame (one per stream that computes borders)."""
        n = self.lib.atmvfi_frame_borders_workspace_ints(int(h), int(w))
        if n < 0:
            raise ValueError(f"frame_borders: {self.lib.atmvfi_last_error().decode()}")
        return torch.empty(n, dtype=torch.int32, device=self.device)

    def frame_borders(self, src_u8, bgr: bool = False, out=None, workspace=None):
        """The line maxima of a resident uint8 [H,W,3] frame: int32 [H + W] on the device = the largest luma of every row, then of
        every column (include/atmvfi.h atmvfi_frame_borders; the bits of ``active.borders_numpy``).  ``out`` is written completely (a
        new tensor when None).  ``workspace``: the call's scratch (``frame_borders_workspace``); None: one kept per (frame size,
        stream) by this object.  Not part of a forward: never recorded into a launch plan."""
        _u8_frame(src_u8, "frame_borders: source")
        sh, sw = src_u8.shape[:2]
        if out is None:
            out = torch.empty(sh + sw, dtype=torch.int32, device=src_u8.device)
        elif out.dtype != torch.int32 or out.numel() != sh + sw or not out.is_contiguous() or not out.is_cuda:
            raise ValueError(f"frame_borders: out must be a contiguous CUDA int32 tensor of H + W = {sh + sw} words")
        if workspace is None:
            cache = self.__dict__.setdefault("_borders_workspaces", {})
            key = (sh, sw, torch.cuda.current_stream(self.device).cuda_stream)
            workspace = cache.get(key)
            if workspace is None:
                workspace = cache[key] = self.frame_borders_workspace(sh, sw)
        elif workspace.dtype != torch.int32 or not workspace.is_contiguous() or not workspace.is_cuda:
            raise ValueError("frame_borders: workspace must be a contiguous CUDA int32 tensor")
        self._check(self.lib.atmvfi_frame_borders(_ptr(src_u8), sh, sw, int(bool(bgr)), _ptr(out), _ptr(workspace), workspace.numel(),
                                                  self._stream()), "frame_borders")
        return out

    def frame_compose(self, dst_u8, border_u8, window, src=None, win_u8=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False):
        """A produced window back into a full frame: ``dst_u8`` (uint8 [H,W,3]) = the bytes of ``border_u8`` (uint8 [H,W,3], the
        caller's channel order) outside ``window`` = (y0, x0, h, w) and, inside, ``frame_f32_to_u8``'s pixel of ``src`` (fp32 planar
        [3,Hp,Wp], the window at (pad_top, pad_left); BGR if ``bgr``) or the bytes of ``win_u8`` (uint8 [h,w,3], already in output
        order) -- exactly one (include/atmvfi.h atmvfi_frame_compose; the bits of ``active.compose_numpy``).  ``dst_u8`` must not
        alias ``border_u8``.  Not part of a forward: never recorded into a launch plan."""
        _u8_frame(dst_u8, "frame_compose: dst")
        _u8_frame(border_u8, "frame_compose: border", tuple(dst_u8.shape[:2]))
        if (src is None) == (win_u8 is None):
            raise ValueError("frame_compose: give exactly one of src and win_u8")
        y0, x0, h, w = (int(v) for v in window)
        hp = wp = 0
        if src is not None:
            _f32_canvas(src, "frame_compose: src")
            hp, wp = src.shape[1:]
        else:
            _u8_frame(win_u8, "frame_compose: win_u8", (h, w))
        sh, sw = dst_u8.shape[:2]
        self._check(self.lib.atmvfi_frame_compose(_ptr(dst_u8), _ptr(border_u8), sh, sw, y0, x0, h, w, _ptr(src), hp, wp, int(pad_top),
                                                  int(pad_left), _ptr(win_u8), int(bool(bgr)), self._stream()), "frame_compose")

    def yuv_borders_workspace(self, h: int, w: int):
        """A fresh int32 scratch tensor for ``yuv_borders`` on an h x w frame of either depth (one per stream that computes borders)."""
        n = self.lib.atmvfi_yuv_borders_workspace_ints(int(h), int(w))
        if n < 0:
            raise ValueError(f"yuv_borders: {self.lib.atmvfi_last_error().decode()}")
        return torch.empty(n, dtype=torch.int32, device=self.device)

    def yuv_borders(self, buf, fmt_or_surface, out=None, workspace=None):
        """The line maxima of the LUMA plane of one resident frame of ``fmt_or_surface`` (a ``yuv.Format`` or ``yuv.Surface``; ``buf`` its
        bytes, a contiguous CUDA uint8 tensor, any alignment and pitch -- an uploaded surface in place): int32 [H + W] on the device = the
        largest luma sample value of every row, then of every column (``msb``: ``>> 6``; include/atmvfi.h atmvfi_yuv_borders; the bits
        of ``active.yuv_borders_numpy``).  Chroma is not read.  ``out`` is written completely (a new tensor when None).
        ``workspace``: the call's scratch (``yuv_borders_workspace``); None: one kept per (frame size, stream) by this object.  Not part
        of a forward: never recorded into a launch plan."""
        if not hasattr(fmt_or_surface, "subsampling_id"):
            raise ValueError(f"yuv_borders: a yuv.Format or yuv.Surface expected (got {type(fmt_or_surface).__name__})")
        s = as_surface(fmt_or_surface)
        _yuv_buf(buf, s, "yuv_borders", "source")
        sh, sw = s.height, s.width
        if out is None:
            out = torch.empty(sh + sw, dtype=torch.int32, device=buf.device)
        elif out.dtype != torch.int32 or out.numel() != sh + sw or not out.is_contiguous() or not out.is_cuda:
            raise ValueError(f"yuv_borders: out must be a contiguous CUDA int32 tensor of H + W = {sh + sw} words")
        if workspace is None:
            cache = self.__dict__.setdefault("_yuv_borders_workspaces", {})
            key = (sh, sw, torch.cuda.current_stream(self.device).cuda_stream)
            workspace = cache.get(key)
            if workspace is None:
                workspace = cache[key] = self.yuv_borders_workspace(sh, sw)
        elif workspace.dtype != torch.int32 or not workspace.is_contiguous() or not workspace.is_cuda:
            raise ValueError("yuv_borders: workspace must be a contiguous CUDA int32 tensor")
        self._check(self.lib.atmvfi_yuv_borders(ctypes.byref(s.desc_block), _ptr(buf), _ptr(out), _ptr(workspace), workspace.numel(),
                                                self._stream()), "yuv_borders")
        return out

    def _packed_pair(self, who: str, packed, buf, planar):
        """the two byte tensors of ``yuv_unpack`` / ``yuv_pack`` checked against ``packed`` (a missing one, the call's output, is made)"""
        if not isinstance(packed, Packed):
            raise ValueError(f"{who}: a yuv.Packed expected (got {type(packed).__name__})")
        mk = lambda n: torch.empty(n, dtype=torch.uint8, device=self.device)
        buf = mk(packed.nbytes) if buf is None else buf
        planar = mk(packed.planar.frame_bytes) if planar is None else planar
        for t, n, role in ((buf, packed.nbytes, f"{packed.layout} frame (pitch {packed.pitch})"),
                           (planar, packed.planar.frame_bytes, "planar 4:2:2 frame")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"{who}: the {role} must be a contiguous CUDA uint8 tensor of {n} bytes ({packed.height} x {packed.width}, "
                                 f"depth {packed.depth})")
        return buf, planar

    def yuv_unpack(self, buf, packed, dst=None):
        """One packed 4:2:2 frame of ``packed`` (a ``yuv.Packed``: uyvy, yuy2, y210 or v210 at its pitch; ``buf`` its bytes on the
        device) -> ``dst``, the bytes of the planar 4:2:2 frame of ``packed.planar`` (a new tensor when None): the sample values,
        moved; padding is never read (include/atmvfi.h atmvfi_yuv_unpack; the bits of ``yuv.unpack_numpy``).  Not part of a forward:
        never recorded into a launch plan."""
        buf, dst = self._packed_pair("yuv_unpack", packed, buf, dst)
        self._check(self.lib.atmvfi_yuv_unpack(_ptr(buf), packed.height, packed.width, packed.layout_id, int(packed.pitch), _ptr(dst),
                                               self._stream()), "yuv_unpack")
        return dst

    def yuv_pack(self, planar, packed, dst=None):
        """The bytes of one planar 4:2:2 frame of ``packed.planar`` -> ``dst``, one frame of the TIGHT ``packed`` (a new tensor when
        None): the sample values, moved; every byte of ``dst`` is written, what holds no sample as zero (include/atmvfi.h
        atmvfi_yuv_pack; the bits of ``yuv.pack_numpy``).  Not part of a forward: never recorded into a launch plan."""
        if isinstance(packed, Packed) and not packed.is_tight:
            raise ValueError("yuv_pack: packed must be at its default pitch (packs write no custom pitch: packed.tight())")
        dst, planar = self._packed_pair("yuv_pack", packed, dst, planar)
        self._check(self.lib.atmvfi_yuv_pack(_ptr(planar), packed.height, packed.width, packed.layout_id, _ptr(dst), self._stream()),
                    "yuv_pack")
        return dst

    def yuv_compose(self, dst, out_surface, border, border_surface, window, src=None, src_u8=None, pad_top: int = 0, pad_left: int = 0):
        """A produced window back into a full YUV frame: ``dst`` (one frame of the TIGHT ``out_surface``, a ``yuv.Format`` or
        ``yuv.Surface``) = the samples of ``border`` (one frame of ``border_surface``: the same size, depth, subsampling, chroma layout
        and msb, any pitch -- the uploaded source frame in place) outside ``window`` = (y0, x0, h, w), verbatim, and inside exactly
        what ``yuv_encode`` writes for the h x w picture as a frame of ``out_surface.cropped(h, w)`` -- from ``src`` (fp32 planar
        [3,Hp,Wp], the window at (pad_top, pad_left)) or ``src_u8`` (uint8 [h,w,3] RGB, depth 8 only), exactly one.  The window begins
        and ends on multiples of the subsampling step or at the frame's edge (include/atmvfi.h atmvfi_yuv_compose; the bits of
        ``active.yuv_compose_numpy``).  ``dst`` must not overlap ``border``.  Never recorded into a launch plan."""
        for d in (out_surface, border_surface):
            if not hasattr(d, "subsampling_id"):
                raise ValueError(f"yuv_compose: a yuv.Format or yuv.Surface expected (got {type(d).__name__})")
        o, b = as_surface(out_surface), as_surface(border_surface)
        if not o.is_tight:
            raise ValueError("yuv_compose: out_surface must be tight (no padding is written: surface.tight())")
        if (o.fmt, o.chroma, o.msb) != (b.fmt, b.chroma, b.msb):
            raise ValueError(f"yuv_compose: border_surface must be of the output's size, format, chroma layout and msb (got {b} for {o})")
        _yuv_buf(dst, o, "yuv_compose", "destination")
        _yuv_buf(border, b, "yuv_compose", "border")
        if (src is None) == (src_u8 is None):
            raise ValueError("yuv_compose: give exactly one of src and src_u8")
        y0, x0, h, w = _window("yuv_compose", o, window)
        hp = wp = 0
        if src is not None:
            _f32_canvas(src, "yuv_compose", ": src")
            hp, wp = src.shape[1:]
        else:
            if o.depth != 8:
                raise ValueError("yuv_compose: src_u8 goes into 8-bit frames only (a 10-bit frame takes the fp32 src)")
            _u8_frame(src_u8, "yuv_compose", (h, w), ": src_u8")
        self._check(self.lib.atmvfi_yuv_compose(ctypes.byref(b.desc_block), _ptr(dst), _ptr(border), y0, x0, h, w, _ptr(src), hp, wp, int(pad_top),
                                                int(pad_left), _ptr(src_u8), self._stream()), "yuv_compose")

    def shutter_accumulate(self, acc, src=None, src_u8=None, weight: int = 1, light: str = "linear", first: bool = False, pad_top: int = 0,
                           pad_left: int = 0, bgr: bool = False):
        """One sample of a blurred output into its accumulator: ``acc`` (contiguous CUDA int32 [3,h,w], always R, G, B) ``=`` (``first``:
        nothing is read, nothing needs zeroing) or ``+=`` ``weight * LUT[q]``, q the uint8 pixel of ``src`` -- fp32 planar RGB
        [3,Hp,Wp] with the window at (pad_top, pad_left): ``frame_f32_to_u8``'s pixel -- or of ``src_u8`` -- uint8 [h,w,3], BGR if
        ``bgr`` -- exactly one (include/atmvfi.h atmvfi_shutter_accumulate; ``shutter.blend_numpy`` is the host twin).  Not part of a
        forward: never recorded into a launch plan."""
        from .shutter import LIGHTS
        if acc.dtype != torch.int32 or acc.dim() != 3 or acc.shape[0] != 3 or not acc.is_contiguous() or not acc.is_cuda:
            raise ValueError("shutter_accumulate: acc must be a contiguous CUDA int32 [3,h,w] tensor")
        if (src is None) == (src_u8 is None):
            raise ValueError("shutter_accumulate: give exactly one of src and src_u8")
        if light not in LIGHTS:
            raise ValueError(f"shutter_accumulate: light must be one of {LIGHTS}, got {light!r}")
        h, w = acc.shape[1:]
        hp = wp = 0
        if src is not None:
            _f32_canvas(src, "shutter_accumulate: src")
            hp, wp = src.shape[1:]
        else:
            _u8_frame(src_u8, "shutter_accumulate: src_u8", (h, w))
        self._check(self.lib.atmvfi_shutter_accumulate(_ptr(acc), h, w, _ptr(src), hp, wp, int(pad_top), int(pad_left), _ptr(src_u8),
                                                       int(bool(bgr)), int(weight), LIGHTS.index(light), int(bool(first)), self._stream()),
                    "shutter_accumulate")

    def shutter_resolve(self, acc, total_weight: int, dst_u8, light: str = "linear", bgr: bool = False):
        """``acc`` (int32 [3,h,w], the sum of ``shutter_accumulate`` calls whose weights add up to ``total_weight``) -> ``dst_u8`` uint8
        [h,w,3] (BGR if ``bgr``): the rounded mean in the light table's domain and the nearest code (include/atmvfi.h
        atmvfi_shutter_resolve).  Never recorded into a launch plan."""
        from .shutter import LIGHTS
        if acc.dtype != torch.int32 or acc.dim() != 3 or acc.shape[0] != 3 or not acc.is_contiguous() or not acc.is_cuda:
            raise ValueError("shutter_resolve: acc must be a contiguous CUDA int32 [3,h,w] tensor")
        if light not in LIGHTS:
            raise ValueError(f"shutter_resolve: light must be one of {LIGHTS}, got {light!r}")
        h, w = acc.shape[1:]
        _u8_frame(dst_u8, "shutter_resolve: dst_u8", (h, w))
        self._check(self.lib.atmvfi_shutter_resolve(_ptr(acc), h, w, int(total_weight), LIGHTS.index(light), _ptr(dst_u8), int(bool(bgr)),
                                                    self._stream()), "shutter_resolve")

    def shutter_table(self, light: str):
        """The library's literal light table as a tuple of 256 ints (``shutter.SHUTTER_TABLES[light]`` on the host side)."""
        from .shutter import LIGHTS
        if light not in LIGHTS:
            raise ValueError(f"shutter_table: light must be one of {LIGHTS}, got {light!r}")
        out = (ctypes.c_uint16 * 256)()
        self._check(self.lib.atmvfi_shutter_table(LIGHTS.index(light), out), "shutter_table")
        return tuple(out)

    # The YUV wrappers: one validator and one launch per direction; the validator also accounts meta["bytes"].  A wrapper adds the
    # refusals that are its own and launches under its own name with the canvas the validator returns (the window is the wrapper's: the
    # frame, or a caller's through ``_window``).  ``desc`` is a pixfmt.Format or Surface (they answer to the same names); its
    # ``desc_block`` (include/atmvfi.h atmvfi_yuv_desc) is built once per descriptor and goes to the library by address.  Both run on
    # every frame of a video loop at every size, so they stay flat: positional arguments, nothing computed that a refusal alone needs.
    @staticmethod
    def _decode_sinks(name, dst_u8, dst, wh, ww, pad_top, pad_left, lib_geometry=False):
        """-> (hp, wp, bytes written): the canvas of a decode of a ``wh`` x ``ww`` window (the window itself without ``dst``) and what its
        outputs weigh.  ``lib_geometry``: whether the canvas holds the window is left to the library (``RuntimeError``), else refused
        here (``ValueError``)."""
        nbytes = 0.0
        if dst is None:
            hp, wp = wh, ww
        else:
            _f32_canvas(dst, name, ": dst")
            _, hp, wp = dst.shape
            if not lib_geometry and (pad_top < 0 or pad_left < 0 or wh + pad_top > hp or ww + pad_left > wp):
                raise ValueError(f"{name}: canvas {hp} x {wp} is smaller than the window {wh} x {ww} plus padding ({pad_top}, {pad_left})")
            nbytes += 12.0 * hp * wp
        if dst_u8 is not None:
            _u8_frame(dst_u8, name, (wh, ww), ": dst_u8")
            nbytes += 3.0 * wh * ww
        return hp, wp, nbytes

    def _yuv_decode_args(self, name, buf, desc, dst_u8, dst, y0, x0, wh, ww, pad_top, pad_left, keep=False, area=1, lib_geometry=False):
        """-> (hp, wp, meta): the canvas and ``meta`` for ``_run`` of a decode of the window ``wh`` x ``ww`` at (y0, x0), in output pixels
        (ints; ``_window`` has held a caller's to the frame), which reads ``area`` source pixels each.  ``lib_geometry``: yuv420_to_rgb
        and yuv420_window (``_decode_sinks``)."""
        _yuv_buf(buf, desc, name, "source")
        if dst is None and dst_u8 is None:
            raise ValueError(f"{name}: give dst, dst_u8 or both")
        if keep:
            if desc.depth != 10:
                raise ValueError(f"{name}: keep_depth needs a 10-bit surface")
            if dst_u8 is not None:
                raise ValueError(f"{name}: dst_u8 holds 8-bit pixels: not with keep_depth")
        if (y0 | x0) & 1:       # (only an odd coordinate can break the origin rule of a subsampling)
            err = _origin_error(name, desc, y0, x0)
            if err is not None:
                raise err
        hp, wp, nbytes = self._decode_sinks(name, dst_u8, dst, wh, ww, pad_top, pad_left, lib_geometry)
        return hp, wp, {"bytes": nbytes + _SAMPLES_PER_PIXEL[desc.subsampling] * (2 if desc.depth == 10 else 1) * area * wh * ww}

    def _yuv_encode_args(self, name, buf, desc, src_u8, src, pad_top, pad_left):
        """-> (hp, wp, meta): the source's size and ``meta`` for ``_run``; the destination is the tight frame of ``desc``."""
        h, w = desc.height, desc.width
        n = _yuv_buf(buf, desc, name, "destination")
        if (src is None) == (src_u8 is None):
            raise ValueError(f"{name}: give exactly one of src_u8 and src")
        if src is not None:
            _f32_canvas(src, name, ": src")
            _, hp, wp = src.shape
            if pad_top < 0 or pad_left < 0 or h + pad_top > hp or w + pad_left > wp:
                raise ValueError(f"{name}: canvas {hp} x {wp} is smaller than the frame {h} x {w} plus padding ({pad_top}, {pad_left})")
            return hp, wp, {"bytes": n + 12.0 * h * w}
        if desc.depth != 8:
            raise ValueError(f"{name}: src_u8 encodes 8-bit surfaces only (a 10-bit surface takes the fp32 src)")
        _u8_frame(src_u8, name, (h, w), ": src_u8")
        return h, w, {"bytes": n + 3.0 * h * w}

    def _launch_yuv_decode(self, name, meta, desc, buf, keep, mode, y0, x0, wh, ww, dst_u8, bgr, dst, hp, wp, pad_top, pad_left):
        self._run(name, meta, self.lib.atmvfi_yuv_decode, ctypes.byref(desc.desc_block), _ptr(buf), int(bool(keep)), int(mode), y0, x0, wh, ww,
                  _ptr(dst_u8), int(bool(bgr)), _ptr(dst), hp, wp, int(pad_top), int(pad_left), self._stream())

    def _launch_yuv_encode(self, name, meta, desc, buf, src_u8, bgr, src, hp, wp, pad_top, pad_left):
        self._run(name, meta, self.lib.atmvfi_yuv_encode, ctypes.byref(desc.desc_block), _ptr(src_u8), int(bool(bgr)), _ptr(src), hp, wp,
                  int(pad_top), int(pad_left), _ptr(buf), self._stream())

    def yuv420_to_rgb(self, yuv, fmt, dst_u8=None, dst=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False):
        """One packed planar I420 frame of ``fmt`` (a ``yuv.Format``; a contiguous CUDA uint8 tensor of ``fmt.frame_bytes`` bytes, any
        alignment) -> ``dst_u8`` uint8 [H,W,3] (BGR if ``bgr``) and / or ``dst`` fp32 planar RGB [3,Hp,Wp] = q / 255 with replicate
        padding, the frame at (pad_top, pad_left) (include/atmvfi.h atmvfi_yuv_decode; the bits of ``yuv.decode_numpy``)."""
        if fmt.subsampling != "420":
            raise _not_420("yuv420_to_rgb", fmt)
        h, w = fmt.height, fmt.width
        hp, wp, meta = self._yuv_decode_args("yuv420_to_rgb", yuv, fmt, dst_u8, dst, 0, 0, h, w, pad_top, pad_left, False, 1, True)
        self._launch_yuv_decode("yuv420_to_rgb", meta, fmt, yuv, False, 0, 0, 0, h, w, dst_u8, bgr, dst, hp, wp, pad_top, pad_left)

    def yuv420_window(self, yuv, fmt, mode: int, y0: int, x0: int, h: int, w: int, dst=None, dst_u8=None, pad_top: int = 0,
                      pad_left: int = 0):
        """One packed planar I420 frame of ``fmt`` (as for ``yuv420_to_rgb``) -> what ``frame_u8_window(mode, y0, x0, h, w)`` makes of
        that frame's RGB decode, in one launch and without the RGB frame: ``dst`` fp32 planar [3,Hp,Wp] (q / 255, replicate padding, the
        window at (pad_top, pad_left)) and / or ``dst_u8`` uint8 [h,w,3] RGB.  The origin must be even (include/atmvfi.h
        atmvfi_yuv_decode with ``mode``; the bits of ``yuv.window_numpy``)."""
        if fmt.subsampling != "420":
            raise _not_420("yuv420_window", fmt)
        y0, x0, h, w = int(y0), int(x0), int(h), int(w)
        hp, wp, meta = self._yuv_decode_args("yuv420_window", yuv, fmt, dst_u8, dst, y0, x0, h, w, pad_top, pad_left, False,
                                             4 if mode == 1 else 1, True)
        self._launch_yuv_decode("yuv420_window", meta, fmt, yuv, False, mode, y0, x0, h, w, dst_u8, False, dst, hp, wp, pad_top, pad_left)

    def rgb_to_yuv420(self, yuv, fmt, src_u8=None, src=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False):
        """``src_u8`` uint8 [H,W,3] (BGR if ``bgr``) or ``src`` fp32 planar RGB [3,Hp,Wp] with the frame at (pad_top, pad_left) --
        exactly one -- -> ``yuv``, a packed 8-bit I420 frame of ``fmt`` (a contiguous CUDA uint8 tensor of ``fmt.frame_bytes`` bytes;
        include/atmvfi.h atmvfi_yuv_encode).  From fp32 the pixel is ``frame_f32_to_u8``'s; the bits of ``yuv.encode_numpy``."""
        if fmt.subsampling != "420":
            raise _not_420("rgb_to_yuv420", fmt)
        if fmt.depth != 8:
            raise ValueError("rgb_to_yuv420: encoding is 8-bit only")
        hp, wp, meta = self._yuv_encode_args("rgb_to_yuv420", yuv, fmt, src_u8, src, pad_top, pad_left)
        self._launch_yuv_encode("rgb_to_yuv420", meta, fmt, yuv, src_u8, bgr, src, hp, wp, pad_top, pad_left)

    def yuv420p10_to_f32(self, yuv, fmt, dst, window=None, pad_top: int = 0, pad_left: int = 0):
        """One packed 10-bit I420 frame of ``fmt`` (a ``yuv.Format`` of depth 10; a contiguous CUDA uint8 tensor of ``fmt.frame_bytes``
        bytes, little-endian uint16 samples, any alignment) -> ``dst`` fp32 planar RGB [3,Hp,Wp] = q / 1023 with the depth kept:
        ``window=(y0, x0, h, w)`` of the frame (default: all of it; even origin) at (pad_top, pad_left), replicate padding
        (include/atmvfi.h atmvfi_yuv_decode with ``keep_depth``; the bits of ``yuv.decode_numpy_f32``)."""
        if fmt.subsampling != "420":
            raise _not_420("yuv420p10_to_f32", fmt)
        if fmt.depth != 10:
            raise ValueError("yuv420p10_to_f32: a 10-bit format expected (yuv420_to_rgb decodes 8-bit frames)")
        if dst is None:         # (the one output)
            raise ValueError("yuv420p10_to_f32: dst must be a contiguous CUDA fp32 [3,Hp,Wp] tensor")
        y0, x0, wh, ww = (0, 0, fmt.height, fmt.width) if window is None else _window("yuv420p10_to_f32", fmt, window)
        hp, wp, meta = self._yuv_decode_args("yuv420p10_to_f32", yuv, fmt, None, dst, y0, x0, wh, ww, pad_top, pad_left, True)
        self._launch_yuv_decode("yuv420p10_to_f32", meta, fmt, yuv, True, 0, y0, x0, wh, ww, None, False, dst, hp, wp, pad_top, pad_left)

    def f32_to_yuv420p10(self, yuv, fmt, src, pad_top: int = 0, pad_left: int = 0):
        """``src`` fp32 planar RGB [3,Hp,Wp] with the frame at (pad_top, pad_left) -> ``yuv``, a packed 10-bit I420 frame of ``fmt`` (a
        ``yuv.Format`` of depth 10; a contiguous CUDA uint8 tensor of ``fmt.frame_bytes`` bytes, little-endian uint16 samples;
        include/atmvfi.h atmvfi_yuv_encode).  The pixel is clip(rint(x * 1023), 0, 1023); the bits of ``yuv.encode_numpy`` of
        an fp32 source."""
        if fmt.subsampling != "420":
            raise _not_420("f32_to_yuv420p10", fmt)
        if fmt.depth != 10:
            raise ValueError("f32_to_yuv420p10: a 10-bit format expected (rgb_to_yuv420 encodes 8-bit frames)")
        if src is None:         # (the one source)
            raise ValueError("f32_to_yuv420p10: src must be a contiguous CUDA fp32 [3,Hp,Wp] tensor")
        hp, wp, meta = self._yuv_encode_args("f32_to_yuv420p10", yuv, fmt, None, src, pad_top, pad_left)
        self._launch_yuv_encode("f32_to_yuv420p10", meta, fmt, yuv, None, False, src, hp, wp, pad_top, pad_left)

    def yuv_surface_decode(self, buf, surface, dst_u8=None, dst=None, window=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False,
                           keep_depth: bool = False):
        """One frame of ``surface`` (a ``yuv.Surface``: NV12 / NV21 / P010 / planar, any pitch and chroma offset; ``buf`` a contiguous
        CUDA uint8 tensor of ``surface.nbytes`` bytes, any alignment -- a decoder's surface in place) -> ``window=(y0, x0, h, w)`` of it
        (default: all; even origin) as ``dst`` fp32 planar RGB [3,Hp,Wp] with replicate padding, the window at (pad_top, pad_left), and /
        or ``dst_u8`` uint8 [h,w,3] (BGR if ``bgr``).  ``keep_depth`` (a 10-bit surface, ``dst`` only): q / 1023, otherwise clip8 RGB
        and q / 255 (include/atmvfi.h atmvfi_yuv_decode; the bits of ``yuv.decode_numpy`` / ``decode_numpy_f32``)."""
        s = surface
        if not isinstance(s, Surface):
            raise ValueError(f"yuv_surface_decode: surface must be a yuv.Surface (got {type(s).__name__})")
        if s.subsampling != "420":
            raise _not_420("yuv_surface_decode", s)
        y0, x0, wh, ww = (0, 0, s.height, s.width) if window is None else _window("yuv_surface_decode", s, window)
        hp, wp, meta = self._yuv_decode_args("yuv_surface_decode", buf, s, dst_u8, dst, y0, x0, wh, ww, pad_top, pad_left, keep_depth)
        self._launch_yuv_decode("yuv_surface_decode", meta, s, buf, keep_depth, 0, y0, x0, wh, ww, dst_u8, bgr, dst, hp, wp, pad_top, pad_left)

    def yuv_surface_encode(self, buf, surface, src_u8=None, src=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False):
        """``src_u8`` uint8 [H,W,3] (BGR if ``bgr``; 8-bit surfaces only) or ``src`` fp32 planar RGB [3,Hp,Wp] with the frame at
        (pad_top, pad_left) -- exactly one -- -> ``buf``, one frame of the TIGHT ``surface`` (a contiguous CUDA uint8 tensor of
        ``surface.nbytes`` bytes).  A 10-bit surface is encoded from ``src`` in units of 1 / 1023 (include/atmvfi.h
        atmvfi_yuv_encode; the bits of ``yuv.encode_numpy``)."""
        s = surface
        if not isinstance(s, Surface):
            raise ValueError(f"yuv_surface_encode: surface must be a yuv.Surface (got {type(s).__name__})")
        if not s.is_tight:
            raise ValueError("yuv_surface_encode: surface must be tight (encodes write no padding: surface.tight())")
        if s.subsampling != "420":
            raise _not_420("yuv_surface_encode", s)
        hp, wp, meta = self._yuv_encode_args("yuv_surface_encode", buf, s, src_u8, src, pad_top, pad_left)
        self._launch_yuv_encode("yuv_surface_encode", meta, s, buf, src_u8, bgr, src, hp, wp, pad_top, pad_left)

    def yuv_sub_decode(self, buf, fmt_or_surface, dst_u8=None, dst=None, window=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False,
                       keep_depth: bool = False):
        """``yuv_surface_decode`` for a ``yuv.Format`` or planar ``yuv.Surface`` of any subsampling (4:2:2, 4:4:4; "420" is the surface
        call itself): the window's origin is a multiple of the subsampling step per axis -- even x0 for 4:2:2, anything for 4:4:4
        (include/atmvfi.h atmvfi_yuv_decode; the bits of ``yuv.decode_numpy`` / ``decode_numpy_f32``)."""
        if not hasattr(fmt_or_surface, "subsampling_id"):
            raise ValueError(f"yuv_sub_decode: a yuv.Format or yuv.Surface expected (got {type(fmt_or_surface).__name__})")
        s = as_surface(fmt_or_surface)
        y0, x0, wh, ww = (0, 0, s.height, s.width) if window is None else _window("yuv_sub_decode", s, window)
        hp, wp, meta = self._yuv_decode_args("yuv_sub_decode", buf, s, dst_u8, dst, y0, x0, wh, ww, pad_top, pad_left, keep_depth)
        self._launch_yuv_decode("yuv_sub_decode", meta, fmt_or_surface, buf, keep_depth, 0, y0, x0, wh, ww, dst_u8, bgr, dst, hp, wp, pad_top, pad_left)

    def yuv_sub_encode(self, buf, fmt_or_surface, src_u8=None, src=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False):
        """``yuv_surface_encode`` for a ``yuv.Format`` or tight planar ``yuv.Surface`` of any subsampling (include/atmvfi.h
        atmvfi_yuv_encode; the bits of ``yuv.encode_numpy``)."""
        if not hasattr(fmt_or_surface, "subsampling_id"):
            raise ValueError(f"yuv_sub_encode: a yuv.Format or yuv.Surface expected (got {type(fmt_or_surface).__name__})")
        s = as_surface(fmt_or_surface)
        if not s.is_tight:
            raise ValueError("yuv_sub_encode: surface must be tight (encodes write no padding: surface.tight())")
        hp, wp, meta = self._yuv_encode_args("yuv_sub_encode", buf, s, src_u8, src, pad_top, pad_left)
        self._launch_yuv_encode("yuv_sub_encode", meta, fmt_or_surface, buf, src_u8, bgr, src, hp, wp, pad_top, pad_left)

    def _rgb16_buf(self, who: str, buf, fmt, role: str):
        if not isinstance(fmt, DeepRGB):
            raise ValueError(f"{who}: a yuv.DeepRGB expected (got {type(fmt).__name__})")
        n = fmt.frame_bytes
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() != n or not buf.is_contiguous() or not buf.is_cuda:
            raise ValueError(f"{who}: {role} buf must be a contiguous CUDA uint8 tensor of {n} bytes ({fmt.height} x {fmt.width} {fmt.layout}, "
                             f"depth {fmt.depth})")
        return n

    def rgb16_decode(self, buf, fmt, dst=None, dst_u8=None, window=None, pad_top: int = 0, pad_left: int = 0):
        """One deep RGB frame of ``fmt`` (a ``yuv.DeepRGB``: rgb48, bgr48 or gbrp at 10, 12 or 16 bit; ``buf`` a contiguous CUDA uint8
        tensor of ``fmt.frame_bytes`` bytes, little-endian uint16 samples, 2-byte aligned) -> ``window=(y0, x0, h, w)`` of it (default: all;
        any origin) as ``dst`` fp32 planar RGB [3,Hp,Wp] = min(q, top) / top with replicate padding, the window at (pad_top, pad_left),
        and / or ``dst_u8``, its 8-bit probe picture uint8 [h,w,3] RGB = min(q, top) >> (depth - 8) (include/atmvfi.h
        atmvfi_rgb16_decode; the bits of ``rgb16.decode_numpy_f32`` / ``probe_numpy``)."""
        self._rgb16_buf("rgb16_decode", buf, fmt, "source")
        if dst is None and dst_u8 is None:
            raise ValueError("rgb16_decode: give dst, dst_u8 or both")
        h, w = fmt.height, fmt.width
        y0, x0, wh, ww = (0, 0, h, w) if window is None else _window("rgb16_decode", fmt, window)
        hp, wp, nbytes = self._decode_sinks("rgb16_decode", dst_u8, dst, wh, ww, pad_top, pad_left)
        self._run("rgb16_decode", {"bytes": nbytes + 6.0 * wh * ww}, self.lib.atmvfi_rgb16_decode, _ptr(buf), h, w, fmt.depth, fmt.layout_id, y0, x0, wh, ww,
                  _ptr(dst), hp, wp, int(pad_top), int(pad_left), _ptr(dst_u8), self._stream())

    def rgb16_encode(self, buf, fmt, src, pad_top: int = 0, pad_left: int = 0):
        """``src`` fp32 planar RGB [3,Hp,Wp] with the frame at (pad_top, pad_left) -> ``buf``, one deep RGB frame of ``fmt`` (a
        ``yuv.DeepRGB``; a contiguous CUDA uint8 tensor of ``fmt.frame_bytes`` bytes): the sample clip(rint(x * top), 0, top) in the
        layout's order (include/atmvfi.h atmvfi_rgb16_encode; the bits of ``rgb16.encode_numpy``)."""
        n = self._rgb16_buf("rgb16_encode", buf, fmt, "destination")
        if src is None:         # (the one source)
            raise ValueError("rgb16_encode: src must be a contiguous CUDA fp32 [3,Hp,Wp] tensor")
        _f32_canvas(src, "rgb16_encode", ": src")
        h, w = fmt.height, fmt.width
        _, hp, wp = src.shape
        if pad_top < 0 or pad_left < 0 or h + pad_top > hp or w + pad_left > wp:
            raise ValueError(f"rgb16_encode: canvas {hp} x {wp} is smaller than the frame {h} x {w} plus padding ({pad_top}, {pad_left})")
        self._run("rgb16_encode", {"bytes": n + 12.0 * h * w}, self.lib.atmvfi_rgb16_encode, _ptr(src), hp, wp, int(pad_top), int(pad_left),
                  _ptr(buf), h, w, fmt.depth, fmt.layout_id, self._stream())

    # The loops' colour conversion: a yuv.Format goes to the planar wrappers as ever, a yuv.Surface to the two surface wrappers, and
    # either with a subsampling other than 4:2:0 to the two sub wrappers -- for their refusals and their names in a profile; all launch
    # atmvfi_yuv_decode / atmvfi_yuv_encode.  A yuv.DeepRGB goes to the two rgb16 calls (its depth is always kept).
    def yuv_decode(self, buf, fmt, dst_u8=None, dst=None, window=None, pad_top: int = 0, pad_left: int = 0, keep_depth: bool = False):
        if isinstance(fmt, DeepRGB):
            return self.rgb16_decode(buf, fmt, dst=dst, dst_u8=dst_u8, window=window, pad_top=pad_top, pad_left=pad_left)
        if fmt.subsampling != "420":
            return self.yuv_sub_decode(buf, fmt, dst_u8=dst_u8, dst=dst, window=window, pad_top=pad_top, pad_left=pad_left, keep_depth=keep_depth)
        if isinstance(fmt, Surface):
            return self.yuv_surface_decode(buf, fmt, dst_u8=dst_u8, dst=dst, window=window, pad_top=pad_top, pad_left=pad_left, keep_depth=keep_depth)
        if keep_depth:
            return self.yuv420p10_to_f32(buf, fmt, dst, window=window, pad_top=pad_top, pad_left=pad_left)
        if window is not None:
            raise ValueError("yuv_decode: a window of a yuv.Format frame is decoded with keep_depth only")
        return self.yuv420_to_rgb(buf, fmt, dst_u8=dst_u8, dst=dst, pad_top=pad_top, pad_left=pad_left)

    def yuv_encode(self, buf, fmt, src_u8=None, src=None, pad_top: int = 0, pad_left: int = 0):
        if isinstance(fmt, DeepRGB):
            if src_u8 is not None:
                raise ValueError("yuv_encode: a yuv.DeepRGB frame is encoded from the fp32 src (src_u8 holds 8-bit pixels)")
            return self.rgb16_encode(buf, fmt, src, pad_top=pad_top, pad_left=pad_left)
        if fmt.subsampling != "420":
            return self.yuv_sub_encode(buf, fmt, src_u8=src_u8, src=src, pad_top=pad_top, pad_left=pad_left)
        if isinstance(fmt, Surface):
            return self.yuv_surface_encode(buf, fmt, src_u8=src_u8, src=src, pad_top=pad_top, pad_left=pad_left)
        if fmt.depth == 10:
            return self.f32_to_yuv420p10(buf, fmt, src, pad_top=pad_top, pad_left=pad_left)
        return self.rgb_to_yuv420(buf, fmt, src_u8=src_u8, src=src, pad_top=pad_top, pad_left=pad_left)

    def frame_f32_to_u8(self, src, dst_u8, pad_top: int, pad_left: int, bgr: bool):
        """fp32 planar [3,Hp,Wp] -> crop -> np.round(x * 255) -> uint8 [H,W,3] device tensor (optional RGB -> BGR)."""
        _f32_canvas(src, "frame_f32_to_u8: source")
        _u8_frame(dst_u8, "frame_f32_to_u8: destination")
        h, w = dst_u8.shape[:2]
        self._run("frame_f32_to_u8", {"bytes": 3.0 * h * w + 12.0 * h * w}, self.lib.atmvfi_frame_f32_to_u8, _ptr(src), src.shape[1],
                  src.shape[2], pad_top, pad_left, _ptr(dst_u8), h, w, int(bgr), self._stream())

    def pool_blocks(self, pool, slots, buf, to_pool: bool = False, block_elems: Optional[int] = None, role: Optional[str] = None):
        """``len(slots)`` blocks between the slots of ``pool`` (contiguous [S, ...]) and the contiguous ``buf`` in one launch
        (include/atmvfi.h atmvfi_pool_blocks).  Gather (``to_pool`` False): block j of ``buf`` = the first ``block_elems`` elements of
        ``pool[slots[j]]`` -- ``torch.index_select``; scatter: the inverse -- ``Tensor.index_copy_``.  ``block_elems`` defaults to a
        whole slot.  ``slots`` is a host sequence of ints; it travels in the kernel arguments.  ``role``: while a launch plan is being
        recorded, the name under which the plan registers this call's slot list (``LaunchPlan.run(lists={role: ...})`` rewrites it
        before every replay); a recording without a role cannot know what the list means on the next call: ``PlanUnsupported``.
        Outside a recording ``role`` is ignored."""
        if self.recording is not None and role is None:
            raise PlanUnsupported("pool_blocks takes a host slot list: give it a role to record it")
        n = len(slots)
        if pool.dim() < 1 or not pool.is_contiguous() or not buf.is_contiguous() or not pool.is_cuda or not buf.is_cuda:
            raise ValueError("pool_blocks: pool and buf must be contiguous CUDA tensors")
        if pool.dtype != buf.dtype:
            raise ValueError(f"pool_blocks: pool is {pool.dtype}, buf {buf.dtype}")
        if not 1 <= n <= 32:
            raise ValueError(f"pool_blocks: 1..32 blocks per launch, got {n}")
        es = pool.element_size()
        slot_elems = pool[0].numel()
        be = slot_elems if block_elems is None else int(block_elems)
        if be <= 0 or be > slot_elems or buf.numel() != n * be:
            raise ValueError(f"pool_blocks: buf holds {buf.numel()} elements, {n} blocks of {be} (slot: {slot_elems}) need {n * be}")
        arr = (ctypes.c_int32 * n)(*[int(s) for s in slots])
        arr.role = role
        self._run("pool_blocks", {"bytes": 2.0 * n * be * es, "blocks": n}, self.lib.atmvfi_pool_blocks, _ptr(pool), slot_elems * es,
                  pool.shape[0], arr, n, be * es, _ptr(buf), int(bool(to_pool)), self._stream())

    def tta_merge(self, pred, pred_flip, out=None, out_u8=None, pad_top: int = 0, pad_left: int = 0, bgr: bool = False):
        """``out`` = (pred + pred_flip.flip(1).flip(2)) / 2 on [3,Hp,Wp] frames and / or ``out_u8`` = ``frame_f32_to_u8`` of it (uint8
        [H,W,3], the crop at (pad_top, pad_left)), in one launch (include/atmvfi.h atmvfi_tta_merge)."""
        _f32_canvas(pred, "tta_merge: pred")
        _f32_canvas(pred_flip, "tta_merge: pred_flip")
        if pred_flip.shape != pred.shape:
            raise ValueError("tta_merge: pred and pred_flip differ in shape")
        if out is None and out_u8 is None:
            raise ValueError("tta_merge: give out, out_u8 or both")
        if out is not None:
            _f32_canvas(out, "tta_merge: out")
            if out.shape != pred.shape:
                raise ValueError("tta_merge: out must have pred's shape")
        h = w = 0
        if out_u8 is not None:
            _u8_frame(out_u8, "tta_merge: out_u8")
            h, w = out_u8.shape[:2]
        hp, wp = pred.shape[1:]
        meta = {"bytes": 24.0 * hp * wp + (12.0 * hp * wp if out is not None else 0.0) + 3.0 * h * w}
        self._run("tta_merge", meta, self.lib.atmvfi_tta_merge, _ptr(pred), _ptr(pred_flip), _ptr(out), _ptr(out_u8), hp, wp, int(pad_top),
                  int(pad_left), h, w, int(bool(bgr)), self._stream())

    def frame_rot180(self, src, dst):
        """``dst`` = ``src.flip(-2).flip(-1)`` of contiguous fp32 [...,Hp,Wp] planes (include/atmvfi.h atmvfi_frame_rot180)."""
        if (src.dtype != torch.float32 or src.dim() < 2 or not src.is_contiguous() or not src.is_cuda or dst.dtype != torch.float32
                or dst.shape != src.shape or not dst.is_contiguous() or not dst.is_cuda):
            raise ValueError("frame_rot180: src and dst must be contiguous CUDA fp32 tensors of one shape [...,Hp,Wp]")
        hp, wp = src.shape[-2:]
        self._run("frame_rot180", {"bytes": 8.0 * src.numel()}, self.lib.atmvfi_frame_rot180, _ptr(src), _ptr(dst), src.numel() // (hp * wp),
                  hp, wp, self._stream())

    # ---------------------------------------------------------------- half-resolution motion (include/atmvfi.h; twins: scaled.py)
    def _run_direct(self, name: str, meta: dict, fn, *args):
        """``_run`` for the entry points that run around a plan's replay, never inside a recording.  (tools/gen_plan_dispatch.py emits a
        case for every entry point of the header, these included; ``synth_up2``'s parameter block and slot lists are HOST memory read at
        the call, so a recorded op would hold dangling pointers: recording them needs a redesign, not a flag.)"""
        if self.recording is not None:
            raise PlanUnsupported(f"{name} is not part of launch plans")
        self._run(name, meta, fn, *args)

    def frame_half(self, src, dst):
        """``dst`` [...,H/2,W/2] = the 2 x 2 box average ``((a + b) + (c + d)) * 0.25`` of the contiguous fp32 planes ``src`` [...,H,W],
        H and W even (include/atmvfi.h atmvfi_frame_half; the bits of ``scaled.frame_half_numpy``)."""
        ok = lambda t: isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.dim() >= 2
        if not ok(src) or not ok(dst):
            raise ValueError("frame_half: src and dst must be contiguous CUDA fp32 tensors [...,H,W] and [...,H/2,W/2]")
        h, w = src.shape[-2:]
        if h % 2 or w % 2 or h < 2 or w < 2 or tuple(dst.shape) != tuple(src.shape[:-2]) + (h // 2, w // 2):
            raise ValueError(f"frame_half: {tuple(src.shape)} -> {tuple(dst.shape)}: H and W must be even and dst [...,H/2,W/2]")
        self._run_direct("frame_half", {"bytes": 5.0 * src.numel()}, self.lib.atmvfi_frame_half, _ptr(src), _ptr(dst), src.numel() // (h * w), h, w,
                         self._stream())

    def synth_up2(self, half: dict, store0, store1=None, slots0=None, slots1=None, dst=None, dst_u8=None, window=None, bgr: bool = False,
                  want=(), path: str = "auto"):
        """Full-size synthesis from the half-size outputs ``half`` of one forward on ``frame_half``'d frames (its ``im_t_list[0]``,
        ``I_t_0``, ``I_t_1``, ``opt_flow_0``, ``opt_flow_1``, ``occ_mask1``; batch B <= 16, size h x w): one launch of
        include/atmvfi.h atmvfi_synth_up2.  ``store0`` / ``store1`` (default: the same) are contiguous fp32 [S,3,2h,2w] frame stores;
        pair b takes ``store0[slots0[b]]`` and ``store1[slots1[b]]`` (host lists; default b).  ``dst``: fp32 [B,3,2h,2w] or None;
        ``dst_u8``: uint8 [B,hh,ww,3] or None, the ``window`` = (pad_top, pad_left, hh, ww) of the canvas as ``frame_f32_to_u8``
        gives it; with neither, ``dst`` is allocated.  ``want``: any of "opt_flow_0", "opt_flow_1", "occ_mask1" at full size.
        ``path``: "direct" (gathers; "auto" is this one, the faster by measurement) or "staged" (LDS boxes of the sources).  -> dict with "I_t" (``dst``), "I_t_u8" and the wanted maps, as given.
        ``scaled.synth_up2_numpy`` is the host twin (the same arithmetic; the GPU tests hold the kernel to the fp64 bound, not to its bits)."""
        names = {"opt_flow_0", "opt_flow_1", "occ_mask1"}
        if set(want) - names:
            raise ValueError(f"synth_up2: want takes {sorted(names)}, got {sorted(set(want) - names)}")
        if path not in ("auto", "direct", "staged"):
            raise ValueError(f"synth_up2: path must be 'auto', 'direct' or 'staged', got {path!r}")
        ins = [half["im_t_list"][0], half["I_t_0"], half["I_t_1"], half["opt_flow_0"], half["opt_flow_1"], half["occ_mask1"]]
        b, _, h, w = ins[0].shape
        for t, c in zip(ins, (3, 3, 3, 2, 2, 1)):
            _planar(t, c, "synth_up2: half-size input")
            if tuple(t.shape) != (b, c, h, w):
                raise ValueError(f"synth_up2: half-size inputs differ in shape ({tuple(t.shape)} against [{b},{c},{h},{w}])")
        if b > 16:
            raise ValueError(f"synth_up2: at most 16 pairs per call, got {b}")
        store1 = store0 if store1 is None else store1
        for st in (store0, store1):
            _planar(st, 3, "synth_up2: frame store")
            if tuple(st.shape[2:]) != (2 * h, 2 * w):
                raise ValueError(f"synth_up2: a frame store of {tuple(st.shape)} does not hold {2 * h} x {2 * w} frames")
        lists = []
        for sl, st in ((slots0, store0), (slots1, store1)):
            sl = list(range(b)) if sl is None else [int(s) for s in sl]
            if len(sl) != b or any(s < 0 or s >= st.shape[0] for s in sl):
                raise ValueError(f"synth_up2: {b} slots inside 0..{st.shape[0] - 1} expected, got {sl}")
            lists.append((ctypes.c_int32 * b)(*sl))
        if dst is None and dst_u8 is None:
            dst = self.empty(b, 3, 2 * h, 2 * w)
        if dst is not None:
            _planar(dst, 3, "synth_up2: dst")
            if tuple(dst.shape) != (b, 3, 2 * h, 2 * w):
                raise ValueError(f"synth_up2: dst must be [{b},3,{2 * h},{2 * w}], got {tuple(dst.shape)}")
        pt = pl = hh = ww = 0
        if dst_u8 is not None:
            pt, pl, hh, ww = (0, 0, 2 * h, 2 * w) if window is None else map(int, window)
            if (not isinstance(dst_u8, torch.Tensor) or dst_u8.dtype != torch.uint8 or not dst_u8.is_cuda or not dst_u8.is_contiguous()
                    or tuple(dst_u8.shape) != (b, hh, ww, 3)):
                raise ValueError(f"synth_up2: dst_u8 must be a contiguous CUDA uint8 [{b},{hh},{ww},3] tensor")
        out = {"I_t": dst, "I_t_u8": dst_u8}
        f0 = f1 = m = None
        if "opt_flow_0" in want or "opt_flow_1" in want:
            f0, f1 = self.empty(b, 2, 2 * h, 2 * w), self.empty(b, 2, 2 * h, 2 * w)
        if "occ_mask1" in want:
            m = self.empty(b, 1, 2 * h, 2 * w)
        for k, t in (("opt_flow_0", f0), ("opt_flow_1", f1), ("occ_mask1", m)):
            if k in want:
                out[k] = t
        vp = lambda t: None if t is None else t.data_ptr()
        prm = SynthUp2Params(*[vp(t) for t in ins], vp(store0), vp(store1), ctypes.cast(lists[0], ctypes.c_void_p), ctypes.cast(lists[1], ctypes.c_void_p),
                             vp(dst), vp(dst_u8), vp(f0), vp(f1), vp(m), None, b, h, w, store0.shape[0], store1.shape[0], pt, pl, hh, ww,
                             int(bool(bgr)), ("auto", "direct", "staged").index(path), 0)
        full = 4.0 * b * 2 * h * 2 * w
        meta = {"bytes": 14.0 * 4 * b * h * w + 6 * full + (3 * full if dst is not None else 0.0) + 3.0 * b * hh * ww
                + (4 * full if f0 is not None else 0.0) + (full if m is not None else 0.0)}
        self._run_direct("synth_up2", meta, self.lib.atmvfi_synth_up2, ctypes.cast(ctypes.pointer(prm), ctypes.c_void_p), self._stream())
        return out

    # ---------------------------------------------------------------- interlaced input (include/atmvfi.h; twins and the loop: fields.py)
    def field_bob(self, src, dst_even=None, dst_odd=None, pad_top: int = 0, pad_left: int = 0, h: Optional[int] = None, w: Optional[int] = None):
        """The two field canvases of the woven canvas ``src`` (contiguous fp32 [planes,Hp,Wp]; its picture is the ``h`` x ``w`` window at
        (pad_top, pad_left); default: everything below and right of the pads): ``dst_even`` / ``dst_odd`` (tensors of ``src``'s shape;
        either may be None, not both) = the replicate-padded ``bob`` of the picture with the even / odd rows kept (include/atmvfi.h atmvfi_field_bob; the bits of ``fields.bob_numpy``).  Not part of a forward: never recorded
        into a launch plan."""
        ts = [t for t in (src, dst_even, dst_odd) if t is not None]
        if src is None or len(ts) < 2:
            raise ValueError("field_bob: a source and at least one of dst_even / dst_odd expected")
        for t in ts:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous() or not t.is_cuda or t.shape != src.shape:
                raise ValueError("field_bob: src and the destinations must be contiguous CUDA fp32 [planes,Hp,Wp] tensors of one shape")
        planes, hp, wp = src.shape
        h = hp - int(pad_top) if h is None else int(h)
        w = wp - int(pad_left) if w is None else int(w)
        n_out = len(ts) - 1
        self._run_direct("field_bob", {"bytes": 4.0 * planes * (h * w + n_out * hp * wp)}, self.lib.atmvfi_field_bob, _ptr(src), _ptr(dst_even),
                         _ptr(dst_odd), planes, hp, wp, int(pad_top), int(pad_left), h, w, self._stream())

    def field_rows(self, dst, src, geometry, parity: int):
        """Rows ``y % 2 == parity`` of up to three planes from the byte tensor ``src`` into the byte tensor ``dst`` (contiguous CUDA
        uint8, any size): ``geometry`` is a sequence of per-plane ``(dst_offset, src_offset, dst_pitch, src_pitch, row_bytes, rows)`` in
        bytes (``fields.plane_geometry`` makes it for a frame layout).  Bytes are moved, nothing else is touched (include/atmvfi.h
        atmvfi_field_rows; the bits of ``fields.rows_numpy``).  The planes are checked against the tensors' sizes here.  Not part of
        a forward: never recorded into a launch plan."""
        for t, role in ((dst, "dst"), (src, "src")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"field_rows: {role} must be a contiguous CUDA uint8 tensor")
        geometry = [tuple(int(v) for v in g) for g in geometry]
        if not 1 <= len(geometry) <= 3 or any(len(g) != 6 for g in geometry):
            raise ValueError("field_rows: one to three planes of (dst_offset, src_offset, dst_pitch, src_pitch, row_bytes, rows) expected")
        moved = 0
        for k, (doff, soff, dp, sp, rb, rows) in enumerate(geometry):
            if min(doff, soff) < 0 or min(dp, sp, rb, rows) < 1 or doff + (rows - 1) * dp + rb > dst.numel() or soff + (rows - 1) * sp + rb > src.numel():
                raise ValueError(f"field_rows: plane {k} {geometry[k]} does not lie inside dst ({dst.numel()} bytes) and src ({src.numel()} bytes)")
            moved += rb * ((rows - int(parity) + 1) // 2)
        arr = (ctypes.c_int64 * (6 * len(geometry)))(*[v for g in geometry for v in g])
        self._run_direct("field_rows", {"bytes": 2.0 * moved}, self.lib.atmvfi_field_rows, _ptr(dst), _ptr(src), len(geometry), arr, int(parity),
                         self._stream())

    def pack_frames(self, im0, im1, dst):
        _planar(im0, 3, "pack_frames.im0"); _planar(im1, 3, "pack_frames.im1")
        b, _, h, w = im0.shape
        if tuple(dst.shape) != (2 * b, h, w, 4) or not dst.is_contiguous():
            raise ValueError("pack_frames: dst must be contiguous [2B,H,W,4]")
        self._run("pack_frames", {"bytes": 4.0 * 2 * b * h * w * 7}, self.lib.atmvfi_pack_frames, _ptr(im0), _ptr(im1), _ptr(dst),
                  b, h, w, self._stream())

    def final_residual(self, it, r, it_sum, it_clamped):
        _planar(it, 3, "final_residual.it"); _planar(it_sum, 3, "final_residual.sum"); _planar(it_clamped, 3, "final_residual.clamped")
        b, _, h, w = it.shape
        rld, rb, rh, rw, rc = nhwc_view(r, "final_residual.r")
        if (rb, rh, rw, rc) != (b, h, w, 3):
            raise ValueError("final_residual: r must be a [B,H,W,3] view")
        self._run("final_residual", {"bytes": 4.0 * b * h * w * 12}, self.lib.atmvfi_final_residual, _ptr(it), _ptr(r), rld,
                  _ptr(it_sum), _ptr(it_clamped), b, h, w, self._stream())

    def l1_mean_workspace_floats(self, n: int, per_sample: int) -> int:
        return int(self.lib.atmvfi_l1_mean_workspace_floats(n, per_sample))

    def l1_mean(self, a, b, out, workspace=None):
        """mean |a - b| per sample, fixed summation order (run-to-run bit-identical).  ``workspace``: fp32 scratch of at least
        ``l1_mean_workspace_floats`` elements (workspace memory of the caller).  Without one (direct callers, tests) the scratch is
        kept on this object per (samples, elements): a temporary would be handed back to torch's allocator after the launch and
        would turn into a stale pointer inside a recorded plan."""
        _chk(a, "l1_mean.a"); _chk(b, "l1_mean.b")
        if not a.is_contiguous() or not b.is_contiguous() or a.shape != b.shape:
            raise ValueError("l1_mean: inputs must be contiguous and of equal shape")
        n = a.shape[0]
        if workspace is None:
            cache = self.__dict__.setdefault("_l1_scratch", {})
            key = (n, a.numel() // n)
            workspace = cache.get(key)
            if workspace is None:
                if self.recording is not None:
                    raise PlanUnsupported("l1_mean scratch created while recording")
                workspace = cache[key] = torch.empty(self.l1_mean_workspace_floats(*key), dtype=torch.float32, device=a.device)
        self._run("l1_mean", {"bytes": 8.0 * a.numel()}, self.lib.atmvfi_l1_mean, _ptr(a), _ptr(b), _ptr(out), n, a.numel() // n,
                  _ptr(workspace), workspace.numel(), self._stream())

    def ssim_psnr_workspace_floats(self, n: int, h: int, w: int) -> int:
        return int(self.lib.atmvfi_ssim_psnr_workspace_floats(n, h, w))

    def ssim_psnr(self, x, y, out, workspace, val_range: float = 0.0, flags: int = 0):
        """ssim_matlab + squared-error mean per sample (include/atmvfi.h atmvfi_ssim_psnr): x = the ground truth, a CUDA fp32 [B,3,H,W]
        view or (``flags & SSIM_X_U8``) a CUDA uint8 [B,H,W,3] view; y = a CUDA fp32 [B,3,H,W] view, any strides; out = CUDA fp64
        [B,3] contiguous (ssim, cs, mse); workspace = CUDA fp32 of at least ``ssim_psnr_workspace_floats(B, H, W)`` elements."""
        _chk(y, "ssim_psnr.y"); _chk(workspace, "ssim_psnr.workspace")
        if y.dim() != 4 or y.shape[1] != 3:
            raise ValueError(f"ssim_psnr: y must be [B,3,H,W], got {tuple(y.shape)}")
        b, _, h, w = y.shape
        if flags & SSIM_X_U8:
            if not x.is_cuda or x.dtype != torch.uint8 or tuple(x.shape) != (b, h, w, 3):
                raise ValueError(f"ssim_psnr: a uint8 x must be a CUDA [B,H,W,3] tensor of y's size, got {x.device} {x.dtype} {tuple(x.shape)}")
            xs = (x.stride(0), x.stride(3), x.stride(1), x.stride(2))
        else:
            _chk(x, "ssim_psnr.x")
            if tuple(x.shape) != tuple(y.shape):
                raise ValueError(f"ssim_psnr: x {tuple(x.shape)} and y {tuple(y.shape)} differ in shape")
            xs = tuple(x.stride())
        if not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (b, 3) or not out.is_contiguous():
            raise ValueError("ssim_psnr: out must be a contiguous CUDA float64 [B,3] tensor")
        if not workspace.is_contiguous() or workspace.numel() < self.ssim_psnr_workspace_floats(b, h, w):
            raise ValueError("ssim_psnr: workspace too small")
        self._run("ssim_psnr", {"bytes": float(x.numel() * x.element_size() + 4 * y.numel())}, self.lib.atmvfi_ssim_psnr, _ptr(x), *xs,
                  _ptr(y), *y.stride(), b, h, w, float(val_range), int(flags), _ptr(out), _ptr(workspace), workspace.numel(), self._stream())

    def ensemble_select(self, losses, cands, out0, out1):
        """Per sample the candidate flow pair of the level with the smallest loss (first on ties): losses = three [B] tensors,
        cands = three (flow0, flow1) pairs of contiguous [B,2,h,w] tensors, out0 / out1 contiguous [B,2,h,w]."""
        b = out0.shape[0]
        per = out0.numel() // b
        ts = [t for pair in cands for t in pair] + [out0, out1]
        if len(losses) != 3 or len(cands) != 3 or any(t.shape != out0.shape or not t.is_contiguous() for t in ts) or any(l.numel() != b for l in losses):
            raise ValueError("ensemble_select: three [B] losses, three pairs of contiguous [B,2,h,w] candidates and two outputs of that shape expected")
        for t in ts + list(losses):
            _chk(t, "ensemble_select")
        self._run("ensemble_select", {"bytes": 4.0 * out0.numel() * 4}, self.lib.atmvfi_ensemble_select, _ptr(losses[0]), _ptr(losses[1]),
                  _ptr(losses[2]), _ptr(cands[0][0]), _ptr(cands[0][1]), _ptr(cands[1][0]), _ptr(cands[1][1]), _ptr(cands[2][0]),
                  _ptr(cands[2][1]), _ptr(out0), _ptr(out1), b, per, self._stream())
