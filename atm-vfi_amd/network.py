"""``Network``: the drop-in replacement for the reference's model class.

Same constructor, attributes, methods, ``state_dict`` and ``forward(im0, im1) -> dict`` as
``network/network_base.py:88-546`` / ``network/network_lite.py``, but
``forward`` is a sequence of hand-written HIP kernel launches (``hip_ops.HipOps`` ->
``libatmvfi_hip.so``) over an NHWC workspace:

* feature maps live channel-last; every ``torch.cat`` / ``einops.rearrange`` of the
  reference is realised by letting the producer write into a channel slice ("view") of
  the consumer's buffer, so none of them moves data;
* ``pad_if_needed`` / ``torch.roll`` / ``window_partition`` and their inverses are int32
  row maps (``windows.py``) consumed by the LayerNorm gather and the GEMM scatter;
* warps generate their coordinates in-kernel; flows and masks are read straight from the
  last five channels of the decoder maps.

The module holds parameters exactly like the reference (236 entries, same names), so
``load_state_dict(strict=True)`` of published checkpoints works; GEMM-layout copies of
the weights are derived lazily and refreshed when a parameter changes.

There is no CPU path: ``forward`` requires CUDA(HIP) tensors and the built library.
"""
from __future__ import annotations

import operator
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import scaled
from . import schema as S
from .hip_ops import GEMM_CONV, GEMM_DECONV, GEMM_LINEAR, HipOps, LaunchPlan, Planes, PlanUnsupported
from .paths import PlanesPath, RowsPath, _r4
from .windows import WindowGeometry, build_window_geometry


_VERSION_OF = operator.attrgetter("_version")
_DATA_PTR_OF = torch.Tensor.data_ptr


_PARAM_EPOCH = [0]       # bumped whenever a Parameter OBJECT is (re)assigned, registered or deleted on any _Node / Network


class _ParamWatch:
    """Mixin: replacing a parameter object (``module.weight = nn.Parameter(...)``, ``register_parameter``, pruning or
    re-parametrisation hooks, ``del module.weight``) OR a whole sub-module (``net.x = other_node``, ``add_module`` /
    ``register_module``, ``del net.x``: parametrize / prune wrappers swap modules) bumps ``_PARAM_EPOCH``, which ``Network._param_sig``
    compares on every forward: its cached parameter list would otherwise keep the OLD objects and the packed weights, plans and graphs
    would stay stale."""

    def __setattr__(self, name, value):
        d = self.__dict__
        if isinstance(value, (nn.Parameter, nn.Module)) or name in d.get("_parameters", ()) or name in d.get("_modules", ()):
            _PARAM_EPOCH[0] += 1
        super().__setattr__(name, value)

    def __delattr__(self, name):
        d = self.__dict__
        if name in d.get("_parameters", ()) or name in d.get("_modules", ()):
            _PARAM_EPOCH[0] += 1
        super().__delattr__(name)

    def register_parameter(self, name, param):
        _PARAM_EPOCH[0] += 1
        super().register_parameter(name, param)

    def add_module(self, name, module):
        _PARAM_EPOCH[0] += 1
        super().add_module(name, module)

    def register_module(self, name, module):
        _PARAM_EPOCH[0] += 1
        super().register_module(name, module)


class _Node(_ParamWatch, nn.Module):
    """Anonymous container used to reproduce the reference's dotted parameter names."""


class BlockRunner:
    """Workspace + one-transformer-block machinery shared by ``Network`` and the stand-alone ``ATMFormer`` / ``RefineBottleneck``
    modules (``atm-vfi_amd/blocks.py``): named device buffers, split-plane buffers, cached window maps, and ``_block``."""

    def _init_runner(self):
        self._ops_obj = None
        self._bufs: Dict[Tuple, object] = {}
        self._geo: Dict[Tuple, Tuple[WindowGeometry, torch.Tensor, Optional[torch.Tensor]]] = {}

    def buf(self, name: str, *shape) -> torch.Tensor:
        key = (name,) + tuple(shape)
        t = self._bufs.get(key)
        if t is None:
            if getattr(self._ops_obj, "recording", None) is not None:
                raise PlanUnsupported(f"workspace buffer {name} created while recording")
            t = self._ops_obj.empty(*shape)
            self._bufs[key] = t
        return t

    def planes(self, name: str, rows: int, c: int) -> Planes:
        """Workspace rows in the split-plane format (zero-initialised once: the pad channels must stay finite)."""
        key = ("planes", name, rows, c)
        p = self._bufs.get(key)
        if p is None:
            if getattr(self._ops_obj, "recording", None) is not None:
                raise PlanUnsupported(f"workspace planes {name} created while recording")
            p = Planes.alloc(rows, c, self._ops_obj.device)
            self._bufs[key] = p
        return p

    def geometry(self, frames, h, w, ws, shift):
        key = (frames, h, w, ws, shift)
        g = self._geo.get(key)
        if g is None:
            if getattr(self._ops_obj, "recording", None) is not None:
                raise PlanUnsupported("window maps created while recording")
            geo = build_window_geometry(frames, h, w, ws, shift)
            ops = self._ops_obj
            g = (geo, ops.to_device_int(geo.row_map), None if geo.labels is None else ops.to_device_int(geo.labels))
            self._geo[key] = g
        return g

    @staticmethod
    def _plane_deconvs(ops) -> bool:
        """Split planes between contraction layers: nn.Linear inputs of the blocks and the decoder deconvs read their operands as
        split planes through the LDS-DMA GEMM (the f16x3 engine of a backend that has the plane sinks)."""
        return getattr(ops, "precision", None) == "f16x3" and getattr(ops, "split_planes_ok", False)

    def _block(self, ops, P, p, x, frames, h, w, ws, shift, cross, out, motion_dst, tag, out_sink=None, motion_sink=None):
        """One shifted-window transformer block (ATMFormer attention.py:265-334 when ``cross``,
        RefineBottleneck :433-495 otherwise).  x/out: token-matrix views in image order."""
        c = x.shape[-1]
        heads = S.NUM_HEADS
        hd = c // heads
        geo, row_map, labels = self.geometry(frames, h, w, ws, shift)
        mw = frames * geo.n_windows * geo.tokens
        bw = frames * geo.n_windows
        # With the f16x3 engine every nn.Linear input is written by its producer as split planes (fp16 hi / lo', same
        # bytes as fp32) and read by the GEMM through LDS-DMA; fp32 copies are kept only where something else reads them
        # (xn is the residual of proj: the reference adds onto the post-norm tensor).
        pl = self._plane_deconvs(ops)
        xn = self.buf(f"{tag}xn", mw, c)
        xn_p = self.planes(f"{tag}xn_p", mw, c) if pl else None
        ops.layernorm(x, xn, P[f"{p}.norm1.weight"], P[f"{p}.norm1.bias"], src_row_map=row_map, **({"planes": xn_p} if pl else {}))
        qkv = self.buf(f"{tag}qkv", mw, 3 * c)
        ops.linear(xn_p if pl else xn, P[f"pk:{p}.attn.qkv.weight"], qkv)
        ao = None if pl else self.buf(f"{tag}ao", mw, c)
        ao_p = self.planes(f"{tag}ao_p", mw, c) if pl else None
        mo = self.buf(f"{tag}mo", mw, heads, 2) if cross else None
        ops.window_attention(qkv, ao, mo, labels, bw, geo.n_windows, ws, heads, hd, bw // 2 if cross else 0,
                             **({"planes": ao_p} if pl else {}))
        xb = self.buf(f"{tag}xb", frames * h * w, c)
        ops.linear(ao_p if pl else ao, P[f"pk:{p}.attn.proj.weight"], xb, bias=P[f"{p}.attn.proj.bias"], residual=xn, out_row_map=row_map)
        if cross:
            mk = {} if motion_sink is None else {"planes": motion_sink[0], "planes_c0": motion_sink[1], "planes_gc": motion_sink[2]}
            ops.motion_head(mo, row_map, P[f"{p}.attn.mlp.0.weight"], P[f"{p}.attn.mlp.0.bias"],
                            P[f"{p}.attn.mlp.2.weight"], P[f"{p}.attn.mlp.2.bias"], motion_dst, **mk)
        hid = P[f"{p}.mlp.fc1.bias"].shape[0]
        f1 = self.buf(f"{tag}fc1", frames, h, w, hid)
        if pl:
            y_p = self.planes(f"{tag}ln2_p", frames * h * w, c)
            ops.layernorm(xb, None, P[f"{p}.norm2.weight"], P[f"{p}.norm2.bias"], planes=y_p)
            ops.linear(y_p, P[f"pk:{p}.mlp.fc1.weight"], f1.reshape(frames * h * w, hid), bias=P[f"{p}.mlp.fc1.bias"])
            f2_p = self.planes(f"{tag}dw_p", frames * h * w, hid)
            ops.dwconv_gelu(f1, None, P[f"pk:{p}.mlp.dwconv.dwconv.weight"], P[f"{p}.mlp.dwconv.dwconv.bias"], planes=f2_p)
            sk = {} if out_sink is None else {"sink": out_sink[0], "sink_c0": out_sink[1], "sink_gc": out_sink[2]}
            ops.linear(f2_p, P[f"pk:{p}.mlp.fc2.weight"], out, bias=P[f"{p}.mlp.fc2.bias"], residual=xb, **sk)
        else:
            y = self.buf(f"{tag}ln2", frames * h * w, c)
            ops.layernorm(xb, y, P[f"{p}.norm2.weight"], P[f"{p}.norm2.bias"])
            ops.linear(y, P[f"pk:{p}.mlp.fc1.weight"], f1.reshape(frames * h * w, hid), bias=P[f"{p}.mlp.fc1.bias"])
            f2 = self.buf(f"{tag}dw", frames, h, w, hid)
            ops.dwconv_gelu(f1, f2, P[f"pk:{p}.mlp.dwconv.dwconv.weight"], P[f"{p}.mlp.dwconv.dwconv.bias"])
            ops.linear(f2.reshape(frames * h * w, hid), P[f"pk:{p}.mlp.fc2.weight"], out, bias=P[f"{p}.mlp.fc2.bias"], residual=xb)


class Network(_ParamWatch, BlockRunner, nn.Module):
    VARIANT = "base"

    SELECTIONS = ("use_plans",)

    def __init__(self, global_motion: bool = True, ensemble_global_motion: bool = False, variant: Optional[str] = None,
                 selections: Optional[Dict[str, bool]] = None):
        """``global_motion`` / ``ensemble_global_motion``: the reference's constructor (network_base.py:89).  ``selections`` (not in
        the reference): overrides of the kernel-selection attributes in ``SELECTIONS`` (all default to the measured-best choice)."""
        super().__init__()
        self.variant_name = variant or self.VARIANT
        v = S.VARIANTS[self.variant_name]
        self._v = v
        # ---- attributes the reference exposes (network_base.py:91-201) ----
        self.pyramid_level = S.PYRAMID_LEVELS
        self.hidden_dims = list(v.hidden_dims)
        self.global_motion = global_motion
        self.ensemble_global_motion = ensemble_global_motion
        self.local_motion_args = {"window_size": v.local_window, "num_heads": S.NUM_HEADS, "patch_size": 1,
                                  "dim": v.local_dim, "enhance_window": 8}
        self.global_motion_args = {"window_size": v.global_window, "num_heads": S.NUM_HEADS, "patch_size": 1,
                                   "dim": v.global_dim}
        if self.variant_name == "lite":
            self.local_motion_args["mlp_ratio"] = v.mlp_ratio
            self.global_motion_args["mlp_ratio"] = v.mlp_ratio
        self.fused_dim = v.fused_dim
        self.motion_out_dim = S.MOTION_OUT
        self.fused_dim1, self.fused_dim2, self.fused_dim3 = v.decoder_widths
        self.fused_dims = [self.fused_dim1, self.fused_dim2, self.fused_dim3, 2 * self.fused_dim1]
        # ---- parameters / buffers under the reference's names ----
        gen = torch.Generator().manual_seed(torch.initial_seed() % (2 ** 31))
        for sp in S.param_schema(v):
            t = S.init_tensor(sp, gen)
            parts = sp.key.split(".")
            node: nn.Module = self
            for name in parts[:-1]:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            if sp.is_buffer:
                node.register_buffer(parts[-1], t)
            else:
                node.register_parameter(parts[-1], nn.Parameter(t))
        # ---- runtime state (not part of the state dict) ----
        self._init_runner()
        self._precision = "f16x3"
        self._checked = False                        # "f16x3-checked": the library build that counts out-of-range operands
        self._prepared: Dict[str, object] = {}
        self._prepared_sig = None
        # Workspaces: one dict of named buffers per (device, input shape, mode) key, least recently used first.  The reference's
        # evaluation loops (benchmark/test_snufilm.py, test_xiph.py) feed one model frames of many sizes and never call
        # release_workspace(), so the cache evicts by itself: at most `max_workspaces` shapes and `workspace_cap_bytes` in total
        # (checked when a forward starts; the workspace in use always stays).  ~13 GB per 1080p shape of the GPU's 288 GB.
        self.max_workspaces = 2
        self.workspace_cap_bytes = 96 << 30
        self._workspaces: Dict[Tuple, Dict[Tuple, object]] = {}
        self._ws_key: Optional[Tuple] = None
        self._bufs: Dict[Tuple, object] = {}
        self._geo: Dict[Tuple, Tuple[WindowGeometry, torch.Tensor, Optional[torch.Tensor]]] = {}
        self.use_graphs = False
        self._frame_cache_on = False
        self._rows_fit_planes = True
        self._frame_cache = None          # (workspace key, tokens of the last call's second frame)
        self._reuse_first = False
        self._graphs: Dict[Tuple, Tuple] = {}
        self._graph_sig = None
        # launch plans (hip_ops.LaunchPlan): from the third forward with one (shape, mode, weights) key on, a forward is ONE
        # atmvfi_plan_run call with fresh output tensors; enable_plans(False) or `Network(selections={"use_plans": False})` turns it
        # off (a constructor argument, not an environment variable: the product reads no environment variable)
        self.use_plans = True
        self._plans: Dict[Tuple, object] = {}       # key -> LaunchPlan | int (eager forwards seen so far) | False (cannot be planned)
        self._plan_sig = None
        # launch plans of forward_pooled: per key a frame-stage plan (the stale slots' tokens) and a pair-stage plan (the rest), both
        # over the pool's three tensors as per-call inputs and the slot lists as per-call host lists.  A dict of their own (keys end
        # with the workspace key like those of _plans); cleared wherever _plans is.
        self._pool_plans: Dict[Tuple, object] = {}
        self._pooled_plans_on = True                # tools only (bench_nx / bench_retime A/B): False keeps forward_pooled eager
        self._splitk_memo: Dict[Tuple, Tuple] = {}  # _frame_stage_splitk per (H, W, frames, mode): host-side, asked per pooled call
        self._scaled_halves: Dict[Tuple, Tuple] = {}   # forward_scaled: the two half-size input frames of the last shape
        self._plan_stats = self._new_plan_stats()
        self._plist = None                          # cached parameter list of the per-forward currency check (_param_sig)
        self._pepoch = -1
        self._primary: Optional["Network"] = None   # set on replicas (replica()): the model whose packed weights this one reads
        self._prepare_lock = None                   # created on the primary with its first replica
        for name, flag in (selections or {}).items():
            if name not in self.SELECTIONS:
                raise ValueError(f"unknown kernel selection {name!r}; one of {self.SELECTIONS}")
            setattr(self, name, bool(flag))

    # ------------------------------------------------------------------ API parity
    def __set_local_window_size__(self, window_size):       # network_base.py:262-265
        self.local_motion_args["window_size"] = window_size
        self._reset_relative_coord("local_motion_atmformer", window_size)

    def __set_global_window_size__(self, window_size):      # network_base.py:267-270
        self.global_motion_args["window_size"] = window_size
        self._reset_relative_coord("global_motion_atmformer", window_size)

    def _reset_relative_coord(self, branch: str, ws: int):
        # attention.py:167-170 re-registers the table for the new window
        for b in range(2):
            attn = self._modules[branch]._modules[str(b)]._modules["attn"]
            dev = attn._buffers["relative_coord"].device
            attn._buffers["relative_coord"] = S.relative_coord_table(ws).to(dev)

    _GLOBAL_PARTS = ("last_feat_extract", "global_feature_fusion", "global_motion_atmformer", "global_motion_mlp")
    _REFINE_PARTS = ("proj", "down1", "down2", "down3", "up1", "up2", "up3", "refine_head")
    _LOCAL_PARTS = ("feat_extracts", "cross_scale_feature_fusion", "local_motion_atmformer", "local_motion_mlp",
                    "feat_enhance_transformer", "upsample_pyramid") + _REFINE_PARTS

    def _grad(self, parts, flag):
        for p in parts:
            self._modules[p].requires_grad_(flag)

    def __freeze_global_motion__(self):       # network_base.py:272-276
        self._grad(self._GLOBAL_PARTS, False)

    def __finetune_global_motion__(self):     # :278-282
        self._grad(self._GLOBAL_PARTS, True)

    def __freeze_local_motion__(self):        # :284-298
        self._grad(self._LOCAL_PARTS, False)

    def __finetune_local_motion__(self):      # :300-314
        self._grad(self._LOCAL_PARTS, True)

    def __finetune_refinenet_only__(self):    # :316-334 (base only in the reference)
        self._grad(self._GLOBAL_PARTS, False)
        self._grad([p for p in self._LOCAL_PARTS if p not in self._REFINE_PARTS], False)
        self._grad(self._REFINE_PARTS, True)

    # ------------------------------------------------------------------ plumbing
    def set_ops(self, ops):
        """Inject the op backend (tests inject a CPU double to check host logic; the
        default is the HIP library and nothing else)."""
        self._ops_obj = ops
        self._drop_device_state()

    def set_precision(self, precision: str):
        """"f16x3" (default): contractions as fp16 hi/lo split, three 16-bit MFMAs per product, fp32 accumulate
        (~22 significand bits, operands must stay within the fp16 range).  "f32": every contraction on the exact-fp32
        MFMA (about 2.5x slower).  "f16x3-checked": the f16x3 arithmetic, bit for bit, on the CHECKED build of the library
        (libatmvfi_hip_checked.so), which counts every activation pair whose split hit the fp16 limit (|x| >= 65488, inf, NaN) --
        ``range_violations()`` reads the count; launch plans and graphs are off in this mode.

        "f16" (opt-in, never a default): single-pass fp16 in the PLANE kernels.  There a product is hi(x) * hi(w) alone -- hi = the
        split's high half, fp16 round-to-nearest-even, saturating -- accumulated in fp32 in the kernels' k order: one 16-bit MFMA
        per product instead of three, about 11 significand bits per operand.  It covers the 3x3 plane kernel (its fused read-out's
        main product included; the read-out's 27-row W2 product stays three-term) and every GEMM on split-plane input (linears,
        deconvs, strided / dilated / 1x1 convs; split-K included).  The stem, window attention, the fp32-input engines, the 1x1 heads
        and the pointwise kernels stay "f16x3"; activations are still handed over as both planes of each kernel's own fp32 result.
        Outside the 1e-3 budget of the default (README "Precision modes": measured error and timing); has no checked twin --
        ``range_violations()`` raises as in "f16x3".  Not part of the reference's API."""
        if precision not in ("f16x3", "f16", "f32", "f16x3-checked"):
            raise ValueError("precision must be 'f16x3', 'f16', 'f32' or 'f16x3-checked'")
        checked = precision == "f16x3-checked"
        if checked != self._checked:
            # another library: packed weights, workspaces, plans and the op backend belong to the one that made them
            self._ops_obj = None
            self._drop_device_state()
        self._checked = checked
        self._precision = "f16x3" if checked else precision
        if self._ops_obj is not None and hasattr(self._ops_obj, "precision"):
            self._apply_precision(self._ops_obj)

    def _apply_precision(self, ops):
        """The op backend's view of the mode: "f16" is the split-plane engines and layouts of "f16x3" (``ops.precision``: the plane
        path stays on) with single-term products in the plane kernels (``ops.plane_terms``)."""
        ops.precision = "f16x3" if self._precision == "f16" else self._precision
        ops.plane_terms = 1 if self._precision == "f16" else 3

    def range_violations(self, reset: bool = False) -> int:
        """Activation pairs split beyond the fp16 operand range since the model entered "f16x3-checked" (or since the last
        ``reset``): 0 means every contraction of every forward so far saw operands the f16x3 engines represent (DESIGN.md section 1,
        deviation 2); anything else means results may differ from the fp32 reference -- use ``set_precision("f32")``.  Synchronises."""
        if not self._checked:
            raise RuntimeError("range_violations(): the model is not in 'f16x3-checked' precision")
        ops = self._ops_obj
        if ops is None or getattr(ops, "range_word", None) is None:
            return 0
        n = int(ops.range_word.item()) & 0xffffffff
        if reset:
            ops.range_word.zero_()
        return n

    def _drop_device_state(self):
        """Everything that lives on one device or was derived there: packed weights, workspaces, window maps, captured graphs."""
        self._prepared = {}
        self._prepared_sig = None
        self._plist = None
        self._graphs.clear()
        self._drop_plans()
        self._splitk_memo.clear()
        self._workspaces.clear()
        self._scaled_halves.clear()
        self._bufs = {}
        self._ws_key = None
        self._geo.clear()
        self._frame_cache = None

    def _ops(self, device: torch.device):
        cur = getattr(self._ops_obj, "device", None)
        if isinstance(self._ops_obj, HipOps) and cur is not None and torch.device(cur) != torch.device(device):
            # the model (or its inputs) moved to another GPU: buffers, packed weights and maps of the old device must not meet
            # tensors of the new one in a launch
            self._ops_obj = None
            self._drop_device_state()
        if self._ops_obj is None:
            if device.type != "cuda":
                raise RuntimeError("atm-vfi_amd.Network.forward runs on MI355X only: move the model and its inputs to "
                                   "'cuda' (HIP). There is no CPU implementation in the product; the CPU oracle lives in oracle/.")
            self._ops_obj = HipOps(device, checked=self._checked)
            self._apply_precision(self._ops_obj)
            self._ops_obj.gemm_workspace = self._gemm_scratch
        return self._ops_obj

    def _gemm_scratch(self, floats: int) -> torch.Tensor:
        """Split-K scratch of the plane-input GEMM (hip_ops.HipOps.gemm_workspace): workspace memory like every other buffer."""
        return self.buf("gemm_splitk_ws", floats)

    def _drop_plans(self):
        """Every recorded launch plan, of ``forward`` and of ``forward_pooled`` alike (and their warm-up counts)."""
        self._plans.clear()
        self._pool_plans.clear()

    def release_workspace(self):
        self._drop_plans()            # recorded plans and
        self._graphs.clear()          # captured graphs launch into the workspace
        self._workspaces.clear()
        self._bufs = {}
        self._ws_key = None
        self._frame_cache = None

    @staticmethod
    def _nbytes(ws: Dict) -> int:
        n = 0
        for t in ws.values():
            t = t.t if isinstance(t, Planes) else t
            n += t.numel() * t.element_size()
        return n

    def workspace_bytes(self) -> int:
        return sum(self._nbytes(ws) for ws in self._workspaces.values())

    def _select_workspace(self, key: Tuple):
        """Make the workspace of ``key`` current (creating it empty) and evict the least recently used others beyond the limits."""
        ws = self._workspaces.pop(key, None)
        self._workspaces[key] = {} if ws is None else ws          # most recently used last
        self._bufs = self._workspaces[key]
        self._ws_key = key
        while len(self._workspaces) > 1 and (len(self._workspaces) > self.max_workspaces or self.workspace_bytes() > self.workspace_cap_bytes):
            old = next(iter(self._workspaces))
            del self._workspaces[old]
            for gk in [g for g in self._graphs if g[-1] == old]:      # graphs captured into that workspace
                del self._graphs[gk]
            for plans in (self._plans, self._pool_plans):              # plans recorded into it
                for gk in [g for g in plans if g[-1] == old]:
                    del plans[gk]
        if len(self._geo) > 64:                                        # window maps are small; bound them all the same
            for gk in list(self._geo)[:len(self._geo) - 64]:
                del self._geo[gk]
            self._drop_plans()                                         # a plan may hold a map that just went
            self._graphs.clear()

    # ------------------------------------------------------------------ weights
    def _apply(self, fn, *a, **k):          # .to() / .cuda() / .float(): parameters get new storage
        self._plist = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._plist = None
        return super().load_state_dict(*a, **k)

    def invalidate_weights(self):
        """Forget the GEMM-layout copies of the weights.  Needed only after replacing a parameter's storage behind the module's back
        (``p.data = ...``): in-place updates, ``load_state_dict`` and ``.to()`` are noticed by themselves."""
        self._plist = None
        self._prepared_sig = None

    def _param_sig(self):
        """Per-forward check that the packed weights are current, ~40 us for the 236 entries: (1) the parameter OBJECTS are the cached
        ones (``_PARAM_EPOCH``: any assignment / registration / deletion of a Parameter on a sub-module re-walks the tree); (2) their
        storage pointers (``p.data = ...`` swaps); (3) their version counters (every in-place update through the parameter bumps
        one).  What nothing sees: writes through ``p.data`` (``p.data.add_()`` has a version counter of its own) --
        ``invalidate_weights()`` is for those."""
        pl = self._plist
        if pl is None or self._pepoch != _PARAM_EPOCH[0]:
            self._pepoch = _PARAM_EPOCH[0]
            pl = self._plist = [p for _, p in self.named_parameters()]
        return (tuple(map(_DATA_PTR_OF, pl)), tuple(map(_VERSION_OF, pl)), tuple(map(id, pl)))

    _RUNTIME_RESET = {"_ops_obj": None, "_prepared_sig": None, "_ws_key": None, "_graph_sig": None, "_plan_sig": None, "_plist": None,
                      "_pepoch": -1, "_frame_cache": None, "_primary": None, "_prepare_lock": None, "_reuse_first": False}
    _RUNTIME_DICTS = ("_bufs", "_geo", "_prepared", "_workspaces", "_graphs", "_plans", "_pool_plans", "_splitk_memo")

    def __getstate__(self):
        """copy.deepcopy / pickle / torch.save(module): parameters, buffers and settings travel; device-side runtime state
        (workspaces, packed weights, plans, graphs, the op backend, a replica's link to its primary and its lock) does not -- the copy
        is a stand-alone model that builds its own on first use."""
        d = dict(self.__dict__)
        d.update(self._RUNTIME_RESET)
        for k in self._RUNTIME_DICTS:
            d[k] = {}
        return d

    def __setstate__(self, state):
        super().__setstate__(state)
        _PARAM_EPOCH[0] += 1

    def replica(self) -> "Network":
        """A second front end on the SAME parameters: shares this model's parameter objects and its GEMM-layout weight copies, owns
        its workspaces, window maps, launch plans and op backend.  What ``host_io.PairStreams`` builds K of to keep K independent
        forwards in flight on K streams (the path's parallel axis is the pair axis: demo_2x.py:129-168,
        benchmark/test_vimeo90k.py:80-110): no buffer is shared between two replicas, so no cross-stream event is needed inside a
        forward.  Results are bit-identical to this model's.  Not part of the reference's API."""
        import copy
        rep = copy.copy(self)                     # nn.Module: _parameters / _buffers / _modules are shared by reference
        rep._ops_obj = None
        # (not through nn.Module.__setattr__: that would register the primary as a sub-module of its own replica)
        object.__setattr__(rep, "_primary", self if self._primary is None else self._primary)
        if rep._primary.__dict__.get("_prepare_lock") is None:
            import threading
            object.__setattr__(rep._primary, "_prepare_lock", threading.Lock())
        rep.local_motion_args = dict(self.local_motion_args)
        rep.global_motion_args = dict(self.global_motion_args)
        rep._prepared, rep._prepared_sig = {}, None
        rep._workspaces, rep._ws_key, rep._bufs, rep._geo = {}, None, {}, {}
        rep._graphs, rep._graph_sig, rep._plans, rep._plan_sig = {}, None, {}, None
        rep._pool_plans, rep._splitk_memo, rep._plan_stats = {}, {}, self._new_plan_stats()
        rep._frame_cache_on, rep._frame_cache, rep._reuse_first = False, None, False
        rep._plist, rep._pepoch = None, -1
        return rep

    def _prepare(self, ops):
        if self._primary is not None:
            # a replica reads the primary's packed weights; if they have to be (re)built now, that happens on THIS call's stream and
            # the other replicas' streams must not read them early: wait for the packing kernels once (rare: a parameter changed)
            pm = self._primary
            with pm._prepare_lock:                 # replicas may run on worker threads (host_io.PairStreams)
                before = pm._prepared_sig
                P = pm._prepare_unlocked(pm._ops(ops.device) if isinstance(ops, HipOps) else ops)
                if pm._prepared_sig is not before and isinstance(ops, HipOps):
                    torch.cuda.current_stream(ops.device).synchronize()
                self._prepared, self._prepared_sig, self._plist = P, pm._prepared_sig, pm._plist
            return P
        lock = self._prepare_lock
        if lock is None:
            return self._prepare_unlocked(ops)
        with lock:                                 # a model with replicas: they may be preparing on other threads right now
            return self._prepare_unlocked(ops)

    def _prepare_unlocked(self, ops):
        sig = self._param_sig()
        if sig == self._prepared_sig:
            return self._prepared
        sd = {k: v for k, v in self.named_parameters()}
        P: Dict[str, object] = {}
        for k, p in sd.items():
            P[k] = p.detach()
        for sp in S.param_schema(self._v):
            k, shp = sp.key, sp.shape
            if sp.is_buffer or not k.endswith(".weight"):
                continue
            w = sd[k].detach()
            if len(shp) == 4 and "dwconv" in k:
                P["pk:" + k] = ops.pack_dw_weight(w)
            elif len(shp) == 4 and shp[2] == 2:                      # ConvTranspose2d (Cin,Cout,2,2)
                P["pk:" + k] = ops.pack_weight(GEMM_DECONV, w)
            elif len(shp) == 4 and shp[2] == 1 and ".proj." in k:    # fusion 1x1 conv used as a row GEMM
                P["pk:" + k] = ops.pack_weight(GEMM_LINEAR, w.reshape(shp[0], shp[1]))
            elif len(shp) == 4:
                P["pk:" + k] = ops.pack_weight(GEMM_CONV, w)
            elif len(shp) == 2 and ".attn.mlp." not in k:
                if k.endswith("attn.kv.weight"):
                    continue
                if k.endswith("attn.q.weight"):                      # [Wq; Wkv] -> one [3C,C] projection
                    kv = sd[k.replace(".q.weight", ".kv.weight")].detach()
                    P["pk:" + k.replace(".q.weight", ".qkv.weight")] = ops.pack_weight(GEMM_LINEAR, torch.cat([w, kv], 0))
                else:
                    P["pk:" + k] = ops.pack_weight(GEMM_LINEAR, w)
        # refiner input as split planes: [dec2 (w3+5) | zeros to the next multiple of 8 | 15 image channels]: the 16-channel pack of
        # warp_blend's plane sink then starts on an 8-channel boundary (proj.0.weight gets zero input channels at the gap)
        w3 = self._v.decoder_widths[2] + S.MOTION_OUT
        gap = (-w3) % 8
        if getattr(ops, "split_planes_ok", False):
            wp = sd["proj.0.weight"].detach()
            wpp = torch.cat([wp[:, :w3], torch.zeros(wp.shape[0], gap, 3, 3, dtype=wp.dtype, device=wp.device), wp[:, w3:]], 1)
            P["pk:proj.0.weight:planes"] = ops.pack_weight(GEMM_CONV, wpp.contiguous())
            P["readout"] = ops.pack_readout(sd["refine_head.1.0.weight"].detach())
            P["stem"] = ops.pack_stem(*(sd[f"feat_extracts.{a}.{b}"].detach() for a in ("0.0", "0.1", "1.0") for b in ("0.weight", "0.bias", "1.weight")))
        # f16x3 contraction operands saturate at +-65504 (deviation 2).  Weights are known here: say so once per
        # parameter version if a checkpoint comes near; for activations there is f16x3_deviation() below.
        if isinstance(ops, HipOps):
            wmax = float(torch.stack([sd[sp.key].detach().abs().max() for sp in S.param_schema(self._v)
                                      if not sp.is_buffer and sp.key.endswith(".weight") and len(sp.shape) >= 2]).max())
            self.weight_abs_max = wmax
            if wmax > 16384.0:
                import warnings
                warnings.warn(f"atm-vfi_amd: largest |weight| of this checkpoint is {wmax:.0f}; the f16x3 engines saturate operands at "
                              "65504 -- check Network.f16x3_deviation(im0, im1) or use set_precision('f32')")
        for st in (1, 2):     # leading PReLU of decoder stages 1-2, applied on the deconv's input load
            P[f"inprelu:{st}"] = ops.pad_channels(sd[f"upsample_pyramid.{st}.0.weight"])
        self._prepared = P
        self._prepared_sig = sig
        return P

    # ------------------------------------------------------------------ the two paths
    def _plane_convs(self, ops) -> bool:
        """THE switch between the forward's two paths (paths.py).  True: 3x3 / stride-1 convs on the split-plane kernel (LDS-DMA halo,
        ping-pong wave groups), their inputs written as split planes by the producing layer's sink, fp32 copies only where something
        other than a contraction reads them."""
        return self._plane_deconvs(ops) and self._rows_fit_planes

    def _path(self, ops):
        """The stages of one eager forward, bound to its backend and current packed weights (made after ``_rows_fit_planes`` is known)."""
        return (PlanesPath if self._plane_convs(ops) else RowsPath)(self, ops, self._prepare(ops))

    @staticmethod
    def _stacked(buf, off, c):
        """View the channel range [off, off+2c) of an [B,h,w,LD] buffer as the frame-stacked token
        matrix [2, B*h*w, c]: '(N B) (H W) C -> B (N C) H W' of the reference without moving data."""
        b, h, w, ld = buf.shape
        flat = buf.reshape(b * h * w, ld)[:, off:off + 2 * c]
        return flat.unflatten(1, (2, c)).permute(1, 0, 2)

    def _motion_branch(self, path, branch, mlp, x_tokens, b, h, w, ws, tag):
        """Two ATMFormer blocks + motion MLP (estimate_{local,global}_motion, network_base.py:367-415).
        Returns (mlp_in buffer, last hidden map) -- the caller runs the 1x1 head into its own slice."""
        c = x_tokens.shape[-1]
        cin = 8 + 2 * c
        mlp_in = self.buf(f"{tag}mlp_in", b, h, w, cin)
        flat = mlp_in.reshape(b * h * w, cin)
        sinks = path.motion_sinks(tag, b * h * w, cin, c)
        x = x_tokens
        for blk in range(2):
            mdst = flat[:, 4 * blk:4 * blk + 4].unflatten(1, (2, 2)).permute(1, 0, 2)       # '(N B) L K -> B L (N K)'
            out = self._stacked(mlp_in, 8, c) if blk == 1 else self.buf(f"{tag}blk0", 2 * b * h * w, c)
            self._block(path.ops, path.P, f"{branch}.{blk}", x, 2 * b, h, w, ws, 0 if blk == 0 else ws // 2, True, out, mdst, tag,
                        out_sink=sinks[blk][0], motion_sink=sinks[blk][1])
            x = out
        return mlp_in, path.motion_mlp(mlp, mlp_in, b, h, w, tag)

    def _global_from_tokens(self, path, tokens, b, h_, w_, tag):
        """The pair half of estimate_global_motion (network_base.py:401-415): two ATMFormer blocks + the motion MLP on the frame-stacked
        tokens [2B*h_*w_, global_dim].  Returns the raw 5-channel map [B,h_,w_,5] (in an 8-float-per-pixel buffer)."""
        _, t2 = self._motion_branch(path, "global_motion_atmformer", "global_motion_mlp", tokens, b, h_, w_,
                                    self.global_motion_args["window_size"], tag + "g")
        gout = self.buf(f"{tag}gout", b, h_, w_, 8)
        path.head1x1("global_motion_mlp.2", t2, b, h_, w_, gout[..., :5])
        return gout

    def _ensemble_flows(self, path, im0, im1):
        """multiscale_global_motion_ensemble (network_base.py:564-605): global flows from the x1, x1/2
        and x1/4 inputs; per sample keep the one whose warped full-resolution frames agree best."""
        ops = path.ops
        b, _, h, w = im0.shape
        cands, losses = [], []
        c0, c1 = im0, im1
        for lvl in range(3):
            if lvl:
                n0 = self.buf(f"ens{lvl}i0", b, 3, h >> lvl, w >> lvl); ops.resize(c0, n0)
                n1 = self.buf(f"ens{lvl}i1", b, 3, h >> lvl, w >> lvl); ops.resize(c1, n1)
                c0, c1 = n0, n1
            hh, ww = h >> lvl, w >> lvl
            if hh % 16 or ww % 16:
                raise ValueError(f"ensemble_global_motion needs H, W divisible by 64 (level {lvl} is {hh}x{ww})")
            x0 = self.buf(f"ens{lvl}x0", 2 * b, hh, ww, 4); ops.pack_frames(c0, c1, x0)
            _, e2, fuse = path.encoder(x0, f"ens{lvl}")
            gtok = path.global_tokens(e2, fuse, f"ens{lvl}")                                     # estimate_global_motion (:391-415)
            gout = self._global_from_tokens(path, gtok, b, hh // 16, ww // 16, f"ens{lvl}")
            f0 = gout[..., 0:2].permute(0, 3, 1, 2)
            f1 = gout[..., 2:4].permute(0, 3, 1, 2)
            factor = 16 << lvl
            u0 = self.buf(f"ens{lvl}u0", b, 2, h, w); ops.resize(f0, u0, float(factor))      # global_alignmentness (:548-562)
            u1 = self.buf(f"ens{lvl}u1", b, 2, h, w); ops.resize(f1, u1, float(factor))
            wa = self.buf("ens_wa", b, 3, h, w); ops.flow_warp(im0, u0, wa)
            wb = self.buf("ens_wb", b, 3, h, w); ops.flow_warp(im1, u1, wb)
            loss = self.buf(f"ens{lvl}loss", b)
            ops.l1_mean(wa, wb, loss, workspace=self.buf("ens_l1_ws", ops.l1_mean_workspace_floats(b, 3 * h * w)) if hasattr(ops, "l1_mean_workspace_floats") else None)
            # candidate at the level-0 flow resolution (H/16): x1, x2, x4 up-sampling of the coarser flows
            k0 = self.buf(f"ens_c0_{lvl}", b, 2, h // 16, w // 16); ops.resize(f0, k0, float(1 << lvl))
            k1 = self.buf(f"ens_c1_{lvl}", b, 2, h // 16, w // 16); ops.resize(f1, k1, float(1 << lvl))
            cands.append((k0, k1)); losses.append(loss)
        if hasattr(ops, "ensemble_select"):                # the pick inside the C ABI: no device arithmetic outside it, plannable
            s0, s1 = self.buf("ens_sel0", b, 2, h // 16, w // 16), self.buf("ens_sel1", b, 2, h // 16, w // 16)
            ops.ensemble_select(losses, cands, s0, s1)
            return s0, s1
        ls = torch.stack(losses, 0)                        # [3,B]; first minimum wins like the reference's if/elif chain
        pick = ls.argmin(dim=0)
        sel0 = torch.stack([c[0] for c in cands], 0)       # [3,B,2,h_,w_]
        sel1 = torch.stack([c[1] for c in cands], 0)
        idx = torch.arange(b, device=pick.device)
        return sel0[pick, idx].contiguous(), sel1[pick, idx].contiguous()

    # ------------------------------------------------------------------ forward
    def enable_graphs(self, flag: bool = True):
        """Replay ``forward`` from a captured HIP graph (one per input shape / mode): the ~140 kernel launches of a pass are
        submitted as one graph launch, which removes the launch gaps (a few % at 1080p, most of the time on small frames).
        The returned tensors are the graph's static outputs: they are overwritten by the next call with the same shape.
        Not part of the reference's API; off by default."""
        self.use_graphs = bool(flag)
        if not flag:
            self._graphs.clear()

    def enable_frame_cache(self, flag: bool = True):
        """Video mode (demo_2x.py:129-168: pair i+1's first frame is pair i's second): keep the second frame's encoder + fusion
        tokens of every call, so that ``forward(im0, im1, reuse_first=True)`` runs ``shared_feat_extraction`` and the cross-scale
        fusion (network_base.py:342-352, 451-455) on the new frame only -- and, with ``global_motion`` on, the per-frame half of
        ``estimate_global_motion`` too (last_feat_extract + the global fusion, :391-400).  Exact: all of that is per frame, the pair
        meets in the ATMFormers.  Not with the ensemble (three input scales).  Not part of the reference's API; off by default."""
        self._frame_cache_on = bool(flag)
        self._frame_cache = None

    def f16x3_deviation(self, im0: torch.Tensor, im1: torch.Tensor) -> float:
        """max |I_t(f16x3) - I_t(exact fp32 engine)| on this frame pair: the run-time check that a checkpoint's activations stay inside
        the fp16 range of the split engines (an operand beyond 65504 saturates silently there; on the stress weights the largest
        |activation| is 24).  Costs one forward on each engine; expect ~1e-4, investigate above 1e-3."""
        keep = "f16x3-checked" if self._checked else self._precision
        try:
            self.set_precision("f32")
            ref = self.forward(im0, im1)["I_t"].clone()
            self.set_precision("f16x3")
            got = self.forward(im0, im1)["I_t"]
            return float((got - ref).abs().max())
        finally:
            self.set_precision(keep)

    def enable_plans(self, flag: bool = True):
        """Launch plans (default on): once a (shape, mode, weights) combination has run twice, its forward is recorded
        (``hip_ops.LaunchPlan``) and every later one is a single ``atmvfi_plan_run`` call -- same launches, same arguments, fresh
        output tensors -- instead of ~120 Python-side op calls.  Not used with the frame cache, graphs or per-launch profiling (those
        forwards contain copies outside the C ABI or need the individual launches).  Ensemble mode is planned too since round 4 (its
        per-sample pick is `atmvfi_ensemble_select`).

        ``forward_pooled`` is planned the same way, as two plans per key -- the frame stage over the stale slots and the pair stage --
        whose inputs are the pool's tensors and whose slot lists are rewritten per call (see its docstring); this switch turns
        those off too.  Calling it, with either value, restarts the counts of ``plan_stats()``."""
        self.use_plans = bool(flag)
        self._plan_stats = self._new_plan_stats()
        if not flag:
            self._drop_plans()

    PLAN_KINDS = ("forward", "pooled_frame", "pooled_pair")

    @classmethod
    def _new_plan_stats(cls) -> Dict[str, Dict[str, int]]:
        return {kind: {"eager": 0, "recorded": 0, "replayed": 0, "refused": 0} for kind in cls.PLAN_KINDS}

    def plan_stats(self) -> Dict[str, Dict[str, int]]:
        """Diagnostic, read-only: how the calls since construction (or the last ``enable_plans``) were submitted, per kind --
        ``"forward"``: ``forward`` calls; ``"pooled_frame"`` / ``"pooled_pair"``: the two stages of ``forward_pooled`` (the frame stage
        counts only in calls that had stale slots).  Each stage of each call lands in exactly one bin: ``eager`` (direct launches:
        warm-up, plans off, profiling, the checked build, graphs' and the frame cache's forwards, a key that cannot be planned),
        ``recorded`` (direct launches that were recorded into a plan that then passed its self-check), ``replayed`` (one
        ``atmvfi_plan_run``), ``refused`` (a recording that could not be expressed or failed its self-check; the key stays eager).
        A copy; not part of the reference's API."""
        return {kind: dict(c) for kind, c in self._plan_stats.items()}

    def _mode_fields(self, ops) -> Tuple:
        return (self.global_motion, self.ensemble_global_motion, self._precision, self._checked, getattr(ops, "attention_f16x3", None),
                self.local_motion_args["window_size"], self.global_motion_args["window_size"], getattr(ops, "warp_tiles", None),
                getattr(ops, "conv3_instance", None), getattr(ops, "gemm_tile_wn", None))

    def _pool_validity_key(self, ops, glob: bool, target) -> Tuple:
        """What a pool slot's tokens were computed under (``forward_pooled``): weights, ``global_motion``, the precision mode ("f16x3" /
        "f16" / "f32"; the checked build), the attention engine, the plane-row regime and the frame stage's split-K target."""
        return (self._prepared_sig, glob, self._precision, self._checked, getattr(ops, "attention_f16x3", None), self._rows_fit_planes, target)

    def _mode_key(self, ops, im0, im1) -> Tuple:
        return (tuple(im0.shape), tuple(im1.shape), str(im0.device)) + self._mode_fields(ops) + (self._workspace_key(im0),)

    def _sync_plan_sig(self):
        if self._plan_sig is not self._prepared_sig:         # parameters changed: recorded launches hold stale weight pointers
            self._drop_plans()
            self._plan_sig = self._prepared_sig

    def forward(self, im0: torch.Tensor, im1: torch.Tensor, reuse_first: bool = False):
        self._reuse_first = bool(reuse_first)
        st = self._plan_stats["forward"]
        if not im0.is_cuda or self._frame_cache_on or self._checked:
            st["eager"] += 1
            return self._forward_eager(im0, im1)
        if self.use_graphs:
            st["eager"] += 1
            return self._forward_graph(im0, im1)
        ops = self._ops_obj
        pl = self._plist
        if (not self.use_plans or not isinstance(ops, HipOps) or ops.profile is not None
                or pl is None or pl[0].device != im0.device or torch.cuda.is_current_stream_capturing()):
            st["eager"] += 1
            return self._forward_eager(im0, im1)         # (also every case that must raise: it validates devices and shapes)
        self._prepare(ops)
        self._sync_plan_sig()
        key = self._mode_key(ops, im0, im1)
        ent = self._plans.get(key, 0)
        if isinstance(ent, LaunchPlan):
            if im0.shape != im1.shape or im0.device != im1.device or im0.device != ops.device:
                st["eager"] += 1
                return self._forward_eager(im0, im1)         # raises the proper error
            self._select_workspace(key[-1])                  # replay counts as a use for the workspace LRU
        with torch.cuda.device(im0.device):
            a = im0.detach().contiguous().float()
            b = im1.detach().contiguous().float()
            if ent == 2 and a.data_ptr() < b.data_ptr() + b.numel() * 4 and b.data_ptr() < a.data_ptr() + a.numel() * 4:
                # aliased / overlapping frames (net(x, x)) on the call that would record: a recording could not tell a pointer into one
                # from a pointer into the other and every later net(a, b) of this shape would replay as net(a, a).  Stay eager and
                # leave the key's state alone; the next call with distinct frames records.
                st["eager"] += 1
                return self._forward_eager(im0, im1)
            return self._planned("forward", self._plans, key, ops, (a, b), lambda: self._forward_eager(a, b))

    def forward_scaled(self, im0: torch.Tensor, im1: torch.Tensor, scale: int = 2, want=()):
        """Half-resolution motion (scaled.py holds the definition): ``forward`` on the 2 x 2 box averages of the two [B,3,H,W] frames
        (B <= 16; H, W even with H/2, W/2 acceptable to ``forward``), then one launch that up-samples flows, mask and residual x2 and
        warps and blends the FULL-SIZE frames (``HipOps.frame_half``, ``HipOps.synth_up2``).  -> {"I_t": fp32 [B,3,H,W], "half":
        ``forward``'s dict at half size} plus any of "opt_flow_0", "opt_flow_1", "occ_mask1" at full size that ``want`` names.  Only
        ``scale=2`` exists.  Precision mode, launch plans and ``global_motion`` are the model's: the half-size forward is an ordinary
        ``forward`` call.  Not part of the reference's API."""
        if scale != 2 or isinstance(scale, bool):
            raise ValueError(f"forward_scaled: only scale=2 is implemented, got {scale!r}")
        if not im0.is_cuda:
            return scaled.forward_scaled_host(self.forward, im0, im1, want)
        if im0.shape != im1.shape or im0.dim() != 4 or im0.shape[1] != 3 or im0.shape[2] % 2 or im0.shape[3] % 2 or im0.device != im1.device:
            raise ValueError(f"forward_scaled: two [B,3,H,W] frames of one device with even H and W expected, got {tuple(im0.shape)} and "
                             f"{tuple(im1.shape)}")
        b, _, H, W = im0.shape
        if b > 16:
            raise ValueError(f"forward_scaled: at most 16 pairs per call, got {b}")
        ops = self._ops(im0.device)
        with torch.cuda.device(im0.device), torch.no_grad():
            a = im0.detach().contiguous().float()
            c = im1.detach().contiguous().float()
            key = (str(im0.device), b, H, W)
            halves = self._scaled_halves.get(key)
            if halves is None:
                self._scaled_halves.clear()                      # one shape at a time
                halves = self._scaled_halves[key] = (ops.empty(b, 3, H // 2, W // 2), ops.empty(b, 3, H // 2, W // 2))
            ops.frame_half(a, halves[0])
            ops.frame_half(c, halves[1])
            o = self.forward(halves[0], halves[1])
            full = ops.synth_up2(o, a, c, want=want)
        out = {"I_t": full["I_t"], "half": o}
        out.update({k: full[k] for k in want})
        return out

    @staticmethod
    def _same_results(x, y) -> bool:
        if isinstance(x, torch.Tensor):
            return isinstance(y, torch.Tensor) and x.shape == y.shape and bool(torch.equal(x, y))
        if isinstance(x, dict):
            return isinstance(y, dict) and x.keys() == y.keys() and all(Network._same_results(v, y[k]) for k, v in x.items())
        if isinstance(x, (list, tuple)):
            return isinstance(y, (list, tuple)) and len(x) == len(y) and all(Network._same_results(u, v) for u, v in zip(x, y))
        return x == y

    def _planned(self, kind: str, plans: Dict, key, ops, inputs, body, lists=None, check=None):
        """THE launch-plan state machine, of ``forward`` ("forward", over ``_plans``) and of the two stages of ``forward_pooled``
        ("pooled_frame", "pooled_pair", over ``_pool_plans``) alike.  The first two calls of a ``key`` run ``body`` (direct launches:
        they build the workspace, maps, kernel attributes), the third records it, later ones replay the plan with ``inputs`` as the
        per-call tensors and ``lists`` as the per-call slot lists.  ``key`` None: not plannable now (plans off, profiling, the checked
        build, stream capture).  Every call lands in exactly one bin of ``plan_stats()[kind]``.
        ``check(out, replay) -> bool``: the record-time self-check, ``replay(**kw)`` running the fresh plan once; a recording that fails
        it, or cannot be expressed, leaves the key on direct launches.  Default: replay into NaN-filled outputs and require ``body``'s
        results bit for bit (the forward is run-to-run deterministic) -- a pointer patched into the wrong slot, a missed patch or a
        launch that was not recorded shows up here, before the plan ever serves a caller."""
        st = self._plan_stats[kind]
        ent = False if key is None else plans.get(key, 0)
        if isinstance(ent, LaunchPlan):
            if tuple(t.data_ptr() & 15 for t in inputs) != ent.align:
                # the recording chose kernels for its inputs' alignment (the LDS-staged warps load rows 16 bytes at a time): a
                # differently aligned view takes the direct launches, which choose again
                st["eager"] += 1
                return body()
            st["replayed"] += 1
            return ent.run(inputs, ops.device, ops._stream(), lists=lists)
        if ent is False or ent < 2:
            if ent is not False:
                plans[key] = ent + 1
            st["eager"] += 1
            return body()
        try:
            ops.begin_plan(inputs)
            out = body()
            plan = ops.end_plan(out)
        except PlanUnsupported:
            ops.abort_plan()
            plan, out = None, body()
        except Exception:
            ops.abort_plan()
            raise
        ok = plan is not None
        if ok:
            replay = lambda **kw: plan.run(inputs, ops.device, ops._stream(), lists=lists, **kw)
            ok = self._same_results(out, replay(poison=True)) if check is None else check(out, replay)
            if not ok:
                import warnings
                warnings.warn("atm-vfi_amd: a recorded launch plan did not reproduce its own forward; this input shape stays on direct launches"
                              if kind == "forward" else
                              f"atm-vfi_amd: a recorded launch plan ({kind}) did not reproduce its own stage; this key stays on direct launches")
        plans[key] = plan if ok else False
        st["recorded" if ok else "refused"] += 1
        return out

    def _forward_graph(self, im0: torch.Tensor, im1: torch.Tensor):
        ops = self._ops(im0.device)
        self._prepare(ops)
        if self._graph_sig is not self._prepared_sig:        # parameters changed: the captured launches hold stale weights
            self._graphs.clear()
            self._graph_sig = self._prepared_sig
        key = self._mode_key(ops, im0, im1)
        ent = self._graphs.get(key)
        if ent is None:
            for _ in range(2):                               # validation, workspace, window maps, packed weights, kernel attributes
                self._forward_eager(im0, im1)
            torch.cuda.synchronize(im0.device)
            s0 = im0.detach().float().contiguous().clone()
            s1 = im1.detach().float().contiguous().clone()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._forward_eager(s0, s1)
            ent = (graph, s0, s1, out)
            self._graphs[key] = ent
        graph, s0, s1, out = ent
        self._select_workspace(key[-1])                      # replay counts as a use: the hot shape must not be the LRU victim
        s0.copy_(im0)
        s1.copy_(im1)
        graph.replay()
        return out

    def _workspace_key(self, im0: torch.Tensor) -> Tuple:
        return (str(im0.device), tuple(im0.shape), bool(self.global_motion), bool(self.ensemble_global_motion))

    def _forward_eager(self, im0: torch.Tensor, im1: torch.Tensor):
        if im0.shape != im1.shape or im0.dim() != 4 or im0.shape[1] != 3:
            raise ValueError(f"expected two [B,3,H,W] frames, got {tuple(im0.shape)} and {tuple(im1.shape)}")
        if im0.device != im1.device:
            raise ValueError(f"the two frames live on different devices ({im0.device}, {im1.device})")
        ops = self._ops(im0.device)
        if im0.is_cuda:
            for prm in self.parameters():
                if prm.device != im0.device:
                    raise RuntimeError(f"model parameters are on {prm.device}, inputs on {im0.device}: move the model with .to(device)")
                break
            with torch.cuda.device(im0.device):       # the kernels launch on the current device's stream
                return self._forward_on_device(ops, im0, im1)
        return self._forward_on_device(ops, im0, im1)

    def _forward_on_device(self, ops, im0: torch.Tensor, im1: torch.Tensor):
        self._select_workspace(self._workspace_key(im0))
        if hasattr(ops, "begin_forward"):
            ops.begin_forward()
        b, _, H, W = im0.shape
        # the plane kernels address a chunk's pixel rows with 32-bit byte offsets (64 B per row): beyond 2^26 rows of the largest
        # map (2 B frames at full resolution; e.g. batch 8 at 4K) the forward takes the fp32-input kernels instead
        self._rows_fit_planes = 2 * b * H * W < (1 << 26)
        need = 16 if self.global_motion else 8
        if H % need or W % need:
            raise ValueError(f"H and W must be multiples of {need} (got {H}x{W}); pad with InputPadder as the reference's callers do")
        v = self._v
        d = v.hidden_dims
        C = v.local_dim
        with torch.no_grad():
            im0 = im0.detach().contiguous().float()
            im1 = im1.detach().contiguous().float()
            path = self._path(ops)
            h, w = H // 8, W // 8
            # image pyramids (network_base.py:444-448)
            # Levels >= 1 of both frames live stacked along the batch axis ([:b] = frame 0, [b:] = frame 1): one launch per level
            # instead of two (the same kernels on 2b images); level 0 are the caller's two tensors.
            pyr_st = [None] + [self.buf(f"pyr_{l}", 2 * b, 3, H >> l, W >> l) for l in range(1, 4)]
            # encoder + local fusion (:451-455)
            x0 = self.buf("x0", 2 * b, H, W, 4)
            if getattr(ops, "pyramid_packs", False):
                ops.image_pyramid(im0, im1, pyr_st[1], pyr_st[2], pyr_st[3], pack=x0)   # one launch: three levels of both frames + torch.cat as NHWC4
            else:
                ops.image_pyramid(im0, im1, pyr_st[1], pyr_st[2], pyr_st[3])
                ops.pack_frames(im0, im1, x0)
            cache_ok = self._frame_cache_on and not (self.global_motion and self.ensemble_global_motion)
            glob = self.global_motion and not self.ensemble_global_motion
            cg = v.global_dim
            ck = (self._ws_key, id(self._prepared_sig))     # same device, shape, mode and weights as the call that filled the cache
            hit = cache_ok and self._reuse_first and self._frame_cache is not None and self._frame_cache[0] == ck
            gtok = None
            if hit:
                # frame 0 of this pair was frame 1 of the previous call: encoder + fusions (everything that is per frame) on the
                # new frame only; the previous call's tokens of the shared frame are copied in front of the new ones
                one, g_one = self._frame_stage(path, x0[b:], "fc", "fcl", glob)                              # [B*h*w, C], [B*h_*w_, cg]
                feat = self.buf("lfnorm", 2 * b * h * w, C)
                feat[:b * h * w].copy_(self._frame_cache[1])
                feat[b * h * w:].copy_(one)
                if glob:
                    n_g = b * (H // 16) * (W // 16)
                    gtok = self.buf("gfnorm", 2 * n_g, cg)
                    gtok[:n_g].copy_(self._frame_cache[2])
                    gtok[n_g:].copy_(g_one)
            else:
                feat, gtok = self._frame_stage(path, x0, "", "l", glob)                                      # [2B*h*w, C], [2B*h_*w_, cg]
            if cache_ok:
                keep = self.buf("frame_cache_tokens", b * h * w, C)
                keep.copy_(feat[b * h * w:])
                keep_g = None
                if glob:
                    n_g = b * (H // 16) * (W // 16)
                    keep_g = self.buf("frame_cache_gtokens", n_g, cg)
                    keep_g.copy_(gtok[n_g:])
                self._frame_cache = (ck, keep, keep_g)
            self._reuse_first = False
            return self._pair_stage(path, im0, im1, pyr_st, feat, gtok)

    def _frame_stage_splitk(self, ops, H: int, W: int, f: int) -> Tuple:
        """The split-K factors the library would choose for the contraction launches of ``_frame_stage`` on ``f`` frames of H x W, in
        launch order (``PlanesPath.frame_stage_splitk``, kept directly below the stages it mirrors).  Empty when the forward is not on
        the plane kernels (nothing splits there)."""
        if not (isinstance(ops, HipOps) and self._plane_convs(ops)):
            return ()
        return PlanesPath.frame_stage_splitk(self, ops, H, W, f, self.global_motion and not self.ensemble_global_motion)

    def forward_pooled(self, pool, left, right, exact: bool = True):
        """``forward`` on frames that live in a ``multiframe.FramePool``: pair j = (slot ``left[j]``, slot ``right[j]``), batch
        ``B = len(left)`` (at most 16).  What is per frame (``_frame_stage``) runs ONCE, as one batch, over the referenced slots whose
        tokens are stale -- never computed, ``put`` since, or computed under other weights / ``global_motion`` / precision -- and is kept
        in the pool; frames and tokens of the pairs are gathered with ``atmvfi_pool_blocks`` and ``_pair_stage`` runs as in
        ``forward``.  Returns ``forward``'s dict of fresh tensors, bit-identical to ``forward`` on the same batch.  A stale slot is
        recomputed, never an error; a pool of another device, another model width or a slot outside the pool raises ``ValueError``.
        With ``ensemble_global_motion`` nothing is per frame: the frames are gathered and the plain path runs.  Every device
        operation is a launch of the C ABI.  An odd number of stale frames is fed to ``pack_frames`` (which takes pairs) by naming the
        last one twice; the encoder runs on the distinct ones only.

        Launch plans (``enable_plans``, default on): the call is two stages, each replayed from a ``hip_ops.LaunchPlan`` once its key
        has run twice with direct launches -- the FRAME stage (gather of the stale frames, ``pack_frames``, ``_frame_stage``, the token
        scatters; keyed by batch size, stale count and the count it is filled up to; runs only when something is stale; no outputs)
        and the PAIR stage (the three gathers of the pairs, the image pyramid, ``_pair_stage``; keyed by batch size; ten fresh
        output tensors).  The pool's three tensors are the plans' per-call inputs and the slot lists are per-call host lists, so
        ANY pool of this shape and slot count, and any slots, replay the same plans: same launches, same arguments as the direct
        path.  Each recording is checked by one replay against what the recording call's direct launches produced, bit for bit; a
        stage that cannot be recorded stays on direct launches.  What stays in Python per call: validation, the stale scan, the
        split-K comparison (memoised), the ``pool.keys`` updates, the workspace LRU.  Direct launches throughout with plans off,
        per-launch profiling (``ops.profile``), the checked build, a capturing stream and the ensemble.  ``plan_stats()`` counts.

        ``exact`` (default): bit-identity with ``forward`` holds for every size.  On small frames some launches of the frame stage
        split K by the number of rows they see (``_frame_stage_splitk``), i.e. by the number of frames in the batch; tokens are then
        valid only for forwards whose plain frame stage (2B frames) would have used the same factors, and a stale batch whose own
        count gives other factors is filled up with repeats of its last frame to the nearest count that gives them (2B at the most).
        At 1088x1920 no launch splits and nothing is ever filled up.  ``exact=False`` skips both: fewest frame encodes, results
        within rounding of ``forward``'s where the factors differ.  Not part of the reference's API."""
        left, right = [int(s) for s in left], [int(s) for s in right]
        b = len(left)
        if b < 1 or b != len(right) or b > 16:
            raise ValueError(f"forward_pooled: need 1..16 pairs, got {len(left)} left and {len(right)} right slots")
        for need in ("frames", "tokens_l", "tokens_g", "keys", "hp", "wp"):
            if not hasattr(pool, need):
                raise TypeError("forward_pooled: pool must be a multiframe.FramePool")
        dev = pool.frames.device
        if any(s < 0 or s >= pool.slots for s in left + right):
            raise ValueError(f"forward_pooled: slot outside 0..{pool.slots - 1}")
        prm = next(self.parameters())
        if prm.device != dev:
            raise ValueError(f"forward_pooled: the pool lives on {dev}, the model on {prm.device}")
        v = self._v
        H, W = pool.hp, pool.wp
        if tuple(pool.tokens_l.shape[1:]) != ((H // 8) * (W // 8), v.local_dim) or pool.tokens_g.shape[2] != v.global_dim:
            raise ValueError("forward_pooled: the pool was made for a model of another shape")
        need = 16 if self.global_motion else 8
        if H % need or W % need:
            raise ValueError(f"H and W must be multiples of {need} (got {H}x{W}); pad with InputPadder as the reference's callers do")
        ops = self._ops(dev)
        self._reuse_first = False
        with torch.cuda.device(dev), torch.no_grad():
            wkey = (str(dev), (b, 3, H, W), bool(self.global_motion), bool(self.ensemble_global_motion))
            self._select_workspace(wkey)                     # (a replay counts as a use for the workspace LRU)
            if self.global_motion and self.ensemble_global_motion:
                self._plan_stats["pooled_pair"]["eager"] += 1
                ims = self.buf("pool_im", 2 * b, 3, H, W)
                ops.pool_blocks(pool.frames, left + right, ims)
                return self._forward_on_device(ops, ims[:b], ims[b:])
            if hasattr(ops, "begin_forward"):
                ops.begin_forward()
            self._rows_fit_planes = 2 * b * H * W < (1 << 26)
            path = self._path(ops)
            inputs = (pool.frames, pool.tokens_l, pool.tokens_g)
            planned = (self.use_plans and self._pooled_plans_on and isinstance(ops, HipOps) and ops.profile is None and not self._checked
                       and not torch.cuda.is_current_stream_capturing())
            if planned:
                self._sync_plan_sig()
            glob = bool(self.global_motion)
            target = self._splitk_of(ops, H, W, 2 * b) if exact else None
            vkey = self._pool_validity_key(ops, glob, target)
            stale = []
            for s in left + right:
                if s not in stale and pool.keys[s] != vkey:
                    stale.append(s)
            if stale:
                f = run = len(stale)
                while exact and run < 2 * b and self._splitk_of(ops, H, W, run) != target:
                    run += 1
                fe = run + (run & 1)
                key = ("pooled_frame", f, run, pool.slots, self._rows_fit_planes) + self._mode_fields(ops) + (wkey,)
                self._planned("pooled_frame", self._pool_plans, key if planned else None, ops, inputs,
                              lambda: self._pooled_frame_stage(path, pool, stale, run, glob),
                              lists={"stale_padded": stale + stale[-1:] * (fe - f), "stale": stale},
                              check=lambda out, replay: self._replay_rewrites_tokens(pool, stale, replay))
                for s in stale:
                    pool.keys[s] = vkey
            key = ("pooled_pair", pool.slots, self._rows_fit_planes) + self._mode_fields(ops) + (wkey,)
            return self._planned("pooled_pair", self._pool_plans, key if planned else None, ops, inputs,
                                 lambda: self._pooled_pair_stage(path, pool, left, right, glob), lists={"pairs": left + right})

    def _splitk_of(self, ops, H: int, W: int, f: int) -> Tuple:
        """``_frame_stage_splitk``, remembered: a function of the size, the frame count and the mode (never of the weights' values), and
        ``forward_pooled`` asks it up to 2B times per call."""
        key = (H, W, f, id(ops), self._rows_fit_planes, getattr(ops, "gemm_workspace", None) is None) + self._mode_fields(ops)
        got = self._splitk_memo.get(key)
        if got is None:
            if len(self._splitk_memo) > 512:
                self._splitk_memo.clear()
            got = self._splitk_memo[key] = self._frame_stage_splitk(ops, H, W, f)
        return got

    def _pooled_frame_stage(self, path, pool, stale, run: int, glob: bool):
        """The frame stage of ``forward_pooled``: the ``stale`` slots' frames (filled up to ``run``, and to an even count for
        ``pack_frames``, with repeats of the last) through ``_frame_stage``; the tokens of the distinct ones go back into the pool.
        Slot lists carry roles: a launch plan rewrites them per replay.  Writes into the pool only; returns None."""
        ops = path.ops
        H, W = pool.hp, pool.wp
        f = len(stale)
        fe = run + (run & 1)
        n_l, n_g = (H // 8) * (W // 8), (H // 16) * (W // 16)
        g = self.buf("pool_stale", fe, 3, H, W)
        ops.pool_blocks(pool.frames, stale + stale[-1:] * (fe - f), g, role="stale_padded")
        x0 = self.buf("pool_x0", fe, H, W, 4)
        ops.pack_frames(g[:fe // 2], g[fe // 2:], x0)
        t_l, t_g = self._frame_stage(path, x0[:run], "fp", "fpl", glob)
        ops.pool_blocks(pool.tokens_l, stale, t_l[:f * n_l], to_pool=True, role="stale")
        if glob:
            ops.pool_blocks(pool.tokens_g, stale, t_g[:f * n_g], to_pool=True, role="stale")

    def _pooled_pair_stage(self, path, pool, left, right, glob: bool):
        """The pair stage of ``forward_pooled``: frames and tokens of the pairs gathered from the pool (role "pairs"), the image
        pyramid, ``_pair_stage``.  Returns the forward's dict of fresh tensors."""
        ops = path.ops
        b = len(left)
        H, W = pool.hp, pool.wp
        v = self._v
        n_l, n_g = (H // 8) * (W // 8), (H // 16) * (W // 16)
        ims = self.buf("pool_im", 2 * b, 3, H, W)
        ops.pool_blocks(pool.frames, left + right, ims, role="pairs")
        im0, im1 = ims[:b], ims[b:]
        feat = self.buf("lfnorm", 2 * b * n_l, v.local_dim)
        ops.pool_blocks(pool.tokens_l, left + right, feat, role="pairs")
        gtok = None
        if glob:
            gtok = self.buf("gfnorm", 2 * b * n_g, v.global_dim)
            ops.pool_blocks(pool.tokens_g, left + right, gtok, role="pairs")
        pyr_st = [None] + [self.buf(f"pyr_{l}", 2 * b, 3, H >> l, W >> l) for l in range(1, 4)]
        ops.image_pyramid(im0, im1, pyr_st[1], pyr_st[2], pyr_st[3])
        return self._pair_stage(path, im0, im1, pyr_st, feat, gtok)

    def _replay_rewrites_tokens(self, pool, stale, replay) -> bool:
        """The record-time self-check of the pooled FRAME stage (``_planned``), which has no outputs: it writes the stale slots' tokens
        into the pool.  Keep those tokens, fill the slots with NaN, replay, compare -- and put the kept ones back if the replay wrote
        anything else."""
        idx = torch.tensor(stale, device=pool.frames.device)
        toks = [pool.tokens_l] + ([pool.tokens_g] if self.global_motion else [])
        kept = [t.index_select(0, idx) for t in toks]
        for t in toks:
            t.index_fill_(0, idx, float("nan"))
        replay()
        ok = all(bool(torch.equal(t.index_select(0, idx), k)) for t, k in zip(toks, kept))
        if not ok:
            for t, k in zip(toks, kept):
                t.index_copy_(0, idx, k)
        return ok

    def _frame_stage(self, path, x0, tag: str, ltag: str, glob: bool):
        """Everything ``forward`` computes PER FRAME, on the F NHWC4-packed frames ``x0`` [F,H,W,4]: shared_feat_extraction, the
        cross-scale fusion and its LayerNorm (network_base.py:342-352, 451-455) and, with ``glob`` (global branch on, ensemble off),
        the per-frame half of estimate_global_motion (:391-400).  Returns the local tokens [F*h*w, C] and the global tokens
        [F*h_*w_, Cg] (or None) in workspace buffers named by ``tag`` / ``ltag``.  The pair meets in ``_pair_stage``."""
        d = self._v.hidden_dims
        e1, e2, fuse_l = path.encoder(x0, tag)
        feat = path.fusion("cross_scale_feature_fusion", e1, e2, fuse_l, d[2], d[1], ltag)
        return feat, (path.global_tokens(e2, fuse_l, tag) if glob else None)

    def _pair_stage(self, path, im0, im1, pyr_st, feat, gtok):
        """The rest of the forward, from the frame-stacked tokens on: ``feat`` [2B*h*w, C] and ``gtok`` [2B*h_*w_, Cg] (left frames
        first, then right frames), the contiguous fp32 frames ``im0`` / ``im1`` [B,3,H,W] and their stacked pyramid levels 1..3
        ``pyr_st`` ([2B,3,H>>l,W>>l]).  Returns the forward's dict.  The skeleton both paths share: the contractions between the
        warps are ``path``'s stages."""
        ops = path.ops
        b, _, H, W = im0.shape
        C = self._v.local_dim
        h, w = H // 8, W // 8
        pyr0 = [im0] + [t[:b] for t in pyr_st[1:]]
        pyr1 = [im1] + [t[b:] for t in pyr_st[1:]]
        it_list: List[torch.Tensor] = []
        w0_list: List[torch.Tensor] = []
        w1_list: List[torch.Tensor] = []

        def blend(p0, p1, mot, *full, **pack):
            a, c, t = (ops.empty(b, 3, *p0.shape[-2:]) for _ in range(3))
            ops.warp_blend(p0, p1, mot, a, c, t, *full, **pack)
            w0_list.insert(0, a); w1_list.insert(0, c); it_list.insert(0, t)
        with torch.no_grad():
            x_tokens = feat
            if self.global_motion:                                                        # (:457-485)
                h_, w_ = H // 16, W // 16
                # the two global flows stacked like the frames: every warp / x2 up-sampling below is one launch for both
                gf = self.buf("gf_3", 2 * b, 2, h, w)
                if self.ensemble_global_motion:
                    g0, g1 = self._ensemble_flows(path, im0, im1)
                    ops.resize(g0, gf[:b], 2.0); ops.resize(g1, gf[b:], 2.0)
                else:
                    gout = self._global_from_tokens(path, gtok, b, h_, w_, "")
                    i_16 = self.buf("im_16", 2 * b, 3, h_, w_); ops.resize(pyr_st[3], i_16)
                    blend(i_16[:b], i_16[b:], gout[..., :5])
                    if b == 1:
                        # one pair: [flow0 | flow1] of the motion map's first four channels IS the stacked layout [2, 2, h, w]: one launch
                        ops.resize(gout[..., 0:4].permute(0, 3, 1, 2), gf.view(1, 4, h, w), 2.0)
                    else:
                        ops.resize(gout[..., 0:2].permute(0, 3, 1, 2), gf[:b], 2.0); ops.resize(gout[..., 2:4].permute(0, 3, 1, 2), gf[b:], 2.0)
                featw = self.buf("featw", 2 * b, h, w, C)
                ops.flow_warp_nhwc(feat.reshape(2 * b, h, w, C), gf, featw)
                x_tokens = featw.reshape(2 * b * h * w, C)
                for i in (3, 2, 1, 0):
                    nw = self.buf(f"pw_{i}", 2 * b, 3, H >> i, W >> i)
                    if i:       # the level's warp and the flow's x2 up-sampling to the next level: one launch
                        u = self.buf(f"gf_{i - 1}", 2 * b, 2, H >> (i - 1), W >> (i - 1))
                        ops.flow_warp_up2(pyr_st[i], gf, nw, u)
                        gf = u
                    else:
                        ops.flow_warp(im0, gf[:b], nw[:b]); ops.flow_warp(im1, gf[b:], nw[b:])
                    pyr0[i], pyr1[i] = nw[:b], nw[b:]
            # local motion (:490) -> raw motion map goes straight into the decoder input
            cdec = 2 * C + S.MOTION_OUT
            dec_in = self.buf("dec_in", b, h, w, _r4(cdec))
            motion8 = dec_in[..., 2 * C:2 * C + 5]
            a, c, t = (ops.empty(b, 3, h, w) for _ in range(3))
            mlp_in, t2 = self._motion_branch(path, "local_motion_atmformer", "local_motion_mlp", x_tokens, b, h, w,
                                             self.local_motion_args["window_size"], "l")
            path.head1x1("local_motion_mlp.2", t2, b, h, w, motion8)
            ops.warp_blend(pyr0[3], pyr1[3], motion8, a, c, t)          # synthesis at H/8 (:496-506)
            # feature enhancement (:493-494)
            e_mid = self.buf("enh0", 2 * b * h * w, C)
            self._block(ops, path.P, "feat_enhance_transformer.0", self._stacked(mlp_in, 8, C), 2 * b, h, w, 8, 0, False, e_mid, None, "e")
            enh = self.buf("enh1", 2 * b, h, w, C)
            self._block(ops, path.P, "feat_enhance_transformer.1", e_mid, 2 * b, h, w, 8, 4, False, enh.reshape(2 * b * h * w, C), None, "e")
            # warped features (:496-506)
            w0_list.insert(0, a); w1_list.insert(0, c); it_list.insert(0, t)
            ops.flow_warp_nhwc(enh[:b], motion8[..., 0:2].permute(0, 3, 1, 2), dec_in[..., 0:C])
            ops.flow_warp_nhwc(enh[b:], motion8[..., 2:4].permute(0, 3, 1, 2), dec_in[..., C:2 * C])
            # decoder (:511-528): three stages, each followed by the synthesis at its scale; the finest one also writes the flows, the
            # masks and the refiner's 15 image channels
            x = path.decoder_input(dec_in[..., 0:cdec], b, H, W)
            for st, scale in enumerate((2, 1, 0)):
                x, mot = path.decoder_stage(st, x, b, H >> scale, W >> scale)
                if scale:
                    blend(pyr0[scale], pyr1[scale], mot)
            a, c, t = (ops.empty(b, 3, H, W) for _ in range(3))
            flow0, flow1 = ops.empty(b, 2, H, W), ops.empty(b, 2, H, W)
            m1, m2 = ops.empty(b, 1, H, W), ops.empty(b, 1, H, W)
            ops.warp_blend(pyr0[0], pyr1[0], mot, a, c, t, flow0, flow1, m1, m2, im0, im1, **path.blend_pack(b, H, W))
            w0_list.insert(0, a); w1_list.insert(0, c); it_list.insert(0, t)
            # residual refinement U-Net (:417-431); the reference adds the residual in place (network_base.py:532)
            it_list[0], it_final = path.refiner(b, H, W, it_list[0])
        return {"I_t": it_final, "im_t_list": it_list, "im0_warped_list": w0_list, "im1_warped_list": w1_list,
                "opt_flow_0": flow0, "opt_flow_1": flow1, "I_t_0": w0_list[0], "I_t_1": w1_list[0],
                "occ_mask1": m1, "occ_mask2": m2}


class NetworkBase(Network):
    VARIANT = "base"


class NetworkLite(Network):
    VARIANT = "lite"
