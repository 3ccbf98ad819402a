"""GPU: the YUV entry points on their one host path (csrc/yuv.hip atmvfi_yuv_decode, csrc/yuv_encode.hip atmvfi_yuv_encode on the frame
descriptor ``atmvfi_yuv_desc``; hip_ops.py ``_launch_yuv_decode`` / ``_launch_yuv_encode``).  ``yuv420_window`` is the one packed-planar
wrapper that no other identity holds to the surface wrapper: mode 0 against ``yuv_surface_decode`` of the tight planar surface, bit for
bit, and mode 1 against ``yuv.window_numpy``, at the smallest scalar (3 x 5, odd chroma edges) and vector (8 x 16) shapes with the frame at
byte offsets 0 and 1.  Then the routing of ``yuv_decode`` / ``yuv_encode``: every descriptor of the table below records the two entry
points with its cached descriptor block, and the plan replays.  Then the descriptor itself: a zero-filled block is the tight planar
frame, and mode 1 refuses every other layout."""
import ctypes
import dataclasses
import importlib
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
yuv = importlib.import_module("atm-vfi_amd.yuv")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    return hip_ops.HipOps(dev)


def samples(desc, seed):
    """One frame of ``desc`` with seeded samples over the whole range (an msb surface's in the upper ten bits)."""
    a = np.random.default_rng(seed).integers(0, 1 << desc.depth, desc.frame_samples).astype(desc.dtype)
    return (a << 6).astype(desc.dtype) if getattr(desc, "msb", False) else a


def to_dev(arr, dev, offset=0):
    """The bytes of ``arr`` on the device as a 1-D uint8 tensor whose pointer is ``offset`` bytes past an allocation's start."""
    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy())
    view = torch.empty(raw.numel() + offset, dtype=torch.uint8, device=dev)[offset:]
    view.copy_(raw)
    return view


def outputs(dev, which, h, w, hp, wp):
    """(dst, dst_u8), poisoned: an element that no lane writes compares unequal (NaN) or shows 0xA5."""
    dst = torch.full((3, hp, wp), float("nan"), dtype=torch.float32, device=dev) if which in ("both", "f32") else None
    d8 = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device=dev) if which in ("both", "u8") else None
    return dst, d8


# ------------------------------------------------------------------------------------------------ yuv420_window is the surface call
CROPS = [((8, 16), (2, 2, 5, 13)), ((8, 16), (0, 4, 8, 12)), ((3, 5), (2, 2, 1, 3))]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("depth", [8, 10])
def test_window_mode_0_is_the_surface_decode_of_the_tight_planar_surface(ops, dev, depth, offset):
    for ((H, W), win), siting in itertools.product(CROPS, ("centre", "left")):
        fmt = yuv.Format(H, W, "bt709", False, siting, depth)
        buf = to_dev(samples(fmt, 3 * H + depth), dev, offset)
        h, w = win[2:]
        for which, (hp, wp, top, left) in itertools.product(("both", "f32", "u8"), [(h, w, 0, 0), (h + 3, w + 4, 1, 4)]):
            a, a8 = outputs(dev, which, h, w, hp, wp)
            b, b8 = outputs(dev, which, h, w, hp, wp)
            ops.yuv420_window(buf, fmt, 0, *win, dst=a, dst_u8=a8, pad_top=top, pad_left=left)
            ops.yuv_surface_decode(buf, yuv.Surface(fmt), dst_u8=b8, dst=b, window=win, pad_top=top, pad_left=left)
            case = (H, W, win, siting, which, hp, wp)
            assert a is None or torch.equal(a, b), case
            assert a8 is None or torch.equal(a8, b8), case


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("depth", [8, 10])
def test_window_mode_1_keeps_its_geometry_on_the_shared_path(ops, dev, depth, offset):
    H, W = 8, 16
    for win, siting in itertools.product([(0, 0, 4, 8), (2, 2, 3, 5)], ("centre", "left")):        # 2h x 2w source pixels: vector, scalar
        fmt = yuv.Format(H, W, "bt601", False, siting, depth)
        frame = samples(fmt, 11 + depth)
        buf = to_dev(frame, dev, offset)
        want = yuv.window_numpy(frame, fmt, 1, *win)
        h, w = win[2:]
        for which in ("both", "f32", "u8"):
            dst, d8 = outputs(dev, which, h, w, h, w)
            ops.yuv420_window(buf, fmt, 1, *win, dst=dst, dst_u8=d8)
            assert d8 is None or np.array_equal(d8.cpu().numpy(), want), (win, siting, which)
            # q / 255 with the bits of the fp32 division (csrc/yuv_common.h q255)
            assert dst is None or np.array_equal(dst.cpu().numpy(), want.transpose(2, 0, 1).astype(np.float32) / np.float32(255)), (win, siting, which)


# ------------------------------------------------------------------------------------------------ routing
H, W = 8, 16
ROUTES = [      # descriptor, keep_depth: what yuv_decode / yuv_encode route by
    (yuv.Format(H, W), False),
    (yuv.Format(H, W, depth=10), True),
    (yuv.Surface.nv12(H, W), False),
    (yuv.Surface.p010(H, W), True),
    (yuv.Format(H, W, subsampling="422"), False),
]
NAMES = ("atmvfi_yuv_decode", "atmvfi_yuv_encode")
RETIRED = ("atmvfi_yuv420_to_rgb", "atmvfi_yuv420_window", "atmvfi_yuv420p10_to_f32", "atmvfi_yuv_surface_decode", "atmvfi_yuv_sub_decode",
           "atmvfi_rgb_to_yuv420", "atmvfi_f32_to_yuv420p10", "atmvfi_yuv_surface_encode", "atmvfi_yuv_sub_encode")


@pytest.mark.parametrize("route", ROUTES, ids=["planar", "planar10-keep", "nv12", "p010-keep", "422"])
def test_yuv_decode_and_yuv_encode_record_the_two_entry_points_with_the_cached_descriptor(ops, dev, route):
    desc, keep = route
    frames = [to_dev(samples(desc, k), dev) for k in range(2)]
    canvases = [torch.full((3, H, W), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    outs = [torch.full((desc.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]
    twin = dataclasses.replace(desc)                    # an equal descriptor, another object

    def both(buf, canvas, out, d=desc):
        ops.yuv_decode(buf, d, dst=canvas, keep_depth=keep)
        ops.yuv_encode(out, d, src=canvas)
    plan = ops.begin_plan([frames[0], canvases[0], outs[0]])
    try:
        both(frames[0], canvases[0], outs[0])
        ids = [ops.lib.atmvfi_plan_fn_id(n.encode()) for n in NAMES]
        assert min(ids) >= 0 and [fid for fid, _ in plan.ops_list] == ids and len(plan.patches) == 4
        # the descriptor travels by address: the block cached on the frozen descriptor, one per descriptor VALUE
        block = ("u", ctypes.addressof(desc.desc_block))
        assert [vals[0] for _, vals in plan.ops_list] == [block, block] and any(b is desc.desc_block for b in plan.keep)
        plan = ops.end_plan(None)
        again = ops.begin_plan([frames[0], canvases[0], outs[0]])              # two calls with equal descriptors record the same address
        both(frames[0], canvases[0], outs[0], twin)
        assert twin is not desc and [vals[0] for _, vals in again.ops_list] == [block, block]
    finally:
        ops.abort_plan()
    assert plan.run([frames[1], canvases[1], outs[1]], dev, ops._stream()) is None
    both(frames[1], canvases[0], outs[2])                                       # the direct launch of the same calls
    assert torch.equal(outs[1], outs[2]) and torch.equal(canvases[1], canvases[0]) and not torch.equal(outs[1], outs[0])


def test_the_nine_retired_names_have_no_plan_id_and_the_two_new_ones_differ(ops):
    assert len(set(RETIRED)) == 9 and all(ops.lib.atmvfi_plan_fn_id(n.encode()) < 0 for n in RETIRED)
    assert all(n not in hip_ops.SIGNATURES and not hasattr(ops.lib, n) for n in RETIRED)
    ids = [ops.lib.atmvfi_plan_fn_id(n.encode()) for n in NAMES]
    assert min(ids) >= 0 and ids[0] != ids[1]


# ------------------------------------------------------------------------------------------------ the descriptor
def lib_decode(ops, block, buf, h, w, dst, d8, keep=0, mode=0):
    return ops.lib.atmvfi_yuv_decode(ctypes.byref(block), hip_ops._ptr(buf), keep, mode, 0, 0, h, w, hip_ops._ptr(d8), 0, hip_ops._ptr(dst), h, w, 0, 0,
                                     ops._stream())


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("size", [(3, 5), (8, 16)])
@pytest.mark.parametrize("depth", [8, 10])
def test_a_zero_filled_descriptor_is_the_tight_planar_surface(ops, dev, depth, size, offset):
    """Only H, W, depth and matrix set: the decode and the encode of the explicit tight planar ``Surface`` of the same frame, bit for bit."""
    h, w = size
    surface = yuv.Surface(yuv.Format(h, w, "bt709", False, "centre", depth))
    assert surface.is_tight and surface.desc_block.pitch == w * surface.itemsize          # explicit strides on that side
    block = hip_ops.YuvDesc(H=h, W=w, depth=depth, matrix=1)
    buf = to_dev(samples(surface, 5 * h + depth), dev, offset)
    for keep in ([0, 1] if depth == 10 else [0]):
        a, a8 = outputs(dev, "f32" if keep else "both", h, w, h, w)
        b, b8 = outputs(dev, "f32" if keep else "both", h, w, h, w)
        assert lib_decode(ops, block, buf, h, w, a, a8, keep) == 0, ops.lib.atmvfi_last_error()
        ops.yuv_surface_decode(buf, surface, dst_u8=b8, dst=b, keep_depth=bool(keep))
        assert torch.equal(a, b) and (a8 is None or torch.equal(a8, b8)), keep
    src = torch.rand(3, h, w, device=dev)
    out = [torch.full((surface.nbytes + offset,), 0xA5, dtype=torch.uint8, device=dev)[offset:] for _ in range(2)]
    assert ops.lib.atmvfi_yuv_encode(ctypes.byref(block), None, 0, hip_ops._ptr(src), h, w, 0, 0, hip_ops._ptr(out[0]), ops._stream()) == 0
    ops.yuv_surface_encode(out[1], surface, src=src)
    assert torch.equal(out[0], out[1]) and not bool((out[0] == 0xA5).all())


@pytest.mark.parametrize("wrong", [dict(chroma=1), dict(chroma=2), dict(depth=10, msb=1), dict(pitch=16), dict(chroma_pitch=8), dict(chroma_offset=128),
                                   dict(subsampling=1), dict(subsampling=2)], ids=lambda d: "-".join(d))
def test_mode_1_refuses_every_layout_but_the_packed_planar_frame(ops, dev, wrong):
    """mode 1 through atmvfi_yuv_decode with a non-zero chroma, msb, stride or subsampling: the mode-1 message, before any launch (the
    strides given are the tight frame's own values: nothing else about the call is wrong)."""
    block = hip_ops.YuvDesc(**{**dict(H=8, W=16, depth=8, matrix=0), **wrong})
    buf = torch.zeros(8 * 16 * 3 * 2, dtype=torch.uint8, device=dev)
    dst, d8 = outputs(dev, "both", 4, 8, 4, 8)
    assert lib_decode(ops, block, buf, 4, 8, dst, d8, mode=1) == -1
    assert ops.lib.atmvfi_last_error() == b"yuv_decode: mode 1 reads packed planar 4:2:0 frames with LSB samples, to pixels 0..255"
    assert bool(torch.isnan(dst).all()) and bool((d8 == 0xA5).all())            # nothing ran
    assert lib_decode(ops, hip_ops.YuvDesc(H=8, W=16, depth=10, matrix=0), buf, 4, 8, dst, None, keep=1, mode=1) == -1       # keep_depth too
    assert b"mode 1 reads packed planar" in ops.lib.atmvfi_last_error()
