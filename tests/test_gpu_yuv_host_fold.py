"""GPU: the YUV entry points on their one host path (csrc/yuv.hip surface_decode, csrc/yuv_encode.hip surface_encode; hip_ops.py
``_yuv_decode_args`` / ``_yuv_encode_args``).  ``atmvfi_yuv420_window`` is the one packed-planar call that no other identity holds to the surface
call: mode 0 against ``yuv_surface_decode`` of the tight planar surface, bit for bit, and mode 1 against ``yuv.window_numpy``, at the
smallest scalar (3 x 5, odd chroma edges) and vector (8 x 16) shapes with the frame at byte offsets 0 and 1.  Then the routing of
``yuv_decode`` / ``yuv_encode``: the entry points a launch plan records are the literal table below, and the plan replays."""
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
ROUTES = [      # descriptor, keep_depth -> the entry points yuv_decode / yuv_encode launch
    (yuv.Format(H, W), False, "atmvfi_yuv420_to_rgb", "atmvfi_rgb_to_yuv420"),
    (yuv.Format(H, W, depth=10), True, "atmvfi_yuv420p10_to_f32", "atmvfi_f32_to_yuv420p10"),
    (yuv.Surface.nv12(H, W), False, "atmvfi_yuv_surface_decode", "atmvfi_yuv_surface_encode"),
    (yuv.Surface.p010(H, W), True, "atmvfi_yuv_surface_decode", "atmvfi_yuv_surface_encode"),
    (yuv.Format(H, W, subsampling="422"), False, "atmvfi_yuv_sub_decode", "atmvfi_yuv_sub_encode"),
]


@pytest.mark.parametrize("route", ROUTES, ids=[f"{r[2][7:]}{'-keep' if r[1] else ''}" for r in ROUTES])
def test_yuv_decode_and_yuv_encode_route_to_the_entry_points_they_always_did(ops, dev, route):
    desc, keep, dec_name, enc_name = route
    frames = [to_dev(samples(desc, k), dev) for k in range(2)]
    canvases = [torch.full((3, H, W), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    outs = [torch.full((desc.frame_bytes,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]

    def both(buf, canvas, out):
        ops.yuv_decode(buf, desc, dst=canvas, keep_depth=keep)
        ops.yuv_encode(out, desc, src=canvas)
    plan = ops.begin_plan([frames[0], canvases[0], outs[0]])
    try:
        both(frames[0], canvases[0], outs[0])
        ids = [ops.lib.atmvfi_plan_fn_id(n.encode()) for n in (dec_name, enc_name)]
        assert min(ids) >= 0 and [fid for fid, _ in plan.ops_list] == ids and len(plan.patches) == 4
        plan = ops.end_plan(None)
    finally:
        ops.abort_plan()
    assert plan.run([frames[1], canvases[1], outs[1]], dev, ops._stream()) is None
    both(frames[1], canvases[0], outs[2])                                       # the direct launch of the same calls
    assert torch.equal(outs[1], outs[2]) and torch.equal(canvases[1], canvases[0]) and not torch.equal(outs[1], outs[0])


def test_the_routing_table_names_eight_different_entry_points(ops):
    names = {n for r in ROUTES for n in r[2:]}
    assert len(names) == 8 and len({ops.lib.atmvfi_plan_fn_id(n.encode()) for n in names}) == 8
