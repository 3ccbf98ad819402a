"""CPU: host logic of the product without a GPU.

* ``Network.forward``'s orchestration (concat-free buffer slicing, window maps, quirk order)
  driven through the CPU *test double* of the op vocabulary (tests/cpu_ops.py) must
  reproduce the reference's golden outputs -- this isolates host bugs from kernel bugs;
* window row maps / labels against the oracle's pad/roll/partition;
* the C-ABI library exports every symbol ``include/atmvfi.h`` declares (no compute call);
* the product refuses to run without the HIP path.
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import golden_util as G
from cpu_ops import CpuOps
from oracle import atmvfi_oracle as O

pkg = importlib.import_module("atm-vfi_amd")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
windows = importlib.import_module("atm-vfi_amd.windows")
host_io = importlib.import_module("atm-vfi_amd.host_io")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nets():
    torch.set_grad_enabled(False)
    out = {}
    for v, cls in (("lite", pkg.NetworkLite), ("base", pkg.NetworkBase)):
        net = cls()
        net.load_state_dict(pkg.synthetic_state_dict(v, seed=1), strict=True)
        net.set_ops(CpuOps())
        out[v] = net
    return out


SMALL = [c for c in G.e2e_cases() if c["H"] * c["W"] * c["B"] <= 192 * 320]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c["name"])
def test_host_orchestration_vs_golden(case, nets):
    net = nets[case["variant"]]
    net.global_motion = case["global"]
    net.ensemble_global_motion = case["ensemble"]
    im0, im1 = G.case_inputs(case)
    out = net(im0, im1)
    for k in ("I_t", "opt_flow_0", "occ_mask1", "occ_mask2"):
        assert not torch.isnan(out[k]).any(), f"{k} has elements the host never produced"
    G.compare_e2e(out, G.load_npz(case["name"]), case["step"], 1e-4)
    assert len(out["im_t_list"]) == case["n_lists"] == len(out["im0_warped_list"]) == len(out["im1_warped_list"])
    assert torch.equal(out["occ_mask2"], 1 - out["occ_mask1"])
    # the reference leaves the refined, unclamped frame in im_t_list[0] (network_base.py:532)
    assert torch.equal(out["I_t"], out["im_t_list"][0].clamp(0, 1))


def test_ensemble_host_path(nets):
    case = [c for c in G.e2e_cases() if c["ensemble"]][0]
    net = nets[case["variant"]]
    net.global_motion, net.ensemble_global_motion = True, True
    im0, im1 = G.case_inputs(case)
    out = net(im0, im1)
    net.ensemble_global_motion = False
    G.compare_e2e(out, G.load_npz(case["name"]), case["step"], 1e-4)


@pytest.mark.parametrize("geo", [(2, 16, 24, 8, 0), (2, 16, 24, 8, 4), (2, 12, 20, 8, 4), (4, 4, 4, 12, 6),
                                 (2, 32, 32, 7, 3), (2, 17, 30, 12, 6), (2, 5, 6, 4, 0)])
def test_window_maps_match_pad_roll_partition(geo):
    frames, h, w, ws, shift = geo
    g = windows.build_window_geometry(frames, h, w, ws, shift)
    x = torch.arange(frames * h * w, dtype=torch.float32).reshape(frames, h, w, 1) + 1.0
    xw, og = O.to_windows(x, ws, shift)
    want = (xw.reshape(-1) - 1).long()              # zero padding -> -1
    assert torch.equal(g.row_map.long(), want)
    assert (og[0], og[1]) == (g.hp, g.wp)
    labels, *_ = O.window_labels(h, w, ws, shift)
    if labels is None:
        assert g.labels is None
    else:
        m_ref = labels[:, :, None] != labels[:, None, :]
        m_mine = g.labels[:, :, None] != g.labels[:, None, :]
        assert torch.equal(m_ref, m_mine)
    # scatter direction: every image token is written exactly once
    rm = g.row_map[g.row_map >= 0].long()
    assert torch.equal(torch.sort(rm).values, torch.arange(frames * h * w))


def test_state_dict_contract_and_api_surface(schema):
    for v, cls in (("base", pkg.NetworkBase), ("lite", pkg.NetworkLite)):
        net = cls()
        got = [(k, tuple(t.shape)) for k, t in net.state_dict().items()]
        assert got == schema.schema_signature(v)
        assert not any("attn_mask" in k or k.endswith("HW") for k, _ in got)
        assert net.pyramid_level == 4 and net.motion_out_dim == 5 and net.global_motion and not net.ensemble_global_motion
        for m in ("__set_local_window_size__", "__set_global_window_size__", "__freeze_global_motion__",
                  "__finetune_global_motion__", "__freeze_local_motion__", "__finetune_local_motion__"):
            assert callable(getattr(net, m))
        net.__freeze_global_motion__()
        assert not net.global_motion_mlp._modules["2"].weight.requires_grad and net.proj._modules["0"].weight.requires_grad
        net.__finetune_global_motion__()
        net.__set_global_window_size__(16)
        assert net.state_dict()["global_motion_atmformer.1.attn.relative_coord"].shape == (1, 1, 2, 256, 256)
        assert net.global_motion_args["window_size"] == 16
    torch.manual_seed(5)
    a = pkg.NetworkLite().state_dict()
    torch.manual_seed(5)
    b = pkg.NetworkLite().state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    rc = a["local_motion_atmformer.0.attn.relative_coord"]
    assert rc[0, 0, 0, 9, 20].item() == (20 % 8) - (9 % 8) and rc[0, 0, 1, 9, 20].item() == (20 // 8) - (9 // 8)


def test_product_fails_loudly_without_hip():
    net = pkg.NetworkLite()
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.rand(1, 3, 64, 64), torch.rand(1, 3, 64, 64))
    with pytest.raises(hip_ops.HipLibraryMissing):
        hip_ops.load_library("/nonexistent/libatmvfi_hip.so")
    # the product package never imports the oracle
    for fn in os.listdir(os.path.join(ROOT, "atm-vfi_amd")):
        if fn.endswith(".py"):
            src = open(os.path.join(ROOT, "atm-vfi_amd", fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), fn


def test_c_abi_exports_every_declared_symbol():
    """include/atmvfi.h <-> libatmvfi_hip.so <-> ctypes signatures agree (no compute call)."""
    header = open(os.path.join(ROOT, "include", "atmvfi.h")).read()
    declared = set(re.findall(r"\b(atmvfi_[a-z0-9_]+)\s*\(", header)) - {"atmvfi_blend"}
    assert declared == set(hip_ops.SIGNATURES), declared ^ set(hip_ops.SIGNATURES)
    if not os.path.exists(hip_ops.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(hip_ops.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/atmvfi.h but not exported"
    lib.atmvfi_version.restype = ctypes.c_int
    assert lib.atmvfi_version() >= 0x000100
    lib.atmvfi_packed_weight_floats.restype = ctypes.c_int64
    assert lib.atmvfi_packed_weight_floats(0, 101, 101, 3, 3) == 112 * 9 * 112
    assert lib.atmvfi_packed_weight_floats(2, 389, 773, 2, 2) == 1568 * 784
    # argument validation happens on the host before any launch: usable without a GPU
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    assert lib.atmvfi_layernorm(None, 4, 0, 0, None, None, 4, None, None, 1, 4, None) == -1
    assert b"null pointer" in lib.atmvfi_last_error()
    p = hip_ops.GemmParams(mode=7)
    assert lib.atmvfi_gemm(ctypes.byref(p), None) == -1


def test_input_padder_and_checkpoint_io(tmp_path, manifest):
    for key, pad in manifest["input_padder"].items():
        hw, dv = key.split("/")
        h, w = map(int, hw.split("x"))
        p = host_io.InputPadder((1, 3, h, w), divisor=int(dv))
        assert p._pad == pad
        x = torch.rand(1, 3, min(h, 40), min(w, 40))
        q = host_io.InputPadder(x.shape, divisor=16)
        a, b = q.pad(x, x)
        assert a.shape[-1] % 16 == 0 and a.shape[-2] % 16 == 0 and torch.equal(q.unpad(a), x)
    net = pkg.NetworkLite()
    sd = dict(net.state_dict())
    sd["local_motion_atmformer.1.attn_mask"] = torch.zeros(2)
    sd["local_motion_atmformer.1.HW"] = torch.zeros(1)
    path = tmp_path / "ck.pt"
    torch.save({"model_state_dict": sd, "optimizer_state_dict": {"o": 1}, "meta_data": {}, "train_metric": {}, "val_metric": {}}, path)
    net2 = pkg.NetworkLite()
    assert host_io.load_model_checkpoint(net2, str(path)) == {"o": 1}
    assert all(torch.equal(net2.state_dict()[k], net.state_dict()[k]) for k in net.state_dict())
    torch.save({k: v for k, v in net.state_dict().items()}, path)       # bare state dict (the reference crashes here)
    host_io.load_model_checkpoint(pkg.NetworkLite(), str(path))


def test_demo_host_path_on_double(nets):
    """inference_2frame: BGR flip, /255, replicate pad to /64, forward, unpad, round -> uint8."""
    import pairs
    case = [c for c in G.demo_cases() if c["name"] == "demo_base_100x180_nog"][0]
    net = nets["base"]
    net.global_motion = False
    f0, f1 = pairs.uint8_pair(case["H"], case["W"], seed=0)
    pred = host_io.inference_2frame(f0, f1, net, isBGR=True)
    gold = G.load_npz(case["name"])["pred"]
    d = np.abs(pred.astype(np.int32) - gold.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3


def test_video_adapters_on_a_fake_codec():
    """host_io.capture_frames / video_2x (demo_2x.py:129-168) without a GPU: an in-memory capture and writer, and a stand-in
    interpolator (the pair mean) in place of the HIP loop.  Checks the adapter's own contract: properties read through
    cap.get(CAP_PROP_*) and truncated like the reference's int(...), the sink opened at 2 x FPS with (W, H), frames copied out of the
    decoder's reused buffer, f0 I f1 I ... f_{n-1} order with the last frame once, both ends released -- also when a frame fails."""
    import pairs
    frames = pairs.uint8_video(4, 32, 48, seed=1)

    class Cap:
        def __init__(self, frs):
            self.frs, self.i, self.open, self.released = frs, 0, True, 0
            self.buf = np.zeros_like(frs[0]) if frs else None

        def get(self, prop):
            return {host_io.CAP_PROP_FPS: 29.97, host_io.CAP_PROP_FRAME_WIDTH: 48.0, host_io.CAP_PROP_FRAME_HEIGHT: 32.0,
                    host_io.CAP_PROP_FRAME_COUNT: float(len(self.frs))}[prop]

        def isOpened(self):
            return self.open

        def read(self):
            if self.i >= len(self.frs):
                return False, None
            self.i += 1
            if self.frs[self.i - 1].shape != self.buf.shape:
                return True, self.frs[self.i - 1]
            np.copyto(self.buf, self.frs[self.i - 1])
            return True, self.buf                       # ONE reused buffer, like OpenCV's decoder

        def release(self):
            self.open = False; self.released += 1

    class Sink:
        def __init__(self, fps, size):
            self.fps, self.size, self.got, self.released = fps, size, [], 0

        def write(self, f):
            self.got.append(f.copy())

        def release(self):
            self.released += 1

    def mean_interpolator(frs, model, isBGR=True, divisor=64, depth=3):
        prev = None
        for f in frs:
            if prev is not None:
                yield prev
                yield ((prev.astype(np.uint16) + f.astype(np.uint16)) // 2).astype(np.uint8)
            prev = f
        if prev is not None:
            yield prev
    assert [f.tolist() for f in host_io.capture_frames(Cap(frames))] == [f.tolist() for f in frames]
    cap, sinks = Cap(frames), []
    info = host_io.video_2x(cap, lambda fps, size: sinks.append(Sink(fps, size)) or sinks[-1], None, interpolator=mean_interpolator)
    assert info == {"fps_in": 29, "fps_out": 58, "size": (48, 32), "frames_in": 4, "frames_out": 7}
    assert sinks[0].fps == 58 and sinks[0].size == (48, 32) and sinks[0].released == 1 and cap.released == 1
    for i, f in enumerate(frames):
        assert np.array_equal(sinks[0].got[2 * i], f)
    assert np.array_equal(sinks[0].got[1], ((frames[0].astype(np.uint16) + frames[1]) // 2).astype(np.uint8))
    # an empty video: nothing written, both ends still released
    cap, sinks = Cap([]), []
    info = host_io.video_2x(cap, lambda fps, size: sinks.append(Sink(fps, size)) or sinks[-1], None, interpolator=mean_interpolator)
    assert info["frames_in"] == 0 and info["frames_out"] == 0 and sinks[0].released == 1 and cap.released == 1
    # a frame of another size than the capture announced: ValueError, and the ends are released all the same
    bad = Cap(frames[:2] + [np.zeros((16, 48, 3), np.uint8)])
    sinks = []
    with pytest.raises(ValueError):
        host_io.video_2x(bad, lambda fps, size: sinks.append(Sink(fps, size)) or sinks[-1], None, interpolator=mean_interpolator)
    assert bad.released == 1 and sinks[0].released == 1


def test_checkpoint_wire_format_and_tta_helpers(tmp_path, nets):
    """save_checkpoint writes the trainer's 5-key dict (trainer.py:438-446); forward_tta is the flip-average of
    benchmark/test_snufilm.py:135-139; psnr is benchmark/psnr_ssim.py:133-135."""
    net = pkg.NetworkLite()
    path = tmp_path / "wire.pt"
    host_io.save_checkpoint(net, str(path), meta={"epoch": 3}, val_metric={"psnr": 30.0})
    ck = torch.load(str(path), map_location="cpu")
    assert list(ck.keys()) == ["model_state_dict", "optimizer_state_dict", "meta_data", "train_metric", "val_metric"]
    assert ck["meta_data"] == {"epoch": 3} and list(ck["model_state_dict"].keys()) == list(net.state_dict().keys())
    net2 = pkg.NetworkLite()
    host_io.load_model_checkpoint(net2, str(path))
    assert all(torch.equal(net2.state_dict()[k], v) for k, v in net.state_dict().items())
    # TTA through the host-logic double: equals the explicit flip / un-flip average of two forwards
    m = nets["lite"]
    m.global_motion = False
    import pairs
    a, b = pairs.smooth_pair(1, 64, 64, seed=3)
    want = (m(a, b)["I_t"] + m(a.flip(2).flip(3), b.flip(2).flip(3))["I_t"].flip(2).flip(3)) / 2
    assert torch.equal(host_io.forward_tta(m, a, b), want)
    assert host_io.psnr(torch.zeros(4), torch.zeros(4)) == float("inf")
    assert abs(host_io.psnr(torch.zeros(100), torch.full((100,), 0.1)) - 20.0) < 1e-5      # 0.1 is a float32 here
    m.global_motion = True


def test_isa_of_counted_lds_waits():
    """The 3x3 kernel reads its MFMA fragments by inline asm under hand-counted s_waitcnt lgkmcnt(N): that is only sound while no
    scalar memory load (same counter, out-of-order return) sits inside a stage's MFMA stream and the stage drains to lgkmcnt(0).
    tools/check_isa.py compiles the kernel to gfx950 assembly and checks exactly that (hipcc cross-compiles without a GPU)."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_isa.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_product_library_reads_no_environment():
    """the C ABI keeps no global mutable state and takes every knob per call.  The product build must not even import
    getenv (the diagnostic `make stamp` / `make ablate` builds do), nor export a process-wide override."""
    import subprocess
    if not os.path.exists(hip_ops.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    und = subprocess.run(["nm", "-D", "--undefined-only", hip_ops.LIB_PATH], capture_output=True, text=True).stdout
    assert not re.search(r"\b(secure_)?getenv\b", und), "libatmvfi_hip.so imports getenv"
    defd = subprocess.run(["nm", "-D", "--defined-only", hip_ops.LIB_PATH], capture_output=True, text=True).stdout
    assert not re.search(r"atmvfi_\w*set_(schedule|tile_width)", defd)


def test_product_package_reads_no_environment_and_plans_are_the_only_selection():
    """the kernel selection (launch plans, the only one) is an attribute / constructor argument, not an
    ATMVFI_* environment variable -- no module of the package touches os.environ."""
    pkg_dir = os.path.join(ROOT, "atm-vfi_amd")
    for fn in sorted(os.listdir(pkg_dir)):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg_dir, fn)).read()
            assert "os.environ" not in src and "getenv" not in src, f"{fn} reads the environment"
    assert pkg.NetworkLite.SELECTIONS == ("use_plans",)
    net = pkg.NetworkLite(selections={"use_plans": False})
    assert net.use_plans is False and pkg.NetworkLite().use_plans is True
    assert all(hasattr(net, name) for name in net.SELECTIONS)
    # the A/B switches of earlier rounds are gone with their paths: naming one is an error, not a silent no-op
    for name in ("use_magic", "use_split_planes", "use_plane_deconvs", "use_plane_convs", "use_unet_planes", "use_fused_stem",
                 "use_fused_tail", "use_splitk", "use_lanes"):
        with pytest.raises(ValueError):
            pkg.NetworkLite(selections={name: True})
    assert pkg.NetworkBase(global_motion=False).global_motion is False       # the reference's positional / keyword arguments unchanged


def test_model_copies_and_pickles_without_runtime_state(nets):
    """copy.deepcopy / torch.save(module) of a model -- also one that has replicas (a lock, a link to its primary) and a workspace --
    carries parameters, buffers and settings, and none of the device-side runtime state."""
    import copy
    import io
    net = nets["lite"]
    G_case = [c for c in G.e2e_cases() if c["name"] == "lite_64x64_g"][0]
    im0, im1 = G.case_inputs(G_case)
    net.global_motion = True
    net.ensemble_global_motion = False
    net(im0, im1)                                            # (through the CPU test double: fills _bufs, _geo, _prepared)
    rep = net.replica()
    assert rep._primary is net and net._prepare_lock is not None and next(rep.parameters()) is next(net.parameters())
    assert list(rep.state_dict()) == list(net.state_dict()) and "_primary" not in rep._modules
    for obj in (net, rep):
        c = copy.deepcopy(obj)
        assert c._primary is None and c._prepare_lock is None and c._ops_obj is None and not c._bufs and not c._prepared and not c._plans
        assert all(torch.equal(a, b) and a is not b for a, b in zip(c.state_dict().values(), net.state_dict().values()))
        assert c.global_motion is True and c.local_motion_args == net.local_motion_args
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert type(back) is type(net) and all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), net.state_dict().values()))
    assert net._bufs and net._ops_obj is not None            # the original keeps its state


def test_tile_plan_and_tiled_stitching():
    """host_io.tile_plan / forward_tiled (the build-defined tiled mode of BASELINE configs[4]): cores partition the frame, every tile
    is its core grown by the overlap where it has a neighbour, and stitching a pixel-wise forward reproduces it exactly."""
    for (h, w, tile, ov) in ((2160, 4096, (1088, 2048), 64), (100, 150, (64, 64), 8), (37, 53, (16, 100), 5), (64, 64, (64, 64), 32)):
        plan = host_io.tile_plan(h, w, tile, ov)
        cover = np.zeros((h, w), np.int32)
        for (y0, y1, x0, x1, cy0, cy1, cx0, cx1) in plan:
            cover[cy0:cy1, cx0:cx1] += 1
            assert 0 <= y0 <= cy0 < cy1 <= y1 <= h and 0 <= x0 <= cx0 < cx1 <= x1 <= w
            assert cy1 - cy0 <= tile[0] and cx1 - cx0 <= tile[1]
            assert y0 == max(cy0 - ov, 0) and y1 == min(cy1 + ov, h) and x0 == max(cx0 - ov, 0) and x1 == min(cx1 + ov, w)
        assert (cover == 1).all()
        assert len(plan) == -(-h // tile[0]) * -(-w // tile[1])
    assert len(host_io.tile_plan(2160, 4096, (1088, 2048), 64)) == 4
    a, b = torch.rand(2, 3, 100, 150), torch.rand(2, 3, 100, 150)
    seen = []

    def mean(x, y):
        seen.append(tuple(x.shape[-2:]))
        return {"I_t": (x + y) / 2}
    out = host_io.forward_tiled(mean, a, b, tile=(64, 64), overlap=8, divisor=16)
    assert torch.equal(out, (a + b) / 2)
    assert len(seen) == 6 and all(hh % 16 == 0 and ww % 16 == 0 for hh, ww in seen)          # every tile padded to the divisor
    with pytest.raises(ValueError):
        host_io.forward_tiled(mean, a, b[:, :, :50], tile=(64, 64))


def test_reference_callers_import_lines_resolve():
    """The reference's own import lines, verbatim, in fresh interpreters: demo_2x.py:7-12 (cwd = repo root), README.md:31, and
    benchmark/test_*.py:12-16 (cwd = benchmark/, `sys.path.append('../')`).  They must resolve to this package's Network."""
    import subprocess
    import sys
    demo = ("import sys\n"
            "from benchmark.utils import InputPadder\n"
            "sys.path.append('./network/')\n"
            "from network_base import Network\n"
            "from network_lite import Network as NetworkLite\n"
            "from network.network_base import Network as ReadmeNetwork\n"
            "import torch\n"
            "m = Network(); assert isinstance(m, torch.nn.Module) and type(m).__module__.startswith('atm-vfi_amd'), type(m).__module__\n"
            "assert ReadmeNetwork is Network and NetworkLite is not Network\n"
            "assert InputPadder((1, 3, 270, 480), divisor=64)._pad == [16, 16, 25, 25]\n"
            "print(sum(p.numel() for p in m.parameters()))\n")
    r = subprocess.run([sys.executable, "-c", demo], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.split()[-1]) > 50_000_000           # network_base: 51.6 M parameters (README)
    bench = ("import sys\n"
             "sys.path.append('../')\n"
             "from network_base import Network\n"
             "from utils import InputPadder\n"
             "print(Network.__module__)\n")
    r = subprocess.run([sys.executable, "-c", bench], cwd=os.path.join(ROOT, "benchmark"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "atm-vfi_amd" in r.stdout, r.stdout + r.stderr[-2000:]


def test_golden_generator_imports_the_reference_not_the_shims(tmp_path):
    """oracle/gen_golden.py must import the reference's `network` / `benchmark` namespace packages although the repo ships regular
    packages of the same names (the round-1 recipe broke exactly there).  Run on a stand-in checkout with the reference's import
    layout (no __init__.py; network_base / network_lite import `flow_warp` and `network.attention`; demo_2x.py imports
    `benchmark.utils`, appends './network/' and imports network_base / network_lite), so that the test needs nothing outside the repo."""
    import subprocess
    import sys
    ref = tmp_path / "ref"
    (ref / "network").mkdir(parents=True)
    (ref / "benchmark").mkdir()
    head = "from flow_warp import flow_warp\nfrom network.attention import ATMFormer\nfrom network.attention import RefineBottleneck as SwinTransformer\n"
    files = {"network/attention.py": "class ATMFormer: pass\nclass RefineBottleneck: pass\n",
             "network/flow_warp.py": "def flow_warp(x, flow): return x\n",
             "network/network_base.py": head + "class Network: pass\n",
             "network/network_lite.py": head + "class Network: pass\n",
             "benchmark/utils.py": "class InputPadder: pass\n",
             "demo_2x.py": "import sys\nfrom benchmark.utils import InputPadder\nsys.path.append('./network/')\n"
                           "from network_base import Network as Network_base\nfrom network_lite import Network as Network_lite\n"}
    for name, text in files.items():
        (ref / name).write_text(text)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "gen_golden.py"), "--imports-only", "--reference", str(ref)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and os.path.join(str(ref), "network", "attention.py") in r.stdout, r.stdout + r.stderr[-2000:]


def test_workspace_cache_evicts_by_itself(nets):
    """Unchanged evaluation loops (benchmark/test_snufilm.py, test_xiph.py) feed one model many frame sizes and never release
    anything: the per-shape workspaces must stay bounded (LRU over shapes + a byte cap), and results must not depend on eviction."""
    import pairs
    net = nets["lite"]
    net.global_motion = True
    net.ensemble_global_motion = False
    net.release_workspace()
    shapes = [(64, 64), (64, 96), (96, 64), (64, 64)]
    first = None
    for i, (h, w) in enumerate(shapes):
        a, b = pairs.smooth_pair(1, h, w, seed=5)
        out = net(a, b)["I_t"].clone()
        assert len(net._workspaces) <= net.max_workspaces
        if i == 0:
            first = out
    assert torch.equal(out, first)                     # (64, 64) again after its workspace had been evicted
    keys = list(net._workspaces)
    assert keys[-1][1] == (1, 3, 64, 64) and keys[0][1] == (1, 3, 96, 64)
    cap, net.workspace_cap_bytes = net.workspace_cap_bytes, 1
    try:
        a, b = pairs.smooth_pair(1, 64, 96, seed=5)
        net(a, b)
        assert len(net._workspaces) == 1               # over the byte cap: only the workspace in use survives
    finally:
        net.workspace_cap_bytes = cap
        net.release_workspace()
    assert net.workspace_bytes() == 0


def _bench(*argv, env=None):
    import subprocess
    import sys
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=e, capture_output=True, text=True, timeout=300)


def test_bench_starts_its_own_ranks():
    """``python bench.py --gpus N`` outside a launcher (how the driver calls it) spawns the N ranks itself: fresh children through
    torch.distributed.run on 127.0.0.1 and a free port; exactly one JSON line on stdout (rank 0's), everything else on stderr."""
    import json
    r = _bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1
    assert "rank 1 of 2: rendezvous at 127.0.0.1:" in r.stderr and "torch.distributed.run" in r.stderr


def test_bench_launcher_with_eight_ranks():
    """The N = 8 form the driver's scaling run uses, rehearsed over gloo: eight fresh ranks rendezvous, the per-rank report (one
    all_gather_into_tensor of every rank's elapsed time) carries eight entries in rank order and the group's own world size."""
    import json
    r = _bench("--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run", env={"OMP_NUM_THREADS": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["collective_world_size"] == 8 and rec["per_rank_ms_per_step"] == [float(i) for i in range(8)]
    assert all(f"rank {i} of 8: rendezvous" in r.stderr for i in range(8))


def test_library_is_built_from_these_sources():
    """The shipped libatmvfi_hip.so carries the sha256 of the sources it was built from; it must be the shipped sources' (VERDICT
    round 3, weak 9a: nothing tied the prebuilt library to the tree)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import source_digest
    lib = hip_ops.load_library()
    assert lib.atmvfi_source_digest().decode() == source_digest.digest(), "rebuild: python -c 'import __graft_entry__ as g; g.build()'"
    assert not [f for f in os.listdir(os.path.join(ROOT, "atm-vfi_amd")) if f.endswith(".so") and f not in ("libatmvfi_hip.so", "libatmvfi_hip_checked.so")], \
        "diagnostic libraries belong in tools/lib/, not in the package"
    # the checked build (Network.set_precision("f16x3-checked")) is the same sources with one -D: same digest, same symbols, and it
    # says what it is; the default build refuses the range word (no kernel of it carries the check)
    chk = hip_ops.load_library(hip_ops.CHECKED_LIB_PATH)
    assert chk.atmvfi_source_digest().decode() == source_digest.digest()
    assert chk.atmvfi_range_checked() == 1 and lib.atmvfi_range_checked() == 0
    assert lib.atmvfi_range_word_set(None, None) == -1 and b"default build" in lib.atmvfi_last_error()


def test_bench_launcher_reports_a_failed_rank():
    r = _bench("--gpus", "2", "--dry-run", env={"ATMVFI_BENCH_DRY_FAIL_RANK": "1"})
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_stdout_is_one_json_line_whatever_native_code_prints():
    """Rank 0's stdout must be exactly one JSON line: RCCL writes a version banner to file descriptor 1 when its communicator starts
    (seen on the GPU box), so bench.py points descriptor 1 at stderr and prints through a saved copy.  Direct form and self-launch."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, ATMVFI_BENCH_DRY_NOISE="1")
    env.pop("WORLD_SIZE", None)
    for argv in (["--dry-run"], ["--dry-run", "--gpus", "2"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        assert json.loads(lines[0])["n_gpus"] == (2 if "--gpus" in argv else 1)
        assert "noise written to file descriptor 1" in r.stderr


def test_bench_single_rank_does_not_spawn_and_rejects_a_wrong_world():
    r = _bench("--gpus", "1", "--dry-run")
    assert r.returncode == 0 and "torch.distributed.run" not in r.stderr and r.stdout.count('"metric"') == 1
    r = _bench("--gpus", "4", "--dry-run", env={"WORLD_SIZE": "2", "RANK": "0"})     # launched with another rank count
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_bench_named_configs_are_baselines():
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    cfg = json.load(open(os.path.join(ROOT, "BASELINE.json")))["configs"]
    assert len(bench.CONFIGS) == len(cfg)
    for i, (k, (variant, h, w, g_on, _)) in enumerate(sorted(bench.CONFIGS.items())):
        text = cfg[i].replace("×", "x")
        assert f"network_{variant}" in text and f"{h}x{w}" in text
        assert ("global_off" in text) == (not g_on)


def test_bench_plain_run_leaves_the_extras_to_full(monkeypatch):
    """A plain ``bench.py`` run measures only the headline figure; --full brings back the instrumented pass, host I/O, the other
    configurations and the CPU baseline, each of which its --no-* option still leaves out."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.no_profile and a.no_host_io and a.no_configs and a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-host-io", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.no_host_io
    assert not (a.no_profile or a.no_configs or a.no_cpu_baseline)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_dump_outputs_stays_in_budget_and_samples_the_same_positions(tmp_path):
    """--dump-outputs: float32 .npy files, at most 64 MB in all; the headline frame whole, small arrays whole, larger ones a sample
    at positions that do not change from run to run."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    named = [("I_t", torch.rand(1, 3, 1088, 1920, generator=g))] + [(f"x{i}", torch.rand(1, 3, 1088, 1920, generator=g)) for i in range(4)]
    named.append(("small", torch.rand(2, 5, generator=g)))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), named)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n, _ in named)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 1000 * 1000
    for name, t in named:
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y)
        if name in ("I_t", "small"):
            assert np.array_equal(x, t.numpy())
        else:
            assert 0 < x.size < t.numel() and np.isin(x, t.numpy()).all()


def test_bench_dumps_what_the_timed_step_returns(nets, tmp_path):
    """bench.outputs_to_dump on a real forward's dict (the CPU test double) and on what sharding.PipelinedGather.drain() really hands
    out (a list of per-rank tensors, fp32 frames or uint8 wire frames): every entry is a tensor with a name of its own, list entries
    are numbered, and the gathered frames are written stacked in rank order."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    import pairs
    sharding = importlib.import_module("atm-vfi_amd.sharding")
    net = nets["lite"]
    net.global_motion, net.ensemble_global_motion = True, False
    a, b = pairs.smooth_pair(1, 64, 64, seed=5)
    out = net(a, b)
    names = [n for n, _ in bench.outputs_to_dump(out)]
    assert names[0] == "I_t" and "I_t_all_ranks" not in names and len(set(names)) == len(names)
    assert {"opt_flow_0", "opt_flow_1", "occ_mask1", "occ_mask2", "I_t_0", "I_t_1"} <= set(names)
    for key in ("im_t_list", "im0_warped_list", "im1_warped_list"):
        assert [n for n in names if n.startswith(key + "_")] == [f"{key}_{j}" for j in range(len(out[key]))]

    def u8(x):                                  # fp32 [1,3,H,W] -> uint8 [H,W,3], the --gather-u8 wire format
        return (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8)
    for shape, dtype, enc in (((1, 3, 64, 64), torch.float32, None), ((64, 64, 3), torch.uint8, u8)):
        g = sharding.PipelinedGather(1, shape, "cpu", dtype, encode=enc)
        g.submit(out["I_t"])
        gathered = g.drain()
        assert isinstance(gathered, list)
        named = bench.outputs_to_dump(out, gathered)
        assert [n for n, _ in named][:2] == ["I_t", "I_t_all_ranks"] and all(torch.is_tensor(t) for _, t in named)
        d = tmp_path / str(dtype).split(".")[-1]
        bench.dump_outputs(str(d), named)
        allr = np.load(d / "I_t_all_ranks.npy")
        want = out["I_t"] if enc is None else enc(out["I_t"])
        assert allr.dtype == np.float32 and allr.shape == (1,) + shape and np.array_equal(allr[0], want.float().numpy())
        assert np.array_equal(np.load(d / "I_t.npy"), out["I_t"].numpy())


def test_plan_dispatch_is_generated_from_the_header():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_plan_dispatch.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_plan_run_on_one_stream_patches_dispatches_and_reports_the_failing_op():
    """atmvfi_plan_run on the CPU box: no launch happens -- the ops below fail their entry point's host-side validation, which is
    exactly what a direct call reports -- but ids, argument counts, slot patching and the failing-op index are all exercised."""
    lib = hip_ops.load_library()
    fid = lib.atmvfi_plan_fn_id(b"atmvfi_pack_frames")
    assert fid >= 0 and lib.atmvfi_plan_fn_id(b"atmvfi_version") == -1 and lib.atmvfi_plan_fn_id(b"nope") == -1
    names = [n for n, (res, args) in hip_ops.SIGNATURES.items() if args and args[-1] is hip_ops.c_f and n != "atmvfi_plan_run"
             and res is hip_ops.c_i and not n.startswith(("atmvfi_packed", "atmvfi_split_weight", "atmvfi_conv3x3_weight"))]
    ids = sorted(lib.atmvfi_plan_fn_id(n.encode()) for n in names)
    assert ids == list(range(len(ids))), "every launch entry point of the binding has a plan id"

    ops = (hip_ops.PlanOp * 2)()
    # op 0: pack_frames(im0, im1, dst, B, H, W) with B = 0 -> EINVAL from the entry point itself
    ops[0].fn, ops[0].nargs = fid, 6
    for j, v in enumerate((0x1000, 0x2000, 0x3000, 0, 8, 8)):
        ops[0].a[j].u = v
    ops[1].fn, ops[1].nargs = fid, 6
    patches = (hip_ops.PlanPatch * 1)()
    patches[0].op, patches[0].arg, patches[0].slot, patches[0].offset = 0, 2, 1, 64
    slots = (ctypes.c_uint64 * 2)(0x10000, 0x20000)
    failed = ctypes.c_int(-5)
    rc = lib.atmvfi_plan_run(ops, 2, patches, 1, slots, 2, ctypes.byref(failed), None)
    assert rc != 0 and failed.value == 0 and lib.atmvfi_last_error()
    assert ops[0].a[2].u == 0x20000 + 64                     # patched in place before the ops run
    # wrong argument count / unknown id are reported with the op index; patches out of range never touch memory
    ops[0].nargs = 5
    assert lib.atmvfi_plan_run(ops, 2, None, 0, None, 0, ctypes.byref(failed), None) != 0 and failed.value == 0
    assert b"arguments" in lib.atmvfi_last_error()
    ops[0].fn = 999
    assert lib.atmvfi_plan_run(ops, 1, None, 0, None, 0, ctypes.byref(failed), None) != 0
    patches[0].slot = 7
    assert lib.atmvfi_plan_run(ops, 2, patches, 1, slots, 2, ctypes.byref(failed), None) != 0 and b"out of range" in lib.atmvfi_last_error()


def test_launch_plan_recorder_on_the_host():
    """hip_ops.LaunchPlan without a GPU: a fake library over real (CPU) tensors.  Pointer arguments are classified by the TENSOR they
    were derived from (hip_ops.TPtr), never by the allocation their raw value falls into: per-call tensors become patches (also when
    the two frames are slices of one stacked tensor), a workspace pointer stays fixed even where its biased value lies inside an
    output's bytes, a raw address inside per-call memory with no tensor is refused, overlapping frames are refused, parameter blocks
    are referenced by address and refused when an operand is per-call, results must be whole output slots."""
    class Fn:
        def __init__(self, name): self.__name__ = name

    class Lib:
        def atmvfi_plan_fn_id(self, n): return {b"atmvfi_pack_frames": 3, b"atmvfi_linear": 5, b"atmvfi_conv3p": 9}.get(n, -1)

    P = hip_ops._ptr
    stacked = torch.zeros(2, 3, 4, 4)                          # both frames are views of ONE storage
    im0, im1 = stacked[0:1], stacked[1:2]
    plan = hip_ops.LaunchPlan(Lib(), (im0, im1))
    assert plan.align == (im0.data_ptr() & 15, im1.data_ptr() & 15)
    out = torch.zeros(2, 4, 4, 4)
    work = torch.zeros(64)                                     # workspace: not a slot
    plan.add_output(out)
    plan.add_op(Fn("atmvfi_pack_frames"), (P(im0, 16), P(im1), P(out), 1, 4, 4, None))
    assert plan.patches == [(0, 0, 0, 16), (0, 1, 1, 0), (0, 2, 2, 0)]
    assert plan.ops_list[0][0] == 3 and [v for _, v in plan.ops_list[0][1]] == [im0.data_ptr() + 16, im1.data_ptr(), out.data_ptr(), 1, 4, 4]
    blk = hip_ops.GemmParams(out=work.data_ptr())
    blk._srcs = (work,)
    plan.add_op(Fn("atmvfi_linear"), (ctypes.byref(blk), None))
    assert plan.ops_list[1][1] == [("u", ctypes.addressof(blk))] and plan.keep == [blk]
    with pytest.raises(hip_ops.PlanUnsupported):               # a block field whose raw value lies in per-call memory
        plan.add_op(Fn("atmvfi_linear"), (ctypes.byref(hip_ops.GemmParams(out=out.data_ptr() + 8)), None))
    bad = hip_ops.GemmParams(out=work.data_ptr())
    bad._srcs = (out,)
    with pytest.raises(hip_ops.PlanUnsupported):               # ... or whose operand tensor is per-call
        plan.add_op(Fn("atmvfi_linear"), (ctypes.byref(bad), None))
    # the 3x3 plane kernel's block (atmvfi_conv3p) goes the same way: by address and kept alive when its operands are workspace ...
    cblk = hip_ops.Conv3pParams(in_hi=work.data_ptr(), in_lo=work.data_ptr(), out=work.data_ptr() + 16, out_cmin=4, terms=3)
    cblk._srcs = (work, None)
    n_ops = len(plan.ops_list)
    plan.add_op(Fn("atmvfi_conv3p"), (ctypes.byref(cblk), None))
    assert plan.ops_list[n_ops] == (9, [("u", ctypes.addressof(cblk))]) and plan.keep[-1] is cblk and len(plan.ops_list) == n_ops + 1
    # ... refused when an operand tensor is per-call, or when `out` (the first stored channel, inside its buffer) lies in an output slot
    cbad = hip_ops.Conv3pParams(in_hi=work.data_ptr(), in_lo=work.data_ptr(), out=work.data_ptr(), terms=3)
    cbad._srcs = (work, im1)
    with pytest.raises(hip_ops.PlanUnsupported):
        plan.add_op(Fn("atmvfi_conv3p"), (ctypes.byref(cbad), None))
    with pytest.raises(hip_ops.PlanUnsupported):
        plan.add_op(Fn("atmvfi_conv3p"), (ctypes.byref(hip_ops.Conv3pParams(in_hi=work.data_ptr(), out=out.data_ptr() + 16, out_cmin=4)), None))
    assert len(plan.ops_list) == n_ops + 1 and plan.keep[-1] is cblk
    with pytest.raises(hip_ops.PlanUnsupported):
        plan.add_op(Fn("atmvfi_version"), (None,))
    # the round-3 fault: a workspace pointer biased IN FRONT of its buffer (the compact view of the 3x3 plane kernel) whose raw value
    # lies inside an output tensor: fixed, because its tensor is workspace
    n0 = len(plan.patches)
    fake = hip_ops.TPtr(out.data_ptr() + 32)
    fake.src = work
    plan.add_op(Fn("atmvfi_pack_frames"), (fake, None, None, 1, 4, 4, None))
    assert len(plan.patches) == n0
    # ... and a per-call tensor's pointer in front of / past its own bytes is still that slot's pointer
    plan.add_op(Fn("atmvfi_pack_frames"), (P(out, -224), P(out, out.numel() * 4), None, 1, 4, 4, None))
    assert plan.patches[-2:] == [(len(plan.ops_list) - 1, 0, 2, -224), (len(plan.ops_list) - 1, 1, 2, out.numel() * 4)]
    # a raw integer inside per-call memory cannot be attributed: refused, not guessed
    with pytest.raises(hip_ops.PlanUnsupported):
        plan.add_op(Fn("atmvfi_pack_frames"), (ctypes.c_void_p(out.data_ptr() + 4), None, None, 1, 4, 4, None))
    plan.add_op(Fn("atmvfi_pack_frames"), (ctypes.c_void_p(work.data_ptr()), None, None, 1, 4, 4, None))      # outside: a fixed pointer
    # aliased / overlapping frames cannot be recorded at all
    x = torch.zeros(1, 3, 4, 4)
    for a, b in ((x, x), (stacked[0:2].reshape(-1)[0:60], stacked[0:2].reshape(-1)[40:96])):
        with pytest.raises(hip_ops.PlanUnsupported):
            hip_ops.LaunchPlan(Lib(), (a, b))


def test_parameter_replacement_and_data_swaps_are_noticed(nets):
    """Network._param_sig: a replaced Parameter OBJECT, a registered / deleted one, a ``p.data = ...`` swap and an
    in-place update all change the signature on the very next call, so packed weights, plans and graphs are re-derived; nothing
    changes it spuriously."""
    net = pkg.NetworkLite()
    net.load_state_dict(pkg.synthetic_state_dict("lite", seed=1), strict=True)
    sig0 = net._param_sig()
    assert net._param_sig() == sig0
    node = net.refine_head._modules["1"]._modules["0"]
    with torch.no_grad():
        node.bias.add_(0.5)
    sig1 = net._param_sig()
    assert sig1 != sig0 and net._param_sig() == sig1
    node.bias.data = node.bias.data.clone()                     # storage swapped behind the module's back
    sig2 = net._param_sig()
    assert sig2 != sig1
    old = node.weight
    node.weight = torch.nn.Parameter(old.detach().clone())     # a NEW Parameter object (pruning / re-parametrisation do this)
    sig3 = net._param_sig()
    assert sig3 != sig2 and net._plist is not None and any(p is node.weight for p in net._plist) and not any(p is old for p in net._plist)
    node.register_parameter("weight", torch.nn.Parameter(old.detach().clone()))
    assert net._param_sig() != sig3
    # end to end on the test double: the replaced weight reaches the forward
    net.set_ops(CpuOps())
    im0, im1 = torch.rand(1, 3, 64, 64), torch.rand(1, 3, 64, 64)
    y0 = net(im0, im1)["I_t"].clone()
    node.weight = torch.nn.Parameter(torch.zeros_like(old))
    node.bias = torch.nn.Parameter(torch.zeros_like(node.bias))
    y1 = net(im0, im1)["I_t"]
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, net(im0, im1)["im_t_list"][0].clamp(0, 1))
    # a whole sub-module swapped (parametrize / prune wrappers replace modules, not parameters): the cached list must
    # follow, by attribute assignment, add_module and deletion + re-registration alike
    import copy
    parent = net.refine_head._modules["1"]
    sig4 = net._param_sig()
    twin = copy.deepcopy(node)
    with torch.no_grad():
        twin.bias.fill_(0.25)
    parent._modules["0"] = node                                  # (same object: the dict write itself is not watched, nothing changed)
    assert net._param_sig() == sig4
    setattr(parent, "0", twin)
    sig5 = net._param_sig()
    assert sig5 != sig4 and any(p is twin.bias for p in net._plist) and not any(p is node.bias for p in net._plist)
    y2 = net(im0, im1)["I_t"]
    assert not torch.equal(y1, y2)
    parent.add_module("0", node)
    assert net._param_sig() != sig5 and any(p is node.bias for p in net._plist)
    assert torch.equal(net(im0, im1)["I_t"], y1)
