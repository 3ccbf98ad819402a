"""CPU: 4x / 8x recursive interpolation (atm-vfi_amd/multiframe.py, benchmark/davis-vid.py of the reference) without a GPU: the schedule,
the order of the loop, the video adapter on a fake codec, the reference chain against the oracle chain, the ABI's host-side checks
and the NumPy models of the three kernels."""
import ctypes
import importlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import multiframe_ref as M
from oracle import atmvfi_oracle as O

mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")

ORACLE_TOL = 2e-5     # tests/test_oracle_golden.py's bound for one forward; the chain needs no wider one (the reference damps its inputs)


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_nx_levels_produce_every_position_once_from_earlier_levels(n):
    levels = mf.nx_levels(n)
    assert levels[0] == [(0, n, n // 2)] and len(levels) == n.bit_length() - 1
    if n >= 4:
        assert levels[1] == [(0, n // 2, n // 4), (n // 2, n, 3 * n // 4)]
    known, made = {0, n}, []
    for l, level in enumerate(levels):
        assert len(level) == 1 << l
        for a, b, o in level:
            assert a in known and b in known and 2 * o == a + b
        for _, _, o in level:                   # a level's pairs are independent: its outputs become known only after it
            made.append(o)
        known |= {o for _, _, o in level}
    assert sorted(made) == list(range(1, n)) and len(set(made)) == n - 1
    assert {Fraction(o, n) for o in made} == {Fraction(k, n) for k in range(1, n)}


@pytest.mark.parametrize("n", [0, 1, 3, 6, -4, 2.0, True])
def test_nx_levels_rejects_other_factors(n):
    with pytest.raises(ValueError):
        mf.nx_levels(n)
    assert host_io.nx_levels is mf.nx_levels and host_io.interpolate_video_nx is mf.interpolate_video_nx


def mean_segment(n):
    """``segment`` from nx_levels with an arithmetic-mean midpoint (float64 frames)."""
    def segment(a, b):
        fr = {0: a, n: b}
        for level in mf.nx_levels(n):
            for x, y, o in level:
                fr[o] = (fr[x] + fr[y]) / 2
        return [fr[k] for k in range(1, n)]
    return segment


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("s,count", [(1, 5), (2, 7), (2, 6), (3, 7), (3, 9), (3, 4), (1, 2)])
def test_nx_sequence_order_values_and_dropped_frames(n, s, count):
    frames = [np.full((2, 3), float(i)) for i in range(count)]
    out = list(mf.nx_sequence(iter(frames), mean_segment(n), n, s))
    starts = list(range(0, count - s, s))
    assert len(out) == len(starts) * n + 1
    k = 0
    for i in starts:
        assert out[k] is frames[i]                                 # originals pass through untouched
        for j in range(n):
            assert np.array_equal(out[k + j], np.full((2, 3), i + j * s / n)), (i, j)
        k += n
    assert out[-1] is frames[starts[-1] + s]


def test_nx_sequence_short_inputs_and_bad_arguments():
    seg = mean_segment(4)
    assert list(mf.nx_sequence([], seg, 4)) == []
    assert list(mf.nx_sequence([np.zeros(1)], seg, 4)) == []
    assert list(mf.nx_sequence([np.zeros(1), np.ones(1)], seg, 4, 2)) == []       # no full segment
    with pytest.raises(ValueError):
        list(mf.nx_sequence([np.zeros(1)] * 3, seg, 3))
    with pytest.raises(ValueError):
        list(mf.nx_sequence([np.zeros(1)] * 3, seg, 4, 0))
    with pytest.raises(ValueError):
        list(mf.nx_sequence([np.zeros(1)] * 3, lambda a, b: [a], 4))               # a segment of the wrong length
    calls = []
    out = mf.nx_sequence(iter([np.zeros(1), np.ones(1), np.ones(1)]), lambda a, b: calls.append(1) or seg(a, b), 4)
    next(out)
    assert calls == [1]                                                             # the segment ran before its first frame came out
    assert mf.centre_window(480, 854, None) == (0, 0, 480, 854)
    assert mf.centre_window(120, 214, (96, 160)) == (12, 27, 96, 160)
    assert mf.centre_window(120, 214, (97, 161)) == (12, 27, 96, 160)               # the script's slice: H//2 - h//2 : H//2 + h//2
    with pytest.raises(ValueError):
        mf.centre_window(120, 214, (121, 10))


def test_video_nx_on_a_fake_codec():
    import pairs
    frames = pairs.uint8_video(7, 32, 48, seed=2)

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

    seen = {}

    def interp(frs, model, factor=4, time_interval=1, crop=None, **kw):
        seen.update(kw, factor=factor, time_interval=time_interval, crop=crop)
        y0, x0, h, w = mf.centre_window(32, 48, crop)

        def seg(a, b):
            return [((a.astype(np.float64) * (factor - k) + b.astype(np.float64) * k) / factor).astype(np.uint8)[y0:y0 + h, x0:x0 + w]
                    for k in range(1, factor)]
        for f in mf.nx_sequence(frs, seg, factor, time_interval):
            yield f if f.shape[:2] == (h, w) else f[y0:y0 + h, x0:x0 + w]
    mk = lambda sinks: (lambda fps, size: sinks.append(Sink(fps, size)) or sinks[-1])
    cap, sinks = Cap(frames), []
    info = host_io.video_nx(cap, mk(sinks), None, factor=4, interpolator=interp, tta=True)
    assert info == {"fps_in": 29, "fps_out": 116, "size": (48, 32), "frames_in": 7, "frames_out": 25}
    assert seen["tta"] is True and seen["factor"] == 4 and seen["time_interval"] == 1
    assert sinks[0].fps == 116 and sinks[0].size == (48, 32) and sinks[0].released == 1 and cap.released == 1
    for i, f in enumerate(frames):
        assert np.array_equal(sinks[0].got[4 * i], f)
    # time_interval 2, factor 8, a crop: rate 8 * 29 // 2, the crop's size, 3 segments
    cap, sinks = Cap(frames), []
    info = mf.video_nx(cap, mk(sinks), None, factor=8, interpolator=interp, time_interval=2, crop=(16, 24))
    assert info == {"fps_in": 29, "fps_out": 116, "size": (24, 16), "frames_in": 7, "frames_out": 25}
    assert all(f.shape == (16, 24, 3) for f in sinks[0].got)
    assert np.array_equal(sinks[0].got[8], frames[2][8:24, 12:36]) and np.array_equal(sinks[0].got[-1], frames[6][8:24, 12:36])
    # fps_out override (the script's hard-coded 10)
    cap, sinks = Cap(frames), []
    assert mf.video_nx(cap, mk(sinks), None, factor=4, fps_out=10, interpolator=interp)["fps_out"] == 10 and sinks[0].fps == 10
    # an empty video: nothing written, both ends released
    cap, sinks = Cap([]), []
    info = mf.video_nx(cap, mk(sinks), None, interpolator=interp)
    assert info["frames_in"] == 0 and info["frames_out"] == 0 and sinks[0].released == 1 and cap.released == 1
    # a frame of another size than announced: ValueError, both ends released all the same
    bad, sinks = Cap(frames[:3] + [np.zeros((16, 48, 3), np.uint8)]), []
    with pytest.raises(ValueError):
        mf.video_nx(bad, mk(sinks), None, interpolator=interp)
    assert bad.released == 1 and sinks[0].released == 1
    with pytest.raises(ValueError):
        mf.video_nx(Cap(frames), mk([]), None, factor=3, interpolator=interp)


@pytest.mark.parametrize("case", M.NX_CASES, ids=lambda c: c[0])
def test_reference_chain_is_the_oracle_chain(case, weights):
    name, v, h, w, g, depth, tta, seed, step = case
    gold = np.load(M.NX_REF)
    im0, im1 = M.case_inputs(case)
    s = gold[f"{name}.in_sums"]
    assert abs(im0.double().sum().item() - s[0]) < 1e-6 * abs(s[0]) and abs(im1.double().sum().item() - s[1]) < 1e-6 * abs(s[1])
    sd = weights(v)
    n = 1 << depth
    pred, shown = M.chain(lambda a, b: O.forward(sd, a, b, global_motion=g)["I_t"], im0, im1, n, tta=tta)
    assert sorted(pred) == list(range(1, n))
    for pos in range(1, n):
        d = float(np.abs(pred[pos][..., ::step, ::step].numpy() - gold[f"{name}.pred.{pos}"]).max())
        print(name, "pred", pos, f"{d:.2e}")
        assert d <= ORACLE_TOL, (pos, d)
        if tta:
            d = float(np.abs(shown[pos][..., ::step, ::step].numpy() - gold[f"{name}.tta.{pos}"]).max())
            print(name, "tta", pos, f"{d:.2e}")
            assert d <= ORACLE_TOL, (pos, d)
    assert os.path.getsize(M.NX_REF) < (1 << 20)


def test_multiframe_abi_is_declared_exported_and_checks_on_the_host():
    hdr = open(os.path.join(M.ROOT, "include", "atmvfi.h")).read()
    lib = hip_ops.load_library()
    lib.atmvfi_last_error.restype = ctypes.c_char_p
    for name in ("atmvfi_pool_blocks", "atmvfi_tta_merge", "atmvfi_frame_rot180"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in hip_ops.SIGNATURES and hasattr(lib, name)
        assert lib.atmvfi_plan_fn_id(name.encode()) >= 0
    assert (lib.atmvfi_version() >> 8) & 255 >= 12
    P = 0x10000       # never dereferenced: every call below fails its host-side checks before a launch
    err = lib.atmvfi_last_error

    def pool(pool=P, slot_bytes=1024, n_slots=4, slots=(0, 1), n=None, block=512, buf=P, to_pool=0):
        arr = (ctypes.c_int32 * max(1, len(slots)))(*slots) if slots is not None else None
        return lib.atmvfi_pool_blocks(pool, slot_bytes, n_slots, arr, len(slots) if n is None else n, block, buf, to_pool, None)
    assert pool(pool=None) == -1 and b"null pool or buffer" in err()
    assert pool(buf=None) == -1 and b"null pool or buffer" in err()
    assert pool(slots=None, n=2) == -1 and b"null slot list" in err()
    assert pool(n=0) == -1 and b"outside 1..32" in err()
    assert pool(slots=tuple(range(33)), n_slots=64) == -1 and b"outside 1..32" in err()
    assert pool(block=520) == -1 and b"multiple of 16" in err()                      # misaligned block_bytes
    assert pool(block=2048) == -1 and b"multiple of 16" in err()                     # larger than a slot
    assert pool(block=0) == -1
    assert pool(slot_bytes=1000) == -1 and b"bad pool geometry" in err()
    assert pool(slots=(0, 4)) == -1 and b"slot 4 (entry 1) outside 0..3" in err()
    assert pool(slots=(-1,)) == -1 and b"slot -1" in err()
    assert pool(pool=P + 4) == -1 and b"16-byte aligned" in err()
    assert pool(buf=P + 8) == -1 and b"16-byte aligned" in err()
    assert pool(slots=(2, 2), to_pool=1) == -1 and b"names slot 2 twice" in err()
    assert pool(slots=(40, 3, 40), n_slots=64, to_pool=1) == -1 and b"names slot 40 twice" in err()

    def merge(pred=P, flip=P, out=P, u8=P, hp=16, wp=24, pt=0, pl=0, h=16, w=24):
        return lib.atmvfi_tta_merge(pred, flip, out, u8, hp, wp, pt, pl, h, w, 0, None)
    assert merge(pred=None) == -1 and b"null prediction" in err()
    assert merge(flip=None) == -1 and b"null prediction" in err()
    assert merge(out=None, u8=None) == -1 and b"both outputs are null" in err()
    assert merge(hp=0) == -1 and b"bad canvas" in err()
    assert merge(pt=1) == -1 and b"bad geometry" in err()
    assert merge(w=25) == -1 and b"bad geometry" in err()
    assert merge(pl=-1) == -1 and b"bad geometry" in err()
    assert lib.atmvfi_frame_rot180(None, P, 3, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.atmvfi_frame_rot180(P, None, 3, 8, 8, None) == -1 and b"null pointer" in err()
    assert lib.atmvfi_frame_rot180(P, P, 3, 8, 8, None) == -1 and b"in place" in err()
    assert lib.atmvfi_frame_rot180(P, P + 64, 0, 8, 8, None) == -1 and b"bad shape" in err()


def test_numpy_models_are_the_torch_expressions():
    g = torch.Generator().manual_seed(5)
    pool = torch.rand(6, 5, 7, generator=g)
    idx = [4, 0, 4, 5]
    assert np.array_equal(M.pool_blocks_model(pool.numpy(), idx), torch.index_select(pool, 0, torch.tensor(idx)).reshape(4, -1).numpy())
    assert np.array_equal(M.pool_blocks_model(pool.numpy(), idx, block_elems=8), pool.reshape(6, -1)[idx, :8].numpy())
    buf = torch.rand(3, 5, 7, generator=g)
    want = pool.clone().index_copy_(0, torch.tensor([5, 1, 2]), buf)
    assert np.array_equal(M.pool_blocks_model(pool.numpy(), [5, 1, 2], buf.numpy()), want.numpy())
    with pytest.raises(ValueError):
        M.pool_blocks_model(pool.numpy(), [1, 1], buf.numpy()[:2])
    for hp, wp in ((16, 24), (7, 9)):
        a, b = torch.rand(1, 3, hp, wp, generator=g) * 1.2 - 0.1, torch.rand(1, 3, hp, wp, generator=g) * 1.2 - 0.1
        assert np.array_equal(M.rot180_model(a.numpy()), a.flip(2).flip(3).numpy())
        want = ((a + b.flip(2).flip(3)) / 2)[0]                                     # host_io.forward_tta / davis-vid.py:112
        for pt, pl, bgr in ((0, 0, False), (1, 3, True)):
            h, w = hp - pt - 1, wp - pl - 2
            out, u8 = M.tta_merge_model(a[0].numpy(), b[0].numpy(), pt, pl, h, w, bgr)
            assert np.array_equal(out, want.numpy())
            ref = np.round(want[:, pt:pt + h, pl:pl + w].numpy().transpose(1, 2, 0) * 255)       # davis-vid.py:114-116
            ref = np.clip(ref, 0, 255).astype(np.uint8)
            assert np.array_equal(u8, ref[:, :, ::-1] if bgr else ref)


def test_interpolate_video_nx_on_a_model_without_the_hip_backend():
    """Any model with ``forward(im0, im1) -> {"I_t"}`` runs the same schedule through torch ops (here: the pair mean on the CPU)."""
    class Mean(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, a, b):
            return {"I_t": (a + b) / 2}
    frames = [np.full((20, 36, 3), 32 * i, np.uint8) for i in range(5)]
    for f in frames:
        f[:, :, 0] += 3                                   # B != R: the colour flip must come back
    out = list(mf.interpolate_video_nx(iter(frames), Mean(), factor=4, time_interval=2, crop=(16, 32), divisor=64, tta=True))
    assert len(out) == 2 * 4 + 1 and all(f.shape == (16, 32, 3) and f.dtype == np.uint8 for f in out)
    for seg, i in enumerate((0, 2)):
        assert np.array_equal(out[4 * seg], frames[i][2:18, 2:34])
        for j in range(1, 4):
            assert np.array_equal(out[4 * seg + j], np.full((16, 32, 3), 32 * i + 16 * j, np.uint8) + np.array([3, 0, 0], np.uint8)), (seg, j)
    assert np.array_equal(out[-1], frames[4][2:18, 2:34])
    mids = mf.inference_nx(frames[0], frames[1], Mean(), factor=2, divisor=None)
    assert len(mids) == 1 and np.array_equal(mids[0], np.full((20, 36, 3), 16, np.uint8) + np.array([3, 0, 0], np.uint8))
