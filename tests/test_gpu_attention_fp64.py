"""GPU: window attention (csrc/attention.hip) held to float64 on every reachable tile count, on closed forms and on the persistent
item walk, with the bounds derived in tests/attention_ref.py (K from CPU emulations, tests/test_attention_ref_cpu.py: never from a
kernel).

* test_every_tile_count      both engines at 14 (ws, hd) pairs: every NT in {1 2 3 4 6 7 8 9 11 13 15 16}, every DCH (DCH 3 both
                             persistent and not), all four hd mod 16 with a motion output, hot logits with a masked key that wins.
* test_closed_forms          Q = 0 (the mean over same-label keys) and exactly one-hot softmaxes: the output IS a row of V, the motion
                             an integer -- a misplaced key, V row or motion column shows as a wrong row, not as a tolerance.
* test_persistent_walk_many_items   vitems >= 2 x the largest grid the device can hold (asserted from its CU count), Bw % 8 != 0,
                             synthetic labels, odd kv_shift: has_next, the prefetch of the next item's K / V / Q rows, the per-item label
                             refresh, the padded tail of the item space and the barrier between items, at op level.
* test_refusals              what the entry point turns away, with the library's message and an untouched output.

Measured worst err / bound per case: DESIGN_NOTES.md, "fp64 bounds of window attention"."""
import importlib

import pytest
import torch

import attention_ref as R
import f16x3_model as M

pytestmark = pytest.mark.gpu

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
GUARD = 3          # rows before and behind each output that no launch may touch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


_MODEL = {}


def model(case):
    """f16x3_model.attention of a case, computed once and left unchanged."""
    if case.name not in _MODEL:
        _MODEL[case.name] = M.attention(case.qkv, *case.args)
    return _MODEL[case.name]


def launch(dev, engine, case, motion=True, planes=None, qkv_dev=None, fp32_rows=True):
    """One launch into NaN-filled outputs with guard rows; -> (out, motion) fp64 on the CPU (None where not asked for).  Every
    value written must be finite and nothing outside [Bw*N, C] / [Bw*N, heads, 2] may be touched."""
    hip = hip_ops.HipOps(dev)
    hip.attention_f16x3 = engine == "f16x3"
    rows = case.bw * case.n
    nan = float("nan")
    obuf = torch.full((rows + 2 * GUARD, case.c), nan, device=dev) if fp32_rows else None
    mbuf = torch.full((rows + 2 * GUARD, case.heads, 2), nan, device=dev) if motion else None
    out = None if obuf is None else obuf[GUARD:GUARD + rows]
    mot = None if mbuf is None else mbuf[GUARD:GUARD + rows]
    lab = None if case.labels is None else case.labels.to(dev)
    hip.window_attention(case.qkv.to(dev) if qkv_dev is None else qkv_dev, out, mot, lab, case.bw, case.nw, case.ws, case.heads, case.hd,
                         case.kv_shift, planes=planes)
    torch.cuda.synchronize()
    res = []
    for buf, what in ((obuf, "out"), (mbuf, "motion")):
        if buf is None:
            res.append(None)
            continue
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + rows:]).all()), f"{case.name} {engine}: {what} guard rows written"
        got = buf[GUARD:GUARD + rows].cpu().double()
        assert bool(torch.isfinite(got).all()), f"{case.name} {engine}: {what} has non-finite or unwritten elements"
        res.append(got)
    return res[0], res[1]


def hold(record_property, what, got, want, bound):
    w = R.worst((got - want).abs(), bound)
    record_property(what, round(w, 3))
    print(f"ATTN_RATIO {what} {w:.3f}")
    assert w <= 1.0, f"{what}: worst {w:.2f}x the bound"


# ------------------------------------------------------------------ 1. every tile count, every head-dim class
@pytest.mark.parametrize("engine,vfam", [("f32", "wide"), ("f16x3", "wide"), ("f16x3", "edge")], ids=["f32-wide", "f16x3-wide", "f16x3-edge"])
@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"ws{p[0]}_hd{p[1]}")
def test_every_tile_count(pair, engine, vfam, dev, record_property):
    """The exact-fp32 kernel against attention64 within B32, the f16x3 kernel against the model within Bx3 (out and motion), on the
    ``hot`` family: logits to +-60 and beyond, V over 2^-20 .. 2^8 (or at the fp16 boundaries of the split), two frames
    cross-attending, geometry labels of padded and shifted windows with a masked key that wins its softmax."""
    ws, hd = pair
    assert R.admissible("f32", ws, hd) and R.admissible("f16x3", ws, hd)
    case = R.hot(ws, hd, vfam)
    ref = R.reference(case)
    out, mot = launch(dev, engine, case)
    tag = f"{case.name}/{engine}"
    if engine == "f32":
        hold(record_property, f"{tag}/out", out, ref.out, R.bound32(ref))
        hold(record_property, f"{tag}/motion", mot, ref.motion, R.bound32_motion(ref))
    else:
        y, m, absr = model(case)
        hold(record_property, f"{tag}/out", out, y, R.bound_x3(ref, absr))
        hold(record_property, f"{tag}/motion", mot, m, R.bound_x3_motion(ref))


# ------------------------------------------------------------------ 2. closed forms
@pytest.mark.parametrize("engine", ["f32", "f16x3"])
@pytest.mark.parametrize("pair", R.ONE_HOT_PAIRS, ids=lambda p: f"ws{p[0]}_hd{p[1]}")
def test_closed_forms(pair, engine, dev, record_property):
    """uniform (Q = 0): the mean of V (of its f16x3 value for that engine) and of the key positions over the same-label keys, within
    the engine's bound with R = the mask terms.  one_hot: out is bit for bit V[pi(q)] (float32(dequant(V[pi(q)])) for f16x3, with V
    at the fp16 boundaries there) and motion bit for bit pi(q)_xy - q_xy, without labels and with pi inside the query's label class."""
    ws, hd = pair
    x3 = engine == "f16x3"
    case = R.uniform(ws, hd)
    ref = R.reference(case)
    want, want_m = R.uniform_closed_form(case, dequant=x3)
    out, mot = launch(dev, engine, case)
    tag = f"{case.name}/{engine}"
    hold(record_property, f"{tag}/out", out, want, R.bound_x3(ref, ref.absr) if x3 else R.bound32(ref))
    hold(record_property, f"{tag}/motion", mot, want_m, R.bound_x3_motion(ref) if x3 else R.bound32_motion(ref))
    for labelled in (False, True):
        case = R.one_hot(ws, hd, labelled, "edge" if x3 and not labelled else "wide")
        if labelled and case.labels is None:
            continue                                   # ws 1: one key, nothing to label
        out, mot = launch(dev, engine, case)
        want = M.dequant(case.expect_out).float().double() if x3 else case.expect_out.double()
        bad = (out != want).any(1)
        assert not bool(bad.any()), f"{case.name} {engine}: {int(bad.sum())} rows are not the chosen row of V, first {int(bad.nonzero()[0])}"
        bad = (mot != case.expect_motion.double()).reshape(mot.shape[0], -1).any(1)
        assert not bool(bad.any()), f"{case.name} {engine}: motion differs from pi(q)_xy - q_xy in {int(bad.sum())} rows"


# ------------------------------------------------------------------ 3. the persistent item walk
@pytest.mark.parametrize("pair", R.WALK_PAIRS, ids=lambda p: f"ws{p[0]}_hd{p[1]}")
def test_persistent_walk_many_items(pair, dev, record_property):
    """f16x3 engine with at least twice as many (window, head) items as the largest grid the device can hold (32 waves per CU, NT per
    workgroup), so every workgroup walks >= 2 items and the last round is ragged.  (a) >= 64 windows -- first, middle and last
    rounds of every residue b mod 8 -- against the model within Bx3; (b) EVERY element against attention64 within the x3-vs-fp64
    bound; (c) ws 8 / hd 48: the plane sink is bit for bit the split of the fp32 rows; (d) two launches are bit-identical; (e) ws 8 /
    hd 48: the exact-fp32 kernel on the same launch against attention64 within B32."""
    ws, hd = pair
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    case = R.walk(ws, hd, cus)
    vitems = (case.bw + 7) // 8 * 8 * case.heads
    assert vitems >= 2 * R.walk_grid_ceiling(ws, cus) + 8 * case.heads and case.bw % 8 and case.bw % case.nw == 0
    assert case.qkv.numel() * 4 <= 256e6
    record_property("vitems", vitems)
    record_property("grid_ceiling", R.walk_grid_ceiling(ws, cus))
    qkv_dev = case.qkv.to(dev)
    out, mot = launch(dev, "f16x3", case, qkv_dev=qkv_dev)
    tag = f"{case.name}/f16x3"
    ref = R.reference(case)
    hold(record_property, f"{tag}/out_vs_fp64", out, ref.out, R.bound_x3_fp64(ref))                      # (b)
    hold(record_property, f"{tag}/motion_vs_fp64", mot, ref.motion, R.bound_x3_fp64_motion(ref))
    wins = R.walk_windows(case.bw)                                                                         # (a)
    assert len(wins) >= min(64, case.bw)
    y, m, absr = R.model_subset(case, wins)
    sub = R.reference(case, wins)
    rows = R.rows_of(wins, case.n)
    hold(record_property, f"{tag}/out_vs_model", out[rows], y, R.bound_x3(sub, absr))
    hold(record_property, f"{tag}/motion_vs_model", mot[rows], m, R.bound_x3_motion(sub))
    out2, mot2 = launch(dev, "f16x3", case, qkv_dev=qkv_dev)                                               # (d)
    assert torch.equal(out, out2) and torch.equal(mot, mot2), "two launches differ"
    if pair == (8, 48):
        planes = hip_ops.Planes.alloc(case.bw * case.n, case.c, dev)                                      # (c)
        launch(dev, "f16x3", case, motion=False, planes=planes, qkv_dev=qkv_dev, fp32_rows=False)
        M.assert_split_of(planes, out.float(), "window attention plane sink on the item walk")
        o32, m32 = launch(dev, "f32", case, qkv_dev=qkv_dev)                                               # (e)
        hold(record_property, f"{case.name}/f32/out", o32, ref.out, R.bound32(ref))
        hold(record_property, f"{case.name}/f32/motion", m32, ref.motion, R.bound32_motion(ref))


# ------------------------------------------------------------------ 4. refusals
REFUSALS = [
    # id, ws, hd, Bw, nW, kv_shift, labels, message, engines
    ("hd68_at_13_tiles", 14, 68, 2, 1, 1, False, "head dim 68 too large for a 196-token window", ("f32", "f16x3")),
    ("ws17", 17, 8, 2, 1, 1, False, "window size 17 outside 1..16", ("f32", "f16x3")),
    ("hd6", 4, 6, 2, 1, 1, False, "head dim 6 must be a multiple of 4, at most 128", ("f32", "f16x3")),
    ("hd132", 4, 132, 2, 1, 1, False, "head dim 132 must be a multiple of 4, at most 128", ("f32", "f16x3")),
    ("lds_ws12_hd128", 12, 128, 2, 1, 1, False, "exceeds the 160 KiB LDS (ws 12, hd 128)", ("f32", "f16x3")),
    ("lds_f32_ws12_hd116", 12, 116, 2, 1, 1, False, "exceeds the 160 KiB LDS (ws 12, hd 116)", ("f32",)),
    ("lds_x3_ws12_hd112_motion", 12, 112, 2, 1, 1, False, "exceeds the 160 KiB LDS (ws 12, hd 112)", ("f16x3",)),
    ("kv_shift_is_bw", 4, 8, 4, 1, 4, False, "kv_shift out of range", ("f32", "f16x3")),
    ("bw_not_multiple_of_nw", 4, 8, 5, 2, 1, True, "Bw 5 must be a positive multiple of nW 2", ("f32", "f16x3")),
]


@pytest.mark.parametrize("case,engine", [(c, e) for c in REFUSALS for e in c[8]], ids=lambda v: v if isinstance(v, str) else v[0])
def test_refusals(case, engine, dev):
    """Each is turned away by the entry point before anything is launched: the wrapper's RuntimeError carries the library's message
    and the sentinel-filled outputs stay as they were.  (ws 12 / hd 112 is inadmissible for the f16x3 engine only WITH a motion
    output -- its four key-position columns open an eighth d-tile -- and ws 12 / hd 116 for both, listed under the fp32 engine.)"""
    name, ws, hd, bw, nw, kv_shift, labelled, msg, engines = case
    if name.startswith("lds"):
        assert R.lds_bytes(engine, ws, hd, True) > R.LDS_LIMIT and hd <= 128 and ws <= 16
    heads, n = 8, ws * ws
    c = heads * hd
    hip = hip_ops.HipOps(dev)
    hip.attention_f16x3 = engine == "f16x3"
    qkv = torch.zeros(bw * n, 3 * c, device=dev)
    out = torch.full((bw * n, c), 9.0, device=dev)
    mot = torch.full((bw * n, heads, 2), 9.0, device=dev)
    lab = torch.zeros(nw, n, dtype=torch.int32, device=dev) if labelled else None
    with pytest.raises(RuntimeError) as e:
        hip.window_attention(qkv, out, mot, lab, bw, nw, ws, heads, hd, kv_shift)
    assert msg in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and bool((mot == 9.0).all())
