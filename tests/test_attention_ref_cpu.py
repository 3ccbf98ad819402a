"""CPU only: the float64 reference, the bounds and the input builders of tests/attention_ref.py have teeth.

* ``attention64`` agrees with torch's float64 softmax / matmul to 1e-12, whole and on a window subset;
* the (ws, hd) pairs of the GPU tests reach every tile count and head-dim class and are admissible for both engines, the refusal
  test's pairs are not;
* well-behaved fp32 arithmetic -- ``emulate32`` and ``emulate_x3``, torch fp32 restatements of the two kernels -- stays inside every
  bound with K = 1 .. K / 2 on EVERY input of tests/test_gpu_attention_fp64.py (the walk inputs at a 2-CU sizing: same family, same
  code), the model within half of the x3-vs-fp64 bound; the worst ratios are reported through record_property and fix K:

      MEASURED (worst emulation / bound with K = 1, over all inputs)            K = smallest power of two >= 2 x worst
        emulate32  / B32           1.53  (hot ws 9 / hd 72)                      4
        emulate32  / B32 motion    0.58  (hot ws 13 / hd 68)                     2
        emulate_x3 / Bx3           1.15  (hot ws 11 / hd 84; edge V 1.13)        4
        emulate_x3 / Bx3 motion    0.54  (hot ws 14 / hd 64)                     2
        emulate_x3 / Bx3-vs-fp64   0.27  (walk ws 8 / hd 72), motion 0.11        1     (model / the same bound: 0.08, motion 0.05)

* each mutant of the emulations leaves its bound by more than 2x on an input the GPU tests use (``MUTANT_INPUTS`` names it);
* ``one_hot`` gives V[pi(q)] bit for bit through ``emulate32``, float32(dequant(V[pi(q)])) through ``emulate_x3`` and the integer
  motion exactly, for every pair (the builder asserts the 110 lead from the float64 logits; no pair lacks a code set).
"""
import math

import pytest
import torch

import attention_ref as R
import f16x3_model as M

CPU_CUS = 2            # the walk inputs here are sized for a 2-CU device: the family and every code path of the builder, 1 / 100 the rows


def gpu_test_inputs():
    """(case, engines) of every input the GPU tests launch."""
    cases = []
    for ws, hd in R.PAIRS:
        cases += [(R.hot(ws, hd, "wide"), ("f32", "f16x3")), (R.hot(ws, hd, "edge"), ("f16x3",)), (R.uniform(ws, hd), ("f32", "f16x3"))]
    cases += [(R.walk(ws, hd, CPU_CUS), ("f32", "f16x3") if (ws, hd) == (8, 48) else ("f16x3",)) for ws, hd in R.WALK_PAIRS]
    return cases


_MODEL = {}


def model(case):
    if case.name not in _MODEL:
        _MODEL[case.name] = M.attention(case.qkv, *case.args)
    return _MODEL[case.name]


def ratios(case, engine, mutant=None, K=None):
    """Worst error / bound of an emulation on a case: {bound name: ratio}.  K: one value for every bound (default: the final ones)."""
    ref = R.reference(case)
    k = (lambda default: default if K is None else K)
    if engine == "f32":
        o, m = R.emulate32(case.qkv, *case.args, mutant=mutant)
        return {"B32": R.worst((o.double() - ref.out).abs(), R.bound32(ref, k(R.K32))),
                "B32_motion": R.worst((m.double() - ref.motion).abs(), R.bound32_motion(ref, k(R.K32_MOTION)))}
    y, mm, absr = model(case)
    o, m = R.emulate_x3(case.qkv, *case.args, mutant=mutant)
    out = {"Bx3": R.worst((o.double() - y).abs(), R.bound_x3(ref, absr, k(R.KX3))),
           "Bx3_motion": R.worst((m.double() - mm).abs(), R.bound_x3_motion(ref, k(R.KX3_MOTION)))}
    if case.name.startswith("walk"):
        out["Bx3_fp64"] = R.worst((o.double() - ref.out).abs(), R.bound_x3_fp64(ref, k(R.KX3_FP64)))
        out["Bx3_fp64_motion"] = R.worst((m.double() - ref.motion).abs(), R.bound_x3_fp64_motion(ref, k(R.KX3_FP64)))
        out["model_Bx3_fp64"] = R.worst((y - ref.out).abs(), R.bound_x3_fp64(ref, k(R.KX3_FP64)))
        out["model_Bx3_fp64_motion"] = R.worst((mm - ref.motion).abs(), R.bound_x3_fp64_motion(ref, k(R.KX3_FP64)))
    return out


# ------------------------------------------------------------------ the reference itself
def test_attention64_agrees_with_torch_float64():
    for case in (R.hot(5, 12, "wide"), R.walk(4, 16, CPU_CUS), R.hot(1, 32, "wide")):
        bw, n, heads, hd = case.bw, case.n, case.heads, case.hd
        t = case.qkv.double().reshape(bw, n, 3, heads, hd)
        src = (torch.arange(bw) + case.kv_shift) % bw
        q, k, v = t[:, :, 0].transpose(1, 2), t[src, :, 1].transpose(1, 2), t[src, :, 2].transpose(1, 2)
        s = (q @ k.transpose(-2, -1)) / math.sqrt(hd)
        if case.labels is not None:
            for b in range(bw):
                lab = case.labels[b % case.nw]
                s[b] -= 100.0 * (lab[:, None] != lab[None, :]).double()
        a = s.softmax(-1)
        want = (a @ v).transpose(1, 2).reshape(bw * n, -1)
        xy = R.key_xy(case.ws)
        want_m = torch.einsum("bhqk,qkc->bqhc", a, xy[None, :, :] - xy[:, None, :]).reshape(bw * n, heads, 2)
        ref = R.reference(case)
        assert float(((ref.out - want).abs() / ref.absr.clamp_min(1.0)).max()) <= 1e-12
        assert float((ref.motion - want_m).abs().max()) <= 1e-12 * 2 * case.ws
        assert bool((ref.absm >= 0).all()) and bool((ref.absr >= ref.out.abs() * (1 - 1e-12)).all())
        wins = [bw - 1, 0, bw // 2]                      # a subset, out of order: the rows of the whole
        sub = R.attention64(case.qkv, *case.args, windows=wins)
        rows = R.rows_of(wins, n)
        assert torch.equal(sub.out, ref.out[rows]) and torch.equal(sub.motion, ref.motion[rows]) and torch.equal(sub.R, ref.R[rows])
        y, m, absr = model(case)
        ys, ms, absrs = R.model_subset(case, wins)
        assert torch.equal(ys, y[rows]) and torch.equal(ms, m[rows]) and torch.equal(absrs, absr[rows])


# ------------------------------------------------------------------ what the GPU tests reach
def test_pairs_reach_every_instance_and_are_admissible():
    reachable = sorted({R.tiles(ws) for ws in range(1, 17)})
    assert reachable == [1, 2, 3, 4, 6, 7, 8, 9, 11, 13, 15, 16]
    assert sorted({R.tiles(ws) for ws, _ in R.PAIRS} | {R.tiles(ws) for ws, _ in R.WALK_PAIRS}) == reachable
    assert {R.dch(hd) for _, hd in R.PAIRS} == {1, 2, 3, 4}
    assert {hd % 16 for _, hd in R.PAIRS} == {0, 4, 8, 12}
    d3 = [(R.tiles(ws) <= 8) for ws, hd in R.PAIRS if R.dch(hd) == 3]
    assert True in d3 and False in d3, "DCH 3 both persistent and one item per workgroup"
    assert any(R.dch(hd) == 3 and R.tiles(ws) <= 8 for ws, hd in R.WALK_PAIRS) and any(R.tiles(ws) == 8 for ws, _ in R.WALK_PAIRS)
    for ws, hd in R.PAIRS + R.WALK_PAIRS:
        for engine in ("f32", "f16x3"):
            assert R.admissible(engine, ws, hd, True) and R.admissible(engine, ws, hd, False), (engine, ws, hd)
    # the refusal test's pairs
    assert not R.admissible("f32", 12, 128) and not R.admissible("f16x3", 12, 128) and not R.admissible("f16x3", 12, 128, False)
    assert not R.admissible("f32", 12, 116) and R.admissible("f32", 12, 112)
    assert not R.admissible("f16x3", 12, 112, True) and R.admissible("f16x3", 12, 112, False)
    assert not R.admissible("f32", 14, 68) and not R.admissible("f16x3", 14, 68) and R.admissible("f16x3", 13, 68)
    assert R.lds_bytes("f16x3", 12, 84, True) == 145984                  # "145 KiB at ws 12 / hd 84" (attention.hip): 145 984 bytes


def test_hot_inputs_have_a_masked_winner_and_reach_the_range():
    for ws, hd in R.PAIRS:
        for vfam in ("wide", "edge"):
            case = R.hot(ws, hd, vfam)                   # (the builder asserts both; restated here with the figures)
            ref = R.reference(case)
            assert ref.logit_absmax >= 59.9, case.name
            assert (case.labels is None) == (ws == 1)
            if ws > 1:
                assert case.labels.unique().numel() > 1 and ref.masked_wmax > 0.99, case.name


def test_walk_sizing():
    for cus in (2, 80, 256):
        for ws, hd in R.WALK_PAIRS:
            bw = R.walk_bw(ws, cus)
            vitems = (bw + 7) // 8 * 8 * R.HEADS
            assert bw % 8 and bw % 3 == 0 and vitems >= 2 * R.walk_grid_ceiling(ws, cus) + 8 * R.HEADS
            assert bw * ws * ws * 3 * R.HEADS * hd * 4 <= 256e6
            wins = R.walk_windows(bw)
            assert len(wins) >= min(64, bw) and (cus < 80 or len(wins) >= 64) and len(set(wins)) == len(wins) and {w % 8 for w in wins} == set(range(8)) and max(wins) == bw - 1
    case = R.walk(8, 72, CPU_CUS)
    assert case.kv_shift % 2 == 1 and 2 * case.kv_shift != case.bw and case.labels.shape == (3, 64)


# ------------------------------------------------------------------ the bounds hold for well-behaved fp32 arithmetic, and fix K
def test_emulations_stay_within_half_of_every_bound(record_property):
    worst = {}
    for case, engines in gpu_test_inputs():
        for engine in engines:
            for name, r in ratios(case, engine, K=1.0).items():
                if r > worst.get(name, (0.0, ""))[0]:
                    worst[name] = (r, case.name)
    for name, (r, where) in sorted(worst.items()):
        record_property(name, f"{r:.3f} at {where}")
        print(f"ATTN_CPU_RATIO {name} {r:.3f} {where}")
    final = {"B32": R.K32, "B32_motion": R.K32_MOTION, "Bx3": R.KX3, "Bx3_motion": R.KX3_MOTION, "Bx3_fp64": R.KX3_FP64,
             "Bx3_fp64_motion": R.KX3_FP64, "model_Bx3_fp64": R.KX3_FP64, "model_Bx3_fp64_motion": R.KX3_FP64}
    for name, (r, where) in worst.items():
        assert r <= final[name] / 2, f"{name}: {r:.3f} at {where} is beyond K / 2 = {final[name] / 2}"


# ------------------------------------------------------------------ mutants
MUTANT_INPUTS = {
    # mutant: (an input of test_every_tile_count, the bound it leaves, [an input of the walk test that also shows it])
    "mask_inf": (("hot", 5, 12), "out", None),                      # the planted masked winner loses all its weight
    "pad_keys_unmasked": (("hot", 1, 32), "out", (11, 32)),          # ws 1: 15 padded keys beside the only real one; ws 11: 7 of 128
    "labels_of_window_0": (("hot", 7, 36), "out", (8, 48)),
    "scale_of_padded_hd": (("hot", 13, 68), "out", (8, 72)),         # hd 68 / 72 scaled as 96
    "motion_q_of_tile": (("hot", 6, 20), "motion", (11, 32)),        # rows 16 .. 35 take the position of rows 0 .. 15
    "p_hi_only": (("hot", 9, 72), "out", (8, 72)),
    "v_lo_other_window": (("hot", 11, 84), "out", (8, 72)),          # on the walk: the stale-item symptom
}


@pytest.mark.parametrize("mutant", R.MUTANTS_X3)
def test_mutants_leave_the_bounds(mutant, record_property):
    (fam, ws, hd), which, walk = MUTANT_INPUTS[mutant]
    cases = [R.hot(ws, hd, "wide")] + ([] if walk is None else [R.walk(*walk, CPU_CUS)])
    for case in cases:
        for engine in ("f32", "f16x3") if mutant in R.MUTANTS32 else ("f16x3",):
            clean, bad = ratios(case, engine), ratios(case, engine, mutant)
            key = {"f32": "B32", "f16x3": "Bx3"}[engine] + ("_motion" if which == "motion" else "")
            record_property(f"{mutant}/{case.name}/{engine}", round(bad[key], 2))
            assert clean[key] <= 0.5 and bad[key] > 2.0, (mutant, case.name, engine, clean[key], bad[key])
    with pytest.raises(ValueError):
        R.emulate32(cases[0].qkv, *cases[0].args, mutant="p_hi_only")


# ------------------------------------------------------------------ one_hot is exact
def test_one_hot_is_exact_through_both_emulations():
    found = [p for p in R.PAIRS if R.one_hot_codes(p[0] ** 2, p[1]) is None]
    assert found == R.ONE_HOT_WITHOUT_CODES and R.ONE_HOT_PAIRS == [p for p in R.PAIRS if p not in found]
    for ws, hd in R.ONE_HOT_PAIRS:
        for labelled, vfam in ((False, "wide"), (False, "edge"), (True, "wide")):
            case = R.one_hot(ws, hd, labelled, vfam)     # (asserts the lead of 110 from the float64 logits, mask included)
            if labelled and case.labels is not None:
                lab = case.labels[torch.arange(case.bw) % case.nw]
                chosen = (case.expect_motion[:, 0].double().reshape(case.bw, case.n, 2) + R.key_xy(ws)) @ torch.tensor([1.0, ws]).double()
                assert torch.equal(torch.gather(lab, 1, chosen.long()), lab), "pi leaves the query's label class"
            if vfam == "wide":
                o, m = R.emulate32(case.qkv, *case.args)
                assert torch.equal(o, case.expect_out) and torch.equal(m, case.expect_motion), case.name
            o, m = R.emulate_x3(case.qkv, *case.args)
            assert torch.equal(o, M.dequant(case.expect_out).float()) and torch.equal(m, case.expect_motion), case.name
            assert bool((case.expect_motion == case.expect_motion.round()).all())
