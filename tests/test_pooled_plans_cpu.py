"""hip_ops.LaunchPlan without a GPU (a fake library over CPU tensors, as tests/test_host_logic.py
``test_launch_plan_recorder_on_the_host``): host integer lists -- the slot list of ``atmvfi_pool_blocks`` -- are per-call arguments of a
plan.  They are recorded by the ADDRESS of their ctypes array under a role, kept alive, and rewritten from ``run(lists=)`` before
every replay (the one-op-at-a-time ``LaunchPlan.debug`` path included); plans take any number of inputs and may have no outputs."""
import ctypes
import importlib

import pytest
import torch

hip_ops = importlib.import_module("atm-vfi_amd.hip_ops")
P = hip_ops._ptr


class Fn:
    def __init__(self, name): self.__name__ = name


class Lib:
    """``atmvfi_plan_run`` that does what the real one does to the arguments (patch, then read every op) and records, per op, the
    values it finds at launch time behind every host list."""
    IDS = {b"atmvfi_pack_frames": 3, b"atmvfi_pool_blocks": 37}

    def __init__(self):
        self.seen = []          # per op issued: (fn, [patched argument values], the host list's values or None)

    def atmvfi_plan_fn_id(self, n): return self.IDS.get(n, -1)

    def atmvfi_last_error(self): return b""

    def atmvfi_plan_run(self, ops, n_ops, patches, n_patches, slots, n_slots, failed, stream):
        for i in range(n_patches):
            p = patches[i]
            ops[p.op].a[p.arg].u = (slots[p.slot] + p.offset) & 0xffffffffffffffff
        for i in range(n_ops):
            op = ops[i]
            vals = [op.a[j].u for j in range(op.nargs)]
            lst = None
            if op.fn == 37:     # (pool, slot_bytes, n_slots, slots*, n, block_bytes, buf, to_pool)
                lst = list((ctypes.c_int32 * op.a[4].i).from_address(op.a[3].u))
            self.seen.append((op.fn, vals, lst))
        return 0


def slot_list(values, role):
    arr = (ctypes.c_int32 * len(values))(*values)
    arr.role = role
    return arr


def pool_args(pool, arr, buf, to_pool=0):
    return (P(pool), pool[0].numel() * 4, pool.shape[0], arr, len(arr), pool[0].numel() * 4, P(buf), to_pool, None)


def three_inputs():
    return torch.zeros(6, 3, 4, 4), torch.zeros(6, 8, 4), torch.zeros(6, 2, 4)


def test_three_inputs_become_slots_with_patches_and_overlap_is_refused():
    frames, tl, tg = three_inputs()
    plan = hip_ops.LaunchPlan(Lib(), (frames, tl, tg))
    assert plan.n_inputs == 3 and [b for b, _ in plan.slots] == [frames.data_ptr(), tl.data_ptr(), tg.data_ptr()]
    assert plan.align == tuple(t.data_ptr() & 15 for t in (frames, tl, tg))
    work = torch.zeros(64)
    plan.add_op(Fn("atmvfi_pack_frames"), (P(frames, 192), P(tl), P(tg, 32), 1, 4, 4, None))
    plan.add_op(Fn("atmvfi_pack_frames"), (P(work), None, P(tg), 1, 4, 4, None))
    assert plan.patches == [(0, 0, 0, 192), (0, 1, 1, 0), (0, 2, 2, 32), (1, 2, 2, 0)]
    # the overlap refusal covers every pair of inputs, not the first two only
    flat = torch.zeros(200)
    a, b, c = flat[0:64], flat[100:164], flat[150:200]
    hip_ops.LaunchPlan(Lib(), (a, b, flat[164:200]))
    for bad in ((a, b, c), (c, a, b), (a, a, b)):
        with pytest.raises(hip_ops.PlanUnsupported):
            hip_ops.LaunchPlan(Lib(), bad)


def test_host_list_is_recorded_by_address_under_its_role():
    frames, tl, tg = three_inputs()
    plan = hip_ops.LaunchPlan(Lib(), (frames, tl, tg))
    buf = torch.zeros(2, 3, 4, 4)                   # workspace
    arr = slot_list([0, 1], "pairs")
    plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(frames, arr, buf))
    fid, vals = plan.ops_list[0]
    assert fid == 37 and vals[3] == ("u", ctypes.addressof(arr)) and vals[4] == ("u", 2)
    assert plan.lists == {"pairs": [arr]} and plan.lists["pairs"][0] is arr          # kept alive by the plan
    assert plan.patches == [(0, 0, 0, 0)]                                            # the pool is per-call, the buffer is workspace
    # a second list of the role must have the recorded length; another role is registered beside it
    arr2 = slot_list([4, 5], "pairs")
    plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(tl, arr2, torch.zeros(2, 8, 4)))
    plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(tg, slot_list([3], "stale"), torch.zeros(1, 2, 4), 1))
    assert sorted(plan.lists) == ["pairs", "stale"] and len(plan.lists["pairs"]) == 2
    with pytest.raises(hip_ops.PlanUnsupported):
        plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(frames, slot_list([1, 2, 3], "pairs"), torch.zeros(3, 3, 4, 4)))
    # no role, or not a ctypes int32 array: the plan cannot know what to rewrite
    with pytest.raises(hip_ops.PlanUnsupported):
        plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(frames, (ctypes.c_int32 * 2)(0, 1), buf))
    with pytest.raises(hip_ops.PlanUnsupported):
        plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(frames, slot_list([0, 1], None), buf))


def test_pool_blocks_without_a_role_is_refused_while_recording():
    frames, tl, tg = three_inputs()
    ops = object.__new__(hip_ops.HipOps)            # no library, no device: the refusal comes before anything is touched
    ops.recording = hip_ops.LaunchPlan(Lib(), (frames, tl, tg))
    with pytest.raises(hip_ops.PlanUnsupported, match="role"):
        ops.pool_blocks(frames, [0, 1], torch.zeros(2, 3, 4, 4))
    assert ops.recording.ops_list == []


@pytest.mark.parametrize("debug", [False, True], ids=["one_call", "debug_one_op_per_call"])
def test_run_rewrites_the_lists_and_returns_none_without_outputs(monkeypatch, debug):
    monkeypatch.setattr(hip_ops.LaunchPlan, "debug", debug)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)     # the debug path synchronises after every op
    lib = Lib()
    frames, tl, tg = three_inputs()
    plan = hip_ops.LaunchPlan(lib, (frames, tl, tg))
    g = torch.zeros(2, 3, 4, 4)
    toks = torch.zeros(1, 8, 4)
    plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(frames, slot_list([0, 0], "stale_padded"), g))
    plan.add_op(Fn("atmvfi_pack_frames"), (P(g), P(g, 192), P(toks), 1, 4, 4, None))
    plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(tl, slot_list([0], "stale"), toks, 1))
    plan.add_op(Fn("atmvfi_pool_blocks"), pool_args(tg, slot_list([0], "stale"), toks, 1))
    assert plan.finish(None) is plan and plan.out_meta == [] and plan.template is None
    # another pool of the same shape, other slots
    f2, l2, g2 = three_inputs()
    assert plan.run((f2, l2, g2), "cpu", None, lists={"stale_padded": [5, 5], "stale": (5,)}) is None
    assert [s[2] for s in lib.seen] == [[5, 5], None, [5], [5]]
    assert [s[1][0] for s in lib.seen if s[0] == 37] == [f2.data_ptr(), l2.data_ptr(), g2.data_ptr()]      # inputs patched
    assert lib.seen[0][1][6] == g.data_ptr()                                                               # workspace fixed
    del lib.seen[:]
    assert plan.run((frames, tl, tg), "cpu", None, lists={"stale_padded": [2, 3], "stale": [2]}) is None
    assert [s[2] for s in lib.seen] == [[2, 3], None, [2], [2]]
    # never a stale list: every role, each of its recorded length, or nothing is launched
    del lib.seen[:]
    for bad in (None, {}, {"stale": [1]}, {"stale_padded": [1, 2]}, {"stale_padded": [1, 2], "stale": [1, 2]},
                {"stale_padded": [1], "stale": [1]}, {"stale_padded": [1, 2], "stale": [1], "pairs": [0, 1]}):
        with pytest.raises(ValueError):
            plan.run((frames, tl, tg), "cpu", None, lists=bad)
    with pytest.raises(ValueError):
        plan.run((frames, tl), "cpu", None, lists={"stale_padded": [1, 2], "stale": [1]})
    assert lib.seen == [] and list(plan.lists["stale_padded"][0]) == [2, 3]


def test_a_plan_without_lists_runs_as_before_and_refuses_unknown_roles():
    lib = Lib()
    im0, im1 = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4)
    plan = hip_ops.LaunchPlan(lib, (im0, im1))
    out = torch.zeros(2, 4, 4, 4)
    plan.add_output(out)
    plan.add_op(Fn("atmvfi_pack_frames"), (P(im0), P(im1), P(out), 1, 4, 4, None))
    plan.finish({"x": out})
    a, b = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4)
    res = plan.run((a, b), "cpu", None)
    assert set(res) == {"x"} and res["x"].shape == out.shape and res["x"].data_ptr() != out.data_ptr()
    assert lib.seen[-1][1][:3] == [a.data_ptr(), b.data_ptr(), res["x"].data_ptr()]
    assert plan.run((a, b), "cpu", None, lists=None)["x"].shape == out.shape
    with pytest.raises(ValueError):                 # a role the plan never registered
        plan.run((a, b), "cpu", None, lists={"pairs": [0, 1]})
