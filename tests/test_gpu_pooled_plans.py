"""GPU: ``Network.forward_pooled`` on launch plans (atm-vfi_amd/network.py, hip_ops.LaunchPlan): a frame-stage plan and a pair-stage
plan per key, the pool's tensors as per-call inputs, the slot lists as per-call host lists.  A planned pooled forward issues the
launches of the direct path with the same arguments, so everything here is BIT-equality: with ``forward`` on the same batch (all ten
outputs, ``Network._same_results``), with a model whose plans are off (tokens left in the pool, frames of the video loops), and
``Network.plan_stats()`` says which path a call took.  Shapes: 64x96 (network_lite and network_base, global branch on and off), once
128x192; the loops on 80x112 padded to 96x128."""
import importlib

import numpy as np
import pytest
import torch

import cpu_framediff as D
import pairs

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("atm-vfi_amd")
mf = importlib.import_module("atm-vfi_amd.multiframe")
host_io = importlib.import_module("atm-vfi_amd.host_io")
scene = importlib.import_module("atm-vfi_amd.scene")
rt = importlib.import_module("atm-vfi_amd.retime")
yuv = importlib.import_module("atm-vfi_amd.yuv")
Network = pkg.Network
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_net(variant, dev, **kw):
    net = (pkg.NetworkLite if variant == "lite" else pkg.NetworkBase)(**kw)
    net.load_state_dict(pkg.synthetic_state_dict(variant, seed=1), strict=True)
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def nets(dev):
    torch.set_grad_enabled(False)
    return {v: make_net(v, dev) for v in ("lite", "base")}


@pytest.fixture(scope="module")
def eager_lite(dev):
    torch.set_grad_enabled(False)
    return make_net("lite", dev, selections={"use_plans": False})


def fresh(net, glob=True):
    """The module's net with no plan, no workspace and zero counts: every test starts its keys at the first call."""
    net.global_motion, net.ensemble_global_motion = glob, False
    net.max_workspaces = 2
    net.release_workspace()
    net.enable_plans(True)
    return net


def n_frames(n, h, w, dev, seed=60):
    fr = []
    for k in range((n + 1) // 2):
        a, b = pairs.smooth_pair(1, h, w, seed + k)
        fr += [a[0], b[0]]
    return torch.stack(fr[:n], 0).to(dev)


def same(x, y, what):
    assert set(x) == set(y) and len(x) == 10
    for k in x:
        assert Network._same_results(x[k], y[k]), f"{what}: {k} differs"


def plain(net, frames, left, right):
    return net(frames[left].contiguous(), frames[right].contiguous())


def poisoned_pool(net, frames, h, w, slots, named):
    """A pool whose slots outside ``named`` hold NaN frames and NaN tokens."""
    pool = mf.FramePool(net, h, w, slots)
    refill(pool, frames, named)
    return pool


def refill(pool, frames, named):
    pool.frames.fill_(NAN); pool.tokens_l.fill_(NAN); pool.tokens_g.fill_(NAN)
    for s in range(pool.slots):
        pool.invalidate(s)
    for s in named:
        pool.put(s, frames[s])


# the recording call (the third) names other slots than the replays after it
SEQUENCES = {
    1: [([0], [1])] * 3 + [([3], [5]), ([5], [2]), ([0], [1])],
    2: [([0, 3], [3, 1])] * 3 + [([4, 2], [2, 5]), ([5, 0], [0, 1]), ([1, 4], [4, 2])],
    4: [([0, 1, 2, 3], [1, 2, 3, 4])] * 3 + [([5, 4, 3, 2], [4, 3, 2, 1]), ([2, 0, 5, 1], [0, 5, 1, 3])],
}


# ------------------------------------------------------------------------------------------------ 1. the slot lists are data
SLOT_CASES = [(v, g, 64, 96, b) for v in ("lite", "base") for g in (True, False) for b in (1, 2, 4)] + [("base", True, 128, 192, 2)]


@pytest.mark.parametrize("variant,glob,h,w,b", SLOT_CASES, ids=lambda v: str(v))
def test_slot_lists_are_data_not_part_of_the_plan(nets, dev, variant, glob, h, w, b):
    net = fresh(nets[variant], glob)
    frames = n_frames(6, h, w, dev)
    pool = mf.FramePool(net, h, w, 6)
    refs = {}
    seq = SEQUENCES[b]
    for i, (left, right) in enumerate(seq):
        key = (tuple(left), tuple(right))
        if key not in refs:
            refs[key] = plain(net, frames, left, right)
        refill(pool, frames, set(left + right))                   # every other slot: NaN frames, NaN tokens
        out = net.forward_pooled(pool, left, right)
        same(refs[key], out, f"{variant} glob={glob} B={b} call {i} slots {left}|{right}")
    st = net.plan_stats()
    assert st["pooled_pair"] == {"eager": 2, "recorded": 1, "replayed": len(seq) - 3, "refused": 0}, st
    # every call had stale slots; the calls that name as many distinct slots as the first share its frame-stage key
    alike = sum(len(set(l + r)) == len(set(seq[0][0] + seq[0][1])) for l, r in seq)
    assert st["pooled_frame"]["refused"] == 0 and st["pooled_frame"]["recorded"] >= 1 and st["pooled_frame"]["replayed"] >= alike - 3, st
    assert sum(st["pooled_frame"].values()) == len(seq)
    torch.cuda.synchronize()
    pool.release()


# ------------------------------------------------------------------------------------------------ 2. stale counts
@pytest.mark.parametrize("variant,glob", [("lite", True), ("base", False)])
def test_stale_counts_and_the_tokens_a_replayed_frame_plan_writes(nets, dev, variant, glob):
    h, w, (left, right) = 64, 96, ([0, 3], [3, 1])
    used = [0, 3, 1]
    net = fresh(nets[variant], glob)
    twin = make_net(variant, dev, selections={"use_plans": False})      # the same sequence on direct launches
    twin.global_motion = glob
    frames = n_frames(6, h, w, dev)
    pools = {id(m): poisoned_pool(m, frames, h, w, 6, used) for m in (net, twin)}
    alt = [frames[1].clone(), frames[4].flip(2).contiguous(), frames[5].flip(1).contiguous()]
    refs = {}

    def step(what, state, f):
        """One call on both models; ``state``: which frame slot 1 holds now; ``f``: the stale slots it must find."""
        before = net.plan_stats()
        outs = [m.forward_pooled(pools[id(m)], left, right) for m in (net, twin)]
        after = net.plan_stats()
        assert sum(after["pooled_frame"].values()) - sum(before["pooled_frame"].values()) == (1 if f else 0), (what, before, after)
        if state not in refs:
            cur = frames.clone()
            cur[1] = alt[state]
            refs[state] = plain(net, cur, left, right)
        same(refs[state], outs[0], f"{variant} {what}: planned")
        same(refs[state], outs[1], f"{variant} {what}: direct")
        a, b = pools[id(net)], pools[id(twin)]
        for tok in ("tokens_l",) + (("tokens_g",) if glob else ()):
            assert torch.equal(getattr(a, tok)[used], getattr(b, tok)[used]), f"{variant} {what}: {tok} of the planned and the direct pool differ"
        return after
    for rnd in range(3):
        for p in pools.values():
            for s in used:
                p.invalidate(s)
        step(f"round {rnd} all stale", rnd % 3 if rnd else 0, 3)
        step(f"round {rnd} none stale", rnd % 3 if rnd else 0, 0)
        for p in pools.values():
            p.invalidate(left[0])
        step(f"round {rnd} one stale", rnd % 3 if rnd else 0, 1)
        for p in pools.values():
            p.put(1, alt[(rnd + 1) % 3])
        st = step(f"round {rnd} one stale after put", (rnd + 1) % 3, 1)
    # f = 1 ran six times under one key: 2 direct, 1 recorded, 3 replayed; f = 3 three times: 2 direct, 1 recorded
    assert st["pooled_frame"] == {"eager": 4, "recorded": 2, "replayed": 3, "refused": 0}, st
    assert st["pooled_pair"] == {"eager": 2, "recorded": 1, "replayed": 9, "refused": 0}, st
    assert all(sum(c.values()) == c["eager"] for c in twin.plan_stats().values())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the fill-up case
def test_the_frame_plan_replays_where_the_stale_batch_is_filled_up(nets, dev):
    """network_base 64x96, global on, B = 4: ``last_feat_extract.1`` splits K below 8 frames, so 1 or 5 stale frames run as 8
    (tests/test_gpu_multiframe.py, FINDING): ``run`` = 8 for f in 1, 5, 8 -- three frame-stage keys, each replayed."""
    h, w = 64, 96
    net = fresh(nets["base"], True)
    ops = net._ops(dev)
    frames = n_frames(8, h, w, dev)
    left, right = [0, 1, 2, 3], [4, 5, 6, 7]
    want = net._frame_stage_splitk(ops, h, w, 8)
    assert all(net._frame_stage_splitk(ops, h, w, f) != want for f in (1, 5)) and net._splitk_of(ops, h, w, 8) == want
    ref = plain(net, frames, left, right)
    pool = poisoned_pool(net, frames, h, w, 8, range(8))
    for f in (8, 5, 1):
        before = net.plan_stats()["pooled_frame"]
        for i in range(4):
            for s in range(f):
                pool.invalidate((s + 3 * i) % 8)                  # other slots in the recording call than in the replay
            same(ref, net.forward_pooled(pool, left, right), f"f={f} call {i}")
        after = net.plan_stats()["pooled_frame"]
        assert {k: after[k] - before[k] for k in after} == {"eager": 2, "recorded": 1, "replayed": 1, "refused": 0}, (f, before, after)
    torch.cuda.synchronize()
    pool.release()


# ------------------------------------------------------------------------------------------------ 4. pools
def test_another_pool_replays_the_same_plans(nets, dev):
    h, w, (left, right) = 64, 96, ([2, 0], [5, 2])
    net = fresh(nets["lite"], True)
    frames = n_frames(6, h, w, dev)
    ref = plain(net, frames, left, right)
    first = poisoned_pool(net, frames, h, w, 6, [0, 2, 5])
    for i in range(4):
        for s in (0, 2, 5):
            first.invalidate(s)
        same(ref, net.forward_pooled(first, left, right), f"first pool call {i}")
    st = net.plan_stats()
    assert st["pooled_pair"]["recorded"] == 1 and st["pooled_frame"]["recorded"] == 1 and st["pooled_pair"]["replayed"] == 1
    # a second pool of the same shape and slot count (what tta=True creates): the first pool's plans, no new recording
    second = poisoned_pool(net, frames, h, w, 6, [0, 2, 5])
    same(ref, net.forward_pooled(second, left, right), "second pool")
    same(ref, net.forward_pooled(second, left, right), "second pool, nothing stale")
    st2 = net.plan_stats()
    assert st2["pooled_pair"] == dict(st["pooled_pair"], replayed=st["pooled_pair"]["replayed"] + 2), st2
    assert st2["pooled_frame"] == dict(st["pooled_frame"], replayed=st["pooled_frame"]["replayed"] + 1), st2
    assert torch.equal(second.tokens_l[[0, 2, 5]], first.tokens_l[[0, 2, 5]])
    # another slot count is another key: its own warm-up and recording, the same bits
    third = poisoned_pool(net, frames, h, w, 7, [0, 2, 5])
    for i in range(4):
        same(ref, net.forward_pooled(third, left, right), f"pool of 7 slots call {i}")
    st3 = net.plan_stats()
    assert st3["pooled_pair"]["eager"] == st2["pooled_pair"]["eager"] + 2 and st3["pooled_pair"]["recorded"] == 2
    assert st3["pooled_pair"]["refused"] == 0 and st3["pooled_pair"]["replayed"] == st2["pooled_pair"]["replayed"] + 1
    same(ref, net.forward_pooled(first, left, right), "the first pool again")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. invalidation
def warm(net, pool, frames, left, right, calls=4):
    """``calls`` pooled forwards, all slots stale each time; the last one's result."""
    for _ in range(calls):
        for s in set(left + right):
            pool.invalidate(s)
        out = net.forward_pooled(pool, left, right)
    return out


def test_other_weights_drop_the_plans(nets, dev):
    h, w, (left, right) = 64, 96, ([0], [1])
    net = fresh(nets["lite"], True)
    frames = n_frames(2, h, w, dev)
    pool = poisoned_pool(net, frames, h, w, 2, [0, 1])
    ref = plain(net, frames, left, right)
    same(ref, warm(net, pool, frames, left, right), "before")
    assert net.plan_stats()["pooled_pair"]["recorded"] == 1 and net.plan_stats()["pooled_frame"]["recorded"] == 1
    try:
        net.load_state_dict({k: v.to(dev) for k, v in pkg.synthetic_state_dict("lite", seed=2).items()}, strict=True)
        ref2 = plain(net, frames, left, right)
        assert not torch.equal(ref2["I_t"], ref["I_t"])
        before = net.plan_stats()
        same(ref2, net.forward_pooled(pool, left, right), "other weights")           # stale tokens AND no replay of the old plans
        after = net.plan_stats()
        assert after["pooled_pair"]["eager"] == before["pooled_pair"]["eager"] + 1 and after["pooled_frame"]["eager"] == before["pooled_frame"]["eager"] + 1
        assert not net._pool_plans or all(isinstance(p, int) for p in net._pool_plans.values())
    finally:
        net.load_state_dict({k: v.to(dev) for k, v in pkg.synthetic_state_dict("lite", seed=1).items()}, strict=True)
    same(ref, warm(net, pool, frames, left, right), "weights restored")
    st = net.plan_stats()
    assert st["pooled_pair"]["recorded"] == 2 and st["pooled_frame"]["recorded"] == 2 and st["pooled_pair"]["refused"] == 0, st
    torch.cuda.synchronize()


@pytest.mark.parametrize("what", ["global_motion", "precision"])
def test_another_mode_records_its_own_plans(nets, dev, what):
    h, w, (left, right) = 64, 96, ([0, 2], [2, 1])
    net = fresh(nets["lite"], True)
    frames = n_frames(4, h, w, dev)
    pool = poisoned_pool(net, frames, h, w, 4, [0, 1, 2])
    ref = plain(net, frames, left, right)
    same(ref, warm(net, pool, frames, left, right), "before")
    rec = net.plan_stats()["pooled_pair"]["recorded"]
    try:
        if what == "global_motion":
            net.global_motion = False
        else:
            net.set_precision("f32")
        ref2 = plain(net, frames, left, right)
        assert not torch.equal(ref2["I_t"], ref["I_t"])
        for i in range(4):                                    # nothing invalidated by hand: the tokens of the other mode are stale
            same(ref2, net.forward_pooled(pool, left, right), f"{what} changed, call {i}")
        st = net.plan_stats()
        assert st["pooled_pair"]["recorded"] == rec + 1 and st["pooled_pair"]["refused"] == 0, st
    finally:
        net.global_motion = True
        net.set_precision("f16x3")
    for i in range(2):
        same(ref, net.forward_pooled(pool, left, right), f"{what} back, call {i}")
    torch.cuda.synchronize()


def test_an_evicted_workspace_takes_its_plans_along(nets, dev):
    """``max_workspaces = 1``: a B = 2 call between two B = 1 calls frees the B = 1 workspace; its plans hold pointers into it and must
    go with it -- seen in the counts (the next B = 1 call is a direct one and the key warms up again), never by running a stale plan."""
    h, w = 64, 96
    net = fresh(nets["lite"], True)
    net.max_workspaces = 1
    try:
        frames = n_frames(4, h, w, dev)
        pool = poisoned_pool(net, frames, h, w, 4, range(4))
        one, two = ([0], [1]), ([0, 2], [1, 3])
        ref1 = plain(net, frames, *one)
        ref2 = plain(net, frames, *two)
        same(ref1, warm(net, pool, frames, *one), "B=1")
        st = net.plan_stats()
        assert st["pooled_pair"] == {"eager": 2, "recorded": 1, "replayed": 1, "refused": 0}
        same(ref2, net.forward_pooled(pool, *two), "B=2 in between")
        assert len(net._workspaces) == 1 and not any(k[-1][1][0] == 1 for k in net._pool_plans)
        mid = net.plan_stats()
        same(ref1, net.forward_pooled(pool, *one), "B=1 after the eviction")
        after = net.plan_stats()
        assert after["pooled_pair"]["replayed"] == mid["pooled_pair"]["replayed"] and after["pooled_pair"]["eager"] == mid["pooled_pair"]["eager"] + 1
        same(ref1, warm(net, pool, frames, *one, calls=3), "B=1 warmed up again")
        end = net.plan_stats()
        assert end["pooled_pair"]["recorded"] == 2 and end["pooled_pair"]["replayed"] == mid["pooled_pair"]["replayed"] + 1, end
    finally:
        net.max_workspaces = 2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. switches
def test_switches_keep_the_direct_path(nets, dev):
    h, w, (left, right) = 64, 96, ([0, 3], [3, 1])
    net = fresh(nets["lite"], True)
    frames = n_frames(4, h, w, dev)
    pool = poisoned_pool(net, frames, h, w, 4, [0, 1, 3])
    ref = plain(net, frames, left, right)
    assert Network.SELECTIONS == ("use_plans",)
    # plans off: direct launches only, and no plan is kept
    net.enable_plans(False)
    try:
        same(ref, warm(net, pool, frames, left, right, calls=5), "plans off")
        st = net.plan_stats()
        assert st["pooled_pair"] == {"eager": 5, "recorded": 0, "replayed": 0, "refused": 0} and not net._pool_plans
        assert st["pooled_frame"] == {"eager": 5, "recorded": 0, "replayed": 0, "refused": 0}
    finally:
        net.enable_plans(True)
    assert all(not any(c.values()) for c in net.plan_stats().values())       # enable_plans restarts the counts
    # per-launch profiling needs the launches: direct, with their records, also where a plan exists
    same(ref, warm(net, pool, frames, left, right), "plans on")
    assert net.plan_stats()["pooled_pair"]["replayed"] == 1
    ops = net._ops(dev)
    for s in (0, 1, 3):
        pool.invalidate(s)
    ops.profile = []
    try:
        out = net.forward_pooled(pool, left, right)
        torch.cuda.synchronize()
        names = [name for name, _, _, _ in ops.profile]
        stem = [int(m["shape"].split("x")[0]) for name, m, _, _ in ops.profile if name == "stem_fused"]
    finally:
        ops.profile = None
    same(ref, out, "profiled")
    assert stem == [3] and names.count("pool_blocks") == 6 and len(names) > 50
    st = net.plan_stats()
    assert st["pooled_pair"]["replayed"] == 1 and st["pooled_pair"]["eager"] == 3 and st["pooled_frame"]["eager"] == 3
    same(ref, net.forward_pooled(pool, left, right), "replay after profiling")
    assert net.plan_stats()["pooled_pair"]["replayed"] == 2
    torch.cuda.synchronize()


def test_the_ensemble_takes_the_plain_path(nets, dev):
    net = fresh(nets["lite"], True)
    net.ensemble_global_motion = True
    try:
        frames = n_frames(4, 128, 192, dev)
        pool = poisoned_pool(net, frames, 128, 192, 4, range(4))
        ref = plain(net, frames, [1, 3], [2, 0])
        for i in range(4):
            same(ref, net.forward_pooled(pool, [1, 3], [2, 0]), f"ensemble call {i}")
        st = net.plan_stats()
        assert st["pooled_pair"] == {"eager": 4, "recorded": 0, "replayed": 0, "refused": 0} and not any(st["pooled_frame"].values())
        assert not net._pool_plans
    finally:
        net.ensemble_global_motion = False
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. the loops
def frames_equal(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k


@pytest.mark.parametrize("factor,max_batch,tta", [(4, 1, False), (4, 4, False), (8, 1, False), (8, 4, False), (8, 4, True)])
def test_the_nx_loop_gives_the_frames_of_a_model_without_plans(nets, eager_lite, dev, factor, max_batch, tta):
    net = fresh(nets["lite"], True)
    video = pairs.uint8_video(7, 80, 112, seed=4)                # 6 segments
    kw = dict(factor=factor, isBGR=True, divisor=32, tta=tta, max_batch=max_batch)
    got = list(host_io.interpolate_video_nx(iter(video), net, **kw))
    want = list(host_io.interpolate_video_nx(iter(video), eager_lite, **kw))
    assert len(got) == 6 * factor + 1
    frames_equal(got, want)
    st = net.plan_stats()
    assert st["pooled_pair"]["replayed"] > 0 and st["pooled_frame"]["replayed"] > 0 and st["pooled_pair"]["refused"] == 0 == st["pooled_frame"]["refused"], st
    assert all(sum(c.values()) == c["eager"] for c in eager_lite.plan_stats().values())
    print(f"{factor}x max_batch={max_batch} tta={tta}: {st}")


def test_the_retimed_loop_with_a_cut_and_a_dropped_duplicate(nets, eager_lite, dev):
    """24 -> 60, levels=3, 13 source frames: the seventh is a duplicate of the sixth (dropped), and the frames behind it are another
    shot (a cut: that segment runs no forward, and replays follow it)."""
    net = fresh(nets["lite"], True)
    a = pairs.uint8_video(6, 80, 112, seed=5)
    b = [(f // 3 + 160).astype(np.uint8) for f in pairs.uint8_video(6, 80, 112, seed=6)]
    video = a + [D.primed(a[-1], 3)] + b
    assert len(video) == 13
    out = []
    for m in (net, eager_lite):
        sc, dd = scene.SceneCuts(), rt.Duplicates()
        out.append(list(host_io.interpolate_video_retimed(iter(video), m, 24, 60, levels=3, isBGR=True, divisor=32, scene=sc, dedup=dd)))
        assert len(dd.dropped) == 1 and len(sc.cuts) == 1, (dd.dropped, sc.cuts)
    frames_equal(*out)
    st = net.plan_stats()
    assert st["pooled_pair"]["replayed"] > 0 and st["pooled_pair"]["refused"] == 0 == st["pooled_frame"]["refused"], st
    print(f"24 -> 60 levels=3: {st}")


def test_ten_bit_i420_with_the_depth_kept(nets, eager_lite, dev):
    net = fresh(nets["lite"], True)
    fmt = yuv.Format(64, 96, depth=10)
    video = [yuv.encode_numpy(f.astype(np.float32) / np.float32(255), fmt) for f in pairs.uint8_video(7, 64, 96, seed=5)]
    kw = dict(factor=4, divisor=32, max_batch=1, pixfmt=fmt, keep_depth=True)
    got = list(host_io.interpolate_video_nx(iter(video), net, **kw))
    want = list(host_io.interpolate_video_nx(iter(video), eager_lite, **kw))
    assert len(got) == 25 and got[1].dtype == np.uint16
    frames_equal(got, want)
    assert net.plan_stats()["pooled_pair"]["replayed"] > 0
