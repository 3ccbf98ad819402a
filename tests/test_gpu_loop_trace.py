"""GPU: the launches of the video loops are pinned.  ``tests/golden/loop_trace.json`` holds, for every case of tests/loop_trace.py, what
``interpolate_video_nx`` / ``interpolate_video_retimed`` launched on the commit before their host layer was folded onto one pair of
segment backends: every ``HipOps`` call outside the network with its byte count and stream (compute or copy), every ``forward`` /
``forward_pooled`` with its batch and frame size, in order.  The tree under test must launch the same, entry for entry.  (Written by
``tools/record_loop_trace.py``; a pull request that changes the launches on purpose records the file again and says so.)"""
import json
import os

import pytest
import torch

import loop_trace

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_trace.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def net():
    assert torch.cuda.is_available()
    return loop_trace.lite_network(torch.device("cuda:0"))


def test_the_golden_file_holds_every_case():
    assert list(GOLDEN) == list(loop_trace.CASES) and all(GOLDEN.values())


@pytest.mark.parametrize("case", list(loop_trace.CASES))
def test_the_loop_launches_what_it_launched(net, case):
    want = GOLDEN[case]
    keep = net.max_workspaces
    got = loop_trace.trace_of(net, case)
    assert net.max_workspaces == keep
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: entry {k} of {len(want)}: launched {g}, recorded {w} (after {got[max(0, k - 3):k]})"
    assert len(got) == len(want), f"{case}: {len(got)} launches, {len(want)} recorded; the first one beyond: {max(got, want, key=len)[min(len(got), len(want)):][:1]}"
