"""GPU: the launches of one eager forward are pinned.  ``tests/golden/forward_trace.json`` holds, for every case of
tests/forward_trace.py, what ``forward`` / ``forward_pooled`` launched on the commit before the forward's orchestration was split into a
rows path and a planes path: every ``HipOps._run`` with its name, byte count and shape string, in order.  The tree under test must
launch the same, entry for entry.  (Written by ``tools/record_forward_trace.py``; a pull request that changes the launches on purpose
records the file again and says so.)"""
import json
import os

import pytest
import torch

import forward_trace

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_trace.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_holds_every_case():
    assert list(GOLDEN) == list(forward_trace.CASES) and all(GOLDEN.values())


@pytest.mark.parametrize("case", list(forward_trace.CASES))
def test_the_forward_launches_what_it_launched(case, weights):
    assert torch.cuda.is_available()
    want = GOLDEN[case]
    got = forward_trace.trace_of(case, torch.device("cuda:0"), weights(forward_trace.CASES[case][0]))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: launch {k} of {len(want)}: launched {g}, recorded {w} (after {got[max(0, k - 3):k]})"
    assert len(got) == len(want), f"{case}: {len(got)} launches, {len(want)} recorded; the first one beyond: {max(got, want, key=len)[min(len(got), len(want)):][:1]}"
