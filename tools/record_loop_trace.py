#!/usr/bin/env python3
"""Record what the video loops launch (tests/loop_trace.py: the recorder and the case list) on the commit it is run on, as JSON:
``{case: [entry, ...]}``, names and numbers only.  ``tests/golden/loop_trace.json`` is this tool's output on the commit BEFORE a change
to the loops' host layer; ``tests/test_gpu_loop_trace.py`` replays the cases on the tree under test and requires equal traces.

    python tools/record_loop_trace.py [--out tests/golden/loop_trace.json] [--cases nx_4x_pool,rt_dedup]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "loop_trace.json"))
    ap.add_argument("--cases", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("record_loop_trace: no GPU")
    import loop_trace
    net = loop_trace.lite_network(torch.device("cuda:0"))
    names = list(loop_trace.CASES) if a.cases is None else a.cases.split(",")
    traces = {}
    for name in names:
        traces[name] = loop_trace.trace_of(net, name)
        print(f"{name:>24}: {len(traces[name])} entries", flush=True)
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in traces.items()) + "\n}\n")


if __name__ == "__main__":
    main()
