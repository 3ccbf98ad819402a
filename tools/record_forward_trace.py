#!/usr/bin/env python3
"""Record what one eager forward launches (tests/forward_trace.py: the recorder and the case list) as JSON: ``{case: [[name, bytes,
shape], ...]}``.  ``tests/golden/forward_trace.json`` is this tool's output on the commit BEFORE a change to the forward's
orchestration (``--package-root``: a checkout of that commit, whose ``atm-vfi_amd`` is then the package traced, with this tree's
recorder and cases); ``tests/test_gpu_forward_trace.py`` replays the cases on the tree under test and requires equal traces.

    python tools/record_forward_trace.py [--out tests/golden/forward_trace.json] [--cases base_64x64_g_b1,...] [--package-root DIR]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "forward_trace.json"))
    ap.add_argument("--cases", default=None)
    ap.add_argument("--package-root", default=ROOT, help="the tree whose atm-vfi_amd package is traced (default: this one)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("record_forward_trace: no GPU")
    sys.path[:0] = [os.path.abspath(a.package_root), os.path.join(ROOT, "tests")]
    import forward_trace
    print(f"tracing {os.path.dirname(forward_trace.pkg.__file__)}", flush=True)
    traces = {}
    for name in list(forward_trace.CASES) if a.cases is None else a.cases.split(","):
        traces[name] = forward_trace.trace_of(name, torch.device("cuda:0"))
        print(f"{name:>40}: {len(traces[name])} launches", flush=True)
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in traces.items()) + "\n}\n")


if __name__ == "__main__":
    main()
