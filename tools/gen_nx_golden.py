#!/usr/bin/env python3
"""Generate ``tests/golden/nx_ref.npz``: the REFERENCE's own ``Network.forward`` on the CPU, chained exactly as its
``benchmark/davis-vid.py:102-112`` chains it (level 1 from the two frames, deeper levels from the unrounded fp32 predictions; with
TTA the flip average of every produced frame next to the un-averaged prediction that feeds the next level).

    python tools/gen_nx_golden.py --reference DIR

Weights: ``schema.synthetic_state_dict(v, seed=1)``; inputs: ``pairs.smooth_pair``; cases: ``tests/multiframe_ref.py::NX_CASES``.
Stored: outputs (``<case>.pred.<position>``, ``<case>.tta.<position>``, sub-sampled by the case's store step) and input checksums
(``<case>.in_sums``).  Nothing of the reference travels.  The reference is imported through ``oracle.gen_golden.import_reference``."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "nx_ref.npz"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT]
    from oracle import gen_golden
    gen_golden.REF = os.path.abspath(args.reference)
    ref = gen_golden.import_reference()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import multiframe_ref as M
    schema = importlib.import_module("atm-vfi_amd.schema")
    torch.set_grad_enabled(False)
    mods = {"base": ref.network_base, "lite": ref.network_lite}
    nets = {}
    arrs = {}
    for case in M.NX_CASES:
        name, v, h, w, g, depth, tta, seed, step = case
        if v not in nets:
            nets[v] = mods[v].Network().eval()
            nets[v].load_state_dict(schema.synthetic_state_dict(v, seed=1), strict=True)
        net = nets[v]
        gen_golden.drop_mask_cache(net)
        net.global_motion = g
        net.ensemble_global_motion = False
        im0, im1 = M.case_inputs(case)
        pred, shown = M.chain(lambda a, b: net.forward(a, b)["I_t"], im0, im1, 1 << depth, tta=tta)
        for pos, t in pred.items():
            arrs[f"{name}.pred.{pos}"] = gen_golden.sub(t, step)
            if tta:
                arrs[f"{name}.tta.{pos}"] = gen_golden.sub(shown[pos], step)
        arrs[f"{name}.in_sums"] = np.array([im0.double().sum().item(), im1.double().sum().item()])
        print(name, {p: float(t.mean()) for p, t in sorted(pred.items())})
    np.savez_compressed(args.out, **arrs)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(arrs)} arrays")


if __name__ == "__main__":
    main()
