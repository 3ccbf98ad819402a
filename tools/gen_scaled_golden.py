#!/usr/bin/env python3
"""Generate ``tests/golden/scaled_ref.npz``: the REFERENCE's own ``Network.forward`` on the CPU, run through the composition that
defines half-resolution motion (``atm-vfi_amd/scaled.py::compose_torch``: F.avg_pool2d, the forward at half size, F.interpolate of
flows, mask and residual, the reference's flow_warp of the full-size frames, the blend).

    python tools/gen_scaled_golden.py --reference DIR

Weights: ``schema.synthetic_state_dict(v, seed=1)``; inputs: ``pairs.smooth_pair``; cases: ``CASES`` below.  Stored per case: the fp32
``<case>.I_t`` at full size, ``<case>.f0``, ``<case>.f1``, ``<case>.m`` (every ``STEP``-th row and column of the full-size maps: the file
stays below the repository's 1 MiB limit for a committed file: 596 695 bytes, against 1 130 751 with the full maps) and the input checksums ``<case>.in_sums``.  Arrays only; nothing
of the reference travels.  The reference is imported through ``oracle.gen_golden.import_reference``."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 2
# name, variant, H, W, global_motion, seed of pairs.smooth_pair
CASES = (("lite_128x192", "lite", 128, 192, False, 7), ("base_128x128_global", "base", 128, 128, True, 11))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scaled_ref.npz"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT]
    from oracle import gen_golden
    gen_golden.REF = os.path.abspath(args.reference)
    ref = gen_golden.import_reference()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import pairs
    schema = importlib.import_module("atm-vfi_amd.schema")
    scaled = importlib.import_module("atm-vfi_amd.scaled")
    torch.set_grad_enabled(False)
    mods = {"base": ref.network_base, "lite": ref.network_lite}
    arrs = {}
    for name, v, h, w, g, seed in CASES:
        net = mods[v].Network().eval()
        net.load_state_dict(schema.synthetic_state_dict(v, seed=1), strict=True)
        net.global_motion = g
        net.ensemble_global_motion = False
        im0, im1 = pairs.smooth_pair(1, h, w, seed=seed)
        out = scaled.compose_torch(lambda a, b: net.forward(a, b), im0, im1)
        for key, short in (("I_t", "I_t"), ("opt_flow_0", "f0"), ("opt_flow_1", "f1"), ("occ_mask1", "m")):
            step = 1 if key == "I_t" else STEP
            arrs[f"{name}.{short}"] = gen_golden.sub(out[key], step).astype(np.float32)
        arrs[f"{name}.in_sums"] = np.array([im0.double().sum().item(), im1.double().sum().item()])
        print(name, {k: float(np.abs(a).mean()) for k, a in arrs.items() if k.startswith(name)})
    np.savez_compressed(args.out, **arrs)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(arrs)} arrays")


if __name__ == "__main__":
    main()
