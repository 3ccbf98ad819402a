#!/usr/bin/env python3
"""Generate ``tests/golden/fields_ref.npz``: the REFERENCE's own ``Network.forward`` on the CPU on the bobbed field canvases of the
deinterlacing loop (atm-vfi_amd/fields.py, ``mode="mc"``, tff): for every interior field k of four woven 64 x 96 frames,
``I_t = forward(B_{k-1}, B_{k+1})`` with ``B_i`` the canvas form of ``fields.bob_numpy`` (the host twin of ``atmvfi_field_bob``).

    python tools/gen_fields_golden.py --reference DIR

Weights: ``schema.synthetic_state_dict(v, seed=1)``; inputs: ``tests/cpu_fields.py::reference_video`` (a moving ``pairs`` picture, even
rows from time 2j, odd rows from time 2j + 1); cases: network_lite and network_base with the global branch on.  Stored: fp32 ``I_t``
of the interior fields (``<case>.it.<k>``, sub-sampled by ``REF_STEP``) and the input checksums (``in_sums``: the fp64 sum of every
field canvas).  Nothing of the reference travels.  The reference is imported through ``oracle.gen_golden.import_reference``."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fields_ref.npz"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT]
    from oracle import gen_golden
    gen_golden.REF = os.path.abspath(args.reference)
    ref = gen_golden.import_reference()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import cpu_fields as M
    schema = importlib.import_module("atm-vfi_amd.schema")
    fields = importlib.import_module("atm-vfi_amd.fields")
    segments = importlib.import_module("atm-vfi_amd.segments")
    torch.set_grad_enabled(False)
    canvas = segments._canvas(M.REF_H, M.REF_W, M.REF_DIVISOR)
    pics = M.reference_pictures()
    B = [torch.from_numpy(fields.bob_numpy(pics[i // 2], fields.field_parity(i, "tff"), canvas)).unsqueeze(0) for i in range(2 * M.REF_N)]
    arrs = {"in_sums": np.array([b.double().sum().item() for b in B])}
    mods = {"base": ref.network_base, "lite": ref.network_lite}
    for name, v in M.REF_CASES:
        net = mods[v].Network().eval()
        net.load_state_dict(schema.synthetic_state_dict(v, seed=1), strict=True)
        gen_golden.drop_mask_cache(net)
        net.global_motion, net.ensemble_global_motion = True, False
        for k in range(1, 2 * M.REF_N - 1):
            it = net.forward(B[k - 1], B[k + 1])["I_t"]
            arrs[f"{name}.it.{k}"] = gen_golden.sub(it[0], M.REF_STEP)
            print(name, k, float(it.mean()))
    np.savez_compressed(args.out, **arrs)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(arrs)} arrays")


if __name__ == "__main__":
    main()
