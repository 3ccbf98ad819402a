#!/usr/bin/env python3
"""Write ``tests/golden/metrics_ref.npz``: the reference's own metric functions (benchmark/pytorch_msssim.py ``ssim_matlab``,
benchmark/psnr_ssim.py ``calculate_psnr`` / ``calculate_ssim``, imported from the reference checkout at generation time and run on
the CPU) on the seeded inputs of ``tests/metric_inputs.py``.  The fixture holds scalars and input checksums only.

    python tools/gen_metric_golden.py --reference DIR"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metric_inputs as MI  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics_ref.npz")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if torch.cuda.is_available():
        sys.exit("run on a machine without a GPU: the reference's modules pick their device at import")
    msssim = _load(os.path.join(a.reference, "benchmark", "pytorch_msssim.py"), "ref_pytorch_msssim")
    psnr_ssim = _load(os.path.join(a.reference, "benchmark", "psnr_ssim.py"), "ref_psnr_ssim")
    torch.set_grad_enabled(False)
    rec = {}
    for name in MI.CASES:
        kind, x, y, kw = MI.case_inputs(name)
        rec[f"{name}/in_sums"] = MI.in_sums(x, y)
        if kind == "ssim":
            r = msssim.ssim_matlab(x, y, **kw)
            ret, cs = r if kw.get("full") else (r, None)
            rec[f"{name}/ssim"] = np.asarray(ret, dtype=np.float64)
            if cs is not None:
                rec[f"{name}/cs"] = np.asarray(cs, dtype=np.float64)
        elif kind.startswith("u8:"):
            psnr, ssim = MI.protocol_reference(kind[3:], x, y, msssim.ssim_matlab)
            rec[f"{name}/psnr"], rec[f"{name}/ssim"] = np.float64(psnr), np.float64(ssim)
        elif kind == "calc":
            rec[f"{name}/psnr"] = np.asarray(psnr_ssim.calculate_psnr(x, y), dtype=np.float64)
            rec[f"{name}/ssim"] = np.asarray(psnr_ssim.calculate_ssim(x, y), dtype=np.float64)
        print(name, {k.split("/")[1]: np.round(v, 7).tolist() for k, v in rec.items() if k.startswith(name + "/") and "sums" not in k})
    np.savez_compressed(a.out, **rec)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes, {len(rec)} arrays)")


if __name__ == "__main__":
    main()
