#!/usr/bin/env python3
"""Write ``tests/golden/xiph_ref.npz``: the reference's ``calculate_psnr`` / ``calculate_ssim`` (benchmark/psnr_ssim.py, imported from
the reference checkout at generation time and run on the CPU) called as benchmark/test_xiph.py calls them -- (prediction, ground truth),
the ground truth as img2tensor makes it (uint8 / 255. in fp32) -- on the seeded pairs of ``tests/cpu_frames.py`` XIPH_CASES.  The
fixture holds scalars and input checksums only.

    python tools/gen_xiph_golden.py --reference DIR"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cpu_frames as CF  # noqa: E402
import metric_inputs as MI  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "xiph_ref.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if torch.cuda.is_available():
        sys.exit("run on a machine without a GPU: the reference's modules pick their device at import")
    bench = os.path.join(a.reference, "benchmark")
    spec = importlib.util.spec_from_file_location("ref_psnr_ssim", os.path.join(bench, "psnr_ssim.py"))
    psnr_ssim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(psnr_ssim)
    torch.set_grad_enabled(False)
    rec = {}
    for name in CF.XIPH_CASES:
        gt, pred = CF.xiph_case(name)
        imgt = torch.tensor(gt).permute(2, 0, 1).unsqueeze(0) / 255.0          # img2tensor
        rec[f"{name}/in_sums"] = MI.in_sums(gt, pred)
        rec[f"{name}/psnr"] = np.asarray(psnr_ssim.calculate_psnr(pred, imgt), dtype=np.float64)
        rec[f"{name}/ssim"] = np.asarray(psnr_ssim.calculate_ssim(pred, imgt), dtype=np.float64)
        print(name, float(rec[f"{name}/psnr"]), float(rec[f"{name}/ssim"]))
    np.savez_compressed(a.out, **rec)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes, {len(rec)} arrays)")


if __name__ == "__main__":
    main()
