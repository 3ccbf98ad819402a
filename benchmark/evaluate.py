#!/usr/bin/env python3
"""Score a checkpoint on Vimeo90K, UCF101 or SNU-FILM with the protocols of the reference's scripts (benchmark/test_vimeo90k.py,
test_ucf101.py, test_snufilm.py) on the HIP hot path and the fused metric kernel.

    python benchmark/evaluate.py --dataset vimeo90k --path DIR --ckpt FILE [--model base|lite] [--tta] [--streams K] [--limit N]
                                 [--global-motion on|off] [--json OUT]
    python benchmark/evaluate.py --dataset snufilm --path DIR/eval_modes --img-data-path DIR/ --ckpt FILE

Prints ``Avg PSNR: … SSIM: …`` per dataset (per level for SNU-FILM), as the reference's scripts do."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module  # noqa: E402

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", required=True, choices=("vimeo90k", "ucf101", "snufilm"))
    ap.add_argument("--path", required=True)
    ap.add_argument("--img-data-path", default=None, help="SNU-FILM: replaces the lists' data/SNU-FILM/test/ prefix")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--model", choices=("base", "lite"), default="base")
    ap.add_argument("--tta", action="store_true", help="flip test-time augmentation")
    ap.add_argument("--streams", type=int, default=1, help="forwards in flight")
    ap.add_argument("--limit", type=int, default=None, help="score only the first N samples")
    ap.add_argument("--global-motion", choices=("on", "off"), default=None, help="override the protocol's global_motion")
    ap.add_argument("--json", default=None, help="write the per-sample records and the means here")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    pkg = import_module("atm-vfi_amd")
    host_io = import_module("atm-vfi_amd.host_io")
    ev = import_module("atm-vfi_amd.evaluate")
    if a.dataset == "snufilm":
        if a.img_data_path is None:
            ap.error("--dataset snufilm needs --img-data-path")
        samples = ev.snufilm(a.path, a.img_data_path)
    else:
        samples = ev.LISTERS[a.dataset](a.path)
    torch.set_grad_enabled(False)
    dev = torch.device(a.device)
    model = pkg.NetworkBase() if a.model == "base" else pkg.NetworkLite()
    print(f"--- loading from checkpoint: {a.ckpt} ---")
    host_io.load_model_checkpoint(model, a.ckpt)
    model.to(dev).eval()
    gm = None if a.global_motion is None else a.global_motion == "on"
    print(f"Dataset: {a.dataset}\t TTA: {a.tta}\t samples: {len(samples) if a.limit is None else min(a.limit, len(samples))}")
    t0 = time.time()
    res = ev.evaluate(model, samples, a.dataset, tta=a.tta, streams=a.streams, limit=a.limit, global_motion=gm,
                      progress=lambda d, n, p, s: print(f"{d}/{n}  PSNR {p:.4f}  SSIM {s:.5f}", flush=True))
    print(ev.format_levels(res))
    print(f"({len(res.records)} samples in {time.time() - t0:.1f} s)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"dataset": a.dataset, "model": a.model, "tta": a.tta, "global_motion": model.global_motion,
                       "levels": res.levels, "records": res.records}, f, indent=1)
    return res


if __name__ == "__main__":
    main()
