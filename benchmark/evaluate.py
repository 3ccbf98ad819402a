#!/usr/bin/env python3
"""Score a checkpoint on Vimeo90K, UCF101, SNU-FILM or Xiph 2K/4K with the protocols of the reference's scripts
(benchmark/test_vimeo90k.py, test_ucf101.py, test_snufilm.py, test_xiph.py) on the HIP hot path and the fused metric kernel.

    python benchmark/evaluate.py --dataset vimeo90k --path DIR --ckpt FILE [--model base|lite] [--tta] [--streams K] [--limit N]
                                 [--global-motion on|off] [--json OUT]
    python benchmark/evaluate.py --dataset snufilm --path DIR/eval_modes --img-data-path DIR/ --ckpt FILE
    python benchmark/evaluate.py --dataset xiph --path ROOT --ckpt FILE [--categories resized-2k,cropped-4k] [--clips A,B] [--frames 2:99:2] [--timings]
                                 [--source auto|png|y4m] [--matrix auto|bt601|bt709]

Prints ``Avg PSNR: … SSIM: …`` per dataset (per level for SNU-FILM, per category with its name in front for Xiph), as the reference's
scripts do.  Xiph: ROOT/<clip>/001.png … 099.png, 4096 x 2160 (the script's ffmpeg download is not reproduced), or the clip as the
4:2:0 Y4M file it is distributed as -- ROOT/<clip>.y4m or ROOT/Netflix_<clip>_4096x2160_60fps_10bit_420.y4m -- read without ffmpeg and
converted on the GPU by this project's own colour conversion (--source auto: the directory when it exists, the Y4M file otherwise);
the means are over all samples of a category (the script's progress bar shows a mean that lags by one sample)."""
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
    ap.add_argument("--dataset", required=True, choices=("vimeo90k", "ucf101", "snufilm", "xiph"))
    ap.add_argument("--path", required=True)
    ap.add_argument("--img-data-path", default=None, help="SNU-FILM: replaces the lists' data/SNU-FILM/test/ prefix")
    ap.add_argument("--categories", default=None, help="Xiph: comma-separated subset of resized-2k,cropped-4k")
    ap.add_argument("--clips", default=None, help="Xiph: comma-separated clip directories under --path (default: the script's eight)")
    ap.add_argument("--frames", default="2:99:2", help="Xiph: middle frames as FIRST:STOP[:STEP] (a Python range; default: the script's 2:99:2)")
    ap.add_argument("--source", choices=("auto", "png", "y4m"), default="auto",
                    help="Xiph: a clip's frames from ROOT/<clip>/NNN.png, from its Y4M file, or (auto) the directory when it exists")
    ap.add_argument("--matrix", choices=("auto", "bt601", "bt709"), default="auto", help="Xiph, Y4M clips: the colour matrix (auto: bt709 from 720 rows up)")
    ap.add_argument("--timings", action="store_true", help="Xiph: print the wall time split into decode, upload, prepare, forward, metric")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--model", choices=("base", "lite"), default="base")
    ap.add_argument("--tta", action="store_true", help="flip test-time augmentation")
    ap.add_argument("--streams", type=int, default=1, help="forwards in flight")
    ap.add_argument("--limit", type=int, default=None, help="score only the first N samples")
    ap.add_argument("--global-motion", choices=("on", "off"), default=None, help="override the protocol's global_motion")
    ap.add_argument("--json", default=None, help="write the per-sample records and the means here")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--precision", choices=("f16x3", "f16", "f32"), default="f16x3", help="contraction arithmetic (Network.set_precision): f16x3 = the default, three 16-bit MFMAs per product; f16 = single-pass fp16 in the plane kernels (faster, about 1e-2 of the frame range); f32 = exact fp32 MFMA (about 2.5x slower)")
    a = ap.parse_args(argv)

    pkg = import_module("atm-vfi_amd")
    host_io = import_module("atm-vfi_amd.host_io")
    ev = import_module("atm-vfi_amd.evaluate")
    xiph_kw = None
    if a.dataset == "xiph":
        cats = tuple(a.categories.split(",")) if a.categories else ev.XIPH_CATEGORIES
        for c in cats:
            if c not in ev.XIPH_CATEGORIES:
                ap.error(f"--categories: unknown category {c!r} (known: {','.join(ev.XIPH_CATEGORIES)})")
        try:
            frames = range(*(int(v) for v in a.frames.split(":")))
        except (TypeError, ValueError):
            ap.error(f"--frames: expected FIRST:STOP[:STEP], got {a.frames!r}")
        xiph_kw = {"categories": cats, "clips": tuple(a.clips.split(",")) if a.clips else ev.XIPH_CLIPS, "frames": frames,
                   "source": a.source, "matrix": a.matrix}
        try:
            samples, _ = ev.xiph_samples(a.path, xiph_kw["clips"], frames, a.source)
        except (FileNotFoundError, ValueError) as e:
            ap.error(f"--path {a.path}: {e}")
    elif a.dataset == "snufilm":
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
    model.set_precision(a.precision)
    gm = None if a.global_motion is None else a.global_motion == "on"
    print(f"Dataset: {a.dataset}\t TTA: {a.tta}\t samples: {len(samples) if a.limit is None else min(a.limit, len(samples))}")
    t0 = time.time()
    progress = lambda d, n, p, s: print(f"{d}/{n}  PSNR {p:.4f}  SSIM {s:.5f}", flush=True)        # noqa: E731
    timings = {} if a.timings else None
    sources = {}
    if xiph_kw is not None:
        res = ev.evaluate_xiph(model, a.path, tta=a.tta, streams=a.streams, limit=a.limit, global_motion=gm, progress=progress,
                               timings=timings, sources=sources, **xiph_kw)
    else:
        res = ev.evaluate(model, samples, a.dataset, tta=a.tta, streams=a.streams, limit=a.limit, global_motion=gm, progress=progress)
    print(ev.format_levels(res))
    print(f"({len(res.records)} samples in {time.time() - t0:.1f} s)")
    if timings is not None:
        print("wall {:.2f} s: ".format(time.time() - t0) + ", ".join(f"{k} {timings.get(k, 0.0):.3f} s" for k in
              ("decode_wait", "decode_cpu", "upload", "prepare", "forward", "metric")))
    if a.json:
        with open(a.json, "w") as f:
            out = {"dataset": a.dataset, "model": a.model, "tta": a.tta, "global_motion": model.global_motion,
                   "levels": res.levels, "records": res.records}
            if xiph_kw is not None:
                out["sources"] = sources
            json.dump(out, f, indent=1)
    return res


if __name__ == "__main__":
    main()
