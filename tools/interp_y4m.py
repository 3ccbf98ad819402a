#!/usr/bin/env python3
"""Y4M in, Y4M out at ``factor`` times the frame rate (``atm-vfi_amd.yuv.interpolate_y4m``): frames travel as planar 4:2:0 and are
converted on the GPU; originals are written as read.  Reads C420 / C420jpeg / C420mpeg2 / C420p10 progressive streams; 10-bit input
is written back as 8-bit, or with ``--keep-depth`` as C420p10 (originals byte for byte, predictions encoded at 10 bits).  ``-`` reads standard input / writes standard output (``ffmpeg -i in.mp4 -f yuv4mpegpipe - | interp_y4m.py
- out.y4m --ckpt ...``).

    python tools/interp_y4m.py IN.y4m OUT.y4m --ckpt CKPT [--model base|lite] [--factor 2|4|8] [--scene] [--tta] [--global-off]
                              [--keep-depth] [--active] [--fps-out R [--levels L] [--dedup] [--shutter ANGLE [--light code|linear]]]

``--fps-out R`` (an integer or a ratio such as 60000/1001) converts the frame rate to exactly R instead of multiplying it: every output
is the nearest of 2**L positions (``--levels``, default 3) between two source frames; ``--dedup`` drops repeated frames first
(``Duplicates()`` defaults); ``--shutter ANGLE`` (degrees, 0 < ANGLE <= 360; 180 is a film camera's) blurs every output over the
positions inside its exposure of ANGLE / 360 output periods, averaged in linear light (``--light code``: in code values); 8-bit output
only."""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--ckpt", default=None, help="checkpoint (the trainer's dict or a bare state dict); without one: synthetic weights")
    ap.add_argument("--model", choices=("base", "lite"), default="base")
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--scene", action="store_true", help="scene-cut detection (SceneCuts() defaults)")
    ap.add_argument("--tta", action="store_true", help="flip test-time augmentation of every produced frame")
    ap.add_argument("--global-off", action="store_true", help="switch the global motion branch off")
    ap.add_argument("--matrix", choices=("auto", "bt601", "bt709"), default="auto", help="a Y4M header cannot name the matrix")
    ap.add_argument("--keep-depth", action="store_true", help="write 10-bit (C420p10) input back as C420p10 instead of 8-bit")
    ap.add_argument("--active", action="store_true", help="run the network on the active picture of letterboxed video (ActiveArea() "
                    "defaults); 10-bit input needs --keep-depth")
    ap.add_argument("--fps-out", default=None, metavar="R", help="convert the frame rate to R (e.g. 60 or 60000/1001); --factor is ignored")
    ap.add_argument("--levels", type=int, default=3, help="with --fps-out: 2**L positions per segment (1..6)")
    ap.add_argument("--dedup", action="store_true", help="with --fps-out: drop repeated frames (Duplicates() defaults)")
    ap.add_argument("--shutter", default=None, metavar="ANGLE", help="with --fps-out: a synthetic shutter of ANGLE degrees (e.g. 180)")
    ap.add_argument("--light", choices=("code", "linear"), default="linear", help="with --shutter: the domain the samples are averaged in")
    ap.add_argument("--precision", choices=("f16x3", "f16", "f32"), default="f16x3", help="contraction arithmetic (Network.set_precision): f16x3 = the default, three 16-bit MFMAs per product; f16 = single-pass fp16 in the plane kernels (faster, about 1e-2 of the frame range); f32 = exact fp32 MFMA (about 2.5x slower)")
    ap.add_argument("--motion-scale", type=int, choices=(1, 2), default=1, help="2: half-resolution motion -- the network runs on 2x reduced frames, one kernel synthesises at full size (about 4x fewer network pixels; not with --shutter)")
    ap.add_argument("--interlaced", choices=("tff", "bff", "auto"), default=None, help="the input is woven interlaced video of this field order"
                    + (" (auto: the It / Ib tag of the header)") + ": it is deinterlaced to field rate first and the loop runs on that stream at twice the rate "
                    "(4:2:2 and 4:4:4 only; 10-bit input needs --keep-depth)")
    ap.add_argument("--deint", choices=("mc", "bob"), default="mc", help="with --interlaced: motion-compensated (one forward per output frame) or the field's own line average")
    ap.add_argument("--deint-only", action="store_true", help="with --interlaced: write the field-rate stream itself, run no further loop")
    a = ap.parse_args()
    if (a.deint != "mc" or a.deint_only) and a.interlaced is None:
        ap.error("--deint and --deint-only need --interlaced")
    if a.motion_scale == 2 and a.shutter is not None:
        ap.error("--motion-scale 2 does not go with --shutter")
    if (a.dedup or a.levels != 3 or a.shutter is not None) and a.fps_out is None:
        ap.error("--levels, --dedup and --shutter need --fps-out")
    if a.light != "linear" and a.shutter is None:
        ap.error("--light needs --shutter")
    if a.active and a.shutter is not None:
        ap.error("--active does not go with --shutter")
    if not torch.cuda.is_available():
        sys.exit("interp_y4m: no GPU")
    pkg = importlib.import_module("atm-vfi_amd")
    yuv = importlib.import_module("atm-vfi_amd.yuv")
    torch.set_grad_enabled(False)
    net = pkg.NetworkBase() if a.model == "base" else pkg.NetworkLite()
    if a.ckpt:
        yuv.load_model_checkpoint(net, a.ckpt)
    else:
        print("interp_y4m: no --ckpt: synthetic weights (the output is not a meaningful interpolation)", file=sys.stderr)
        net.load_state_dict(pkg.synthetic_state_dict(a.model, seed=1), strict=True)
    net = net.to(torch.device("cuda:0")).eval()
    net.global_motion = not a.global_off
    net.set_precision(a.precision)
    area = yuv.ActiveArea() if a.active else None
    src = sys.stdin.buffer if a.src == "-" else a.src
    dst = sys.stdout.buffer if a.dst == "-" else a.dst
    info = yuv.interpolate_y4m(src, dst, net, factor=a.factor, scene=yuv.SceneCuts() if a.scene else None, tta=a.tta, matrix=a.matrix,
                               keep_depth=a.keep_depth, **({"active": area} if area is not None else {}),
                               **({"motion_scale": 2} if a.motion_scale == 2 else {}),
                               **(dict(interlaced=a.interlaced, deint=a.deint, deint_only=a.deint_only) if a.interlaced else {}),
                               **(dict(fps_out=a.fps_out, levels=a.levels, dedup=yuv.Duplicates() if a.dedup else None,
                                       shutter=yuv.Shutter(a.shutter, a.light) if a.shutter is not None else None) if a.fps_out else {}))
    print({k: (str(v) if k.startswith("fps") else v) for k, v in info.items()}, file=sys.stderr)
    if area is not None:
        print(f"interp_y4m: active window (y0, x0, h, w) = {area.window} after {area.probed} frames, fallback_at = {area.fallback_at}", file=sys.stderr)


if __name__ == "__main__":
    main()
