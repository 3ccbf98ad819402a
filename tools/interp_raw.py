#!/usr/bin/env python3
"""Headerless video in, headerless video out at ``factor`` times the frame rate (``atm-vfi_amd.yuv.interpolate_raw``): the frames of an
``ffmpeg -f rawvideo -pix_fmt nv12|nv21|p010le|yuv420p|yuv420p10le|yuv422p|yuv422p10le|yuv444p|yuv444p10le`` pipe travel as they are and are converted on the GPU; nothing is
repacked on the host.  The output has the same pixel format without row padding; 10-bit input is written back as its 8-bit
counterpart (p010le -> nv12), or with ``--keep-depth`` at 10 bits.  Packed 4:2:2 capture frames travel the same way: ``--pix-fmt
uyvy422|yuyv422|y210le|v210`` (unpacked and packed on the GPU; without ``--keep-depth`` y210le is written as yuyv422 and v210 as
uyvy422).  ffmpeg writes v210 as a codec, not as a ``-pix_fmt``: ``ffmpeg -i in.mov -c:v v210 -f rawvideo -``; its rows are padded to
128 bytes per 48 pixels, which is this tool's default pitch for v210.  Deep RGB -- ``--pix-fmt rgb48le|bgr48le|gbrp10le|gbrp12le|gbrp16le``,
tight frames -- runs with ``--keep-depth`` only (no 8-bit down-conversion of RGB is defined) and without ``--active`` / ``--shutter``
(``ffmpeg -i in.mov -f rawvideo -pix_fmt gbrp12le - | interp_raw.py - out.rgb --pix-fmt gbrp12le --size 1920x1080 --fps 24 --keep-depth``).  ``-`` reads standard input / writes standard output
(``ffmpeg -i in.mp4 -f rawvideo -pix_fmt nv12 - | interp_raw.py - out.nv12 --pix-fmt nv12 --size 1920x1080 --fps 30000/1001 --ckpt ...``).

    python tools/interp_raw.py IN OUT --pix-fmt FMT --size WxH --fps R [--pitch N] [--matrix auto|bt601|bt709] [--siting centre|left]
                              [--full-range] --ckpt CKPT [--model base|lite] [--factor 2|4|8] [--scene] [--tta] [--global-off]
                              [--keep-depth] [--active] [--fps-out R [--levels L] [--dedup] [--shutter ANGLE [--light code|linear]]]

``--pitch N``: the input's luma row stride in bytes (a decoder's surface dump; interleaved chroma rows share it, planar ones have
half, 4:4:4 ones all of it); of a packed 4:2:2 format the stride of its rows (a multiple of 4, v210: of 16).  Everything from ``--factor`` on is ``interp_y4m.py``'s."""
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
    ap.add_argument("--pix-fmt", required=True, choices=("nv12", "nv21", "p010le", "yuv420p", "yuv420p10le", "yuv422p", "yuv444p", "yuv422p10le", "yuv444p10le",
                                                           "uyvy422", "yuyv422", "y210le", "v210", "rgb48le", "bgr48le", "gbrp10le", "gbrp12le", "gbrp16le"))
    ap.add_argument("--size", required=True, metavar="WxH")
    ap.add_argument("--fps", required=True, metavar="R", help="the input's frame rate (e.g. 25 or 30000/1001)")
    ap.add_argument("--pitch", type=int, default=None, metavar="N", help="luma row stride of the input in bytes (default: tight)")
    ap.add_argument("--matrix", choices=("auto", "bt601", "bt709"), default="auto")
    ap.add_argument("--siting", choices=("centre", "left"), default="left", help="chroma siting (decoders deliver left-sited 4:2:0 and 4:2:2; 4:4:4 has none)")
    ap.add_argument("--full-range", action="store_true")
    ap.add_argument("--ckpt", default=None, help="checkpoint (the trainer's dict or a bare state dict); without one: synthetic weights")
    ap.add_argument("--model", choices=("base", "lite"), default="base")
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--scene", action="store_true", help="scene-cut detection (SceneCuts() defaults)")
    ap.add_argument("--tta", action="store_true", help="flip test-time augmentation of every produced frame")
    ap.add_argument("--global-off", action="store_true", help="switch the global motion branch off")
    ap.add_argument("--keep-depth", action="store_true", help="write 10-bit input back at 10 bits instead of 8")
    ap.add_argument("--active", action="store_true", help="run the network on the active picture of letterboxed video (ActiveArea() "
                    "defaults); 10-bit input needs --keep-depth")
    ap.add_argument("--fps-out", default=None, metavar="R", help="convert the frame rate to R (e.g. 60 or 60000/1001); --factor is ignored")
    ap.add_argument("--levels", type=int, default=3, help="with --fps-out: 2**L positions per segment (1..6)")
    ap.add_argument("--dedup", action="store_true", help="with --fps-out: drop repeated frames (Duplicates() defaults)")
    ap.add_argument("--shutter", default=None, metavar="ANGLE", help="with --fps-out: a synthetic shutter of ANGLE degrees (e.g. 180)")
    ap.add_argument("--light", choices=("code", "linear"), default="linear", help="with --shutter: the domain the samples are averaged in")
    ap.add_argument("--precision", choices=("f16x3", "f16", "f32"), default="f16x3", help="contraction arithmetic (Network.set_precision): f16x3 = the default, three 16-bit MFMAs per product; f16 = single-pass fp16 in the plane kernels (faster, about 1e-2 of the frame range); f32 = exact fp32 MFMA (about 2.5x slower)")
    ap.add_argument("--motion-scale", type=int, choices=(1, 2), default=1, help="2: half-resolution motion -- the network runs on 2x reduced frames, one kernel synthesises at full size (about 4x fewer network pixels; not with --shutter)")
    ap.add_argument("--interlaced", choices=("tff", "bff"), default=None, help="the input is woven interlaced video of this field order"
                    + ("") + ": it is deinterlaced to field rate first and the loop runs on that stream at twice the rate "
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
    try:
        w, h = (int(v) for v in a.size.lower().split("x"))
    except ValueError:
        ap.error(f"--size must be WxH (got {a.size!r})")
    yuv = importlib.import_module("atm-vfi_amd.yuv")
    siting = "centre" if a.pix_fmt.startswith("yuv444p") else a.siting
    if a.pix_fmt in yuv.PIX_FMTS_RGB:       # (tight RGB: no matrix, range or siting; what the loops refuse is refused before the model is made)
        try:
            surface = yuv.surface_of(a.pix_fmt, h, w, pitch=a.pitch)
            yuv.deep_rgb_refusals("interp_raw", surface, a.keep_depth, active=a.active or None, shutter=a.shutter)
        except ValueError as e:
            sys.exit(str(e))
    else:
        surface = yuv.surface_of(a.pix_fmt, h, w, pitch=a.pitch, matrix=a.matrix, siting=siting, full_range=a.full_range)
    if not torch.cuda.is_available():
        sys.exit("interp_raw: no GPU")
    pkg = importlib.import_module("atm-vfi_amd")
    torch.set_grad_enabled(False)
    net = pkg.NetworkBase() if a.model == "base" else pkg.NetworkLite()
    if a.ckpt:
        yuv.load_model_checkpoint(net, a.ckpt)
    else:
        print("interp_raw: no --ckpt: synthetic weights (the output is not a meaningful interpolation)", file=sys.stderr)
        net.load_state_dict(pkg.synthetic_state_dict(a.model, seed=1), strict=True)
    net = net.to(torch.device("cuda:0")).eval()
    net.global_motion = not a.global_off
    net.set_precision(a.precision)
    area = yuv.ActiveArea() if a.active else None
    src = sys.stdin.buffer if a.src == "-" else a.src
    dst = sys.stdout.buffer if a.dst == "-" else a.dst
    info = yuv.interpolate_raw(src, dst, net, surface, a.fps, factor=a.factor, scene=yuv.SceneCuts() if a.scene else None, tta=a.tta,
                               keep_depth=a.keep_depth, **({"active": area} if area is not None else {}),
                               **({"motion_scale": 2} if a.motion_scale == 2 else {}),
                               **(dict(interlaced=a.interlaced, deint=a.deint, deint_only=a.deint_only) if a.interlaced else {}),
                               **(dict(fps_out=a.fps_out, levels=a.levels, dedup=yuv.Duplicates() if a.dedup else None,
                                       shutter=yuv.Shutter(a.shutter, a.light) if a.shutter is not None else None) if a.fps_out else {}))
    print({k: (str(v) if k.startswith("fps") else v) for k, v in info.items()}, file=sys.stderr)
    if area is not None:
        print(f"interp_raw: active window (y0, x0, h, w) = {area.window} after {area.probed} frames, fallback_at = {area.fallback_at}", file=sys.stderr)


if __name__ == "__main__":
    main()
