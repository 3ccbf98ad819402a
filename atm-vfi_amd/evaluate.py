"""Benchmark evaluation loops of the reference's scripts (benchmark/test_vimeo90k.py, test_ucf101.py, test_snufilm.py) on top of the
HIP hot path: dataset listers that read only files on disk, and ``evaluate`` -- PNG decode on a bounded thread pool, uint8 upload,
``frame_u8_to_f32`` (+ InputPadder replicate padding), the forward (flip-TTA optional, K forwards in flight optional) and the fused
metric kernel on the uint8 ground truth and the un-padded prediction view.  Per-sample values stay on the device until the end."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import host_io, metrics
from .metrics import PROTOCOLS, Protocol  # noqa: F401

SNU_LEVELS = ("test-easy", "test-medium", "test-hard", "test-extreme")
SNU_PREFIX = "data/SNU-FILM/test/"


@dataclass(frozen=True)
class Sample:
    name: str
    level: str
    frames: tuple        # (first frame, ground truth, last frame) paths


def vimeo90k(path: str) -> List[Sample]:
    """``tri_testlist.txt`` -> sequences/<name>/im{1,2,3}.png (test_vimeo90k.py:82-95; lines of one character or less are skipped)."""
    out = []
    with open(os.path.join(path, "tri_testlist.txt")) as f:
        for line in f:
            name = line.strip()
            if len(name) <= 1:
                continue
            d = os.path.join(path, "sequences", name)
            out.append(Sample(name, "vimeo90k", (os.path.join(d, "im1.png"), os.path.join(d, "im2.png"), os.path.join(d, "im3.png"))))
    return out


def ucf101(path: str) -> List[Sample]:
    """Every directory holding frame_00.png, frame_01_gt.png and frame_02.png, sorted by name (the reference walks os.listdir order;
    sorted keeps runs reproducible)."""
    out = []
    for d in sorted(os.listdir(path)):
        fr = tuple(os.path.join(path, d, f) for f in ("frame_00.png", "frame_01_gt.png", "frame_02.png"))
        if all(os.path.isfile(p) for p in fr):
            out.append(Sample(d, "ucf101", fr))
    return out


def snufilm(path: str, img_data_path: str) -> List[Sample]:
    """The four lists ``test-{easy,medium,hard,extreme}.txt`` under ``path``; each line names three frames, with the reference's
    rewrite of the ``data/SNU-FILM/test/`` prefix to ``img_data_path`` (test_snufilm.py:111-123).  Each list is its own level."""
    out = []
    for level in SNU_LEVELS:
        with open(os.path.join(path, level + ".txt")) as f:
            for line in f:
                parts = line.replace(SNU_PREFIX, img_data_path).strip().split(" ")
                if len(parts) < 3:
                    continue
                fr = tuple(os.path.join(path, p) for p in parts[:3])
                out.append(Sample(parts[1], level, fr))
    return out


LISTERS = {"vimeo90k": vimeo90k, "ucf101": ucf101, "snufilm": snufilm}


def read_rgb(path: str) -> np.ndarray:
    """uint8 [H,W,3] RGB: the 8-bit pixels of cv2.imread + the scripts' BGR -> RGB flip."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


@dataclass
class EvalResult:
    records: List[dict]                          # per sample: name, level, psnr, ssim
    levels: Dict[str, dict]                      # per level: psnr, ssim (means), n
    predictions: Optional[List[torch.Tensor]] = field(default=None)    # un-padded I_t [3,H,W] per sample (keep_predictions)


def evaluate(model, samples, protocol, *, tta: bool = False, streams: int = 1, limit: Optional[int] = None,
             keep_predictions: bool = False, global_motion: Optional[bool] = None, progress=None, decode_workers: int = 8) -> EvalResult:
    """Score ``model`` (an atm-vfi_amd Network on the GPU) on ``samples`` (a lister's output) under ``protocol`` (a PROTOCOLS name or
    a ``Protocol``).  The model's ``global_motion`` (and for SNU-FILM ``ensemble_global_motion``) are set as the script sets them,
    ``global_motion`` overrides.  ``streams`` > 1 keeps that many forwards in flight (host_io.PairStreams; per-sample results are
    identical to one stream).  ``progress``: a callable (done, total, running psnr, running ssim) called every 100 samples (one
    device read each)."""
    p = PROTOCOLS[protocol] if isinstance(protocol, str) else protocol
    ops, dev = host_io._hip_ops_of(model)
    if ops is None:
        raise RuntimeError("evaluate needs an atm-vfi_amd Network on the GPU (model.to('cuda'))")
    samples = list(samples)[:limit] if limit is not None else list(samples)
    n = len(samples)
    model.global_motion = p.global_motion if global_motion is None else bool(global_motion)
    if p.ensemble_global_motion is not None:
        model.ensemble_global_motion = p.ensemble_global_motion
    raw = torch.zeros(max(n, 1), 3, dtype=torch.float64, device=dev)        # (ssim, cs, mse) per sample
    preds: Optional[List[torch.Tensor]] = [] if keep_predictions else None
    gts: Dict[int, torch.Tensor] = {}
    padders: Dict[int, host_io.InputPadder] = {}

    def upload(i, frames):
        """uint8 frames -> device; the two inputs through frame_u8_to_f32 (/ 255 + replicate padding) as [1,3,Hp,Wp]."""
        f0, gt, f2 = frames
        h, w = f0.shape[:2]
        padder = host_io.InputPadder((h, w), divisor=p.divisor) if p.divisor else None
        hp, wp = (padder.ht + sum(padder._pad[2:]), padder.wd + sum(padder._pad[:2])) if padder else (h, w)
        top, left = (padder._pad[2], padder._pad[0]) if padder else (0, 0)
        ims = []
        for fr in (f0, f2):
            u8 = torch.from_numpy(fr).to(dev, non_blocking=False)
            t = torch.empty(3, hp, wp, dtype=torch.float32, device=dev)
            ops.frame_u8_to_f32(u8, t, top, left, False)
            ims.append(t.unsqueeze(0))
        gts[i] = torch.from_numpy(gt).to(dev)
        padders[i] = padder
        return ims

    def pairs():
        with ThreadPoolExecutor(max_workers=max(1, min(16, decode_workers))) as pool:
            window = 2 * max(1, min(16, decode_workers))
            futs = {}
            for j in range(min(window, n)):
                futs[j] = pool.submit(lambda s: tuple(read_rgb(q) for q in s.frames), samples[j])
            for i in range(n):
                frames = futs.pop(i).result()
                if i + window < n:
                    futs[i + window] = pool.submit(lambda s: tuple(read_rgb(q) for q in s.frames), samples[i + window])
                im0, im1 = upload(i, frames)
                yield im0, im1
                if tta:
                    yield im0.flip(2).flip(3).contiguous(), im1.flip(2).flip(3).contiguous()

    def score(i, pred):
        padder = padders.pop(i)
        if padder is not None:
            pred = padder.unpad(pred)
        metrics.ssim_psnr_raw(pred, gts.pop(i), round_pred=p.round_pred, mse_f32=p.mse_f32, out=raw[i:i + 1])
        if preds is not None:
            preds.append(pred[0].clone())
        if progress is not None and (i + 1) % 100 == 0:
            r = raw[:i + 1].cpu()
            progress(i + 1, n, float(np.mean([metrics.psnr_from_mse(v) for v in r[:, 2].tolist()])), float(r[:, 0].mean()))

    def outputs():
        if streams > 1:
            with host_io.PairStreams(model, streams) as ps:
                yield from (o["I_t"] for o in ps.map(pairs()))
        else:
            for a, b in pairs():
                yield model.forward(a, b)["I_t"]

    it = outputs()
    for i in range(n):
        pred = next(it)
        if tta:
            pred = (pred + next(it).flip(2).flip(3)) / 2
        score(i, pred)
    for _ in it:        # close the generator (releases the streams)
        pass

    vals = raw[:n].cpu().numpy()
    records = [{"name": s.name, "level": s.level, "psnr": metrics.psnr_from_mse(float(v[2])), "ssim": float(v[0])}
               for s, v in zip(samples, vals)]
    levels: Dict[str, dict] = {}
    for r in records:
        lv = levels.setdefault(r["level"], {"psnr": [], "ssim": []})
        lv["psnr"].append(r["psnr"])
        lv["ssim"].append(r["ssim"])
    levels = {k: {"psnr": float(np.mean(v["psnr"])), "ssim": float(np.mean(v["ssim"])), "n": len(v["psnr"])} for k, v in levels.items()}
    return EvalResult(records, levels, preds)


def format_levels(result: EvalResult) -> str:
    """The scripts' closing lines: ``Avg PSNR: … SSIM: …`` per dataset or level (SNU-FILM: preceded by ``Testing level:<name>``)."""
    lines = []
    for name, v in result.levels.items():
        if name.startswith("test-"):
            lines.append("Testing level:" + name)
        lines.append("Avg PSNR: {} SSIM: {}".format(v["psnr"], v["ssim"]))
    return "\n".join(lines)


__all__ = ["Sample", "vimeo90k", "ucf101", "snufilm", "LISTERS", "read_rgb", "evaluate", "EvalResult", "format_levels", "PROTOCOLS",
           "SNU_LEVELS"]
