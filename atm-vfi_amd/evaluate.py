"""Benchmark evaluation loops of the reference's scripts (benchmark/test_vimeo90k.py, test_ucf101.py, test_snufilm.py) on top of the
HIP hot path: dataset listers that read only files on disk, and ``evaluate`` -- PNG decode on a bounded thread pool, uint8 upload,
``frame_u8_to_f32`` (+ InputPadder replicate padding), the forward (flip-TTA optional, K forwards in flight optional) and the fused
metric kernel on the uint8 ground truth and the un-padded prediction view.  Per-sample values stay on the device until the end.

``evaluate_xiph`` is the fourth script (benchmark/test_xiph.py, 4096 x 2160 frames scored as "resized-2k" and "cropped-4k"): every PNG
is decoded and uploaded once, and every network input and ground truth of both categories is cut from the resident uint8 frame by
``frame_u8_window`` on the GPU.  A clip may also be the 4:2:0 Y4M file it is distributed as (``ROOT/<clip>.y4m`` or the download
name): its frames are read by one thread, uploaded as their I420 bytes, and ``yuv420_window`` makes the same inputs and ground truths
from the resident I420 frame -- no host decode and no RGB frame."""
from __future__ import annotations

import glob
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import host_io, metrics, yuv
from .metrics import PROTOCOLS, Protocol  # noqa: F401

SNU_LEVELS = ("test-easy", "test-medium", "test-hard", "test-extreme")
SNU_PREFIX = "data/SNU-FILM/test/"
XIPH_CLIPS = ("BoxingPractice", "Crosswalk", "DrivingPOV", "FoodMarket", "FoodMarket2", "RitualDance", "SquareAndTimelapse", "Tango")
XIPH_CATEGORIES = ("resized-2k", "cropped-4k")
XIPH_SOURCES = ("auto", "png", "y4m")


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


def xiph(path: str, clips=XIPH_CLIPS, frames=range(2, 99, 2)) -> List[Sample]:
    """One sample per (clip, middle frame n): <path>/<clip>/<n-1:03d>.png, <n:03d>.png, <n+1:03d>.png as (first, ground truth, last)
    (test_xiph.py:107-113), clip-major; both categories are cut from these same frames, so ``level`` is just "xiph".  Reads only the
    disk (the script's download step is not reproduced); a missing file raises FileNotFoundError naming it."""
    out = []
    for clip in clips:
        d = os.path.join(path, clip)
        for n in frames:
            fr = tuple(os.path.join(d, f"{k:03d}.png") for k in (n - 1, n, n + 1))
            for q in fr:
                if not os.path.isfile(q):
                    raise FileNotFoundError(f"Xiph frame {q} is missing")
            out.append(Sample(f"{clip}/{n:03d}", "xiph", fr))
    return out


def xiph_y4m_file(path: str, clip: str) -> Optional[str]:
    """The Y4M file of ``clip`` under ``path``: ``<path>/<clip>.y4m``, or the single match of ``<path>/*_<clip>_*.y4m`` (the download
    name, ``Netflix_<clip>_4096x2160_60fps_10bit_420.y4m``; the underscores keep FoodMarket from matching FoodMarket2).  None when
    there is none; two matches raise ``ValueError`` naming both."""
    plain = os.path.join(path, clip + ".y4m")
    if os.path.isfile(plain):
        return plain
    found = sorted(q for q in glob.glob(os.path.join(glob.escape(path), "*_" + glob.escape(clip) + "_*.y4m")) if os.path.isfile(q))
    if len(found) > 1:
        raise ValueError(f"Xiph clip {clip}: more than one Y4M file matches: {' and '.join(found)}")
    return found[0] if found else None


def xiph_sources(path: str, clips=XIPH_CLIPS, source: str = "auto") -> Dict[str, tuple]:
    """clip -> ("png", directory) or ("y4m", file).  ``source`` "auto" decides per clip: the directory ``<path>/<clip>/`` when it exists
    (the PNG tree), the clip's Y4M file (``xiph_y4m_file``) otherwise; "png" / "y4m" force one.  A clip that has neither raises
    ``FileNotFoundError`` naming both places looked in."""
    if source not in XIPH_SOURCES:
        raise ValueError(f"unknown Xiph source {source!r} (known: {', '.join(XIPH_SOURCES)})")
    out = {}
    for clip in clips:
        d = os.path.join(path, clip)
        if source == "png" or (source == "auto" and os.path.isdir(d)):
            out[clip] = ("png", d)
            continue
        f = xiph_y4m_file(path, clip)
        if f is None:
            y4m = f"no Y4M file {os.path.join(path, clip + '.y4m')} or {os.path.join(path, '*_' + clip + '_*.y4m')}"
            if source == "auto":        # (the PNG lister's words first: what a caller of the PNG-only evaluation saw)
                raise FileNotFoundError(f"Xiph frame {os.path.join(d, '001.png')} is missing (clip {clip}: no directory {d}{os.sep}), "
                                        f"and there is {y4m}")
            raise FileNotFoundError(f"Xiph clip {clip}: {y4m}")
        out[clip] = ("y4m", f)
    return out


def xiph_y4m(file: str, clip: str, frames=range(2, 99, 2)) -> List[Sample]:
    """``xiph``'s samples of one clip read from its Y4M file: a frame is (file, index) with PNG number k = stream frame k - 1 (ffmpeg's
    ``%03d`` starts at 001).  The stream's length is found out when it is read."""
    return [Sample(f"{clip}/{n:03d}", "xiph", tuple((file, k - 1) for k in (n - 1, n, n + 1))) for n in frames]


def xiph_samples(path: str, clips=XIPH_CLIPS, frames=range(2, 99, 2), source: str = "auto"):
    """(samples, {clip: "png" | "y4m"}): the triplets of ``clips`` in order, each clip from the source ``xiph_sources`` gives it --
    ``xiph`` for a PNG directory, ``xiph_y4m`` for a Y4M file.  What ``evaluate_xiph`` walks."""
    where = xiph_sources(path, tuple(clips), source)
    samples = []
    for c in clips:
        samples += xiph(path, (c,), frames) if where[c][0] == "png" else xiph_y4m(where[c][1], c, frames)
    return samples, {c: where[c][0] for c in clips}


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
                yield upload(i, frames)

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

    for i, pred in enumerate(_predictions(model, pairs(), tta, streams)):
        score(i, pred)

    vals = raw[:n].cpu().numpy()
    records = [{"name": s.name, "level": s.level, "psnr": metrics.psnr_from_mse(float(v[2])), "ssim": float(v[0])}
               for s, v in zip(samples, vals)]
    return EvalResult(records, _level_means(records), preds)


def _predictions(model, pairs, tta: bool, streams: int, timings: Optional[dict] = None):
    """``I_t`` of every (im0, im1) of ``pairs``, in order: flip-TTA as the scripts do it (the average with the un-flipped forward of the
    flipped pair), ``streams`` > 1 through ``host_io.PairStreams``.  ``timings``: adds the forwards' seconds (one stream only; it
    synchronises around each forward)."""
    def fed():
        for im0, im1 in pairs:
            yield im0, im1
            if tta:
                yield im0.flip(2).flip(3).contiguous(), im1.flip(2).flip(3).contiguous()

    def outputs():
        if streams > 1:
            with host_io.PairStreams(model, streams) as ps:
                yield from (o["I_t"] for o in ps.map(fed()))
        else:
            for a, b in fed():
                if timings is None:
                    yield model.forward(a, b)["I_t"]
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.forward(a, b)["I_t"]
                torch.cuda.synchronize()
                timings["forward"] = timings.get("forward", 0.0) + time.perf_counter() - t0
                yield out

    it = outputs()
    for pred in it:         # (exhausting the generator releases the streams)
        if tta:
            pred = (pred + next(it).flip(2).flip(3)) / 2
        yield pred


def _level_means(records) -> Dict[str, dict]:
    levels: Dict[str, dict] = {}
    for r in records:
        lv = levels.setdefault(r["level"], {"psnr": [], "ssim": []})
        lv["psnr"].append(r["psnr"])
        lv["ssim"].append(r["ssim"])
    return {k: {"psnr": float(np.mean(v["psnr"])), "ssim": float(np.mean(v["ssim"])), "n": len(v["psnr"])} for k, v in levels.items()}


def xiph_geometry(height: int, width: int, category: str):
    """(mode, y0, x0, h, w) of ``frame_u8_window`` for one category on H x W frames: "resized-2k" = the whole frame reduced 2x
    (cv2.resize to (W/2, H/2), INTER_AREA), "cropped-4k" = rows [H/4, H - H/4), columns [W/4, W - W/4).  For 2160 x 4096 these are the
    script's dsize=(2048, 1080) and [540:-540, 1024:-1024]."""
    if height <= 0 or width <= 0 or height % 4 or width % 4:
        raise ValueError(f"Xiph frames must have H % 4 == 0 and W % 4 == 0 (the 2x resize and the centre crop are exact then), got {height}x{width}")
    if category == "resized-2k":
        return 1, 0, 0, height // 2, width // 2
    if category == "cropped-4k":
        return 0, height // 4, width // 4, height - 2 * (height // 4), width - 2 * (width // 4)
    raise ValueError(f"unknown Xiph category {category!r} (known: {', '.join(XIPH_CATEGORIES)})")


def _upload_i420(frame: np.ndarray, dev) -> torch.Tensor:
    """One I420 frame as read (uint8, or uint16 for 10 bit) -> its bytes on the device."""
    return torch.from_numpy(frame.view(np.uint8)).to(dev)


def _y4m_jobs(samples) -> List[tuple]:
    """[(clip, file, frame indices)] for the reader thread: the distinct Y4M frames of ``samples`` in the order of their first use,
    one job per file.  A stream is walked forward exactly once, so the first uses of a file's frames must ascend and a file must not
    be come back to after another one: anything else (a descending ``frames`` range, a clip named twice with another one in between)
    raises ``ValueError`` here, before anything is read."""
    jobs: List[list] = []
    seen, done = set(), set()
    for s in samples:
        for q in s.frames:
            if isinstance(q, str) or q in seen:
                continue
            seen.add(q)
            clip = s.name.split("/")[0]
            if q[1] < 0:
                raise ValueError(f"{s.name}: frame numbers start at 001 (stream frame {q[1]} wanted)")
            if not jobs or jobs[-1][1] != q[0]:
                if q[0] in done:
                    raise ValueError(f"{s.name}: the Y4M file {q[0]} is wanted again after another clip; a stream is read forward once")
                done.add(q[0])
                jobs.append([clip, q[0], []])
            if jobs[-1][2] and jobs[-1][2][-1] >= q[1]:
                raise ValueError(f"{s.name}: stream frame {q[1]} (PNG number {q[1] + 1:03d}) is wanted after frame {jobs[-1][2][-1]}; a Y4M "
                                 f"clip is read forward once, so `frames` must ascend (a PNG tree takes any order)")
            jobs[-1][2].append(q[1])
    return [tuple(j) for j in jobs]


_FEED_END = object()         # the reader thread's last word: nothing more will come


class _Y4MFeed:
    """The reader thread of ``evaluate_xiph``: walks each clip's stream forward exactly once, in the order the frames are wanted, and
    hands them over through a bounded queue.  ``jobs``: [(clip, file, sorted frame indices)].  Unneeded frames are skipped
    (``Y4MReader.skip``: a seek when the file is seekable), nothing is read after a clip's last needed frame."""

    def __init__(self, jobs, matrix: str, depth: int = 3):
        self.jobs, self.matrix = jobs, matrix
        self.q: "queue.Queue" = queue.Queue(maxsize=depth)
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._run, name="xiph-y4m-reader", daemon=True)
        self.thread.start()

    def _put(self, item) -> bool:
        while not self.stop.is_set():
            try:
                self.q.put(item, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def _run(self):
        try:
            for clip, file, wanted in self.jobs:
                with yuv.Y4MReader(file, matrix=self.matrix) as rd:
                    fmt = rd.fmt
                    if fmt.height % 8 or fmt.width % 8:
                        raise ValueError(f"Xiph clip {clip} ({file}): Y4M frames must have H % 8 == 0 and W % 8 == 0 (the centre-crop origin "
                                         f"of a 4:2:0 frame must be even), got {fmt.height}x{fmt.width}")
                    it, pos = iter(rd), 0
                    for k in wanted:
                        t0 = time.perf_counter()
                        pos += rd.skip(k - pos)
                        fr = next(it, None) if pos == k else None
                        if fr is None:
                            raise ValueError(f"Xiph clip {clip} ({file}): frame {k} (PNG number {k + 1:03d}) wanted, the stream has only "
                                             f"{pos} frames")
                        pos += 1
                        if not self._put(((file, k), fr, fmt, time.perf_counter() - t0)):
                            return
            self._put(_FEED_END)
        except BaseException as e:          # handed to the consumer, which raises it
            self._put(e)

    def get(self, key):
        item = self.q.get()
        if isinstance(item, BaseException):
            raise item
        if item is _FEED_END:               # (stays the last word for any later call)
            self.q.put(item)
            raise RuntimeError(f"evaluate_xiph: {key} was wanted after the reader had delivered every frame of its jobs")
        if item[0] != key:
            raise RuntimeError(f"evaluate_xiph: the reader delivered {item[0]} where {key} was wanted")
        return item[1:]

    def close(self):
        self.stop.set()
        self.thread.join()


def evaluate_xiph(model, path: str, *, categories=XIPH_CATEGORIES, clips=XIPH_CLIPS, frames=range(2, 99, 2), tta: bool = False,
                  streams: int = 1, limit: Optional[int] = None, keep_predictions: bool = False, global_motion: Optional[bool] = None,
                  progress=None, decode_workers: int = 8, timings: Optional[dict] = None, source: str = "auto", matrix: str = "auto",
                  sources: Optional[dict] = None) -> EvalResult:
    """benchmark/test_xiph.py on the HIP hot path: ``model`` scored on the triplets of ``xiph(path, clips, frames)`` under
    ``metrics.XIPH``, once per category (calculate_psnr / calculate_ssim on frames in [0, 1]: the script detects SSIM's value range on the
    prediction, the metric kernel on the ground truth; both lie in [0, 1], so L = 1 either way).  ``levels`` is keyed by category;
    ``records`` (and ``predictions``) come category-major, then clip, then frame, as the script walks them; ``limit`` counts triplets
    per category.

    The work is done triplet-major: every PNG is decoded once and uploaded once however many triplets and categories use it, and at
    most the three uint8 frames of the current triplet are resident (a frame is dropped after its last use; decoded frames wait on the
    host, ``decode_workers`` + 3 at most).  Inputs and ground truths come from ``frame_u8_window`` alone -- mode 1 on the whole frame
    for "resized-2k", mode 0 on the centre window for "cropped-4k" -- the ground truth as its uint8 output, which the metric kernel
    reads in place.  ``tta``, ``streams``, ``keep_predictions``, ``global_motion`` as in ``evaluate``; ``progress`` is called after
    every 100 forwards with (done, total, running psnr, running ssim) over what has been scored.
    ``timings``: a dict that receives the seconds spent in decode_wait (this thread blocked on the decoders), decode_cpu (summed over
    the decoder threads), upload, prepare, forward and metric; it synchronises after every stage, so use it with ``streams`` = 1.

    ``source`` ("auto", "png", "y4m"; ``xiph_sources``): where a clip's frames come from -- "auto" takes the directory
    ``path/<clip>/`` when it exists (everything above, unchanged) and the clip's Y4M file otherwise.  From a Y4M file (8- or 10-bit
    4:2:0; PNG number k is stream frame k - 1) one reader thread walks the stream forward once, skipping what no triplet needs; every
    needed frame is read once and uploaded once as its I420 bytes, at most three are resident, and every input and ground truth is
    one ``yuv420_window`` call on the resident I420 frame with ``xiph_geometry``'s mode and window -- no RGB frame exists on the
    device.  The pixels are ``yuv.decode_numpy``'s (this project's colour conversion, not swscale's).  ``matrix``: the Y4M reader's
    ("auto": bt709 from 720 rows up).  Y4M frames need H % 8 == 0 and W % 8 == 0; a stream shorter than the frames wanted raises
    ``ValueError``, and so does -- before anything is read -- a ``frames`` order in which a Y4M clip's frames do not ascend (a stream
    is read forward once; a PNG tree takes any order).  decode_wait is then this thread blocked on the reader and decode_cpu the reader thread's time.
    ``sources``: a dict that receives {clip: "png" | "y4m"}."""
    p = metrics.XIPH
    ops, dev = host_io._hip_ops_of(model)
    if ops is None:
        raise RuntimeError("evaluate_xiph needs an atm-vfi_amd Network on the GPU (model.to('cuda'))")
    categories = tuple(categories)
    for c in categories:
        if c not in XIPH_CATEGORIES:
            raise ValueError(f"unknown Xiph category {c!r} (known: {', '.join(XIPH_CATEGORIES)})")
    samples, where = xiph_samples(path, tuple(clips), frames, source)
    if sources is not None:
        sources.update(where)
    samples = samples[:limit] if limit is not None else samples
    n, nc = len(samples), len(categories)
    model.global_motion = p.global_motion if global_motion is None else bool(global_motion)
    raw = torch.zeros(max(n * nc, 1), 3, dtype=torch.float64, device=dev)        # (ssim, cs, mse), row = category * n + triplet
    preds: Optional[List[Optional[torch.Tensor]]] = [None] * (n * nc) if keep_predictions else None
    gts: Dict[int, torch.Tensor] = {}
    padders: Dict[int, host_io.InputPadder] = {}
    order: List = []                           # the distinct frames in order of first use, and how many triplets use each
    uses: Dict = {}                            # (a frame is a PNG path, or (Y4M file, stream index))
    for s in samples:
        for q in s.frames:
            if q not in uses:
                order.append(q)
            uses[q] = uses.get(q, 0) + 1
    png_order = [q for q in order if isinstance(q, str)]
    y4m_jobs = _y4m_jobs(samples)

    def clock(key, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[key] = timings.get(key, 0.0) + time.perf_counter() - t0

    def decode(q):
        t0 = time.perf_counter()
        fr = read_rgb(q)
        return fr, time.perf_counter() - t0

    def prepare(fr, cat, want_gt):
        """One category's view of one resident frame: the padded fp32 input [1,3,Hp,Wp], or the uint8 ground truth [h,w,3].  ``fr``: a
        uint8 [H,W,3] frame (frame_u8_window), or (I420 bytes, format) (yuv420_window)."""
        if isinstance(fr, tuple):
            window = lambda mode, y0, x0, h, w, **kw: ops.yuv420_window(fr[0], fr[1], mode, y0, x0, h, w, **kw)      # noqa: E731
            height, width = fr[1].height, fr[1].width
        else:
            window = lambda mode, y0, x0, h, w, **kw: ops.frame_u8_window(fr, mode, y0, x0, h, w, **kw)             # noqa: E731
            height, width = fr.shape[0], fr.shape[1]
        mode, y0, x0, h, w = xiph_geometry(height, width, cat)
        if want_gt:
            gt = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
            window(mode, y0, x0, h, w, dst_u8=gt)
            return gt
        padder = host_io.InputPadder((h, w), divisor=p.divisor)
        left, right, top, bottom = padder._pad
        t = torch.empty(3, h + top + bottom, w + left + right, dtype=torch.float32, device=dev)
        window(mode, y0, x0, h, w, dst=t, pad_top=top, pad_left=left)
        return t.unsqueeze(0), padder

    def size_of(fr):
        return (fr[1].height, fr[1].width) if isinstance(fr, tuple) else tuple(fr.shape[:2])

    def pairs():
        resident: Dict = {}
        workers = max(1, min(16, decode_workers))
        feed = _Y4MFeed(y4m_jobs, matrix) if y4m_jobs else None
        try:
            with ThreadPoolExecutor(max_workers=workers) as pool:
                futs, nxt = {}, 0
                for i, s in enumerate(samples):
                    for q in s.frames:
                        if q in resident:
                            continue
                        if not isinstance(q, str):          # a Y4M frame: the reader thread delivers them in this very order
                            t0 = time.perf_counter()
                            fr, fmt, dt = feed.get(q)
                            if timings is not None:
                                timings["decode_wait"] = timings.get("decode_wait", 0.0) + time.perf_counter() - t0
                                timings["decode_cpu"] = timings.get("decode_cpu", 0.0) + dt
                            t0 = time.perf_counter()
                            resident[q] = (_upload_i420(fr, dev), fmt)
                            clock("upload", t0)
                            continue
                        while nxt < len(png_order) and len(futs) < workers + 3:        # (png_order[nxt:] always starts at or before q)
                            futs[png_order[nxt]] = pool.submit(decode, png_order[nxt])
                            nxt += 1
                        t0 = time.perf_counter()
                        fr, dt = futs.pop(q).result()
                        if timings is not None:
                            timings["decode_wait"] = timings.get("decode_wait", 0.0) + time.perf_counter() - t0
                            timings["decode_cpu"] = timings.get("decode_cpu", 0.0) + dt
                        if fr.ndim != 3 or fr.shape[2] != 3:
                            raise ValueError(f"{q}: expected an RGB frame, got shape {fr.shape}")
                        xiph_geometry(fr.shape[0], fr.shape[1], XIPH_CATEGORIES[0])
                        t0 = time.perf_counter()
                        resident[q] = torch.from_numpy(fr).to(dev)
                        clock("upload", t0)
                    f0, gt, f2 = (resident[q] for q in s.frames)
                    if size_of(f0) != size_of(gt) or size_of(f2) != size_of(gt):
                        raise ValueError(f"{s.name}: the three frames differ in size")
                    for ci, cat in enumerate(categories):
                        t0 = time.perf_counter()
                        (im0, padder), (im1, _) = prepare(f0, cat, False), prepare(f2, cat, False)
                        gts[ci * n + i], padders[ci * n + i] = prepare(gt, cat, True), padder
                        clock("prepare", t0)
                        yield im0, im1
                    for q in s.frames:          # drop what no later triplet reads (the kernels above are queued on this stream already)
                        uses[q] -= 1
                        if uses[q] == 0:
                            del resident[q]
        finally:
            if feed is not None:
                feed.close()

    done = 0
    for k, pred in enumerate(_predictions(model, pairs(), tta, streams, timings)):
        i, ci = divmod(k, nc)
        row = ci * n + i
        t0 = time.perf_counter()
        pred = padders.pop(row).unpad(pred)
        metrics.ssim_psnr_raw(pred, gts.pop(row), round_pred=p.round_pred, mse_f32=p.mse_f32, out=raw[row:row + 1])
        clock("metric", t0)
        if preds is not None:
            preds[row] = pred[0].clone()
        done += 1
        if progress is not None and done % 100 == 0:
            rows = [c * n + j for j in range(i + 1) for c in range(nc) if j < i or c <= ci]
            r = raw[rows].cpu()
            progress(done, n * nc, float(np.mean([metrics.psnr_from_mse(v) for v in r[:, 2].tolist()])), float(r[:, 0].mean()))

    vals = raw[:n * nc].cpu().numpy()
    records = [{"name": s.name, "level": cat, "psnr": metrics.psnr_from_mse(float(vals[ci * n + i][2])), "ssim": float(vals[ci * n + i][0])}
               for ci, cat in enumerate(categories) for i, s in enumerate(samples)]
    return EvalResult(records, _level_means(records), preds)


def format_levels(result: EvalResult) -> str:
    """The scripts' closing lines: ``Avg PSNR: … SSIM: …`` per dataset or level (SNU-FILM: preceded by ``Testing level:<name>``)."""
    lines = []
    for name, v in result.levels.items():
        if name.startswith("test-"):
            lines.append("Testing level:" + name)
        if name in XIPH_CATEGORIES:
            lines.append("{}  Avg PSNR: {} SSIM: {}".format(name, v["psnr"], v["ssim"]))
            continue
        lines.append("Avg PSNR: {} SSIM: {}".format(v["psnr"], v["ssim"]))
    return "\n".join(lines)


__all__ = ["Sample", "vimeo90k", "ucf101", "snufilm", "xiph", "xiph_y4m", "xiph_y4m_file", "xiph_sources", "xiph_samples", "XIPH_SOURCES", "LISTERS", "read_rgb", "evaluate", "evaluate_xiph", "xiph_geometry",
           "EvalResult", "format_levels", "PROTOCOLS", "SNU_LEVELS", "XIPH_CLIPS", "XIPH_CATEGORIES"]
