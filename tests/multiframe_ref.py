"""Shared by the multi-frame tests and ``tools/gen_nx_golden.py``: the fixture's case table, the recursion of
``benchmark/davis-vid.py:102-112`` over any ``forward(im0, im1) -> I_t`` callable, and NumPy models of the three kernels of
``atm-vfi_amd/csrc/multiframe.hip``."""
import importlib
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_REF = os.path.join(ROOT, "tests", "golden", "nx_ref.npz")

# (name, variant, H, W, global, depth (factor = 2^depth), tta, input seed, store step)
NX_CASES = [
    ("lite_64x96_g_d3", "lite", 64, 96, True, 3, False, 51, 1),
    ("base_128x192_g_d2", "base", 128, 192, True, 2, False, 52, 2),
    ("lite_128x192_nog_d2_tta", "lite", 128, 192, False, 2, True, 53, 2),
]


def nx_levels(factor):
    return importlib.import_module("atm-vfi_amd.multiframe").nx_levels(factor)


def chain(forward, im0, im1, factor, tta=False, given=None):
    """The script's recursion: ``forward(a, b)`` -> I_t [1,3,H,W]; level 1 from the two frames, deeper levels from the UNROUNDED
    predictions.  Returns ``(pred, shown)``: position -> [1,3,H,W]; ``shown`` is the flip-TTA average of every produced frame when
    ``tta`` (else ``pred`` itself); the next level always consumes ``pred`` (davis-vid.py:102-112).  ``given``: position -> frame to
    use as a deeper level's INPUT instead of this chain's own prediction (one forward from the reference's frames)."""
    fr = {0: im0, factor: im1}
    pred, shown = {}, {}
    for level in nx_levels(factor):
        for a, b, o in level:
            p = forward(fr[a], fr[b])
            pred[o] = p
            if tta:
                pf = forward(fr[a].flip(2).flip(3).contiguous(), fr[b].flip(2).flip(3).contiguous())
                shown[o] = (p + pf.flip(2).flip(3)) / 2
            else:
                shown[o] = p
            fr[o] = p if given is None or o not in given else given[o]
    return pred, shown


# ---------------------------------------------------------------------------------------------- NumPy models of the kernels
def pool_blocks_model(pool, slots, buf=None, block_elems=None):
    """Gather (``buf`` None): -> [n, block_elems] = the first block_elems elements of pool[slots[j]]; scatter: writes ``buf`` blocks into
    a copy of ``pool`` (a slot named twice is an error) and returns it."""
    flat = pool.reshape(pool.shape[0], -1)
    be = flat.shape[1] if block_elems is None else block_elems
    if buf is None:
        return np.stack([flat[s, :be] for s in slots], 0)
    if len(set(slots)) != len(slots):
        raise ValueError("scatter names a slot twice")
    out = flat.copy()
    for j, s in enumerate(slots):
        out[s, :be] = buf.reshape(len(slots), -1)[j]
    return out.reshape(pool.shape)


def rot180_model(x):
    """flip(H).flip(W) of [...,H,W] = the flattened reversal of every plane."""
    sh = x.shape
    return x.reshape(-1, sh[-2] * sh[-1])[:, ::-1].reshape(sh).copy()


def f32_to_u8_model(x, pad_top, pad_left, h, w, bgr):
    """frame_f32_to_u8: crop, x * 255 in fp32, round half to even, clamp, [H,W,3], optional RGB -> BGR."""
    c = x[:, pad_top:pad_top + h, pad_left:pad_left + w].astype(np.float32) * np.float32(255.0)
    q = np.clip(np.rint(c), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    return q[:, :, ::-1].copy() if bgr else q.copy()


def tta_merge_model(pred, pred_flip, pad_top=0, pad_left=0, h=None, w=None, bgr=False):
    """-> (out fp32 [3,Hp,Wp], out_u8 [H,W,3])."""
    out = ((pred.astype(np.float32) + rot180_model(pred_flip.astype(np.float32))) / np.float32(2.0)).astype(np.float32)
    h = pred.shape[1] - pad_top if h is None else h
    w = pred.shape[2] - pad_left if w is None else w
    return out, f32_to_u8_model(out, pad_top, pad_left, h, w, bgr)


def case_inputs(case):
    import pairs
    _, _, h, w, _, _, _, seed, _ = case
    return pairs.smooth_pair(1, h, w, seed)


def ref_frames(gold, name, factor, what="pred", full_only=False):
    """position -> stored array of a case ([1,3,H/step,W/step])."""
    return {p: gold[f"{name}.{what}.{p}"] for p in range(1, factor)}
