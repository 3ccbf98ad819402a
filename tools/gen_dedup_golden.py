#!/usr/bin/env python3
"""Make tests/golden/dedup_ref.npz, the fixture the duplicate thresholds of atm-vfi_amd/retime.py are placed from (README "Frame-rate
conversion"; tests/test_retime_cpu.py asserts the margins): the five pictures of tests/golden/scene_ref.npz re-encoded with PIL's JPEG
encoder at quality 95 and 90 and decoded again -- what a repeated frame looks like after a lossy codec.  Reads nothing but
scene_ref.npz.

Stored per picture and quality: ``<name>.q<Q>`` = decoded - original as int8 (the residual of a q90 re-encode stays within +-127; the
tool asserts it), not the decoded uint8 array itself: the ten decoded arrays deflate to 1.3 MB, over the 1 MiB a committed file may
have, their residuals to 0.84 MB.  ``tests/cpu_framediff.reencodes()`` adds the original back: the decoded array, bit for bit.

    python tools/gen_dedup_golden.py [--check]        # --check: decode again and compare with the committed file (same PIL / libjpeg only)"""
import argparse
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "golden", "scene_ref.npz")
DST = os.path.join(ROOT, "tests", "golden", "dedup_ref.npz")
QUALITIES = (95, 90)


def residuals():
    from PIL import Image
    z = np.load(SRC)
    out = {}
    for name in z.files:
        pic = z[name]
        for q in QUALITIES:
            buf = io.BytesIO()
            Image.fromarray(pic).save(buf, format="JPEG", quality=q)
            buf.seek(0)
            dec = np.asarray(Image.open(buf).convert("RGB"))
            diff = dec.astype(np.int16) - pic.astype(np.int16)
            assert dec.shape == pic.shape and np.abs(diff).max() <= 127, (name, q, int(np.abs(diff).max()))
            out[f"{name}.q{q}"] = diff.astype(np.int8)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    out = residuals()
    if a.check:
        z = np.load(DST)
        bad = [k for k in out if k not in z.files or not np.array_equal(z[k], out[k])]
        print("dedup_ref.npz:", "reproduced" if not bad else f"differs in {bad} (another JPEG library?)")
        sys.exit(1 if bad else 0)
    np.savez_compressed(DST, **out)
    print(f"wrote {DST}: {len(out)} arrays, {os.path.getsize(DST)} bytes")


if __name__ == "__main__":
    main()
