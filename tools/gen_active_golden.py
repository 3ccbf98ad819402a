#!/usr/bin/env python3
"""Make tests/golden/active_ref.npz, the fixture the ``peak`` default of atm-vfi_amd/active.py is placed from (README "Active picture";
tests/test_active_cpu.py asserts the margins): the five 300 x 207 pictures of tests/golden/scene_ref.npz, each in a letterbox +
pillarbox canvas (bars of 40 rows above and below, 37 columns left and right) at black 0 and at black 16 (lifted black), re-encoded with
PIL's JPEG encoder at quality 95, 90 and 75 and decoded again -- what bars and picture edges look like after a lossy codec.  Reads
nothing but scene_ref.npz.

Stored per picture, black level and quality: ``<name>.b<black>.q<Q>`` = decoded - canvas as int8 (the tool asserts the range), not the
decoded uint8 canvases, and only where a statistic reads it: the bars and the picture's outermost RING = 8 rows and columns.  The
picture's interior is stored as zero (there ``decoded_canvases()`` gives the undistorted picture): the thirty full residuals deflate
to 2.9 MB, over the 1 MiB a committed file may have, these to 0.63 MB.  Both statistics are unchanged by that, by construction: a bar
line at least 8 lines from the picture lies in the bars, and each of the picture's outermost 8 rows and columns lies, over its whole
length, inside the ring.  ``tests/cpu_active.decoded_canvases()`` adds the canvas back.

    python tools/gen_active_golden.py [--check]        # --check: decode again and compare with the committed file (same PIL / libjpeg only)"""
import argparse
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cpu_active as A  # noqa: E402

DST = A.ACTIVE_REF
RING = A.KEEP            # rows and columns of the picture's edge whose residual is kept: what the statistics read


def residuals(full: bool = False):
    from PIL import Image
    out = {}
    for name, pic in A.cpu_scene.pictures().items():
        for black in A.BLACKS:
            base = A.canvas(pic, black)
            for q in A.QUALITIES:
                buf = io.BytesIO()
                Image.fromarray(base).save(buf, format="JPEG", quality=q)
                buf.seek(0)
                dec = np.asarray(Image.open(buf).convert("RGB"))
                diff = dec.astype(np.int16) - base.astype(np.int16)
                assert dec.shape == base.shape and np.abs(diff).max() <= 127, (name, black, q, int(np.abs(diff).max()))
                if not full:
                    diff[A.BAR_ROWS + RING:base.shape[0] - A.BAR_ROWS - RING, A.BAR_COLS + RING:base.shape[1] - A.BAR_COLS - RING] = 0
                out[f"{name}.b{black}.q{q}"] = diff.astype(np.int8)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    out = residuals()
    if a.check:
        z = np.load(DST)
        bad = [k for k in out if k not in z.files or not np.array_equal(z[k], out[k])]
        print("active_ref.npz:", "reproduced" if not bad else f"differs in {bad} (another JPEG library?)")
        sys.exit(1 if bad else 0)
    np.savez_compressed(DST, **out)
    print(f"wrote {DST}: {len(out)} arrays, {os.path.getsize(DST)} bytes")


if __name__ == "__main__":
    main()
