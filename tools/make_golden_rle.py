"""Writes tests/golden/g13_rle.npz: a handful of binary masks and the strings the reference's mask2rle (utilities/utilities.py:36-45)
produces for them.  The reference is imported HERE, at generation time, never by a test:

    python tools/make_golden_rle.py --reference /path/to/the/reference/checkout

Masks: a blobby 200 x 200 one (the reference's NEU-Seg plane size), an empty, a full, a single pixel, a run that ends at the last
pixel of the walk, a ragged 5 x 7, a run that crosses a column end, and vertical stripes."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def masks():
    rng = np.random.default_rng(13)
    out = {}
    blobs = rng.random((50, 40)) < 0.3
    out["blobs200"] = blobs.repeat(4, axis=0).repeat(5, axis=1)
    out["empty"] = np.zeros((6, 9), dtype=bool)
    out["full"] = np.ones((8, 5), dtype=bool)
    one = np.zeros((7, 4), dtype=bool)
    one[3, 2] = True
    out["single"] = one
    last = np.zeros((6, 5), dtype=bool)
    last[2:, 4] = True                        # ends at the last pixel of the column-major walk
    last[0, 0] = True                         # and one that starts at the first
    out["last"] = last
    out["ragged5x7"] = rng.random((5, 7)) < 0.5
    cross = np.zeros((5, 6), dtype=bool)
    cross[3:, 1] = True                       # runs on through the column end into the next column
    cross[:2, 2] = True
    out["cross"] = cross
    stripes = np.zeros((9, 10), dtype=bool)
    stripes[:, ::3] = True
    out["stripes"] = stripes
    return {k: v.astype(np.uint8) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds utilities/utilities.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g13_rle.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_utilities", os.path.join(args.reference, "utilities", "utilities.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ms = masks()
    names = sorted(ms)
    data = {"names": np.array(names)}
    for n in names:
        data["mask_" + n] = ms[n]
        data["rle_" + n] = np.array(mod.mask2rle(ms[n]))
    np.savez_compressed(args.out, **data)
    print("wrote", args.out, os.path.getsize(args.out), "bytes;", {n: len(str(data["rle_" + n]).split()) // 2 for n in names})


if __name__ == "__main__":
    sys.exit(main())
