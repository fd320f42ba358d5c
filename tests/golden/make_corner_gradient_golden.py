"""Generates tests/golden/corner_gradient_kat.npz, the known-answer vectors of the corner gradient size (tests/corner_def.py;
include/vstab.h "Corner gradient size"): python tests/golden/make_corner_gradient_golden.py

One frame, the 66 x 33 cut of synth.luma(13) (corner_def.dense_frames' "66x33"), and per pair (B, G) of the six that no "Corner block
size" call serves -- G in (5, 7), B in (3, 5, 7):

  gray                              the frame
  b<B>_g<G>_min_eig, _harris        the dense responses of the definition (k = 0.04)

Fixtures are data only: inputs and expected outputs.  They pin the definition, not the library: an edit of the definition shows.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import corner_def as D  # noqa: E402


def gray():
    return D.dense_frames(3, 5)["66x33"]


def answers(g, block, gradient):
    return {"min_eig": D.min_eig(g, block, gradient), "harris": D.corner_harris(g, block, gradient)}


def main():
    g = gray()
    out = {"gray": g}
    for block, gradient in D.NEW_PAIRS:
        for k, v in answers(g, block, gradient).items():
            out[f"b{block}_g{gradient}_{k}"] = v
    path = os.path.join(HERE, "corner_gradient_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote corner_gradient_kat.npz:", len(D.NEW_PAIRS), "pairs,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
