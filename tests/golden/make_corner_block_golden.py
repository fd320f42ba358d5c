"""Generates tests/golden/corner_block_kat.npz, the known-answer vectors of the corner block size (tests/corner_def.py; include/vstab.h
"Corner block size"): python tests/golden/make_corner_block_golden.py

The frames are small: a 4 x 5 cut (several folds of the border), synth.luma(13) at 40 x 24, the 2-px checkerboard at 33 x 20 and the
dark-noise frame whose double sums are not all exact.  Per frame <name> and block B in (5, 7):

  <name>_gray                       the frame
  <name>_b<B>_min_eig, _harris      the dense responses of the definition (k = 0.04)
  <name>_b<B>_corners, _corners_harris, _corners_masked
                                    good_features with max_corners 50, quality 0.01, min_distance 3 (masked: under mask_def.checkerboard
                                    of 3 x 5 cells, minimum eigenvalue)

Fixtures are data only: inputs and expected outputs.  They pin the definition, not the library: an edit of the definition shows.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import corner_def as D  # noqa: E402
import corner_tiles as C  # noqa: E402
import mask_def as M  # noqa: E402
import synth  # noqa: E402

PARAMS = (50, 0.01, 3.0)


def frames():
    return {"cut_4x5": np.ascontiguousarray(synth.luma(13, 16, 16)[:5, :4]), "luma_40x24": synth.luma(13, 40, 24), "checker_33x20": C.checker(33, 20),
            "dark_noise": D.dark_noise()}


def answers(g, block):
    mc, q, md = PARAMS
    mask = M.checkerboard(*g.shape, 3, 5)
    return {"min_eig": D.min_eig(g, block), "harris": D.corner_harris(g, block),
            "corners": D.good_features(g, None, mc, q, md, block), "corners_harris": D.good_features(g, None, mc, q, md, block, harris=True),
            "corners_masked": D.good_features(g, mask, mc, q, md, block)}


def main():
    out = {}
    for name, g in frames().items():
        out[name + "_gray"] = g
        for block in (5, 7):
            for k, v in answers(g, block).items():
                out[f"{name}_b{block}_{k}"] = v
    path = os.path.join(HERE, "corner_block_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote corner_block_kat.npz:", len(frames()), "frames,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
