"""Generates tests/golden/keep_kat.npz, the known-answer vectors of the keep-edge remap (tests/warp_def.py; include/vstab.h "Keep edges"):
python tests/golden/make_keep_golden.py

  case<k>_src      small sources of width and height 1, 2, 3 and even sizes, with 1, 2 and 3 channels
  case<k>_mapx/y   make_border_golden.kat_maps: positions over the source and around it, exact half-steps of 1/32 pixel (cvRound's ties), NaN,
                   +-inf, +-1e30 and +-32768 entries, and a sweep across each edge
  case<k>_prev     the frame to keep, random bytes
  case<k>_out      the keep-edge remap as warp_def states it

Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import warp_def as wd  # noqa: E402
from make_border_golden import SHAPES, kat_maps  # noqa: E402


def main():
    rng = np.random.default_rng(20261019)
    out = {}
    for k, (sw, sh, cn, dw, dh) in enumerate(SHAPES):
        src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
        prev = rng.integers(0, 256, (dh, dw, cn) if cn > 1 else (dh, dw), dtype=np.uint8)
        mx, my = kat_maps(rng, sw, sh, dw, dh)
        out[f"case{k}_src"], out[f"case{k}_mapx"], out[f"case{k}_mapy"], out[f"case{k}_prev"] = src, mx, my, prev
        out[f"case{k}_out"] = wd.remap(src, mx, my, "linear", wd.TRANSPARENT, 0, prev)
    np.savez_compressed(os.path.join(HERE, "keep_kat.npz"), **out)
    print("wrote keep_kat.npz:", len(SHAPES), "cases")


if __name__ == "__main__":
    main()
