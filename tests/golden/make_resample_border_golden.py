"""Generates tests/golden/resample_border_kat.npz, the known-answer vectors of the border modes of the cubic and Lanczos resamplers
(tests/warp_def.py; include/vstab.h "Border modes of the cubic and Lanczos resamplers"):
    python tests/golden/make_resample_border_golden.py

  case<k>_src        small sources of width and height 1, 2, 3 and even sizes, with 1, 2 and 3 channels
  case<k>_mapx/y     maps over the source and several frame widths around it, exact half-steps of 1/32 pixel (cvRound's ties), NaN, +-inf,
                     +-1e30 and +-32768 entries (make_border_golden.kat_maps)
  case<k>_resampler  0 = INTER_CUBIC, 1 = INTER_LANCZOS4
  case<k>_mode       the border mode (REPLICATE, REFLECT, REFLECT_101)
  case<k>_out        cv::remap(resampler, mode) as warp_def states it

Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_border_golden  # noqa: E402
import warp_def as wd  # noqa: E402

RESAMPLERS = ("cubic", "lanczos4")
# (sw, sh, channels, dw, dh): widths and heights 1, 2, 3 and even sizes
SHAPES = [(1, 1, 1, 12, 9), (2, 2, 3, 13, 10), (3, 3, 2, 11, 9), (1, 3, 3, 10, 8), (3, 1, 1, 12, 7), (2, 3, 2, 9, 9), (8, 6, 3, 14, 11),
          (12, 8, 1, 16, 12), (6, 10, 2, 13, 12)]


def main():
    rng = np.random.default_rng(20261017)
    out = {}
    k = 0
    for r, resampler in enumerate(RESAMPLERS):
        for sw, sh, cn, dw, dh in SHAPES:
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            for mode in wd.MODES:
                mx, my = make_border_golden.kat_maps(rng, sw, sh, dw, dh)
                out[f"case{k}_src"], out[f"case{k}_mapx"], out[f"case{k}_mapy"] = src, mx, my
                out[f"case{k}_resampler"] = np.array(r, np.int32)
                out[f"case{k}_mode"] = np.array(mode, np.int32)
                out[f"case{k}_out"] = wd.remap(src, mx, my, resampler, mode)
                k += 1
    np.savez_compressed(os.path.join(HERE, "resample_border_kat.npz"), **out)
    print("wrote resample_border_kat.npz:", k, "cases")


if __name__ == "__main__":
    main()
