"""Generates tests/golden/cubic_kat.npz, the known-answer vectors of the bicubic resampler (tests/warp_def.py; include/vstab.h "Bicubic
resampling"):  python tests/golden/make_cubic_golden.py

  table            the (1024, 4, 4) integer weight table
  case<k>_src      small sources with 1, 2 and 3 channels
  case<k>_mapx/y   maps with footprints straddling every edge and corner, exact half-steps of 1/32 pixel (cvRound's ties), NaN, +-inf
                   and +-1e9 entries
  case<k>_border   the border value per channel
  case<k>_out      cv::remap(INTER_CUBIC, BORDER_CONSTANT) as warp_def states it

Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import warp_def as wd  # noqa: E402


def kat_maps(rng, sw, sh, dw, dh):
    """Random positions over the source and one pixel around it, with every special value and tie the definition has to settle."""
    mx = rng.uniform(-3.0, sw + 2.0, (dh, dw)).astype(np.float32)
    my = rng.uniform(-3.0, sh + 2.0, (dh, dw)).astype(np.float32)
    # exact half-steps of 1/32 (ties of cvRound) and integer positions
    tie_x = ((rng.integers(-96, 32 * sw + 96, (dh, dw)) + 0.5) / 32.0).astype(np.float32)
    tie_y = ((rng.integers(-96, 32 * sh + 96, (dh, dw)) + 0.5) / 32.0).astype(np.float32)
    sel = rng.random((dh, dw)) < 0.25
    mx[sel], my[sel] = tie_x[sel], tie_y[sel]
    ints = rng.random((dh, dw)) < 0.1
    mx[ints], my[ints] = np.floor(mx[ints]), np.floor(my[ints])
    special = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 2147483520.0, -2147483648.0, 3e9], np.float32)
    for m in (mx, my):
        pick = rng.random((dh, dw)) < 0.06
        m[pick] = rng.choice(special, int(pick.sum()))
    # the corners and edges of the source, just inside and just outside
    edge = np.array([-2.5, -1.97, -1.0, -0.03125, 0.0, 0.5, sw - 1.5, sw - 1.0, sw - 0.5, sw + 0.96875], np.float32)
    mx[0, : len(edge)] = edge
    my[0, : len(edge)] = 0.25
    mx[1, : len(edge)] = 0.75
    my[1, : len(edge)] = np.array([-2.5, -1.97, -1.0, -0.03125, 0.0, 0.5, sh - 1.5, sh - 1.0, sh - 0.5, sh + 0.96875], np.float32)
    return mx, my


def main():
    rng = np.random.default_rng(20261015)
    out = {"table": wd.cubic_table().astype(np.int16)}
    cases = [(1, 1, 1, 12, 9, (37,)), (3, 3, 1, 16, 11, (200,)), (17, 9, 1, 23, 13, (16,)), (12, 8, 2, 19, 10, (128, 128)),
             (21, 14, 3, 25, 17, (0, 0, 0)), (5, 4, 3, 14, 12, (255, 7, 90))]
    for i, (sw, sh, cn, dw, dh, border) in enumerate(cases):
        src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
        mx, my = kat_maps(rng, sw, sh, dw, dh)
        out[f"case{i}_src"], out[f"case{i}_mapx"], out[f"case{i}_mapy"] = src, mx, my
        out[f"case{i}_border"] = np.array(border, np.int32)
        out[f"case{i}_out"] = wd.remap(src, mx, my, "cubic", wd.CONSTANT, border)
    np.savez_compressed(os.path.join(HERE, "cubic_kat.npz"), **out)
    print("wrote cubic_kat.npz:", len(cases), "cases")


if __name__ == "__main__":
    main()
