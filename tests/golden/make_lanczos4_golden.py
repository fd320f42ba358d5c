"""Generates tests/golden/lanczos4_kat.npz, the known-answer vectors of the Lanczos resampler (tests/warp_def.py; include/vstab.h
"Lanczos resampling"), and prints the sin / cos literals video-annotator_amd/csrc/vstab_lanczos4.hpp commits:
python tests/golden/make_lanczos4_golden.py

  s0, c0           the 32 sin / cos values of interpolateLanczos4 (float64), from this host's libm
  table            the (1024, 8, 8) integer weight table
  case<k>_src      small sources with 1, 2 and 3 channels
  case<k>_mapx/y   maps with footprints straddling every edge and corner, exact half-steps of 1/32 pixel (cvRound's ties), NaN, +-inf
                   and +-1e9 entries
  case<k>_border   the border value per channel
  case<k>_out      cv::remap(INTER_LANCZOS4, BORDER_CONSTANT) as warp_def states it

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
    """Random positions over the source and four pixels around it, with every special value and tie the definition has to settle."""
    mx = rng.uniform(-5.0, sw + 4.0, (dh, dw)).astype(np.float32)
    my = rng.uniform(-5.0, sh + 4.0, (dh, dw)).astype(np.float32)
    tie_x = ((rng.integers(-160, 32 * sw + 160, (dh, dw)) + 0.5) / 32.0).astype(np.float32)
    tie_y = ((rng.integers(-160, 32 * sh + 160, (dh, dw)) + 0.5) / 32.0).astype(np.float32)
    sel = rng.random((dh, dw)) < 0.25
    mx[sel], my[sel] = tie_x[sel], tie_y[sel]
    ints = rng.random((dh, dw)) < 0.1
    mx[ints], my[ints] = np.floor(mx[ints]), np.floor(my[ints])
    special = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 2147483520.0, -2147483648.0, 3e9], np.float32)
    for m in (mx, my):
        pick = rng.random((dh, dw)) < 0.06
        m[pick] = rng.choice(special, int(pick.sum()))
    # the corners and edges of the source, just inside and just outside the 8 x 8 footprint
    ex = np.array([-4.5, -3.97, -3.0, -1.0, -0.03125, 0.0, 0.5, sw - 1.5, sw - 1.0, sw + 1.5, sw + 2.96875, sw + 3.0], np.float32)
    ey = np.array([-4.5, -3.97, -3.0, -1.0, -0.03125, 0.0, 0.5, sh - 1.5, sh - 1.0, sh + 1.5, sh + 2.96875, sh + 3.0], np.float32)
    mx[0, : len(ex)] = ex
    my[0, : len(ex)] = 0.25
    mx[1, : len(ey)] = 0.75
    my[1, : len(ey)] = ey
    return mx, my


def literals(name, vals):
    """A C++ array of hex-float literals (float.hex round-trips every double exactly)."""
    body = ",\n".join("    " + ", ".join(float(v).hex() for v in vals[i:i + 4]) for i in range(0, 32, 4))
    return f"constexpr double LANCZOS4_{name}[32] = {{\n{body}}};"


def main():
    rng = np.random.default_rng(20261016)
    s0, c0 = wd.sincos()
    out = {"s0": np.array(s0, np.float64), "c0": np.array(c0, np.float64), "table": wd.lanczos4_table().astype(np.int16)}
    cases = [(1, 1, 1, 12, 9, (37,)), (3, 5, 1, 16, 11, (200,)), (17, 9, 1, 23, 13, (16,)), (12, 8, 2, 19, 10, (128, 128)),
             (21, 14, 3, 25, 17, (0, 0, 0)), (7, 4, 3, 14, 12, (255, 7, 90))]
    for i, (sw, sh, cn, dw, dh, border) in enumerate(cases):
        src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
        mx, my = kat_maps(rng, sw, sh, dw, dh)
        out[f"case{i}_src"], out[f"case{i}_mapx"], out[f"case{i}_mapy"] = src, mx, my
        out[f"case{i}_border"] = np.array(border, np.int32)
        out[f"case{i}_out"] = wd.remap(src, mx, my, "lanczos4", wd.CONSTANT, border)
    np.savez_compressed(os.path.join(HERE, "lanczos4_kat.npz"), **out)
    print(literals("S0", s0))
    print(literals("C0", c0))
    print("wrote lanczos4_kat.npz:", len(cases), "cases")


if __name__ == "__main__":
    main()
