"""Generates tests/golden/border_kat.npz, the known-answer vectors of the border modes (tests/warp_def.py; include/vstab.h "Border
modes"):  python tests/golden/make_border_golden.py

  case<k>_src      small sources of width and height 1, 2, 3 and even sizes, with 1, 2 and 3 channels
  case<k>_mapx/y   maps over the source and several frame widths around it, exact half-steps of 1/32 pixel (cvRound's ties), NaN, +-inf,
                   +-1e30 and +-32768 entries
  case<k>_mode     the border mode (REPLICATE, REFLECT, REFLECT_101)
  case<k>_out      cv::remap(INTER_LINEAR, mode) as warp_def states it

Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import warp_def as wd  # noqa: E402

# (sw, sh, channels, dw, dh): widths and heights 1, 2, 3 and even sizes
SHAPES = [(1, 1, 1, 12, 9), (2, 2, 3, 16, 11), (3, 3, 2, 15, 10), (1, 3, 3, 11, 8), (3, 1, 1, 13, 7), (2, 3, 2, 9, 9), (8, 6, 3, 19, 13),
          (12, 8, 1, 21, 12), (6, 10, 2, 17, 14)]


def kat_maps(rng, sw, sh, dw, dh):
    """Positions over the source and up to four frame sizes around it, with every special value and tie the definition has to settle."""
    mx = rng.uniform(-4.0 * sw - 3, 5.0 * sw + 3, (dh, dw)).astype(np.float32)
    my = rng.uniform(-4.0 * sh - 3, 5.0 * sh + 3, (dh, dw)).astype(np.float32)
    near = rng.random((dh, dw)) < 0.4  # near the edges, where the four taps straddle them
    mx[near] = rng.uniform(-2.0, sw + 1.0, int(near.sum())).astype(np.float32)
    my[near] = rng.uniform(-2.0, sh + 1.0, int(near.sum())).astype(np.float32)
    tie_x = ((rng.integers(-96 * sw - 64, 32 * sw + 96 * sw + 64, (dh, dw)) + 0.5) / 32.0).astype(np.float32)
    tie_y = ((rng.integers(-96 * sh - 64, 32 * sh + 96 * sh + 64, (dh, dw)) + 0.5) / 32.0).astype(np.float32)
    sel = rng.random((dh, dw)) < 0.2
    mx[sel], my[sel] = tie_x[sel], tie_y[sel]
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 32768.0, -32768.0, 32767.0, -32769.0, 2147483520.0, -2147483648.0], np.float32)
    for m in (mx, my):
        pick = rng.random((dh, dw)) < 0.08
        m[pick] = rng.choice(special, int(pick.sum()))
    edge = np.array([-3.5, -1.5, -1.0, -0.5, -0.03125, 0.0, 0.5, sw - 1.5, sw - 1.0, sw - 0.5, sw, sw + 0.5], np.float32)
    n = min(len(edge), dw)
    mx[0, :n], my[0, :n] = edge[:n], 0.25
    mx[1, :n] = 0.75
    my[1, :n] = np.array([-3.5, -1.5, -1.0, -0.5, -0.03125, 0.0, 0.5, sh - 1.5, sh - 1.0, sh - 0.5, sh, sh + 0.5], np.float32)[:n]
    return mx, my


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    k = 0
    for sw, sh, cn, dw, dh in SHAPES:
        src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
        for mode in wd.MODES:
            mx, my = kat_maps(rng, sw, sh, dw, dh)
            out[f"case{k}_src"], out[f"case{k}_mapx"], out[f"case{k}_mapy"] = src, mx, my
            out[f"case{k}_mode"] = np.array(mode, np.int32)
            out[f"case{k}_out"] = wd.remap(src, mx, my, "linear", mode)
            k += 1
    np.savez_compressed(os.path.join(HERE, "border_kat.npz"), **out)
    print("wrote border_kat.npz:", k, "cases")


if __name__ == "__main__":
    main()
