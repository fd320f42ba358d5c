"""Generates tests/golden/p010_resample_kat.npz, the known-answer vectors of vstab_warp_p010_planar_ex (tests/warp10_def.py;
include/vstab.h, "Cubic and Lanczos resampling at 10 bits"):  python tests/golden/make_p010_resample_golden.py

  case<k>_y16 / _uv16   P010 planes (words with junk in the low six bits), 48 x 32 luma and 24 x 16 interleaved chroma pairs
  case<k>_params        the 17 map parameters (cameras and the first row's rotation), float32
  case<k>_rot_bottom    the last row's rotation, 9 float32 (absent: one rotation)
  case<k>_mode          map mode 0 .. 4
  case<k>_resample      VSTAB_RESAMPLE_* (2 INTER_CUBIC, 4 INTER_LANCZOS4)
  case<k>_border        the border mode (cv::BorderTypes)
  case<k>_size          (dw, dh) = (63, 31): an odd output, ceil-sized chroma
  case<k>_luma / _chroma   the warped planes, words

Both resamplers, every border mode, with and without a rotation per row.  The maps are the oracle's C statement, so this file does not depend
on a GPU.  Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import fullrange  # noqa: E402
import warp10_def as w10  # noqa: E402
import warp_def as wd  # noqa: E402

SW, SH, DW, DH = 48, 32, 63, 31
# (mode, rotation per row, resampler, border mode)
CASES = [
    (0, True, "cubic", wd.CONSTANT),
    (1, False, "cubic", wd.REFLECT_101),
    (1, True, "cubic", wd.REPLICATE),
    (3, False, "cubic", wd.REFLECT),
    (0, False, "lanczos4", wd.CONSTANT),
    (1, True, "lanczos4", wd.REFLECT_101),
    (2, False, "lanczos4", wd.REPLICATE),
    (1, True, "lanczos4", wd.REFLECT),
]


def build():
    out = {}
    p, rb = wd.case_params(SW, SH, DW, DH, 24.0, 16.0)
    for k, (mode, rot, resampler, border) in enumerate(CASES):
        y16, uv16, _, _ = fullrange.p010_extreme_frame(900 + k, SW, SH, block=8)
        mx, my = wd.maps(p, DW, DH, mode, rb if rot else None)
        out[f"case{k}_y16"], out[f"case{k}_uv16"], out[f"case{k}_params"] = y16, uv16, np.asarray(p, np.float32)
        if rot:
            out[f"case{k}_rot_bottom"] = rb
        out[f"case{k}_mode"], out[f"case{k}_size"] = np.array(mode, np.int32), np.array([DW, DH], np.int32)
        out[f"case{k}_resample"], out[f"case{k}_border"] = np.array(wd.RESAMPLE[resampler], np.int32), np.array(border, np.int32)
        out[f"case{k}_luma"], out[f"case{k}_chroma"] = w10.planar10(y16, uv16, mx, my, resampler, border)
    return out


def main():
    out = build()
    np.savez_compressed(os.path.join(HERE, "p010_resample_kat.npz"), **out)
    print("wrote p010_resample_kat.npz:", len(CASES), "cases")


if __name__ == "__main__":
    main()
