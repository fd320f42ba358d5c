"""Generates tests/golden/rs_resample_kat.npz, the known-answer vectors of vstab_warp_nv12_rs_ex (tests/warp_def.py;
include/vstab.h):  python tests/golden/make_rs_resample_golden.py

  case<k>_src         a packed NV12 frame, 48 x 32
  case<k>_params      the 17 map parameters (cameras and the first row's rotation), float32
  case<k>_rot_bottom  the last row's rotation, 9 float32
  case<k>_dist        k1..k4, float64 (absent: the ideal lens)
  case<k>_mode        map mode 0 or 1
  case<k>_resample    VSTAB_RESAMPLE_* (0 INTER_LINEAR, 2 INTER_CUBIC, 4 INTER_LANCZOS4)
  case<k>_border      the border mode (cv::BorderTypes)
  case<k>_size        (dw, dh) = (64, 32)
  case<k>_bgr         cvtColor + cv::remap(resampler, border mode) with the per-row map
  case<k>_luma / _chroma   the plane-wise warp with that map

Each resampler with a rotation per row, map modes 0 and 1, with and without a calibrated lens.  The mode 0 maps are the oracle's C
statement, so this file does not depend on a GPU.  Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import distort_def  # noqa: E402
import warp_def as wd  # noqa: E402
import synth  # noqa: E402

SW, SH, DW, DH = 48, 32, 64, 32
# (mode, D or None, resampler, border mode)
CASES = [
    (0, None, "cubic", wd.CONSTANT),
    (1, None, "cubic", wd.REFLECT_101),
    (0, None, "lanczos4", wd.REPLICATE),
    (1, None, "lanczos4", wd.CONSTANT),
    (1, distort_def.D_A, "cubic", wd.REFLECT),
    (1, distort_def.D_B, "lanczos4", wd.REFLECT_101),
    (1, distort_def.D_A, "linear", wd.CONSTANT),
    (1, distort_def.D_B, "linear", wd.REPLICATE),
]


def build():
    out = {}
    p, rb = wd.case_params(SW, SH, DW, DH, 24.0, 16.0)
    for k, (mode, D, resampler, border) in enumerate(CASES):
        f = synth.nv12(500 + k, SW, SH, full_range=True)
        e = wd.Expected(f, *wd.maps(p, DW, DH, mode, rb, D))
        out[f"case{k}_src"], out[f"case{k}_params"], out[f"case{k}_rot_bottom"] = f, np.asarray(p, np.float32), rb
        if D is not None:
            out[f"case{k}_dist"] = np.array(D, np.float64)
        out[f"case{k}_mode"], out[f"case{k}_size"] = np.array(mode, np.int32), np.array([DW, DH], np.int32)
        out[f"case{k}_resample"], out[f"case{k}_border"] = np.array(wd.RESAMPLE[resampler], np.int32), np.array(border, np.int32)
        out[f"case{k}_bgr"] = e.bgr(resampler, border)
        out[f"case{k}_luma"], out[f"case{k}_chroma"] = e.planar(resampler, border)
    return out


def main():
    out = build()
    np.savez_compressed(os.path.join(HERE, "rs_resample_kat.npz"), **out)
    print("wrote rs_resample_kat.npz:", len(CASES), "cases")


if __name__ == "__main__":
    main()
