"""Generates tests/golden/distort_resample_kat.npz, the known-answer vectors of vstab_warp_nv12_dist_ex (tests/warp_def.py;
include/vstab.h):  python tests/golden/make_distort_resample_golden.py

  case<k>_src       a small packed NV12 frame (64 x 36 or smaller)
  case<k>_params    the 17 map parameters (cameras and rotation), float32
  case<k>_dist      k1..k4, float64
  case<k>_mode      map mode 1 (fisheye -> pinhole) or 2 (fisheye -> fisheye)
  case<k>_resample  VSTAB_RESAMPLE_* (0 INTER_LINEAR, 2 INTER_CUBIC, 4 INTER_LANCZOS4)
  case<k>_border    the border mode (cv::BorderTypes)
  case<k>_size      (dw, dh)
  case<k>_bgr       cvtColor + cv::remap(resampler, border mode) with the distorted map
  case<k>_luma / _chroma   the plane-wise warp with that map

Each of the three kernel families once (the bilinear border kernel, the constant-border resampler tiles, the resamplers' border tiles), both
map modes, BGR and plane-wise.  Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import distort_def  # noqa: E402
import warp_def as wd  # noqa: E402
import oracle  # noqa: E402
import synth  # noqa: E402

# (sw, sh, dw, dh, mode, D, rotation vector, fy / fx of the input camera, resampler, border mode)
CASES = [
    (64, 36, 70, 37, 1, distort_def.D_A, (0.02, -0.03, 0.01), 1.0, "linear", wd.REFLECT_101),
    (64, 36, 67, 35, 2, distort_def.D_B, (-0.15, 0.1, 0.3), 1.0, "cubic", wd.CONSTANT),
    (48, 32, 66, 20, 1, distort_def.D_A, (0.0, 1.2, 0.0), 1.0, "lanczos4", wd.CONSTANT),     # part of the frame is behind the camera
    (64, 36, 65, 33, 2, distort_def.D_C, (0.0, 0.0, 0.0), 1.25, "cubic", wd.REPLICATE),      # anisotropic input camera, axis pixel
    (32, 16, 70, 18, 1, distort_def.D_B, (0.05, 0.4, -0.1), 1.0, "lanczos4", wd.REFLECT),
]


def case_params(sw, sh, dw, dh, mode, rv, aniso):
    Kin = oracle.lens_camera(oracle.PROJ_FISH, 150.0, sw, sh)
    Kin[1, 1] *= aniso
    Kout = oracle.lens_camera(oracle.PROJ_RECT if mode == 1 else oracle.PROJ_FISH, 110.0 if mode == 1 else 165.0, dw, dh)
    return oracle.map_params(Kin, Kout, oracle.rodrigues(rv))


def build():
    out = {}
    for k, (sw, sh, dw, dh, mode, D, rv, aniso, resampler, border) in enumerate(CASES):
        f = synth.nv12(300 + k, sw, sh, full_range=True)
        p = np.asarray(case_params(sw, sh, dw, dh, mode, rv, aniso), np.float32)
        e = wd.Expected(f, *wd.maps(p, dw, dh, mode, None, D))
        out[f"case{k}_src"], out[f"case{k}_params"], out[f"case{k}_dist"] = f, p, np.array(D, np.float64)
        out[f"case{k}_mode"], out[f"case{k}_size"] = np.array(mode, np.int32), np.array([dw, dh], np.int32)
        out[f"case{k}_resample"], out[f"case{k}_border"] = np.array(wd.RESAMPLE[resampler], np.int32), np.array(border, np.int32)
        out[f"case{k}_bgr"] = e.bgr(resampler, border)
        out[f"case{k}_luma"], out[f"case{k}_chroma"] = e.planar(resampler, border)
    return out


def main():
    out = build()
    np.savez_compressed(os.path.join(HERE, "distort_resample_kat.npz"), **out)
    print("wrote distort_resample_kat.npz:", len(CASES), "cases")


if __name__ == "__main__":
    main()
