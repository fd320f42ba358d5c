"""Generates tests/golden/distort_kat.npz, the known-answer vectors of the lens distortion (tests/distort_def.py; include/vstab.h "Lens
distortion"):  python tests/golden/make_distort_golden.py

  case<k>_src      a small packed NV12 frame
  case<k>_params   the 17 map parameters (cameras and rotation), float32
  case<k>_dist     k1..k4, float64
  case<k>_mode     map mode 1 (fisheye -> pinhole) or 2 (fisheye -> fisheye)
  case<k>_size     (dw, dh)
  case<k>_mapx/y   the distorted map planes (the cases that carry them)
  case<k>_bgr      cvtColor + cv::remap(INTER_LINEAR) with that map
  case<k>_luma / _chroma   the plane-wise warp with that map

Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import distort_def  # noqa: E402
import oracle  # noqa: E402
import synth  # noqa: E402

# (sw, sh, dw, dh, mode, D, rotation vector, fy / fx of the input camera, map planes stored)
CASES = [
    (128, 72, 96, 64, 1, distort_def.D_A, (0.02, -0.03, 0.01), 1.0, True),
    (128, 72, 130, 70, 2, distort_def.D_B, (-0.15, 0.1, 0.3), 1.0, False),
    (128, 72, 130, 70, 1, distort_def.D_A, (0.0, 1.2, 0.0), 1.0, False),       # part of the frame is behind the camera
    (64, 32, 67, 35, 2, distort_def.D_C, (0.0, 0.0, 0.0), 1.25, True),         # anisotropic input camera, axis pixel
]


def case_params(sw, sh, dw, dh, mode, rv, aniso):
    Kin = oracle.lens_camera(oracle.PROJ_FISH, 150.0, sw, sh)
    Kin[1, 1] *= aniso
    Kout = oracle.lens_camera(oracle.PROJ_RECT if mode == 1 else oracle.PROJ_FISH, 110.0 if mode == 1 else 165.0, dw, dh)
    return oracle.map_params(Kin, Kout, oracle.rodrigues(rv))


def build():
    out = {}
    for k, (sw, sh, dw, dh, mode, D, rv, aniso, with_maps) in enumerate(CASES):
        src = synth.nv12(40 + k, sw, sh)
        p = np.asarray(case_params(sw, sh, dw, dh, mode, rv, aniso), np.float32)
        out[f"case{k}_src"], out[f"case{k}_params"], out[f"case{k}_dist"] = src, p, np.asarray(D, np.float64)
        out[f"case{k}_mode"], out[f"case{k}_size"] = np.int32(mode), np.array([dw, dh], np.int32)
        if with_maps:
            out[f"case{k}_mapx"], out[f"case{k}_mapy"] = distort_def.maps(p, dw, dh, mode, D)
        out[f"case{k}_bgr"] = distort_def.warp_bgr(src, p, dw, dh, mode, D)
        out[f"case{k}_luma"], out[f"case{k}_chroma"] = distort_def.warp_planar(src, p, dw, dh, mode, D)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "distort_kat.npz"), **build())
    print("wrote distort_kat.npz:", len(CASES), "cases")
