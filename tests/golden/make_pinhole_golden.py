"""Generates tests/golden/pinhole_kat.npz, the known-answer vectors of the pinhole lens distortion (tests/pinhole_def.py; include/vstab.h,
"Pinhole lens distortion"):  python tests/golden/make_pinhole_golden.py

  map<k>_params   the 17 map parameters (cameras and rotation), float32
  map<k>_dist     k1, k2, p1, p2, k3, float64
  map<k>_mode     map mode 3 (pinhole -> pinhole) or 4 (pinhole -> fisheye)
  map<k>_size     (dw, dh)
  map<k>_x / _y   pinhole_def.maps: the float32 map planes (NaN where the map is outside)
  pts_K           the camera matrix of the points
  pts_in          (n, 2) pixels, float64
  pts<j>_dist     the coefficients of point set j
  pts<j>_out      pinhole_def.undistort_points(pts_in, pts_K, pts<j>_dist)
  pts<j>_out_rp   the same through a rotation R and a new camera P (pts_R, pts_P)

Fixtures are data only: inputs and expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
import pinhole_def as pd  # noqa: E402

# (sw, sh, dw, dh, mode, D, rotation vector, fy / fx of the input camera)
MAPS = [
    (64, 36, 70, 37, 3, pd.D_P, (0.02, -0.03, 0.01), 1.0),
    (64, 36, 67, 35, 4, pd.D_Q, (-0.15, 0.1, 0.3), 1.0),
    (48, 32, 66, 20, 3, pd.D_M, (0.0, 1.2, 0.0), 1.0),          # part of the frame is behind the camera
    (64, 36, 65, 33, 4, pd.D_P, (0.0, 0.0, 0.0), 1.25),         # anisotropic input camera, axis pixel, rays beyond 180 degrees
]
POINT_SETS = [pd.D_P, pd.D_Q, pd.D_M, pd.D_0]


def case_params(sw, sh, dw, dh, mode, rv, aniso):
    Kin = oracle.lens_camera(oracle.PROJ_RECT, 100.0, sw, sh)
    Kin[1, 1] *= aniso
    Kout = oracle.lens_camera(oracle.PROJ_RECT if mode == 3 else oracle.PROJ_FISH, 80.0 if mode == 3 else 300.0, dw, dh)
    return oracle.map_params(Kin, Kout, oracle.rodrigues(rv))


def build():
    out = {}
    for k, (sw, sh, dw, dh, mode, D, rv, aniso) in enumerate(MAPS):
        p = np.asarray(case_params(sw, sh, dw, dh, mode, rv, aniso), np.float32)
        mx, my = pd.maps(p, dw, dh, mode, D)
        out[f"map{k}_params"], out[f"map{k}_dist"] = p, np.array(D, np.float64)
        out[f"map{k}_mode"], out[f"map{k}_size"] = np.array(mode, np.int32), np.array([dw, dh], np.int32)
        out[f"map{k}_x"], out[f"map{k}_y"] = mx, my
    w, h = 640, 360
    K = oracle.lens_camera(oracle.PROJ_RECT, 100.0, w, h)
    K[1, 1] *= 1.07
    rng = np.random.default_rng(23)
    pts = np.concatenate([rng.uniform((0, 0), (w, h), (60, 2)), [[K[0, 2], K[1, 2]], [0.0, 0.0], [w - 1.0, h - 1.0], [-200.0, 900.0]]])
    R, P = oracle.rodrigues((0.03, -0.02, 0.05)), oracle.lens_camera(oracle.PROJ_RECT, 80.0, 480, 270)
    out["pts_K"], out["pts_in"], out["pts_R"], out["pts_P"] = K, pts, np.asarray(R, np.float64), P
    for j, D in enumerate(POINT_SETS):
        out[f"pts{j}_dist"] = np.array(D, np.float64)
        out[f"pts{j}_out"] = pd.undistort_points(pts, K, D)
        out[f"pts{j}_out_rp"] = pd.undistort_points(pts, K, D, R, P)
    return out


def main():
    out = build()
    np.savez_compressed(os.path.join(HERE, "pinhole_kat.npz"), **out)
    print("wrote pinhole_kat.npz:", len(MAPS), "maps,", len(POINT_SETS), "point sets")


if __name__ == "__main__":
    main()
