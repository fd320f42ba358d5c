"""Generates tests/golden/colour_kat.npz, the known-answer vectors of the colour matrix and range (include/vstab.h "Colour matrix and
range"; tests/colour_def.py): python tests/golden/make_colour_golden.py

  nv12_<k>            small packed NV12 frames (2 x 2, 8 x 4, 16 x 6): random bytes, and one of range extremes
  bgr_<k>             small BGR frames of the same sizes: random bytes, and the cube-corner frame (16 x 2)
  fwd_<k>_<spec>      nv12_<k> converted to BGR with every spec
  inv_<k>_<spec>      bgr_<k> converted to packed NV12 with the inverse of every spec

The expected outputs are computed here pixel by pixel in Python integers from the header's formulas and the issue's coefficient table
written out below -- not through colour_def's numpy code, which the tests compare against these vectors.  Fixtures are data only: inputs
and expected outputs.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# spec name -> CY, CUB, CUG, CVG, CVR, yoff, CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV
TABLE = {
    "cvtcolor": (1220542, 2116026, -409993, -852492, 1673527, 16, 269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448),
    "bt601_limited": (1220945, 2115221, -410793, -852458, 1673555, 16, 269262, 528618, 102662, -155423, -305128, 460551, -385654, -74897),
    "bt601_full": (1048576, 1858077, -360853, -748826, 1470104, 0, 313524, 615514, 119538, -176932, -347356, 524288, -439026, -85262),
    "bt709_limited": (1220945, 2215014, -223607, -558796, 1879825, 16, 191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230),
    "bt709_full": (1048576, 1945738, -196424, -490864, 1651297, 0, 222927, 749942, 75707, -120138, -404150, 524288, -476214, -48074),
    "bt2020_limited": (1220945, 2245811, -196426, -682019, 1760217, 16, 236572, 610567, 53402, -128614, -331937, 460551, -423510, -37041),
    "bt2020_full": (1048576, 1972791, -172546, -599107, 1546230, 0, 275461, 710935, 62181, -146413, -377875, 524288, -482120, -42168),
}


def sat8(v):
    return 0 if v < 0 else 255 if v > 255 else v


def forward(nv12, t):
    cy, cub, cug, cvg, cvr, yoff = t[:6]
    rows, w = nv12.shape
    h = rows * 2 // 3
    out = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            Y, U, V = int(nv12[y, x]), int(nv12[h + y // 2, x & ~1]), int(nv12[h + y // 2, (x & ~1) + 1])
            u, v, l = U - 128, V - 128, max(Y - yoff, 0) * cy + (1 << 19)
            out[y, x] = sat8((l + cub * u) >> 20), sat8((l + cvg * v + cug * u) >> 20), sat8((l + cvr * v) >> 20)
    return out


def inverse(bgr, t):
    yoff, cry, cgy, cby, cru, cgu, cbu, cgv, cbv = t[5:]
    h, w = bgr.shape[:2]
    out = np.zeros((h * 3 // 2, w), np.uint8)
    for y in range(h):
        for x in range(w):
            B, G, R = (int(c) for c in bgr[y, x])
            out[y, x] = sat8((cry * R + cgy * G + cby * B + (1 << 19) + (yoff << 20)) >> 20)
            if not (y & 1) and not (x & 1):
                out[h + y // 2, x] = sat8((cru * R + cgu * G + cbu * B + (1 << 19) + (128 << 20)) >> 20)
                out[h + y // 2, x + 1] = sat8((cbu * R + cgv * G + cbv * B + (1 << 19) + (128 << 20)) >> 20)
    return out


def main():
    rng = np.random.default_rng(20261020)
    out = {}
    ext = np.array([0, 1, 15, 16, 17, 128, 234, 235, 236, 240, 254, 255], np.uint8)
    nv12s = [rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for (w, h) in ((2, 2), (8, 4), (16, 6))]
    nv12s.append(ext[rng.integers(0, 12, (9, 12))])  # 12 x 6 of extremes
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    bgrs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (w, h) in ((2, 2), (8, 4), (16, 6))]
    bgrs.append(np.repeat(np.repeat(corners.reshape(1, 8, 3), 2, axis=0), 2, axis=1))  # the cube-corner frame, 16 x 2
    for k, f in enumerate(nv12s):
        out[f"nv12_{k}"] = f
        for name, t in TABLE.items():
            out[f"fwd_{k}_{name}"] = forward(f, t)
    for k, f in enumerate(bgrs):
        out[f"bgr_{k}"] = f
        for name, t in TABLE.items():
            out[f"inv_{k}_{name}"] = inverse(f, t)
    np.savez_compressed(os.path.join(HERE, "colour_kat.npz"), **out)
    print("wrote colour_kat.npz:", len(nv12s), "NV12 frames,", len(bgrs), "BGR frames,", len(TABLE), "specs")


if __name__ == "__main__":
    main()
