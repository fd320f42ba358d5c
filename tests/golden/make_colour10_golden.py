"""Generates tests/golden/colour10_kat.npz, the known-answer vectors of the colour matrix and range at 10 bits (include/vstab.h "Colour
matrix and range at 10 bits"; tests/colour10_def.py): python tests/golden/make_colour10_golden.py

  y_<k>, uv_<k>       16 x 4 P010 frames (luma (4, 16), chroma (2, 16) words): random words, and one of range extremes with junk low bits
  bgr_<k>             16 x 4 BGR frames, values 0..1023: random, and the cube-corner frame twice over
  fwd_<k>_<spec>      (y_<k>, uv_<k>) converted to BGR with every spec
  invy_<k>_<spec>, invuv_<k>_<spec>   bgr_<k> converted to P010 planes with the inverse of every spec

The expected outputs are computed here pixel by pixel in Python integers from the header's formulas and the coefficient table written out
below -- not through colour10_def's numpy code, which the tests compare against these vectors.  Fixtures are data only: inputs and
expected outputs.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# spec name -> CY, CUB, CUG, CVG, CVR, yoff, CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV
TABLE = {
    "cvtcolor": (1220542, 2116026, -409993, -852492, 1673527, 64, 269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448),
    "bt601_limited": (1224536, 2121442, -412001, -854966, 1678478, 64, 268472, 527068, 102361, -154967, -304233, 459200, -384523, -74677),
    "bt601_full": (1048576, 1858077, -360853, -748826, 1470104, 0, 313524, 615514, 119538, -176932, -347356, 524288, -439026, -85262),
    "bt709_limited": (1224536, 2221529, -224265, -560439, 1885354, 64, 190894, 642179, 64828, -105223, -353977, 459200, -417094, -42106),
    "bt709_full": (1048576, 1945738, -196424, -490864, 1651297, 0, 222927, 749942, 75707, -120138, -404150, 524288, -476214, -48074),
    "bt2020_limited": (1224536, 2252416, -197003, -684025, 1765394, 64, 235879, 608777, 53246, -128236, -330964, 459200, -422268, -36933),
    "bt2020_full": (1048576, 1972791, -172546, -599107, 1546230, 0, 275461, 710935, 62181, -146413, -377875, 524288, -482120, -42168),
}


def sat10(v):
    return 0 if v < 0 else 1023 if v > 1023 else v


def forward(yp, uvp, t):
    cy, cub, cug, cvg, cvr, yoff = t[:6]
    h, w = yp.shape
    out = np.zeros((h, w, 3), np.uint16)
    for y in range(h):
        for x in range(w):
            Y, U, V = int(yp[y, x]) >> 6, int(uvp[y // 2, x & ~1]) >> 6, int(uvp[y // 2, (x & ~1) + 1]) >> 6
            u, v, l = U - 512, V - 512, max(Y - yoff, 0) * cy + (1 << 19)
            out[y, x] = sat10((l + cub * u) >> 20), sat10((l + cvg * v + cug * u) >> 20), sat10((l + cvr * v) >> 20)
    return out


def inverse(bgr, t):
    yoff, cry, cgy, cby, cru, cgu, cbu, cgv, cbv = t[5:]
    h, w = bgr.shape[:2]
    yp, uvp = np.zeros((h, w), np.uint16), np.zeros((h // 2, w), np.uint16)
    for y in range(h):
        for x in range(w):
            B, G, R = (int(c) for c in bgr[y, x])
            yp[y, x] = sat10((cry * R + cgy * G + cby * B + (1 << 19) + (yoff << 20)) >> 20) << 6
            if not (y & 1) and not (x & 1):
                uvp[y // 2, x] = sat10((cru * R + cgu * G + cbu * B + (1 << 19) + (512 << 20)) >> 20) << 6
                uvp[y // 2, x + 1] = sat10((cbu * R + cgv * G + cbv * B + (1 << 19) + (512 << 20)) >> 20) << 6
    return yp, uvp


def main():
    rng = np.random.default_rng(20261020)
    out = {}
    w, h = 16, 4
    ext = np.array([0, 1, 63, 64, 65, 512, 939, 940, 941, 960, 1022, 1023], np.uint16)
    p010s = [(rng.integers(0, 65536, (h, w)).astype(np.uint16), rng.integers(0, 65536, (h // 2, w)).astype(np.uint16)),
             ((ext[rng.integers(0, 12, (h, w))] << 6) | rng.integers(0, 64, (h, w)).astype(np.uint16),
              (ext[rng.integers(0, 12, (h // 2, w))] << 6) | rng.integers(0, 64, (h // 2, w)).astype(np.uint16))]
    corners = np.array([[b, g, r] for b in (0, 1023) for g in (0, 1023) for r in (0, 1023)], np.uint16)
    bgrs = [rng.integers(0, 1024, (h, w, 3)).astype(np.uint16), np.repeat(np.repeat(corners.reshape(1, 8, 3), 4, axis=0), 2, axis=1)]
    for k, (yp, uvp) in enumerate(p010s):
        out[f"y_{k}"], out[f"uv_{k}"] = yp.astype(np.uint16), uvp.astype(np.uint16)
        for name, t in TABLE.items():
            out[f"fwd_{k}_{name}"] = forward(yp, uvp, t)
    for k, f in enumerate(bgrs):
        out[f"bgr_{k}"] = f
        for name, t in TABLE.items():
            out[f"invy_{k}_{name}"], out[f"invuv_{k}_{name}"] = inverse(f, t)
    np.savez_compressed(os.path.join(HERE, "colour10_kat.npz"), **out)
    print("wrote colour10_kat.npz:", len(p010s), "P010 frames,", len(bgrs), "BGR frames,", len(TABLE), "specs")


if __name__ == "__main__":
    main()
