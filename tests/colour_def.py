"""The colour matrix and range of the BGR path (include/vstab.h, "Colour matrix and range"), restated in numpy: the coefficient table
derived with fractions.Fraction, the forward and the inverse conversion.  Test infrastructure only (a plain module, imported by the tests).

(CVTCOLOR, LIMITED) is cvtColor's arithmetic with OpenCV's constants; the other six specs are the same 20-bit fixed-point forms with
coefficients from (Kr, Kb) and the range, every rint the round-half-to-even of the exact rational value."""
from fractions import Fraction

import numpy as np

CVTCOLOR, BT601, BT709, BT2020 = range(4)
LIMITED, FULL = 0, 1
SPECS = [(CVTCOLOR, LIMITED)] + [(m, r) for m in (BT601, BT709, BT2020) for r in (LIMITED, FULL)]
NAMES = {(CVTCOLOR, LIMITED): "cvtcolor", (BT601, LIMITED): "bt601_limited", (BT601, FULL): "bt601_full", (BT709, LIMITED): "bt709_limited",
         (BT709, FULL): "bt709_full", (BT2020, LIMITED): "bt2020_limited", (BT2020, FULL): "bt2020_full"}
KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000)),
         BT2020: (Fraction(2627, 10000), Fraction(593, 10000))}
# OpenCV's constants: forward CY, CUB, CUG, CVG, CVR, yoff, inverse CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV
CVTCOLOR_ROW = (1220542, 2116026, -409993, -852492, 1673527, 16, 269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448)


def rint(v):
    """round half to even of an exact rational"""
    return int(round(Fraction(v)))   # Fraction.__round__ without ndigits rounds half to even


def coefficients(matrix, rng):
    """-> the 14 integers of a spec, in vstab_colour_coefficients' order"""
    if (matrix, rng) == (CVTCOLOR, LIMITED):
        return CVTCOLOR_ROW
    if matrix not in KR_KB or rng not in (LIMITED, FULL):
        raise ValueError("no such colour spec")
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc, yoff = (Fraction(255, 219), Fraction(255, 224), 16) if rng == LIMITED else (Fraction(1), Fraction(1), 0)
    one = 1 << 20
    cy, cvr, cub = rint(one * sy), rint(one * sc * 2 * (1 - kr)), rint(one * sc * 2 * (1 - kb))
    cug, cvg = -rint(one * sc * 2 * kb * (1 - kb) / kg), -rint(one * sc * 2 * kr * (1 - kr) / kg)
    cry, cgy, cby = rint(one * kr / sy), rint(one * kg / sy), rint(one * kb / sy)
    cbu = rint(one / (2 * sc))
    cru, cgu = -rint(one * kr / (2 * (1 - kb) * sc)), -rint(one * kg / (2 * (1 - kb) * sc))
    cgv, cbv = -rint(one * kg / (2 * (1 - kr) * sc)), -rint(one * kb / (2 * (1 - kr) * sc))
    return (cy, cub, cug, cvg, cvr, yoff, cry, cgy, cby, cru, cgu, cbu, cgv, cbv)


def _sat8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def yuv_to_bgr(Y, U, V, spec):
    """integer arrays of one shape -> (..., 3) uint8 BGR"""
    cy, cub, cug, cvg, cvr, yoff = coefficients(*spec)[:6]
    y = np.maximum(np.asarray(Y, np.int64) - yoff, 0) * cy + (1 << 19)
    u, v = np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    return np.stack([_sat8((y + cub * u) >> 20), _sat8((y + cvg * v + cug * u) >> 20), _sat8((y + cvr * v) >> 20)], axis=-1)


def nv12_to_bgr(nv12, spec):
    """(h * 3 / 2, w) packed NV12 -> (h, w, 3) uint8 BGR"""
    nv12 = np.asarray(nv12)
    rows, w = nv12.shape
    h = rows * 2 // 3
    uv = nv12[h:].reshape(h // 2, w // 2, 2)
    U, V = (np.repeat(np.repeat(uv[..., k], 2, axis=0), 2, axis=1) for k in (0, 1))
    return yuv_to_bgr(nv12[:h], U, V, spec)


def bgr_to_yuv_unsaturated(bgr, spec):
    """(..., 3) BGR -> the three sums >> 20 before sat8, int64 (..., 3): Y, U, V"""
    yoff, cry, cgy, cby, cru, cgu, cbu, cgv, cbv = coefficients(*spec)[5:]
    p = np.asarray(bgr).astype(np.int64)
    B, G, R = p[..., 0], p[..., 1], p[..., 2]
    half = 1 << 19
    return np.stack([(cry * R + cgy * G + cby * B + half + (yoff << 20)) >> 20, (cru * R + cgu * G + cbu * B + half + (128 << 20)) >> 20,
                     (cbu * R + cgv * G + cbv * B + half + (128 << 20)) >> 20], axis=-1)


def bgr_to_nv12(bgr, spec):
    """(h, w, 3) BGR, any size -> (y (h, w), uv (ceil(h / 2), ceil(w / 2), 2)) uint8: chroma from the top-left pixel of each 2 x 2 block"""
    yuv = bgr_to_yuv_unsaturated(bgr, spec)
    return _sat8(yuv[..., 0]), _sat8(yuv[::2, ::2, 1:])


def pack(y, uv):
    """(y, uv) of bgr_to_nv12 for even sizes -> packed NV12"""
    h, w = y.shape
    return np.concatenate([y, uv.reshape(h // 2, w)], axis=0)


CUBE_CORNERS = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)


def cube_corner_frame():
    """a 16 x 2 BGR frame whose 2 x 2 blocks are the eight corners of the colour cube"""
    return np.repeat(np.repeat(CUBE_CORNERS.reshape(1, 8, 3), 2, axis=0), 2, axis=1)


def extremes_frame(w, h):
    """packed NV12 of every combination of Y, U, V in {0, 1, 15, 16, 17, 128, 234, 235, 236, 240, 254, 255}, cycled over the frame"""
    vals = np.array([0, 1, 15, 16, 17, 128, 234, 235, 236, 240, 254, 255], np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = vals[(xx + 5 * yy) % 12]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    uv = out[h:].reshape(h // 2, w // 2, 2)
    uv[..., 0] = vals[(cx // 1 + 7 * cy) % 12]
    uv[..., 1] = vals[(cx // 12 + cy) % 12]
    return out
