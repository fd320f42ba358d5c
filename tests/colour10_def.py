"""The colour matrix and range of the 10-bit path (include/vstab.h, "Colour matrix and range at 10 bits"), restated in numpy: the coefficient
table derived with fractions.Fraction, the forward and the inverse conversion, the warp with a spec.  Test infrastructure only (a plain
module, imported by the tests).

(CVTCOLOR, LIMITED) is the 8-bit cvtColor row with yoff = 64, the 10-bit path's arithmetic as it always was; the other six specs are the
formulas of colour_def with the 10-bit scales 1023/876 and 1023/896, every rint the round-half-to-even of the exact rational value."""
from fractions import Fraction

import numpy as np

import colour_def
from colour_def import BT601, BT709, BT2020, CVTCOLOR, FULL, KR_KB, LIMITED, NAMES, SPECS, rint  # noqa: F401  (the specs are the 8-bit path's)

CVTCOLOR_ROW = colour_def.CVTCOLOR_ROW[:5] + (64,) + colour_def.CVTCOLOR_ROW[6:]
DEFAULT = (CVTCOLOR, LIMITED)


def coefficients(matrix, rng):
    """-> the 14 integers of a spec, in vstab_colour_coefficients10's order"""
    if (matrix, rng) == (CVTCOLOR, LIMITED):
        return CVTCOLOR_ROW
    if matrix not in KR_KB or rng not in (LIMITED, FULL):
        raise ValueError("no such colour spec")
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc, yoff = (Fraction(1023, 876), Fraction(1023, 896), 64) if rng == LIMITED else (Fraction(1), Fraction(1), 0)
    one = 1 << 20
    cy, cvr, cub = rint(one * sy), rint(one * sc * 2 * (1 - kr)), rint(one * sc * 2 * (1 - kb))
    cug, cvg = -rint(one * sc * 2 * kb * (1 - kb) / kg), -rint(one * sc * 2 * kr * (1 - kr) / kg)
    cry, cgy, cby = rint(one * kr / sy), rint(one * kg / sy), rint(one * kb / sy)
    cbu = rint(one / (2 * sc))
    cru, cgu = -rint(one * kr / (2 * (1 - kb) * sc)), -rint(one * kg / (2 * (1 - kb) * sc))
    cgv, cbv = -rint(one * kg / (2 * (1 - kr) * sc)), -rint(one * kb / (2 * (1 - kr) * sc))
    return (cy, cub, cug, cvg, cvr, yoff, cry, cgy, cby, cru, cgu, cbu, cgv, cbv)


def _sat10(v):
    return np.clip(v, 0, 1023).astype(np.uint16)


def yuv10_to_bgr10(Y, U, V, spec):
    """10-bit values (integer arrays of one shape) -> (..., 3) uint16 BGR, 0..1023; the sums in 64 bits"""
    cy, cub, cug, cvg, cvr, yoff = coefficients(*spec)[:6]
    y = np.maximum(np.asarray(Y, np.int64) - yoff, 0) * cy + (1 << 19)
    u, v = np.asarray(U, np.int64) - 512, np.asarray(V, np.int64) - 512
    return np.stack([_sat10((y + cub * u) >> 20), _sat10((y + cvg * v + cug * u) >> 20), _sat10((y + cvr * v) >> 20)], axis=-1)


def p010_to_bgr10(y, uv, spec):
    """P010 planes y (h, w), uv (h / 2, w) uint16 words -> (h, w, 3) uint16 BGR; the low six bits of every word are ignored"""
    y, uv = np.asarray(y).astype(np.uint16), np.asarray(uv).astype(np.uint16)
    h, w = y.shape
    c = (uv >> 6).reshape(h // 2, w // 2, 2)
    U, V = (np.repeat(np.repeat(c[..., k], 2, axis=0), 2, axis=1) for k in (0, 1))
    return yuv10_to_bgr10(y >> 6, U, V, spec)


def bgr10_to_yuv_unsaturated(bgr, spec):
    """(..., 3) BGR in 0..1023 -> the three sums >> 20 before sat10, int64 (..., 3): Y, U, V"""
    yoff, cry, cgy, cby, cru, cgu, cbu, cgv, cbv = coefficients(*spec)[5:]
    p = np.asarray(bgr).astype(np.int64)
    B, G, R = p[..., 0], p[..., 1], p[..., 2]
    half = 1 << 19
    return np.stack([(cry * R + cgy * G + cby * B + half + (yoff << 20)) >> 20, (cru * R + cgu * G + cbu * B + half + (512 << 20)) >> 20,
                     (cbu * R + cgv * G + cbv * B + half + (512 << 20)) >> 20], axis=-1)


def bgr10_to_p010(bgr, spec):
    """(h, w, 3) BGR, any size -> (y (h, w), uv (ceil(h / 2), 2 * ceil(w / 2))) uint16 P010 words: chroma from the top-left pixel of each 2 x 2 block"""
    yuv = bgr10_to_yuv_unsaturated(bgr, spec)
    c = _sat10(yuv[::2, ::2, 1:])
    return _sat10(yuv[..., 0]) << 6, (c << 6).reshape(c.shape[0], 2 * c.shape[1])


def warp_p010(y, uv, params, dw, dh, spec, rot_bottom=None, mode=0, blend=0):
    """The 10-bit warp with a spec: the oracle's chain (its map, its 10-bit remap) with the conversion exchanged.  Modes 0..4: the maps
    oracle.warp_p010 composes (create_map_ex / create_map_rs); mode 5: the reference kernel's own map, run on this GPU (warp_def.maps)."""
    import warp_def as wd
    import oracle
    mx, my = wd.maps(params, dw, dh, mode, rot_bottom)
    return oracle.remap_bilinear10(p010_to_bgr10(y, uv, spec), mx, my, blend)


def warp_p010_planes(y, uv, params, dw, dh, spec, rot_bottom=None, mode=0, blend=0):
    """Planes out: that frame through the spec's inverse."""
    return bgr10_to_p010(warp_p010(y, uv, params, dw, dh, spec, rot_bottom, mode, blend), spec)


CUBE_CORNERS = np.array([[b, g, r] for b in (0, 1023) for g in (0, 1023) for r in (0, 1023)], np.uint16)


def cube_corner_frame():
    """a 16 x 2 BGR frame whose 2 x 2 blocks are the eight corners of the colour cube"""
    return np.repeat(np.repeat(CUBE_CORNERS.reshape(1, 8, 3), 2, axis=0), 2, axis=1)


EXTREMES = np.array([0, 1, 63, 64, 65, 512, 939, 940, 941, 960, 1022, 1023], np.uint16)


def extremes_frame(w, h, seed=0):
    """P010 planes (y (h, w), uv (h / 2, w)) cycling Y, U, V over EXTREMES, with random junk in the low six bits of every word"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = (EXTREMES[(xx + 5 * yy) % 12] << 6) | rng.integers(0, 64, (h, w)).astype(np.uint16)
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    uv = np.empty((h // 2, w // 2, 2), np.uint16)
    uv[..., 0] = EXTREMES[(cx + 7 * cy) % 12]
    uv[..., 1] = EXTREMES[(cx // 12 + cy) % 12]
    uv = (uv << 6) | rng.integers(0, 64, uv.shape).astype(np.uint16)
    return y.astype(np.uint16), uv.reshape(h // 2, w)
