"""numpy statement of vstab_warp_nv12_rs_ex (include/vstab.h): nothing new is defined -- compositions of the definitions the suite
already holds.

  map       without D: border_def.maps (the map of a mode; rot_bottom: the oracle's map with a rotation per output row, modes 0, 1 and 5).
            with D: the distorted lens's map (distort_def.maps, map mode 1) evaluated row by row, row y with the matrix
                m_k = fma(t, rot_bottom[k] - params[8 + k], params[8 + k]),  t = float32(y) / float32(max(dh - 1, 1))
            -- the difference and the quotient each an IEEE binary32 operation, the fma an exact product and sum rounded once to binary32
            (row_matrices) -- in place of the rotation, everything else op for op as distort_def states it.
  resample  distort_resample_def.remap_bgr / remap_planar: linear, cubic, lanczos4 under CONSTANT, REPLICATE, REFLECT and REFLECT_101.

and the tile states of the kernels that run the cubic and Lanczos warps with a rotation per row (k_warp_cubic_rs / k_warp_lanczos4_rs over
resample_tile_rs of vstab_resample.hpp): resample_border_tiles' model for the non-constant border modes, cubic_tiles' / lanczos4_tiles'
for BORDER_CONSTANT.  Test infrastructure only (a plain module, imported by the tests)."""
from fractions import Fraction

import numpy as np

import border_def
import cubic_tiles
import distort_def as dd
import distort_resample_def as drd
import lanczos4_tiles
import resample_border_tiles

F = np.float32
CONSTANT, REPLICATE, REFLECT, REFLECT_101 = border_def.CONSTANT, border_def.REPLICATE, border_def.REFLECT, border_def.REFLECT_101
ALL_BORDERS = (CONSTANT, REPLICATE, REFLECT, REFLECT_101)
RESAMPLERS, RESAMPLE = drd.RESAMPLERS, drd.RESAMPLE


def round_f32(x):
    """The binary32 value nearest the exact rational x, ties to even: one rounding."""
    f = F(float(x))                      # within one binary32 step of the answer (a double rounding at worst)
    best = None
    for c in (np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - x)
        even = (int(np.asarray(c).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, c)
    return best[2]


def fma_f32(a, b, c):
    """fmaf(a, b, c) of three binary32 values: the exact a * b + c rounded once."""
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def row_matrices(params, rot_bottom, dh):
    """(dh, 9) float32: the rotation entries of every output row."""
    p, rb = np.asarray(params, F), np.asarray(rot_bottom, F).reshape(9)
    d = rb - p[8:17]                                     # binary32 subtraction
    den = F(max(dh - 1, 1))
    out = np.empty((dh, 9), F)
    for y in range(dh):
        t = F(y) / den                                   # IEEE division
        out[y] = [fma_f32(t, d[k], p[8 + k]) for k in range(9)]
    return out


def maps(params, dw, dh, mode, rot_bottom, D=None):
    """(mapx, mapy) float32 (dh, dw) of vstab_warp_nv12_rs_ex.  rot_bottom None: one rotation."""
    if D is None:
        return border_def.maps(params, dw, dh, mode, rot_bottom)
    if rot_bottom is None:
        return dd.maps(params, dw, dh, mode, D)
    assert mode == 1
    m = row_matrices(params, rot_bottom, dh)
    mx, my = np.empty((dh, dw), F), np.empty((dh, dw), F)
    for y in range(dh):
        p = np.asarray(params, F).copy()
        p[8:17] = m[y]
        rx, ry = dd.maps(p, dw, y + 1, 1, D)             # rows 0 .. y with row y's matrix: row y is the statement's
        mx[y], my[y] = rx[y], ry[y]
    return mx, my


def warp_bgr(resampler, nv12, params, dw, dh, mode, rot_bottom, D, border_mode):
    mx, my = maps(params, dw, dh, mode, rot_bottom, D)
    return drd.remap_bgr(resampler, nv12, mx, my, border_mode)


def warp_planar(resampler, nv12, params, dw, dh, mode, rot_bottom, D, border_mode):
    mx, my = maps(params, dw, dh, mode, rot_bottom, D)
    return drd.remap_planar(resampler, nv12, mx, my, border_mode)


class Expected:
    """One frame, parameter set and size: the map evaluated once, the definition's frames of any (resampler, border) from it."""

    def __init__(self, nv12, params, dw, dh, mode, rot_bottom, D=None):
        self.f = np.asarray(nv12)
        self.mx, self.my = maps(params, dw, dh, mode, rot_bottom, D)
        self._done = {}

    def bgr(self, resampler, border_mode):
        k = ("bgr", resampler, border_mode)
        if k not in self._done:
            self._done[k] = drd.remap_bgr(resampler, self.f, self.mx, self.my, border_mode)
        return self._done[k]

    def planar(self, resampler, border_mode):
        k = ("planar", resampler, border_mode)
        if k not in self._done:
            self._done[k] = drd.remap_planar(resampler, self.f, self.mx, self.my, border_mode)
        return self._done[k]


# ---------------------------------------------------------------------------------------------------------------------
# tile states of k_warp_cubic_rs / k_warp_lanczos4_rs
# ---------------------------------------------------------------------------------------------------------------------
def tile_states(resampler, mapx, mapy, sw, sh, border_mode):
    """-> {plane: {state: count}} of the kernel vstab_warp_nv12_rs_ex launches for a cubic or Lanczos warp with a rotation per row, from
    the committed CPU models of the boxes: resample_border_tiles' for REPLICATE / REFLECT / REFLECT_101 (every footprint, virtual
    coordinates), cubic_tiles' / lanczos4_tiles' for CONSTANT (the footprints that touch the source; a tile with none has no box)."""
    if border_mode != CONSTANT:
        return resample_border_tiles.tile_states(resampler, mapx, mapy, sw, sh)
    return (cubic_tiles if resampler == "cubic" else lanczos4_tiles).tile_states(mapx, mapy, sw, sh)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the tests (tests/test_rs_resample_cpu.py asserts their tile states, tests/test_rs_resample_gpu.py runs them)
# ---------------------------------------------------------------------------------------------------------------------
R0, R_BOTTOM = (0.02, -0.03, 0.05), (0.03, -0.02, 0.04)


def centred_camera(f, w, h):
    return np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], np.float64)


def case_params(sw, sh, dw, dh, f_in, f_out, r0=R0, r_bottom=R_BOTTOM):
    """-> (params[17], rot_bottom[9]) float32: cameras with their centres at the image centres, the first row's rotation rodrigues(r0),
    the last row's rodrigues(r_bottom) @ rodrigues(r0)."""
    import oracle
    Kin, Kout = centred_camera(f_in, sw, sh), centred_camera(f_out, dw, dh)
    Rt = oracle.rodrigues(r0)
    p = oracle.map_params(Kin, Kout, Rt)
    return p, np.asarray(oracle.map_params(Kin, Kout, oracle.rodrigues(r_bottom) @ Rt)[8:], F)


ZOOMED_OUT = (128, 72, 200, 100, 60.0, 40.0)                        # sw, sh, dw, dh, f_in, f_out
GATHERS = (2048, 512, 128, 32, 900.0, 12.0)
GATHERS_R0, GATHERS_R_BOTTOM = (0.0, 0.0, 0.003), (0.01, 0.0, 0.0)
