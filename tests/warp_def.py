"""numpy statement of the 8-bit warp the warp kernels are held to: OpenCV 4.5's cv::remap(src, dst, mapx, mapy, interpolation, borderMode,
borderValue), CPU path (include/vstab.h: "Bicubic resampling", "Lanczos resampling", "Border modes", "Border modes of the cubic and
Lanczos resamplers", "Keep edges", vstab_warp_nv12_dist_ex, vstab_warp_nv12_rs_ex).  Test infrastructure only (a plain module).

  quantisation  sx = cvRound(32 * mapx) (half to even; NaN / outside the int range -> INT_MIN), X = sat16(sx >> 5), fx = sx & 31; same for y
  footprint     K x K taps at rows Y - LO .. Y - LO + K - 1 and columns likewise: linear K = 2, LO = 0; cubic 4, 1; Lanczos 8, 3
  weights       entry fy * 32 + fx of the resampler's table, K x K integers that sum to 1 << shift (linear 10, cubic and Lanczos 15)
  taps          CONSTANT: a tap outside the source enters as the border value.  REPLICATE, REFLECT, REFLECT_101: every tap is read at
                (borderInterpolate(x, w), borderInterpolate(y, h)); every table entry sums to one, so OpenCV's cval * ONE + sum((S - cval) * w)
                is sum(S * w).  TRANSPARENT (keep edges, bilinear only): CONSTANT where the sample is `written`, prev's sample elsewhere
  blend         sat_u8((sum_k w_k * tap_k + (1 << (shift - 1))) >> shift) per channel

Order of the module: quantise; the tables; borderInterpolate; remap; the maps; the NV12 warps (planes_of, planar, bgr, Expected); the float
cross-check; the known-answer files; the cases of the rolling-shutter tests.  Maps come from the oracle or from the distorted lens
(distort_def); colour conversion is oracle.cvt_nv12_bgr, chroma maps oracle.chroma_maps.  One branch is not this module's own arithmetic:
bgr / planar with linear + CONSTANT answer with the oracle's C statement (see bgr)."""
import math
import os
from fractions import Fraction

import numpy as np

import distort_def
import oracle

F = np.float32
INT_MIN = -(2 ** 31)
CONSTANT, REPLICATE, REFLECT, REFLECT_101, TRANSPARENT = 0, 1, 2, 4, 5      # VSTAB_BORDER_*; 5 is cv::BORDER_TRANSPARENT (vstab.h, "Keep edges")
MODES = (REPLICATE, REFLECT, REFLECT_101)                                    # the modes that read through borderInterpolate
ALL_BORDERS = (CONSTANT,) + MODES
RESAMPLERS = ("linear", "cubic", "lanczos4")
RESAMPLE = {"linear": 0, "cubic": 2, "lanczos4": 4}                          # VSTAB_RESAMPLE_*
FOOTPRINT = {"linear": (2, 0), "cubic": (4, 1), "lanczos4": (8, 3)}          # resampler -> (K, LO)
SHIFT = {"linear": 10, "cubic": 15, "lanczos4": 15}


def quantise(mapx, mapy):
    """-> X, Y (int64, saturated to int16), table index fy * 32 + fx."""
    def q(m):
        a = (np.asarray(m, F) * F(32)).astype(F)
        with np.errstate(invalid="ignore"):
            ok = (a >= F(-2147483648.0)) & (a < F(2147483648.0))
        s = np.where(ok, np.rint(np.where(ok, a, F(0))).astype(np.int64), INT_MIN)
        return np.clip(s >> 5, -32768, 32767), s & 31
    X, fx = q(mapx)
    Y, fy = q(mapy)
    return X, Y, fy * 32 + fx


# ---------------------------------------------------------------------------------------------------------------------
# the weight tables: entry fy * 32 + fx, w[k1][k2] weighs tap (X - LO + k2, Y - LO + k1)
# ---------------------------------------------------------------------------------------------------------------------
# initInterTab2D's correction window: rows / columns {ksize / 2, ksize / 2 + 1} of the K x K entry (video-annotator_amd/csrc/vstab_cubic.hpp,
# CUBIC_FIX_LO; vstab_lanczos4.hpp, LANCZOS4_FIX_LO).  The one detail nobody can check here without OpenCV:
# test_cubic_matches_opencv_when_present / test_lanczos4_matches_opencv_when_present do where cv2 exists.
FIX_WINDOW = {"cubic": (2, 3), "lanczos4": (4, 5)}
_S45 = 0.70710678118654752440084436210485
_CS = ((1, 0), (-_S45, -_S45), (0, 1), (_S45, -_S45), (-1, 0), (_S45, _S45), (0, -1), (-_S45, _S45))
CV_PI = 3.1415926535897932384626433832795


def bilinear_table():
    """(1024, 2, 2) int32: (32 - fx)(32 - fy), fx (32 - fy) / (32 - fx) fy, fx fy -- the bilinear warp's weights (oracle/vstab_oracle.c,
    vo_remap_pixel), which sum to 1024."""
    f = np.arange(32)
    a = np.stack([32 - f, f], axis=1)                                        # [f, k]
    return (a[:, None, :, None] * a[None, :, None, :]).reshape(1024, 2, 2).astype(np.int32)


def _fixed_point(c, window):
    """initInterTab2D(fixpt) of the 1-D rows c (32, K) float32: w[k1][k2] = saturate_cast<short>(cvRound(c_fy[k1] * c_fx[k2] * 32768.f)), the
    product in fp32, then the correction that makes the K * K weights sum to 32768, searched in k1, k2 in the window
    -> (weights (1024, K, K) int32, the fp32 products before rounding)."""
    K = c.shape[1]
    prod = ((c[:, None, :, None] * c[None, :, None, :]).astype(F) * F(32768)).astype(F).reshape(1024, K, K)   # [fy, fx, k1, k2]
    w = np.clip(np.rint(prod).astype(np.int64), -32768, 32767)
    lo, hi = window
    for e in range(1024):
        t = w[e]
        diff = int(t.sum()) - 32768
        if diff == 0:
            continue
        mk = Mk = (lo, lo)
        for k1 in range(lo, hi + 1):
            for k2 in range(lo, hi + 1):
                if t[k1, k2] < t[mk]:
                    mk = (k1, k2)
                elif t[k1, k2] > t[Mk]:
                    Mk = (k1, k2)
        if diff < 0:
            t[Mk] -= diff
        else:
            t[mk] -= diff
        t[:] = (t + 32768) % 65536 - 32768   # (short) of the corrected weight
    return w.astype(np.int32), prod


def cubic_coeffs():
    """(32, 4) float32: interpolateCubic(k / 32) (A = -0.75) for k = 0..31, every operation rounded to fp32 in imgwarp.cpp's order."""
    A = F(-0.75)
    x = (np.arange(32, dtype=F) * F(1.0 / 32)).astype(F)
    one = F(1)
    xp = (x + one).astype(F)
    c0 = (((((A * xp).astype(F) - F(5) * A).astype(F) * xp).astype(F) + F(8) * A).astype(F) * xp).astype(F) - F(4) * A
    c1 = ((((F(A + F(2)) * x).astype(F) - F(A + F(3))).astype(F) * x).astype(F) * x).astype(F) + one
    xm = (one - x).astype(F)
    c2 = ((((F(A + F(2)) * xm).astype(F) - F(A + F(3))).astype(F) * xm).astype(F) * xm).astype(F) + one
    c3 = (((one - c0.astype(F)).astype(F) - c1.astype(F)).astype(F) - c2.astype(F)).astype(F)
    return np.stack([c0.astype(F), c1.astype(F), c2.astype(F), c3], axis=1)


def cubic_table():
    """(1024, 4, 4) int32 of initInterTab2D(INTER_CUBIC, fixpt)."""
    return _fixed_point(cubic_coeffs(), FIX_WINDOW["cubic"])[0]


def sincos():
    """The 32 (s0, c0) pairs of interpolateLanczos4 in double, from this host's libm: what vstab_lanczos4.hpp commits as literals."""
    s0, c0 = [], []
    for k in range(32):
        x = F(k) * F(1.0 / 32)
        y0 = -float(F(x + F(3))) * CV_PI * 0.25
        s0.append(math.sin(y0))
        c0.append(math.cos(y0))
    return s0, c0


def lanczos4_coeffs(s0=None, c0=None, variant="early"):
    """(32, 8) float32: interpolateLanczos4(k / 32) for k = 0..31 from the given sin / cos values (default: sincos()): s0 = sin(y0),
    c0 = cos(y0) of y0 = -(x + 3) * pi / 4 in double, coefficient i = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)) with
    y = -(x + 3 - i) * pi / 4, summed in fp32 in order i = 0..7, each multiplied by 1.f / sum in fp32.  variant 'early': x = 0 returns the
    unit row (OpenCV's early return); 'sentinel': tap 3 at x = 0 is 1e30f and goes through the normalisation like the others (OpenCV's
    other version; it gives the same integer table)."""
    if s0 is None:
        s0, c0 = sincos()
    out = np.zeros((32, 8), F)
    for k in range(32):
        x = F(k) * F(1.0 / 32)
        if variant == "early" and x < np.finfo(F).eps:
            out[k, 3] = 1
            continue
        c = np.zeros(8, F)
        s = F(0)
        for i in range(8):
            t = F(F(x + F(3)) - F(i))
            if variant == "sentinel" and abs(float(t)) < 1e-6:
                c[i] = F(1e30)
            else:
                y = -float(t) * CV_PI * 0.25
                c[i] = F((_CS[i][0] * s0[k] + _CS[i][1] * c0[k]) / (y * y))
            s = F(s + c[i])
        out[k] = (c * (F(1) / s)).astype(F)
    return out


def lanczos4_table(s0=None, c0=None, variant="early", products=False):
    """(1024, 8, 8) int32 of initInterTab2D(INTER_LANCZOS4, fixpt).  products=True also returns the fp32 products c_fy[k1] * c_fx[k2] *
    32768.f before rounding (1024, 8, 8)."""
    w, prod = _fixed_point(lanczos4_coeffs(s0, c0, variant), FIX_WINDOW["lanczos4"])
    return (w, prod) if products else w


_TABLES = {}


def table(resampler):
    """(1024, K, K) int64 weights of the resampler (computed once)."""
    if resampler not in _TABLES:
        _TABLES[resampler] = {"linear": bilinear_table, "cubic": cubic_table, "lanczos4": lanczos4_table}[resampler]().astype(np.int64)
    return _TABLES[resampler]


# ---------------------------------------------------------------------------------------------------------------------
# borderInterpolate
# ---------------------------------------------------------------------------------------------------------------------
def border_interpolate_loop(p, n, mode):
    """OpenCV's borderInterpolate(p, len, borderType) as its source states it, for an array of positions p: REPLICATE clamps; REFLECT /
    REFLECT_101 run do { p = p < 0 ? -p - 1 + delta : len - 1 - (p - len) - delta; } while ((unsigned)p >= len), len == 1 -> 0.  Positions
    already inside are returned as they are (the loop is not entered).  The independent statement: remap does not use it."""
    p = np.array(p, np.int64, copy=True)
    if mode == REPLICATE:
        return np.clip(p, 0, n - 1)
    assert mode in (REFLECT, REFLECT_101)
    if n == 1:
        return np.zeros_like(p)
    delta = 1 if mode == REFLECT_101 else 0
    idx = np.nonzero((p < 0) | (p >= n))[0]
    q = p[idx]
    while idx.size:
        q = np.where(q < 0, -q - 1 + delta, n - 1 - (q - n) - delta)
        done = (q >= 0) & (q < n)
        p[idx[done]] = q[done]
        idx, q = idx[~done], q[~done]
    return p


def border_interpolate(p, n, mode):
    """The closed form the kernels use (csrc/vstab_resample.hpp, border_index): REPLICATE clamps; REFLECT folds by the period 2 n and
    REFLECT_101 by 2 n - 2 (n == 1 -> 0); CONSTANT leaves p as it is.  Equal to the loop over every position a footprint reaches
    (test_closed_form_equals_opencv_loop, test_closed_form_equals_opencv_loop_over_footprints)."""
    p = np.asarray(p, np.int64)
    if mode == CONSTANT:
        return p
    inside = (p >= 0) & (p < n)
    if mode == REPLICATE:
        return np.where(inside, p, np.where(p < 0, 0, n - 1))
    d = 1 if mode == REFLECT_101 else 0
    if d and n == 1:
        return np.zeros_like(p)
    per = 2 * n - 2 * d
    q = np.fmod(p, per)
    q = q + np.where(q < 0, per, 0)
    return np.where(inside, p, np.where(q < n, q, per - 1 + d - q))


# ---------------------------------------------------------------------------------------------------------------------
# remap
# ---------------------------------------------------------------------------------------------------------------------
def inlier(X, Y, sw, sh):
    """The quantised positions whose 2 x 2 footprint lies wholly inside the plane: 0 <= X <= sw - 2 and 0 <= Y <= sh - 2 -- cv::remap's
    inlier test (unsigned)X < w - 1.  So an exact hit on the last column or row is none, a NaN entry (X = Y = -32768) is none, and a plane
    with a length below 2 has none."""
    return (X >= 0) & (X <= sw - 2) & (Y >= 0) & (Y <= sh - 2)


def written(mapx, mapy, sw, sh):
    """-> bool (dh, dw): the samples the keep-edge warp writes, the inliers; every other keeps prev's sample."""
    X, Y, _ = quantise(mapx, mapy)
    return inlier(X, Y, sw, sh)


def remap(src, mapx, mapy, resampler="linear", border_mode=CONSTANT, border=0, prev=None):
    """cv::remap(src, mapx, mapy, INTER_LINEAR / _CUBIC / _LANCZOS4, border_mode, border).  src (h, w) or (h, w, cn) uint8, cn 1..3; border
    (CONSTANT only) a number or one per channel; prev (TRANSPARENT only) shaped as the output, not modified.  Vectorised by tap: K * K
    gathers over the whole output."""
    assert border_mode in ALL_BORDERS or (border_mode == TRANSPARENT and resampler == "linear"), (resampler, border_mode)
    s = np.asarray(src, np.uint8)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    (K, LO), shift = FOOTPRINT[resampler], SHIFT[resampler]
    fold = border_mode in MODES
    bd = np.broadcast_to(np.asarray(border, np.int64), (cn,))
    X, Y, f = quantise(mapx, mapy)
    w = table(resampler)[f]                       # (dh, dw, K, K)
    rows = [border_interpolate(Y - LO + k, sh, border_mode) if fold else Y - LO + k for k in range(K)]
    cols = [border_interpolate(X - LO + k, sw, border_mode) if fold else X - LO + k for k in range(K)]
    acc = np.full(X.shape + (cn,), 1 << (shift - 1), np.int64)
    for k1, ys in enumerate(rows):
        yin = (ys >= 0) & (ys < sh)
        yc = np.clip(ys, 0, sh - 1)
        for k2, xs in enumerate(cols):
            v = s[yc, np.clip(xs, 0, sw - 1)].astype(np.int64)
            if not fold:
                v = np.where((yin & (xs >= 0) & (xs < sw))[..., None], v, bd)
            acc += w[..., k1, k2][..., None] * v
    out = np.clip(acc >> shift, 0, 255).astype(np.uint8)
    if border_mode == TRANSPARENT:
        out = np.where(written(mapx, mapy, sw, sh)[..., None], out, np.asarray(prev, np.uint8).reshape(out.shape))
    return out[:, :, 0] if flat else out


# ---------------------------------------------------------------------------------------------------------------------
# the maps
# ---------------------------------------------------------------------------------------------------------------------
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
    """(dh, 9) float32: the rotation entries of every output row of the distorted lens with a rotation per row,
    m_k = fma(t, rot_bottom[k] - params[8 + k], params[8 + k]), t = float32(y) / float32(max(dh - 1, 1)) -- the difference and the quotient
    each an IEEE binary32 operation, the fma an exact product and sum rounded once to binary32."""
    p, rb = np.asarray(params, F), np.asarray(rot_bottom, F).reshape(9)
    d = rb - p[8:17]                                     # binary32 subtraction
    den = F(max(dh - 1, 1))
    out = np.empty((dh, 9), F)
    for y in range(dh):
        t = F(y) / den                                   # IEEE division
        out[y] = [fma_f32(t, d[k], p[8 + k]) for k in range(9)]
    return out


def maps(params, dw, dh, mode=0, rot_bottom=None, D=None):
    """(mapx, mapy) float32 (dh, dw), bit for bit what the kernels evaluate.  Without D: modes 0..4 the oracle's IEEE statement, 5 the
    reference kernel on this GPU; rot_bottom: the rotation per output row (modes 0, 1, 5).  With D: the distorted fisheye lens's map
    (distort_def.maps), with rot_bottom (map mode 1) evaluated row by row, row y with row_matrices' matrix in place of the rotation."""
    if D is None:
        if rot_bottom is None:
            return oracle.create_map_ref_gfx950(params, dw, dh) if mode == 5 else oracle.create_map_ex(params, dw, dh, mode)
        if mode == 5:
            return oracle.create_map_ref_gfx950_rs(params, rot_bottom, dw, dh)
        return oracle.create_map_rs(params, rot_bottom, dw, dh, mode)
    if rot_bottom is None:
        return distort_def.maps(params, dw, dh, mode, D)
    assert mode == 1
    m = row_matrices(params, rot_bottom, dh)
    mx, my = np.empty((dh, dw), F), np.empty((dh, dw), F)
    for y in range(dh):
        p = np.asarray(params, F).copy()
        p[8:17] = m[y]
        rx, ry = distort_def.maps(p, dw, y + 1, 1, D)    # rows 0 .. y with row y's matrix: row y is the statement's
        mx[y], my[y] = rx[y], ry[y]
    return mx, my


# ---------------------------------------------------------------------------------------------------------------------
# the NV12 warps
# ---------------------------------------------------------------------------------------------------------------------
def planes_of(nv12):
    """Packed NV12 (3 h / 2, w) -> luma (h, w), interleaved chroma (h / 2, w / 2, 2)."""
    nv12 = np.asarray(nv12)
    rows, w = nv12.shape
    h = rows * 2 // 3
    return nv12[:h], nv12[h:].reshape(h // 2, w // 2, 2)


def planar(nv12, mx, my, resampler="linear", border_mode=CONSTANT, prev_y=None, prev_uv=None):
    """VSTAB_OUT_NV12_PLANAR: luma with the map, border 16; interleaved chroma with map(2 cx, 2 cy) * 0.5f, border (128, 128), its border
    mode (and, keeping edges, its written samples) decided over the chroma plane's own size; prev_y (dh, dw) and prev_uv (ceil(dh / 2),
    2 * ceil(dw / 2)) with TRANSPARENT -> (y (dh, dw), uv (ceil(dh / 2), 2 * ceil(dw / 2))) uint8."""
    y, uv = planes_of(nv12)
    if resampler == "linear" and border_mode == CONSTANT:                    # the kept branch: see bgr
        return oracle.warp_planar_mapped(y, np.asarray(nv12)[y.shape[0]:], mx, my)
    cmx, cmy = oracle.chroma_maps(mx, my)
    oy = remap(y, mx, my, resampler, border_mode, 16, prev_y)
    ouv = remap(uv, cmx, cmy, resampler, border_mode, (128, 128), prev_uv)
    return oy, ouv.reshape(ouv.shape[0], -1)


def bgr(nv12, mx, my, resampler="linear", border_mode=CONSTANT, prev=None):
    """VSTAB_OUT_BGR8: cvtColor(NV12 -> BGR) of the frame, then the remap (CONSTANT: border 0; TRANSPARENT: over prev (dh, dw, 3))
    -> (dh, dw, 3) uint8.  The one deliberate branch: linear + CONSTANT answers with the oracle's C statement (oracle.remap_bilinear; planar:
    oracle.warp_planar_mapped), so the GPU tests of the bilinear path stay on the older, independent statement;
    test_constant_equals_oracle_bilinear and test_constant_warp_equals_oracle_warps hold remap against it."""
    src = oracle.cvt_nv12_bgr(np.asarray(nv12))
    if resampler == "linear" and border_mode == CONSTANT:
        return oracle.remap_bilinear(src, mx, my)
    return remap(src, mx, my, resampler, border_mode, 0, prev)


class Expected:
    """One frame and one map: the definition's frames of any (resampler, border mode), each computed once."""

    def __init__(self, nv12, mx, my):
        self.f, self.mx, self.my = np.asarray(nv12), mx, my
        self._done = {}

    def _once(self, fn, resampler, border_mode):
        k = (fn, resampler, border_mode)
        if k not in self._done:
            self._done[k] = fn(self.f, self.mx, self.my, resampler, border_mode)
        return self._done[k]

    def bgr(self, resampler, border_mode):
        return self._once(bgr, resampler, border_mode)

    def planar(self, resampler, border_mode):
        return self._once(planar, resampler, border_mode)


# ---------------------------------------------------------------------------------------------------------------------
# the float cross-check
# ---------------------------------------------------------------------------------------------------------------------
def _cubic_axis(t):
    A = -0.75
    c = [((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
         ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1]
    return np.stack(c + [1 - c[0] - c[1] - c[2]], axis=-1)


def _lanczos4_axis(t):
    d = t[..., None] + 3 - np.arange(8)
    c = np.sinc(d) * np.sinc(d / 4)
    return c / c.sum(-1, keepdims=True)


def remap_float(src, mapx, mapy, resampler):
    """Float bicubic (A = -0.75) or Lanczos4 (sinc products normalised per axis), separable with exact coefficients, of the SAME quantised
    position, border 0 -- a loose cross-check (within a level) of the integer table, not the definition."""
    s = np.asarray(src, np.float64)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    K, LO = FOOTPRINT[resampler]
    axis = {"cubic": _cubic_axis, "lanczos4": _lanczos4_axis}[resampler]
    X, Y, f = quantise(mapx, mapy)
    cx, cy = axis((f & 31) / 32.0), axis((f >> 5) / 32.0)
    acc = np.zeros(X.shape + (cn,))
    for k1 in range(K):
        ys = Y - LO + k1
        for k2 in range(K):
            xs = X - LO + k2
            inside = (ys >= 0) & (ys < sh) & (xs >= 0) & (xs < sw)
            v = np.where(inside[..., None], s[np.clip(ys, 0, sh - 1), np.clip(xs, 0, sw - 1)], 0.0)
            acc += (cy[..., k1] * cx[..., k2])[..., None] * v
    out = np.clip(np.floor(acc + 0.5), 0, 255)
    return out[:, :, 0] if flat else out


# ---------------------------------------------------------------------------------------------------------------------
# the known-answer files
# ---------------------------------------------------------------------------------------------------------------------
def golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


def golden_cases(name, *fields):
    """(k, case<k>_<field> for each field) of every case of tests/golden/<name>.npz; a field of no dimension comes as an int."""
    g = golden(name)
    k = 0
    while f"case{k}_{fields[0]}" in g:
        yield (k,) + tuple(g[f"case{k}_{f}"] if g[f"case{k}_{f}"].ndim else int(g[f"case{k}_{f}"]) for f in fields)
        k += 1


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the rolling-shutter tests (tests/test_rs_resample_cpu.py asserts their tile states, tests/test_rs_resample_gpu.py runs them)
# ---------------------------------------------------------------------------------------------------------------------
R0, R_BOTTOM = (0.02, -0.03, 0.05), (0.03, -0.02, 0.04)


def centred_camera(f, w, h):
    return np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], np.float64)


def case_params(sw, sh, dw, dh, f_in, f_out, r0=R0, r_bottom=R_BOTTOM):
    """-> (params[17], rot_bottom[9]) float32: cameras with their centres at the image centres, the first row's rotation rodrigues(r0),
    the last row's rodrigues(r_bottom) @ rodrigues(r0)."""
    Kin, Kout = centred_camera(f_in, sw, sh), centred_camera(f_out, dw, dh)
    Rt = oracle.rodrigues(r0)
    p = oracle.map_params(Kin, Kout, Rt)
    return p, np.asarray(oracle.map_params(Kin, Kout, oracle.rodrigues(r_bottom) @ Rt)[8:], F)


ZOOMED_OUT = (128, 72, 200, 100, 60.0, 40.0)                        # sw, sh, dw, dh, f_in, f_out
GATHERS = (2048, 512, 128, 32, 900.0, 12.0)
GATHERS_R0, GATHERS_R_BOTTOM = (0.0, 0.0, 0.003), (0.01, 0.0, 0.0)
