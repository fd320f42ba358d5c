"""numpy statement of the Lanczos resampler the Lanczos kernels are held to: OpenCV 4.5's cv::remap(..., INTER_LANCZOS4, BORDER_CONSTANT,
border), CPU path, 8-bit data (include/vstab.h, "Lanczos resampling").

  quantisation  as INTER_LINEAR and INTER_CUBIC (cubic_def.quantise): sx = cvRound(32 * mapx), X = sat16(sx >> 5), fx = sx & 31
  footprint     rows Y - 3 .. Y + 4, columns X - 3 .. X + 4
  1-D rows      interpolateLanczos4(k / 32), k = 0..31: s0 = sin(y0), c0 = cos(y0) of y0 = -(x + 3) * pi / 4 in double, coefficient i =
                (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)) with y = -(x + 3 - i) * pi / 4, summed in fp32 in order i = 0..7, each
                multiplied by 1.f / sum in fp32; x = 0 is the unit row [0, 0, 0, 1, 0, 0, 0, 0] (OpenCV's early return; its other
                version, a 1e30f sentinel for tap 3, gives the same integer table: lanczos4_table(variant="sentinel"))
  weights       entry fy * 32 + fx of initInterTab2D(INTER_LANCZOS4, fixpt): w[k1][k2] = saturate_cast<short>(cvRound(c_fy[k1] * c_fx[k2]
                * 32768.f)), the product in fp32, then the correction that makes the 64 weights sum to 32768, searched in k1, k2 in {4, 5}
  blend         sat_u8((sum_k w_k * (tap_k inside ? S_k : border) + (1 << 14)) >> 15) per channel

Maps, colour conversion and chroma maps are those of the cubic statement (cubic_def.maps, oracle.cvt_nv12_bgr, oracle.chroma_maps): the
Lanczos warp differs from the cubic one in the footprint and the table alone."""
import math

import numpy as np

import cubic_def
import oracle

F = np.float32
# initInterTab2D's correction window: rows / columns {ksize / 2, ksize / 2 + 1} of the 8 x 8 entry (video-annotator_amd/csrc/vstab_lanczos4.hpp,
# LANCZOS4_FIX_LO)
FIX_WINDOW = (4, 5)
_S45 = 0.70710678118654752440084436210485
_CS = ((1, 0), (-_S45, -_S45), (0, 1), (_S45, -_S45), (-1, 0), (_S45, _S45), (0, -1), (-_S45, _S45))
CV_PI = 3.1415926535897932384626433832795

quantise = cubic_def.quantise
maps = cubic_def.maps


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
    """(32, 8) float32: interpolateLanczos4(k / 32) for k = 0..31 from the given sin / cos values (default: sincos()).  variant 'early':
    x = 0 returns the unit row; 'sentinel': tap 3 at x = 0 is 1e30f and goes through the normalisation like the others."""
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
    """(1024, 8, 8) int32: entry fy * 32 + fx, w[k1][k2] weighs tap (X - 3 + k2, Y - 3 + k1).  products=True also returns the fp32
    products c_fy[k1] * c_fx[k2] * 32768.f before rounding (1024, 8, 8)."""
    c = lanczos4_coeffs(s0, c0, variant)
    prod = ((c[:, None, :, None] * c[None, :, None, :]).astype(F) * F(32768)).astype(F).reshape(1024, 8, 8)   # [fy, fx, k1, k2]
    w = np.clip(np.rint(prod).astype(np.int64), -32768, 32767)
    lo, hi = FIX_WINDOW
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
    w = w.astype(np.int32)
    return (w, prod) if products else w


_TAB = None


def _table():
    global _TAB
    if _TAB is None:
        _TAB = lanczos4_table().astype(np.int64)
    return _TAB


def remap_lanczos4(src, mapx, mapy, border=0):
    """cv::remap(src, mapx, mapy, INTER_LANCZOS4, BORDER_CONSTANT, border).  src (h, w) or (h, w, cn) uint8, cn 1..3; border a number or
    one per channel.  Vectorised by tap: 64 gathers over the whole output."""
    s = np.asarray(src, np.uint8)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    bd = np.broadcast_to(np.asarray(border, np.int64), (cn,))
    X, Y, f = quantise(mapx, mapy)
    w = _table()[f]                               # (dh, dw, 8, 8)
    acc = np.full(X.shape + (cn,), 1 << 14, np.int64)
    for k1 in range(8):
        ys = Y - 3 + k1
        yin = (ys >= 0) & (ys < sh)
        yc = np.clip(ys, 0, sh - 1)
        for k2 in range(8):
            xs = X - 3 + k2
            inside = yin & (xs >= 0) & (xs < sw)
            v = np.where(inside[..., None], s[yc, np.clip(xs, 0, sw - 1)].astype(np.int64), bd)
            acc += w[..., k1, k2][..., None] * v
    out = np.clip(acc >> 15, 0, 255).astype(np.uint8)
    return out[:, :, 0] if flat else out


def warp_nv12_lanczos4(nv12, params, dw, dh, mode=0):
    """VSTAB_OUT_BGR8: cvtColor(NV12 -> BGR) of the frame, then the Lanczos remap with border 0 -> (dh, dw, 3) uint8."""
    mx, my = maps(params, dw, dh, mode)
    return remap_lanczos4(oracle.cvt_nv12_bgr(np.asarray(nv12)), mx, my, 0)


def warp_nv12_planar_lanczos4(nv12, params, dw, dh, mode=0):
    """VSTAB_OUT_NV12_PLANAR: luma with the map, border 16; interleaved chroma with map(2 cx, 2 cy) * 0.5f, border (128, 128)
    -> (y (dh, dw), uv (ceil(dh / 2), 2 * ceil(dw / 2))) uint8."""
    mx, my = maps(params, dw, dh, mode)
    return planar_mapped(nv12, mx, my)


def planar_mapped(nv12, mx, my):
    nv12 = np.asarray(nv12)
    rows, w = nv12.shape
    h = rows * 2 // 3
    y, uv = nv12[:h], nv12[h:].reshape(h // 2, w // 2, 2)
    cmx, cmy = oracle.chroma_maps(mx, my)
    oy = remap_lanczos4(y, mx, my, 16)
    ouv = remap_lanczos4(uv, cmx, cmy, (128, 128))
    return oy, ouv.reshape(ouv.shape[0], -1)


def remap_lanczos4_float(src, mapx, mapy):
    """Float Lanczos4 (separable, exact sinc products normalised per axis) of the SAME quantised position, border 0 -- a loose
    cross-check (within a level) of the integer table, not the definition."""
    s = np.asarray(src, np.float64)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    X, Y, f = quantise(mapx, mapy)

    def k(t):
        d = t[..., None] + 3 - np.arange(8)
        c = np.sinc(d) * np.sinc(d / 4)
        return c / c.sum(-1, keepdims=True)
    cx, cy = k((f & 31) / 32.0), k((f >> 5) / 32.0)
    acc = np.zeros(X.shape + (cn,))
    for k1 in range(8):
        ys = Y - 3 + k1
        for k2 in range(8):
            xs = X - 3 + k2
            inside = (ys >= 0) & (ys < sh) & (xs >= 0) & (xs < sw)
            v = np.where(inside[..., None], s[np.clip(ys, 0, sh - 1), np.clip(xs, 0, sw - 1)], 0.0)
            acc += (cy[..., k1] * cx[..., k2])[..., None] * v
    out = np.clip(np.floor(acc + 0.5), 0, 255)
    return out[:, :, 0] if flat else out
