"""numpy statement of the border modes of the cubic and Lanczos resamplers: OpenCV 4.5's cv::remap(src, dst, mapx, mapy, INTER_CUBIC or
INTER_LANCZOS4, borderMode), CPU remapBicubic / remapLanczos4, 8-bit data, on the branch taken when borderMode is not BORDER_CONSTANT
(include/vstab.h, "Border modes of the cubic and Lanczos resamplers").

  quantisation  cubic_def.quantise: X = sat16(cvRound(32 * mapx) >> 5), f = fy * 32 + fx
  taps          (X - LO + i, Y - LO + j), i, j in 0 .. K - 1 (cubic K = 4, LO = 1; Lanczos K = 8, LO = 3), read at
                (borderInterpolate(x, w), borderInterpolate(y, h)) -- border_def.border_interpolate, the closed form the kernels use, equal
                to OpenCV's loop (border_def.border_interpolate_loop) over every position a footprint reaches (tests/test_resample_border_cpu.py)
  weights       the resampler's table (cubic_def.cubic_table, lanczos4_def.lanczos4_table), every entry summing to 32768, so OpenCV's
                cval * ONE + sum((S - cval) * w) is sum(S * w)
  blend         sat_u8((sum + 2^14) >> 15)
  CONSTANT      cubic_def.remap_cubic / lanczos4_def.remap_lanczos4 with the border value

Maps come from the oracle (cubic_def.maps), colour conversion from oracle.cvt_nv12_bgr, chroma maps from oracle.chroma_maps."""
import numpy as np

import border_def
import cubic_def
import lanczos4_def
import oracle

CONSTANT, REPLICATE, REFLECT, REFLECT_101 = border_def.CONSTANT, border_def.REPLICATE, border_def.REFLECT, border_def.REFLECT_101
MODES = border_def.MODES
FOOTPRINT = {"cubic": (4, 1), "lanczos4": (8, 3)}   # resampler -> (K, LO)


def table(resampler):
    """(1024, K, K) int64 weights of the resampler."""
    return cubic_def._table() if resampler == "cubic" else lanczos4_def._table()


def remap_resample_border(resampler, src, mapx, mapy, mode, border=0):
    """cv::remap(src, mapx, mapy, INTER_CUBIC / INTER_LANCZOS4, mode, border).  src (h, w) or (h, w, cn) uint8, cn 1..3; border (CONSTANT
    only) a number or one per channel.  Vectorised by tap: K * K gathers over the whole output."""
    if mode == CONSTANT:
        f = cubic_def.remap_cubic if resampler == "cubic" else lanczos4_def.remap_lanczos4
        return f(src, mapx, mapy, border)
    assert mode in MODES, mode
    K, LO = FOOTPRINT[resampler]
    s = np.asarray(src, np.uint8)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, _ = s.shape
    X, Y, f = cubic_def.quantise(mapx, mapy)
    w = table(resampler)[f]                       # (dh, dw, K, K)
    acc = np.full(X.shape + (s.shape[2],), 1 << 14, np.int64)
    for k1 in range(K):
        ys = border_def.border_interpolate(Y - LO + k1, sh, mode)
        for k2 in range(K):
            xs = border_def.border_interpolate(X - LO + k2, sw, mode)
            acc += w[..., k1, k2][..., None] * s[ys, xs].astype(np.int64)
    out = np.clip(acc >> 15, 0, 255).astype(np.uint8)
    return out[:, :, 0] if flat else out


def remap_cubic_border(src, mapx, mapy, mode, border=0):
    return remap_resample_border("cubic", src, mapx, mapy, mode, border)


def remap_lanczos4_border(src, mapx, mapy, mode, border=0):
    return remap_resample_border("lanczos4", src, mapx, mapy, mode, border)


def warp_nv12(resampler, nv12, params, dw, dh, mode=0, border_mode=REFLECT_101):
    """VSTAB_OUT_BGR8: cvtColor(NV12 -> BGR) of the frame, then the remap with the border mode (CONSTANT: 0) -> (dh, dw, 3) uint8."""
    mx, my = cubic_def.maps(params, dw, dh, mode)
    return remap_resample_border(resampler, oracle.cvt_nv12_bgr(np.asarray(nv12)), mx, my, border_mode, 0)


def warp_nv12_planar(resampler, nv12, params, dw, dh, mode=0, border_mode=REFLECT_101):
    """VSTAB_OUT_NV12_PLANAR: luma with the map; interleaved chroma with map(2 cx, 2 cy) * 0.5f, folded over the chroma plane's own size
    (CONSTANT: 16 and (128, 128)) -> (y (dh, dw), uv (ceil(dh / 2), 2 * ceil(dw / 2))) uint8."""
    mx, my = cubic_def.maps(params, dw, dh, mode)
    return planar_mapped(resampler, nv12, mx, my, border_mode)


def planar_mapped(resampler, nv12, mx, my, border_mode):
    nv12 = np.asarray(nv12)
    rows, w = nv12.shape
    h = rows * 2 // 3
    y, uv = nv12[:h], nv12[h:].reshape(h // 2, w // 2, 2)
    cmx, cmy = oracle.chroma_maps(mx, my)
    oy = remap_resample_border(resampler, y, mx, my, border_mode, 16)
    ouv = remap_resample_border(resampler, uv, cmx, cmy, border_mode, (128, 128))
    return oy, ouv.reshape(ouv.shape[0], -1)
