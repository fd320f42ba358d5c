"""numpy statement of the border modes the border kernels are held to: OpenCV 4.5's cv::remap(src, dst, mapx, mapy, INTER_LINEAR, borderMode,
borderValue), CPU path, 8-bit data (include/vstab.h, "Border modes").

  quantisation  sx = cvRound(32 * mapx) (half to even; NaN / outside the int range -> INT_MIN), X = sat16(sx >> 5), fx = sx & 31; same for y
  taps          (X + i, Y + j), i, j in {0, 1}, read at (borderInterpolate(X + i, w), borderInterpolate(Y + j, h)); CONSTANT: the border value
                where the tap lies outside
  blend         sat_u8((w00 p00 + w01 p01 + w10 p10 + w11 p11 + 512) >> 10), w00 = (32 - fx)(32 - fy), w01 = fx (32 - fy), w10 = (32 - fx) fy,
                w11 = fx fy -- the bilinear warp's (oracle/vstab_oracle.c, vo_remap_pixel)

Maps come from the oracle (oracle.create_map_ex / create_map_rs, oracle.create_map_ref_gfx950 / _rs), colour conversion from
oracle.cvt_nv12_bgr, chroma maps from oracle.chroma_maps: the border warp differs from the bilinear one in its border handling alone."""
import numpy as np

import cubic_def
import oracle

CONSTANT, REPLICATE, REFLECT, REFLECT_101 = 0, 1, 2, 4
MODES = (REPLICATE, REFLECT, REFLECT_101)


def border_interpolate_loop(p, n, mode):
    """OpenCV's borderInterpolate(p, len, borderType) as its source states it, for an array of positions p: REPLICATE clamps; REFLECT /
    REFLECT_101 run do { p = p < 0 ? -p - 1 + delta : len - 1 - (p - len) - delta; } while ((unsigned)p >= len), len == 1 -> 0.  Positions
    already inside are returned as they are (the loop is not entered)."""
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
    REFLECT_101 by 2 n - 2 (n == 1 -> 0); CONSTANT leaves p as it is."""
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


def remap_border(src, mapx, mapy, mode, border=0):
    """cv::remap(src, mapx, mapy, INTER_LINEAR, mode, border).  src (h, w) or (h, w, cn) uint8, cn 1..3; border (CONSTANT only) a number or
    one per channel."""
    s = np.asarray(src, np.uint8)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    bd = np.broadcast_to(np.asarray(border, np.int64), (cn,))
    X, Y, f = cubic_def.quantise(mapx, mapy)
    fx, fy = f & 31, f >> 5
    w = [[(32 - fx) * (32 - fy), fx * (32 - fy)], [(32 - fx) * fy, fx * fy]]
    acc = np.full(X.shape + (cn,), 512, np.int64)
    for j in range(2):
        ys = border_interpolate_loop((Y + j).ravel(), sh, mode).reshape(Y.shape) if mode != CONSTANT else Y + j
        for i in range(2):
            xs = border_interpolate_loop((X + i).ravel(), sw, mode).reshape(X.shape) if mode != CONSTANT else X + i
            inside = (xs >= 0) & (xs < sw) & (ys >= 0) & (ys < sh)
            v = np.where(inside[..., None], s[np.clip(ys, 0, sh - 1), np.clip(xs, 0, sw - 1)].astype(np.int64), bd)
            acc += w[j][i][..., None] * v
    out = np.clip(acc >> 10, 0, 255).astype(np.uint8)
    return out[:, :, 0] if flat else out


def maps(params, dw, dh, mode=0, rot_bottom=None):
    """The map of a mode, bit for bit what the kernels evaluate: modes 0..4 the oracle's IEEE statement, 5 the reference kernel on this GPU;
    rot_bottom: vstab_warp_nv12_rs's rotation per output row (modes 0, 1, 5)."""
    if rot_bottom is None:
        return cubic_def.maps(params, dw, dh, mode)
    if mode == 5:
        return oracle.create_map_ref_gfx950_rs(params, rot_bottom, dw, dh)
    return oracle.create_map_rs(params, rot_bottom, dw, dh, mode)


def warp_nv12_border(nv12, params, dw, dh, mode=0, border_mode=REFLECT_101, rot_bottom=None):
    """VSTAB_OUT_BGR8: cvtColor(NV12 -> BGR) of the frame, then the remap with the border mode (CONSTANT: 0) -> (dh, dw, 3) uint8."""
    mx, my = maps(params, dw, dh, mode, rot_bottom)
    return remap_border(oracle.cvt_nv12_bgr(np.asarray(nv12)), mx, my, border_mode, 0)


def warp_nv12_planar_border(nv12, params, dw, dh, mode=0, border_mode=REFLECT_101, rot_bottom=None):
    """VSTAB_OUT_NV12_PLANAR: luma with the map; interleaved chroma with map(2 cx, 2 cy) * 0.5f, border-interpolated over the chroma plane's
    own size (CONSTANT: 16 and (128, 128)) -> (y (dh, dw), uv (ceil(dh / 2), 2 * ceil(dw / 2))) uint8."""
    mx, my = maps(params, dw, dh, mode, rot_bottom)
    return planar_mapped(nv12, mx, my, border_mode)


def planar_mapped(nv12, mx, my, border_mode):
    nv12 = np.asarray(nv12)
    rows, w = nv12.shape
    h = rows * 2 // 3
    y, uv = nv12[:h], nv12[h:].reshape(h // 2, w // 2, 2)
    cmx, cmy = oracle.chroma_maps(mx, my)
    oy = remap_border(y, mx, my, border_mode, 16)
    ouv = remap_border(uv, cmx, cmy, border_mode, (128, 128))
    return oy, ouv.reshape(ouv.shape[0], -1)
