"""numpy statement of the keep-edge warp (include/vstab.h, "Keep edges"): cv::remap(INTER_LINEAR) where the 2 x 2 footprint lies wholly inside
the plane it reads, the caller's previous frame everywhere else -- cv::remap's BORDER_TRANSPARENT for 1- and 2-channel data, vid.stab's `keep`.

  quantisation  sx = cvRound(32 * mapx) (half to even; NaN / outside the int range -> INT_MIN), X = sat16(sx >> 5), fx = sx & 31; same for y
                (cubic_def.quantise)
  written       0 <= X <= len_x - 2 and 0 <= Y <= len_y - 2 -- cv::remap's inlier test (unsigned)X < w - 1
  value         (w00 p00 + w01 p01 + w10 p10 + w11 p11 + 512) >> 10, w00 = (32 - fx)(32 - fy), w01 = fx (32 - fy), w10 = (32 - fx) fy,
                w11 = fx fy: the four taps are all inside, no border value enters
  kept          every other sample is prev's at the same position (all channels of a sample together)

So an exact hit on the last column or row is kept, a NaN entry (X = Y = -32768) is kept, and a plane with len < 2 keeps everything.
Maps come from the oracle as in border_def; BGR converts before the remap; the plane-wise chroma plane is decided on its own, with
map(2 cx, 2 cy) * 0.5f over (w / 2) x (h / 2)."""
import numpy as np

import border_def
import cubic_def
import oracle


def written(mapx, mapy, sw, sh):
    """-> bool (dh, dw): the samples that are written."""
    X, Y, _ = cubic_def.quantise(mapx, mapy)
    return (X >= 0) & (X <= sw - 2) & (Y >= 0) & (Y <= sh - 2)


def remap_keep(src, mapx, mapy, prev):
    """src (h, w) or (h, w, cn) uint8; prev shaped as the output (dh, dw[, cn]) -> the output; prev is not modified."""
    s = np.asarray(src, np.uint8)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    X, Y, f = cubic_def.quantise(mapx, mapy)
    m = (X >= 0) & (X <= sw - 2) & (Y >= 0) & (Y <= sh - 2)
    out = np.array(prev, np.uint8, copy=True).reshape(X.shape + (cn,))
    x, y, fx, fy = X[m], Y[m], (f & 31)[m][:, None], (f >> 5)[m][:, None]
    p = s.astype(np.int64)
    acc = (32 - fx) * (32 - fy) * p[y, x] + fx * (32 - fy) * p[y, x + 1] + (32 - fx) * fy * p[y + 1, x] + fx * fy * p[y + 1, x + 1] + 512
    out[m] = (acc >> 10).astype(np.uint8)
    return out[:, :, 0] if flat else out


def warp_nv12_keep(nv12, params, dw, dh, prev, mode=0, rot_bottom=None):
    """VSTAB_OUT_BGR8: cvtColor(NV12 -> BGR) of the frame, then the keep-edge remap over prev (dh, dw, 3) -> (dh, dw, 3) uint8."""
    mx, my = border_def.maps(params, dw, dh, mode, rot_bottom)
    return remap_keep(oracle.cvt_nv12_bgr(np.asarray(nv12)), mx, my, np.asarray(prev).reshape(dh, dw, 3))


def planes_of(nv12):
    nv12 = np.asarray(nv12)
    rows, w = nv12.shape
    h = rows * 2 // 3
    return nv12[:h], nv12[h:].reshape(h // 2, w // 2, 2)


def warp_nv12_planar_keep(nv12, params, dw, dh, prev_y, prev_uv, mode=0, rot_bottom=None):
    """VSTAB_OUT_NV12_PLANAR: luma over prev_y (dh, dw); interleaved chroma over prev_uv (ceil(dh / 2), 2 * ceil(dw / 2)), decided over the
    chroma plane's own size -> (y, uv) uint8."""
    mx, my = border_def.maps(params, dw, dh, mode, rot_bottom)
    y, uv = planes_of(nv12)
    cmx, cmy = oracle.chroma_maps(mx, my)
    ch, cw = cmx.shape
    oy = remap_keep(y, mx, my, np.asarray(prev_y).reshape(dh, dw))
    ouv = remap_keep(uv, cmx, cmy, np.asarray(prev_uv).reshape(ch, cw, 2))
    return oy, ouv.reshape(ch, 2 * cw)


def masks(params, sw, sh, dw, dh, mode=0, rot_bottom=None):
    """-> (luma / BGR mask (dh, dw), chroma mask (ceil(dh / 2), ceil(dw / 2))) of a warp from a sw x sh frame."""
    mx, my = border_def.maps(params, dw, dh, mode, rot_bottom)
    cmx, cmy = oracle.chroma_maps(mx, my)
    return written(mx, my, sw, sh), written(cmx, cmy, sw >> 1, sh >> 1)
