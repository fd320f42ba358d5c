"""numpy statement of vstab_warp_nv12_dist_ex (include/vstab.h): nothing new is defined -- the distorted lens's map (distort_def.maps) fed
to the resampler's own definition:

  linear    CONSTANT: the oracle's bilinear remap and plane-wise warp (what vstab_warp_nv12_dist is held to, distort_def.warp_bgr /
            warp_planar); other border modes: border_def.remap_border / planar_mapped
  cubic     resample_border_def (CONSTANT: cubic_def.remap_cubic / planar_mapped)
  lanczos4  resample_border_def (CONSTANT: lanczos4_def.remap_lanczos4 / planar_mapped)

and the tile states of the kernels that run it, from the committed CPU models of their boxes (cubic_tiles, lanczos4_tiles, border_tiles,
resample_border_tiles) over the same maps.  Test infrastructure only (a plain module, imported by the tests)."""
import numpy as np

import border_def
import border_tiles
import cubic_tiles
import distort_def as dd
import lanczos4_tiles
import oracle
import resample_border_def as rbd
import resample_border_tiles

CONSTANT, REPLICATE, REFLECT, REFLECT_101 = border_def.CONSTANT, border_def.REPLICATE, border_def.REFLECT, border_def.REFLECT_101
BORDERS = border_def.MODES
RESAMPLERS = ("linear", "cubic", "lanczos4")
RESAMPLE = {"linear": 0, "cubic": 2, "lanczos4": 4}      # VSTAB_RESAMPLE_*


def remap_bgr(resampler, nv12, mx, my, border_mode):
    """cvtColor(NV12 -> BGR), then cv::remap(resampler, border_mode; CONSTANT: 0) with the map planes -> (dh, dw, 3) uint8."""
    src = oracle.cvt_nv12_bgr(np.asarray(nv12))
    if resampler != "linear":
        return rbd.remap_resample_border(resampler, src, mx, my, border_mode, 0)
    if border_mode == CONSTANT:
        return oracle.remap_bilinear(src, mx, my)
    return border_def.remap_border(src, mx, my, border_mode, 0)


def remap_planar(resampler, nv12, mx, my, border_mode):
    """The plane-wise warp with the map planes -> (luma (dh, dw), chroma (ceil(dh / 2), 2 ceil(dw / 2))) uint8."""
    nv12 = np.asarray(nv12)
    if resampler != "linear":
        return rbd.planar_mapped(resampler, nv12, mx, my, border_mode)
    if border_mode == CONSTANT:
        h = nv12.shape[0] * 2 // 3
        return oracle.warp_planar_mapped(nv12[:h], nv12[h:], mx, my)
    return border_def.planar_mapped(nv12, mx, my, border_mode)


def warp_bgr(resampler, nv12, p, dw, dh, mode, D, border_mode):
    mx, my = dd.maps(p, dw, dh, mode, D)
    return remap_bgr(resampler, nv12, mx, my, border_mode)


def warp_planar(resampler, nv12, p, dw, dh, mode, D, border_mode):
    mx, my = dd.maps(p, dw, dh, mode, D)
    return remap_planar(resampler, nv12, mx, my, border_mode)


class Expected:
    """Both output formats of one case from one evaluation of the map."""

    def __init__(self, resampler, nv12, p, dw, dh, mode, D, border_mode):
        mx, my = dd.maps(p, dw, dh, mode, D)
        self.bgr = remap_bgr(resampler, nv12, mx, my, border_mode)
        self.luma, self.chroma = remap_planar(resampler, nv12, mx, my, border_mode)


def tile_states(resampler, mx, my, sw, sh, border_mode):
    """{plane: {state: count}} of the kernel vstab_warp_nv12_dist_ex launches for (resampler, border_mode), from that kernel's CPU model.
    linear + CONSTANT has no such kernel (vstab_warp_nv12_dist's kernels probe their box): border_tiles' model of k_warp_border is not it."""
    assert not (resampler == "linear" and border_mode == CONSTANT)
    if resampler == "linear":
        return border_tiles.tile_states(mx, my, sw, sh, border_mode)
    if border_mode != CONSTANT:
        return resample_border_tiles.tile_states(resampler, mx, my, sw, sh)
    return (cubic_tiles if resampler == "cubic" else lanczos4_tiles).tile_states(mx, my, sw, sh)
