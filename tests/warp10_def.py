"""numpy statement of the plane-wise 10-bit warp with cv::remap's cubic and Lanczos resamplers (include/vstab.h, "Cubic and Lanczos
resampling at 10 bits"; vstab_warp_p010_planar_ex, vstab_set_resample10): the 8-bit definition of warp_def on the ten significant bits.
Test infrastructure only (a plain module).

  sample   s = word >> 6 (0..1023; the low six bits of a source word are ignored), output word = v << 6
  map      warp_def.quantise, warp_def.table, warp_def.FOOTPRINT and warp_def.border_interpolate, unchanged
  taps     CONSTANT: a tap outside the plane enters as the border value (64 luma, 512 chroma); the other modes: every tap at its
           borderInterpolate position
  blend    v = clip((sum w s + 2^14) >> 15, 0, 1023), an arithmetic shift
  chroma   oracle.chroma_maps (0.5f * map at the even pixels of even rows, quantised again), the border decided over the chroma plane's own
           size, U and V blended separately

Also here: the tile budgets of the 10-bit kernels (the model is warp_tiles') and the parameter sets found for them."""
import numpy as np

import oracle
import warp_def as wd
import warp_tiles as wt

BORDER_Y, BORDER_UV = 64, (512, 512)
RESAMPLERS = ("cubic", "lanczos4")
SHIFT = 15
# 24 KiB of LDS in halves: 6144 luma words, 3072 chroma pair dwords (video-annotator_amd/csrc/vstab_warp_p010_resample.hip)
BUDGET = {"luma": 6144, "chroma": 3072}


def remap10(src, mapx, mapy, resampler, border_mode=wd.CONSTANT, border=0, clamp=True):
    """src (h, w) or (h, w, cn) of ten-bit SAMPLES (any integer type, values 0..1023) -> the remapped samples, int64, same channel layout.
    border (CONSTANT only): a number or one per channel.  clamp=False: (sum + 2^14) >> 15 before the clamp to 0..1023."""
    assert resampler in RESAMPLERS and border_mode in wd.ALL_BORDERS, (resampler, border_mode)
    s = np.asarray(src).astype(np.int64)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    K, LO = wd.FOOTPRINT[resampler]
    fold = border_mode in wd.MODES
    bd = np.broadcast_to(np.asarray(border, np.int64), (cn,))
    X, Y, f = wd.quantise(mapx, mapy)
    w = wd.table(resampler)[f]                    # (dh, dw, K, K)
    rows = [wd.border_interpolate(Y - LO + k, sh, border_mode) if fold else Y - LO + k for k in range(K)]
    cols = [wd.border_interpolate(X - LO + k, sw, border_mode) if fold else X - LO + k for k in range(K)]
    acc = np.full(X.shape + (cn,), 1 << (SHIFT - 1), np.int64)
    for k1, ys in enumerate(rows):
        yin = (ys >= 0) & (ys < sh)
        yc = np.clip(ys, 0, sh - 1)
        for k2, xs in enumerate(cols):
            v = s[yc, np.clip(xs, 0, sw - 1)]
            if not fold:
                v = np.where((yin & (xs >= 0) & (xs < sw))[..., None], v, bd)
            acc += w[..., k1, k2][..., None] * v
    out = np.clip(acc >> SHIFT, 0, 1023) if clamp else acc >> SHIFT
    return out[:, :, 0] if flat else out


def planar10(y16, uv16, mx, my, resampler, border_mode=wd.CONSTANT):
    """P010 planes (words; luma (h, w), chroma (h / 2, w) interleaved) and the luma map -> (luma (dh, dw), chroma (ceil(dh / 2),
    2 * ceil(dw / 2))) uint16 words."""
    y10 = np.asarray(y16).view(np.uint16) >> 6
    uv = np.asarray(uv16).view(np.uint16) >> 6
    uv10 = uv.reshape(uv.shape[0], uv.shape[1] // 2, 2)
    cmx, cmy = oracle.chroma_maps(mx, my)
    oy = remap10(y10, mx, my, resampler, border_mode, BORDER_Y)
    ouv = remap10(uv10, cmx, cmy, resampler, border_mode, BORDER_UV)
    return (oy << 6).astype(np.uint16), (ouv.reshape(ouv.shape[0], -1) << 6).astype(np.uint16)


def remap10_float(src, mapx, mapy, resampler, border=0):
    """warp_def.remap_float widened to 1023 and a border value: float bicubic / Lanczos4 of the same quantised position, constant border."""
    s = np.asarray(src, np.float64)
    sh, sw = s.shape
    K, LO = wd.FOOTPRINT[resampler]
    axis = {"cubic": wd._cubic_axis, "lanczos4": wd._lanczos4_axis}[resampler]
    X, Y, f = wd.quantise(mapx, mapy)
    cx, cy = axis((f & 31) / 32.0), axis((f >> 5) / 32.0)
    acc = np.zeros(X.shape)
    for k1 in range(K):
        ys = Y - LO + k1
        for k2 in range(K):
            xs = X - LO + k2
            inside = (ys >= 0) & (ys < sh) & (xs >= 0) & (xs < sw)
            acc += cy[..., k1] * cx[..., k2] * np.where(inside, s[np.clip(ys, 0, sh - 1), np.clip(xs, 0, sw - 1)], float(border))
    return np.clip(np.floor(acc + 0.5), 0, 1023)


def accumulator_bound(resampler):
    """(largest sum of |w| of an entry, the bound of |sum w s + 2^14| for samples in 0..1023)."""
    a = int(np.abs(wd.table(resampler)).sum((1, 2)).max())
    return a, a * 1023 + (1 << (SHIFT - 1))


# ---------------------------------------------------------------------------------------------------------------------
# tiles: warp_tiles' model with the 10-bit budgets
# ---------------------------------------------------------------------------------------------------------------------
def tile_areas(mapx, mapy, sw, sh, resampler, border_mode):
    """-> {plane: (area, have, partial)} per 64 x 16 tile, planes 'luma' and 'chroma': the element count of the tile's box under the rule of
    the border mode (CONSTANT: the footprints that touch; else every footprint), whether it has one, and whether the output's edge cuts it."""
    dh, dw = np.asarray(mapx).shape
    boxes = wt.tile_boxes(mapx, mapy, sw, sh, resampler, wt.kernel_rule(resampler, border_mode))
    out = {}
    for plane in ("luma", "chroma"):
        x0, y0, bw, bh, have = boxes[plane]
        partial = np.zeros(have.shape, bool)
        partial[:, -1] |= dw % wt.TW != 0
        partial[-1, :] |= dh % wt.TH != 0
        out[plane] = (bw * bh, have, partial)
    return out


def tile_states(mapx, mapy, sw, sh, resampler, border_mode):
    """-> {plane: {none, staged, gathered, partial_staged, at_budget, over_by_one, largest_staged, least_gathered}}"""
    out = {}
    for plane, (area, have, partial) in tile_areas(mapx, mapy, sw, sh, resampler, border_mode).items():
        cap = BUDGET[plane]
        staged, gathered = have & (area <= cap), have & (area > cap)
        out[plane] = {"none": int((~have).sum()), "staged": int(staged.sum()), "gathered": int(gathered.sum()),
                      "partial_staged": int((staged & partial).sum()), "at_budget": int((have & (area == cap)).sum()),
                      "over_by_one": int((have & (area == cap + 1)).sum()),
                      "largest_staged": int(area[staged].max()) if staged.any() else None,
                      "least_gathered": int(area[gathered].min()) if gathered.any() else None}
    return out


def set_states(kernel, name, border_mode=None):
    """tile_states of a warp_tiles.TILE_SETS entry with the 10-bit budgets, under its kernel's border mode (or another)."""
    params, sw, sh, dw, dh, mode = wt.set_params(kernel, name)
    resampler, bm = wt.KERNELS[kernel]
    return tile_states(*wd.maps(params, dw, dh, mode), sw, sh, resampler, bm if border_mode is None else border_mode)


# A chroma box of exactly 3072 pairs: no committed set of warp_tiles has one.  Found by scanning anamorphic's sx, sy against the model, as
# warp_tiles' own at-budget sets were (sy in steps of 0.005; the middle of the run that has it): resampler -> (sw, sh, dw, dh, sx, sy, roll,
# map mode).  Two tiles.  CONSTANT: one chroma box of 3072 and one below it, both luma boxes gathered.  REFLECT_101: the box of 3072, and
# the other tile holds map mode 0's axis pixel at -32768, so its boxes are gathered.
CHROMA_AT_BUDGET = {"cubic": (64, 4096, 64, 32, 0.26, 36.06, 0.0, 0), "lanczos4": (64, 4096, 64, 32, 0.26, 26.355, 0.0, 0)}


def chroma_set_params(resampler):
    """-> (params, sw, sh, dw, dh, mode) of a CHROMA_AT_BUDGET entry."""
    sw, sh, dw, dh, sx, sy, roll, mode = CHROMA_AT_BUDGET[resampler]
    return wt.anamorphic(sw, sh, dw, dh, sx, sy, roll), sw, sh, dw, dh, mode
