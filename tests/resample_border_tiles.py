"""CPU model of the tile boxes of the cubic and Lanczos border warps (k_warp_cubic_border / k_warp_lanczos4_border,
video-annotator_amd/csrc/vstab_warp_cubic.hip / vstab_warp_lanczos4.hip over resample_tile of vstab_resample.hpp), restated from exact map
planes.  Test infrastructure only (a plain module).

As tests/border_tiles.py states it for the bilinear border warp, with the resampler's footprint: per 64 x 16 output tile and plane, every
pixel's quantised tap (X, Y) counts (chroma: the even lanes of the even rows, from 0.5f * map over the chroma plane), and the box in virtual
coordinates covers columns min X - LO .. max X - LO + K - 1 and rows likewise (cubic K = 4, LO = 1; Lanczos K = 8, LO = 3).  It is staged
when its area is within the budget (6144 BGRx dwords, 12288 luma bytes, 6144 chroma pairs), gathered from global memory otherwise."""
import numpy as np

import border_tiles
import cubic_def
import oracle
import resample_border_def

TW, TH = border_tiles.TW, border_tiles.TH
BUDGET = border_tiles.BUDGET
STATES = ("staged", "gathered", "at_budget", "outside_staged", "cross_l", "cross_r", "cross_t", "cross_b", "odd_w", "even_w")


def _boxes(X, Y, ty, tx, rh, rw, K, LO):
    X, Y = border_tiles._tiled(X, ty, tx, rh, rw), border_tiles._tiled(Y, ty, tx, rh, rw)
    x0, y0 = X.min(-1) - LO, Y.min(-1) - LO
    return x0, y0, X.max(-1) - LO + K - x0, Y.max(-1) - LO + K - y0


def tile_boxes(resampler, mapx, mapy, sw, sh):
    """Exact map planes (dh, dw) of a warp from a sw x sh source -> {plane: (x0, y0, bw, bh)}, arrays of shape (tile rows, tile columns)."""
    K, LO = resample_border_def.FOOTPRINT[resampler]
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    dh, dw = mapx.shape
    ty, tx = -(-dh // TH), -(-dw // TW)
    pad = ((0, ty * TH - dh), (0, tx * TW - dw))
    mx, my = np.pad(mapx, pad, mode="edge"), np.pad(mapy, pad, mode="edge")
    X, Y, _ = cubic_def.quantise(mx, my)
    full = _boxes(X, Y, ty, tx, TH, TW, K, LO)
    cx, cy, _ = cubic_def.quantise(mx[::2, ::2] * np.float32(0.5), my[::2, ::2] * np.float32(0.5))
    return {"bgr": full, "luma": full, "chroma": _boxes(cx, cy, ty, tx, TH // 2, TW // 2, K, LO)}


def tile_states(resampler, mapx, mapy, sw, sh):
    """-> {plane: {state: count}} with the states of border_tiles.tile_states."""
    out = {}
    for plane, (x0, y0, bw, bh) in tile_boxes(resampler, mapx, mapy, sw, sh).items():
        w, h = (sw, sh) if plane != "chroma" else (sw >> 1, sh >> 1)
        area = bw * bh
        staged = area <= BUDGET[plane]
        outside = (x0 + bw <= 0) | (x0 >= w) | (y0 + bh <= 0) | (y0 >= h)
        out[plane] = {
            "staged": int(staged.sum()), "gathered": int((~staged).sum()), "at_budget": int((area == BUDGET[plane]).sum()),
            "outside_staged": int((staged & outside).sum()),
            "cross_l": int((staged & (x0 < 0) & (x0 + bw > 0)).sum()), "cross_r": int((staged & (x0 < w) & (x0 + bw > w)).sum()),
            "cross_t": int((staged & (y0 < 0) & (y0 + bh > 0)).sum()), "cross_b": int((staged & (y0 < h) & (y0 + bh > h)).sum()),
            "odd_w": int((staged & (bw % 2 == 1)).sum()), "even_w": int((staged & (bw % 2 == 0)).sum()),
        }
    return out


# (resampler, name): (sw, sh, dw, dh, sx, sy, roll, {plane: {state: least count}}) -- border_tiles.anamorphic's pinhole maps, map mode 3; the
# counts each set is committed to reach (tests/test_resample_border_cpu.py checks them, tests/test_resample_border_gpu.py runs the sets)
TILE_SETS = {}
for _r in ("cubic", "lanczos4"):
    # a small source seen from far away: tiles wholly outside on every side (they stage reflected picture), boxes across all four edges
    TILE_SETS[(_r, "zoomed_out")] = (96, 64, 512, 256, 0.4, 0.4, 0.1, {p: {"outside_staged": 8, "cross_l": 1, "cross_r": 1, "cross_t": 1,
                                                                              "cross_b": 1, "odd_w": 1, "even_w": 1} for p in ("bgr", "chroma")})
    # strong minification: every plane's boxes over the budget
    TILE_SETS[(_r, "gathers")] = (4096, 256, 192, 48, 16.0, 3.0, 0.003, {p: {"gathered": 9} for p in ("bgr", "luma", "chroma")})
TILE_SETS.update({
    # boxes of exactly the budget (6144 BGRx dwords; 12288 luma bytes with BGR gathered in the same frame; 6144 chroma pairs), found by
    # scanning sx and sy against this model
    ("cubic", "bgr_at_budget"): (4096, 256, 192, 48, 3.99, 1.3, 0.003, {"bgr": {"at_budget": 2, "staged": 9}}),
    ("cubic", "luma_at_budget"): (4096, 256, 192, 48, 8.05, 1.3, 0.003, {"bgr": {"gathered": 9}, "luma": {"at_budget": 3, "staged": 9}}),
    ("cubic", "chroma_at_budget"): (4096, 256, 192, 48, 16.345, 1.1, 0.003, {"chroma": {"at_budget": 1, "staged": 9}, "luma": {"gathered": 9}}),
    ("lanczos4", "bgr_at_budget"): (4096, 256, 192, 48, 3.935, 1.1, 0.003, {"bgr": {"at_budget": 1, "staged": 1, "gathered": 8}}),
    ("lanczos4", "luma_at_budget"): (4096, 256, 192, 48, 7.995, 1.1, 0.003, {"bgr": {"gathered": 9}, "luma": {"at_budget": 1, "staged": 1}}),
    ("lanczos4", "chroma_at_budget"): (4096, 256, 192, 48, 12.1, 1.1, 0.003, {"chroma": {"at_budget": 2, "staged": 9}, "luma": {"gathered": 9}}),
})


def set_params(key):
    """-> (params, sw, sh, dw, dh, mode) of a TILE_SETS entry."""
    sw, sh, dw, dh, sx, sy, roll, _ = TILE_SETS[key]
    return border_tiles.anamorphic(sw, sh, dw, dh, sx, sy, roll), sw, sh, dw, dh, oracle.MAP_RECT_TO_RECT


def states_of(key):
    params, sw, sh, dw, dh, mode = set_params(key)
    mx, my = cubic_def.maps(params, dw, dh, mode)
    return tile_states(key[0], mx, my, sw, sh)
