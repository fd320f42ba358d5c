"""CPU model of the border warp kernel's tile boxes (k_warp_border, video-annotator_amd/csrc/vstab_warp_border.hip), restated from exact map
planes.  Test infrastructure only (a plain module, imported by the tests).

Per 64 x 16 output tile and plane:
  pixels    every pixel of the tile, those right of / below the image evaluated at the last column / row (min(x, dw - 1), min(y, dh - 1))
  luma/BGR  the quantised map (cubic_def.quantise) of each pixel, every pixel counts (no "touches the source" filter)
  chroma    the even lanes (even x) of rows y0 and y0 + 2 of each wave -- the even rows of the tile --, quantised from 0.5f * map
            against the (sw / 2) x (sh / 2) chroma plane
  box       in virtual (not border-interpolated) coordinates: columns min X .. max X + 1, rows min Y .. max Y + 1; under BORDER_CONSTANT
            X is first clamped to [-2, w] and Y to [-2, h]
  path      staged (w * h <= budget) or gathered from global memory (over the budget)
  budgets   6144 BGRx dwords, 12288 luma bytes, 6144 chroma pairs (24 KiB of LDS; the plane-wise kernel gives luma and chroma half each)

The kernel's box is exact and its map is bit for bit oracle.create_map_ex for modes 0..4, so the model predicts the path of every tile."""
import numpy as np

import border_def
import cubic_def
import oracle

TW, TH = 64, 16
BUDGET = {"bgr": 6144, "luma": 12288, "chroma": 6144}


def _tiled(a, ty, tx, rh, rw):
    """(ty * rh, tx * rw) -> (ty, tx, rh * rw)"""
    return a.reshape(ty, rh, tx, rw).transpose(0, 2, 1, 3).reshape(ty, tx, rh * rw)


def _boxes(X, Y, w, h, ty, tx, rh, rw, border_mode):
    """Tile boxes from quantised tap positions (already at the tile's sample grid) -> (x0, y0, bw, bh), each (ty, tx)."""
    if border_mode == border_def.CONSTANT:
        X, Y = np.clip(X, -2, w), np.clip(Y, -2, h)
    X, Y = _tiled(X, ty, tx, rh, rw), _tiled(Y, ty, tx, rh, rw)
    x0, y0 = X.min(-1), Y.min(-1)
    return x0, y0, X.max(-1) - x0 + 2, Y.max(-1) - y0 + 2


def tile_boxes(mapx, mapy, sw, sh, border_mode=border_def.REFLECT_101):
    """Exact map planes (dh, dw) of a warp from a sw x sh source -> {plane: (x0, y0, bw, bh)} with arrays of shape (tile rows, tile columns),
    planes 'bgr' / 'luma' (the same box) and 'chroma'."""
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    dh, dw = mapx.shape
    ty, tx = -(-dh // TH), -(-dw // TW)
    pad = ((0, ty * TH - dh), (0, tx * TW - dw))
    mx, my = np.pad(mapx, pad, mode="edge"), np.pad(mapy, pad, mode="edge")   # the clamped coordinates of the kernel's step 1
    X, Y, _ = cubic_def.quantise(mx, my)
    full = _boxes(X, Y, sw, sh, ty, tx, TH, TW, border_mode)
    cx, cy, _ = cubic_def.quantise(mx[::2, ::2] * np.float32(0.5), my[::2, ::2] * np.float32(0.5))
    chroma = _boxes(cx, cy, sw >> 1, sh >> 1, ty, tx, TH // 2, TW // 2, border_mode)
    return {"bgr": full, "luma": full, "chroma": chroma}


def tile_states(mapx, mapy, sw, sh, border_mode=border_def.REFLECT_101):
    """-> {plane: counts}: tiles 'staged' / 'gathered'; boxes of exactly the budget ('at_budget'); staged boxes wholly outside the source
    ('outside_staged': under BORDER_CONSTANT such a tile is never read, here it carries reflected picture); staged boxes crossing the left,
    right, top and bottom edge of the plane ('cross_l', 'cross_r', 'cross_t', 'cross_b'); staged boxes of odd and even width ('odd_w',
    'even_w')."""
    out = {}
    for plane, (x0, y0, bw, bh) in tile_boxes(mapx, mapy, sw, sh, border_mode).items():
        w, h = (sw, sh) if plane != "chroma" else (sw >> 1, sh >> 1)
        cap = BUDGET[plane]
        area = bw * bh
        staged = area <= cap
        outside = (x0 + bw <= 0) | (x0 >= w) | (y0 + bh <= 0) | (y0 >= h)
        out[plane] = {
            "staged": int(staged.sum()), "gathered": int((~staged).sum()), "at_budget": int((area == cap).sum()),
            "outside_staged": int((staged & outside).sum()),
            "cross_l": int((staged & (x0 < 0) & (x0 + bw > 0)).sum()), "cross_r": int((staged & (x0 < w) & (x0 + bw > w)).sum()),
            "cross_t": int((staged & (y0 < 0) & (y0 + bh > 0)).sum()), "cross_b": int((staged & (y0 < h) & (y0 + bh > h)).sum()),
            "odd_w": int((staged & (bw % 2 == 1)).sum()), "even_w": int((staged & (bw % 2 == 0)).sum()),
        }
    return out


def anamorphic(sw, sh, dw, dh, sx, sy, roll):
    """Source focal lengths 100 sx / 100 sy against an output camera of focal length 100, both principal points centred, rolled about the
    optical axis (pinhole maps, mode 3): the source box of a 64 x 16 tile is about 64 sx wide and 16 sy tall, and an output larger than
    the source over sx, sy reaches beyond every edge."""
    Ki = np.array([[100.0 * sx, 0, sw / 2], [0, 100.0 * sy, sh / 2], [0, 0, 1]])
    Ko = np.array([[100.0, 0, dw / 2], [0, 100.0, dh / 2], [0, 0, 1]])
    return oracle.map_params(Ki, Ko, oracle.rodrigues((0.0, 0.0, roll)))


# name: (sw, sh, dw, dh, sx, sy, roll, {plane: {state: least count}}) -- map mode 3 (RECT_TO_RECT), BORDER_REFLECT_101; the counts each
# set is committed to reach at least (tests/test_border_tiles_cpu.py checks them, test_border_gpu.py runs the sets)
TILE_SETS = {
    # a small source seen from far away: tiles wholly outside on every side (they stage reflected picture), boxes across all four edges
    "zoomed_out": (96, 64, 512, 256, 0.25, 0.25, 0.1,
                   {p: {"outside_staged": 8, "cross_l": 1, "cross_r": 1, "cross_t": 1, "cross_b": 1, "odd_w": 1, "even_w": 1} for p in ("bgr", "chroma")}),
    # strong minification: every plane's boxes over the budget
    "gathers": (4096, 256, 192, 48, 16.0, 3.0, 0.003, {"bgr": {"gathered": 9}, "luma": {"gathered": 9}, "chroma": {"gathered": 9}}),
    # boxes of exactly the budget: BGR (6144 dwords), luma (12288 bytes) with BGR gathered in the same frame, chroma (6144 pairs)
    "bgr_at_budget": (4096, 256, 192, 48, 4.02, 1.4, 0.003, {"bgr": {"at_budget": 2, "staged": 9}}),
    "luma_at_budget": (4096, 256, 192, 48, 8.08, 1.4, 0.003, {"bgr": {"gathered": 9}, "luma": {"at_budget": 1, "staged": 9}}),
    "chroma_at_budget": (4096, 256, 192, 48, 16.43, 1.3, 0.003, {"chroma": {"at_budget": 1, "staged": 9}, "luma": {"gathered": 1}}),
}


def set_params(name):
    """-> (params, sw, sh, dw, dh, mode) of a TILE_SETS entry."""
    sw, sh, dw, dh, sx, sy, roll, _ = TILE_SETS[name]
    return anamorphic(sw, sh, dw, dh, sx, sy, roll), sw, sh, dw, dh, oracle.MAP_RECT_TO_RECT


def states_of(name, border_mode=border_def.REFLECT_101):
    params, sw, sh, dw, dh, mode = set_params(name)
    mx, my = cubic_def.maps(params, dw, dh, mode)
    return tile_states(mx, my, sw, sh, border_mode)
