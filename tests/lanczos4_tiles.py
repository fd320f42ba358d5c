"""CPU model of the Lanczos warp kernel's tile boxes (k_warp_lanczos4, video-annotator_amd/csrc/vstab_warp_lanczos4.hip), restated from
exact map planes.  Test infrastructure only (a plain module, imported by the tests).

The kernel's tiles, pixels, chroma samples and LDS budgets are k_warp_cubic's (tests/cubic_tiles.py); only the footprint differs:
  touches   X + 4 >= 0, X - 3 < w, Y + 4 >= 0, Y - 3 < h
  box       columns min X - 3 .. max X + 4, rows min Y - 3 .. max Y + 4 of the touching footprints
The model needs no margin: the map is bit for bit oracle.create_map_ex for modes 0..4, and the box is exact."""
import numpy as np

import cubic_def
import cubic_tiles

TW, TH = cubic_tiles.TW, cubic_tiles.TH
BUDGET = cubic_tiles.BUDGET


def _boxes(X, Y, w, h, ty, tx, rh, rw):
    """Tile boxes from quantised tap positions (already at the tile's sample grid) -> (x0, y0, bw, bh, have), each (ty, tx)."""
    X, Y = cubic_tiles._tiled(X, ty, tx, rh, rw), cubic_tiles._tiled(Y, ty, tx, rh, rw)
    t = (X + 4 >= 0) & (X - 3 < w) & (Y + 4 >= 0) & (Y - 3 < h)
    big = np.int64(1) << 40
    mnx, mxx = np.where(t, X, big).min(-1), np.where(t, X, -big).max(-1)
    mny, mxy = np.where(t, Y, big).min(-1), np.where(t, Y, -big).max(-1)
    have = t.any(-1)
    bw = np.where(have, mxx - mnx + 8, 0)
    bh = np.where(have, mxy - mny + 8, 0)
    return mnx - 3, mny - 3, bw, bh, have


def tile_boxes(mapx, mapy, sw, sh):
    """Exact map planes (dh, dw) of a warp from a sw x sh source -> {plane: (x0, y0, bw, bh, have)} with arrays of shape (tile rows,
    tile columns), planes 'bgr' / 'luma' (the same box) and 'chroma'."""
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    dh, dw = mapx.shape
    ty, tx = -(-dh // TH), -(-dw // TW)
    pad = ((0, ty * TH - dh), (0, tx * TW - dw))
    mx, my = np.pad(mapx, pad, mode="edge"), np.pad(mapy, pad, mode="edge")   # the clamped coordinates of the kernel's step 1
    X, Y, _ = cubic_def.quantise(mx, my)
    full = _boxes(X, Y, sw, sh, ty, tx, TH, TW)
    cx, cy, _ = cubic_def.quantise(mx[::2, ::2] * np.float32(0.5), my[::2, ::2] * np.float32(0.5))
    chroma = _boxes(cx, cy, sw >> 1, sh >> 1, ty, tx, TH // 2, TW // 2)
    return {"bgr": full, "luma": full, "chroma": chroma}


def tile_states(mapx, mapy, sw, sh):
    """cubic_tiles.tile_states with the Lanczos boxes: {plane: counts of 'none', 'staged', 'gathered', 'at_budget', 'over_by_one',
    'least_over', 'odd_w', 'even_w', 'partial_staged'}."""
    mapx = np.asarray(mapx)
    dh, dw = mapx.shape
    out = {}
    for plane, (x0, y0, bw, bh, have) in tile_boxes(mapx, mapy, sw, sh).items():
        cap = BUDGET[plane]
        area = bw * bh
        staged = have & (area <= cap)
        gathered = have & (area > cap)
        ty, tx = have.shape
        partial = np.zeros(have.shape, bool)
        if dw % TW:
            partial[:, tx - 1] = True
        if dh % TH:
            partial[ty - 1, :] = True
        out[plane] = {
            "none": int((~have).sum()), "staged": int(staged.sum()), "gathered": int(gathered.sum()),
            "at_budget": int((have & (area == cap)).sum()), "over_by_one": int((have & (area == cap + 1)).sum()),
            "least_over": int((area[gathered] - cap).min()) if gathered.any() else None,
            "odd_w": int((staged & (bw % 2 == 1)).sum()), "even_w": int((staged & (bw % 2 == 0)).sum()),
            "partial_staged": int((staged & partial).sum()),
        }
    return out


def states_of(params, dw, dh, sw, sh, mode):
    """tile_states of the warp of a parameter set (modes 0..4: the oracle's map is the kernel's, bit for bit)."""
    assert 0 <= mode <= 4, "mode 5 is the reference kernel's map: it runs on a GPU only"
    mx, my = cubic_def.maps(params, dw, dh, mode)
    return tile_states(mx, my, sw, sh)
