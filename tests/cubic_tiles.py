"""CPU model of the cubic warp kernel's tile boxes (k_warp_cubic, video-annotator_amd/csrc/vstab_warp_cubic.hip), restated from exact
map planes.  Test infrastructure only (a plain module, imported by the tests).

Per 64 x 16 output tile and plane:
  pixels    every pixel of the tile, those right of / below the image evaluated at the last column / row (min(x, dw - 1), min(y, dh - 1))
  luma/BGR  the quantised map (cubic_def.quantise) of each pixel; only footprints that touch the source (Cubic::touches) count
  chroma    the even lanes (even x) of rows y0 and y0 + 2 of each wave -- the even rows of the tile --, quantised from 0.5f * map
            against the (sw / 2) x (sh / 2) chroma plane
  box       X / Y extremes of the touching footprints, columns min X - 1 .. max X + 2, rows min Y - 1 .. max Y + 2
  path      no box (nothing touches), staged (w * h <= budget) or gathered from global memory (over the budget)
  budgets   6144 BGRx dwords, 12288 luma bytes, 6144 chroma pairs (24 KiB of LDS; the plane-wise kernel gives luma and chroma half each)

The kernel's box is exact, not probed, and its map is bit for bit oracle.create_map_ex for modes 0..4 (what cubic_def feeds the
definition), so the model needs no margin: it predicts the path of every tile."""
import numpy as np

import cubic_def

TW, TH = 64, 16
BUDGET = {"bgr": 6144, "luma": 12288, "chroma": 6144}


def _tiled(a, ty, tx, rh, rw):
    """(ty * rh, tx * rw) -> (ty, tx, rh * rw)"""
    return a.reshape(ty, rh, tx, rw).transpose(0, 2, 1, 3).reshape(ty, tx, rh * rw)


def _boxes(X, Y, w, h, ty, tx, rh, rw):
    """Tile boxes from quantised tap positions (already at the tile's sample grid) -> (x0, y0, bw, bh, have), each (ty, tx)."""
    X, Y = _tiled(X, ty, tx, rh, rw), _tiled(Y, ty, tx, rh, rw)
    t = (X + 2 >= 0) & (X - 1 < w) & (Y + 2 >= 0) & (Y - 1 < h)
    big = np.int64(1) << 40
    mnx, mxx = np.where(t, X, big).min(-1), np.where(t, X, -big).max(-1)
    mny, mxy = np.where(t, Y, big).min(-1), np.where(t, Y, -big).max(-1)
    have = t.any(-1)
    bw = np.where(have, mxx - mnx + 4, 0)
    bh = np.where(have, mxy - mny + 4, 0)
    return mnx - 1, mny - 1, bw, bh, have


def tile_boxes(mapx, mapy, sw, sh):
    """Exact map planes (dh, dw) of a warp from a sw x sh source -> {plane: (x0, y0, bw, bh, have)} with arrays of shape (tile rows,
    tile columns), planes 'bgr' / 'luma' (the same box: both are the map's footprints against the full-size source) and 'chroma'."""
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
    """-> {plane: counts} with counts of tiles with 'none' (no box), 'staged', 'gathered'; boxes of exactly the budget ('at_budget')
    and one element over it ('over_by_one'); the least element count over the budget of any gathered box ('least_over', None when
    nothing gathers); staged boxes of odd and even width ('odd_w', 'even_w'); and staged tiles that are partial, cut by the right or
    bottom edge of the output ('partial_staged')."""
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
