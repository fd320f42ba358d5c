"""CPU model of the keep-edge warp kernel's tiles (k_warp_keep, video-annotator_amd/csrc/vstab_warp_keep.hip), restated from exact map planes.
Test infrastructure only (a plain module, imported by the tests).

Per 64 x 16 output tile and plane:
  samples   luma / BGR: the pixels of the tile inside the image; chroma: its even columns of its even rows (32 x 8 chroma samples), quantised
            from 0.5f * map against the (sw / 2) x (sh / 2) chroma plane
  written   keep_def.written: the 2 x 2 footprint wholly inside the plane
  kind      all_kept (no written sample: the tile copies prev, or returns in place), all_written, mixed; ragged: the image's right or bottom
            edge cuts the tile
  box       over the written samples only: columns min X .. max X + 1, rows min Y .. max Y + 1 -- always inside the plane
  path      staged (w * h <= budget) or gathered from global memory; an all_kept tile has no box and neither path
  budgets   6144 BGRx dwords, 12288 luma bytes, 6144 chroma pairs (border_tiles.BUDGET)

The kernel's box is exact and its map is bit for bit oracle.create_map_ex for modes 0..4, so the model predicts the path of every tile."""
import numpy as np

import border_tiles
import cubic_def
import oracle

TW, TH = border_tiles.TW, border_tiles.TH
BUDGET = border_tiles.BUDGET
STATES = ("all_kept", "all_written", "mixed", "staged", "gathered", "ragged_mixed", "staged_mixed", "gathered_mixed")


def _plane_states(X, Y, w, h, tw, th, cap):
    """Quantised positions of a plane's sample grid (rows, cols) read from a w x h plane, tiles of tw x th samples -> counts by state."""
    m = (X >= 0) & (X <= w - 2) & (Y >= 0) & (Y <= h - 2)
    rows, cols = X.shape
    out = dict.fromkeys(STATES, 0)
    for r0 in range(0, rows, th):
        for c0 in range(0, cols, tw):
            sl = (slice(r0, min(rows, r0 + th)), slice(c0, min(cols, c0 + tw)))
            mm = m[sl]
            if not mm.any():
                out["all_kept"] += 1
                continue
            x, y = X[sl][mm], Y[sl][mm]
            staged = (x.max() - x.min() + 2) * (y.max() - y.min() + 2) <= cap
            mixed = not mm.all()
            ragged = mm.shape != (th, tw)
            out["staged" if staged else "gathered"] += 1
            out["mixed" if mixed else "all_written"] += 1
            if mixed:
                out["staged_mixed" if staged else "gathered_mixed"] += 1
                out["ragged_mixed"] += ragged
    return out


def tile_states(mapx, mapy, sw, sh):
    """Exact map planes (dh, dw) of a warp from a sw x sh source -> {plane: counts by state}; planes 'bgr', 'luma' (the same tiles, each with
    its own budget) and 'chroma'."""
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    X, Y, _ = cubic_def.quantise(mapx, mapy)
    cx, cy, _ = cubic_def.quantise(*oracle.chroma_maps(mapx, mapy))
    return {"bgr": _plane_states(X, Y, sw, sh, TW, TH, BUDGET["bgr"]), "luma": _plane_states(X, Y, sw, sh, TW, TH, BUDGET["luma"]),
            "chroma": _plane_states(cx, cy, sw >> 1, sh >> 1, TW // 2, TH // 2, BUDGET["chroma"])}


def kept_share(mapx, mapy, sw, sh):
    X, Y, _ = cubic_def.quantise(mapx, mapy)
    return 1.0 - float(((X >= 0) & (X <= sw - 2) & (Y >= 0) & (Y <= sh - 2)).mean())


# name: (sw, sh, dw, dh, sx, sy, roll, {plane: {state: least count}}) -- border_tiles.anamorphic in map mode 3 (RECT_TO_RECT); the counts each
# set is committed to reach at least (tests/test_keep_tiles_cpu.py checks them, test_keep_gpu.py runs the sets)
TILE_SETS = {
    # a small source seen from far away: tiles wholly outside on every side, wholly inside in the middle, mixed around the picture
    "zoomed_out": (96, 64, 512, 256, 0.25, 0.25, 0.1,
                   {p: {"all_kept": 8, "all_written": 8, "mixed": 8, "staged_mixed": 8} for p in ("bgr", "luma", "chroma")}),
    # the same with an image that ends inside its last tile column and row: mixed tiles with ragged edges
    "zoomed_out_ragged": (96, 64, 500, 250, 0.25, 0.25, 0.1, {p: {"ragged_mixed": 1, "all_kept": 8} for p in ("bgr", "luma", "chroma")}),
    # strong minification over the source's edges: mixed tiles whose box is over the budget
    "gathers_edge": (2048, 128, 192, 48, 16.0, 3.0, 0.003,
                     {"bgr": {"gathered_mixed": 2}, "luma": {"gathered_mixed": 2}, "chroma": {"gathered_mixed": 2, "staged_mixed": 2}}),
    # and well inside it: every tile gathered, every sample written
    "gathers_in": (4096, 256, 192, 48, 16.0, 3.0, 0.003, {p: {"gathered": 9, "all_written": 9} for p in ("bgr", "luma", "chroma")}),
}


def set_params(name):
    """-> (params, sw, sh, dw, dh, mode) of a TILE_SETS entry."""
    sw, sh, dw, dh, sx, sy, roll, _ = TILE_SETS[name]
    return border_tiles.anamorphic(sw, sh, dw, dh, sx, sy, roll), sw, sh, dw, dh, oracle.MAP_RECT_TO_RECT


def states_of(name):
    params, sw, sh, dw, dh, mode = set_params(name)
    mx, my = cubic_def.maps(params, dw, dh, mode)
    return tile_states(mx, my, sw, sh)
