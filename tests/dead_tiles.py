"""The dead-tile rule of the fused warp kernels (vstab_warp_tile.hpp: tile_dead_rule on probe_tile's 64 perimeter samples), restated in
numpy, beside the exact fp64 map it is judged against.  Test infrastructure only (a plain module, imported by the tests).

A tile is "dead" when the probe decides that every pixel maps outside the source; the kernel then stores zeros without mapping or
sampling.  A pixel is live iff -1 <= X <= sw - 1 and -1 <= Y <= sh - 1 with X, Y = floor(rint(32 * map) / 32): one of its four taps is
inside the source."""
import numpy as np

MARGIN = 16            # DEAD_MARGIN, source pixels
GUARD = 3 * MARGIN // 4  # DEAD_GUARD
BIG = 2097152.0        # |32 * map| below this at every sample
STRETCH = 1.67         # DEAD_STRETCH >= max (1 + r) atan(r) / r


def exact_map(params, xs, ys, nan_behind=False):
    """fp64 map of output pixels (xs, ys broadcast) -> (mapx, mapy, wz, r), the fisheye -> pinhole projection of createMap.cl.
    nan_behind (MAP_FISH_TO_RECT): rays with wz <= 0 map nowhere."""
    p = np.asarray(params, np.float64)
    icx, icy, ifx, ify, ocx, ocy, ofx, ofy = p[:8]
    R = p[8:17].reshape(3, 3)
    vx, vy = (np.asarray(xs, np.float64) - ocx) / ofx, (np.asarray(ys, np.float64) - ocy) / ofy
    wx = R[0, 0] * vx + R[0, 1] * vy + R[0, 2]
    wy = R[1, 0] * vx + R[1, 1] * vy + R[1, 2]
    wz = R[2, 0] * vx + R[2, 1] * vy + R[2, 2]
    with np.errstate(all="ignore"):
        ux, uy = wx / wz, wy / wz
        r = np.sqrt(ux * ux + uy * uy)
        k = np.where(r > 0, np.arctan(r) / r, 1.0)
        mx, my = icx + ifx * ux * k, icy + ify * uy * k
    if nan_behind:
        mx, my = np.where(wz > 0, mx, np.nan), np.where(wz > 0, my, np.nan)
    return mx, my, wz, r


def live_pixels(params, dw, dh, sw, sh, nan_behind=False):
    """(dh, dw) bool: the pixel has a tap inside the source."""
    mx, my = exact_map(params, np.arange(dw)[None, :], np.arange(dh)[:, None], nan_behind)[:2]
    with np.errstate(all="ignore"):
        X, Y = np.floor(np.rint(32.0 * mx) / 32.0), np.floor(np.rint(32.0 * my) / 32.0)
        return (X >= -1) & (X <= sw - 1) & (Y >= -1) & (Y <= sh - 1)   # NaN compares false


def perimeter(th):
    """probe_tile's 64 tile-local perimeter points (px, py) for a 64 x th tile, lane by lane."""
    lane = np.arange(64)
    l16 = lane & 15
    side = (l16 * (th - 1) + 7) // 15
    px = np.where(lane < 16, 4 * l16, np.where(lane < 32, 4 * l16 + 3, np.where(lane < 48, 0, 63)))
    py = np.where(lane < 16, 0, np.where(lane < 32, th - 1, side))
    return px, py


def rule(params, dw, dh, sw, sh, th, nan_behind=False, dtype=np.float32):
    """The rule for every 64 x th tile of a dw x dh output -> (rows, cols) bool.  The samples are rounded to `dtype` (the probe works in
    fp32 with approximate reciprocals; the margin dwarfs the difference) and compared as the kernel compares them."""
    px, py = perimeter(th)
    rows, cols = -(-dh // th), -(-dw // 64)
    x0, y0 = 64 * np.arange(cols)[None, :, None], th * np.arange(rows)[:, None, None]
    xs = x0 + np.minimum(px[None, None, :], dw - 1 - x0)
    ys = y0 + np.minimum(py[None, None, :], dh - 1 - y0)
    mx, my, wz, r = exact_map(params, xs + 0 * ys, ys + 0 * xs, nan_behind)
    p = np.asarray(params, np.float64)
    with np.errstate(all="ignore"):
        ax, ay = (32.0 * mx).astype(dtype), (32.0 * my).astype(dtype)
        # neighbour guard: lane - 1 inside each 16-lane side; the first lane of a side compares with itself
        prev = np.arange(64) - 1
        prev[::16] += 1
        ok = (wz > 0) & (np.abs(ax) < BIG) & (np.abs(ay) < BIG) & (np.abs(ax - ax[..., prev]) < 32.0 * GUARD) & (np.abs(ay - ay[..., prev]) < 32.0 * GUARD)
        lo, hx, hy = -32.0 * (1 + MARGIN), 32.0 * (sw + MARGIN), 32.0 * (sh + MARGIN)
        side = (ax < lo).all(-1) | (ax >= hx).all(-1) | (ay < lo).all(-1) | (ay >= hy).all(-1)
        # the slope bound at every sample
        slope = max(p[2], p[3]) * max(1.0 / p[6], 1.0 / p[7])
        ok &= 2.0 * STRETCH * slope / wz <= MARGIN - 1
    return ok.all(-1) & side


def tiles_any(mask, th):
    """(dh, dw) bool -> (rows, cols) bool: any pixel of the 64 x th tile set."""
    dh, dw = mask.shape
    rows, cols = -(-dh // th), -(-dw // 64)
    pad = np.zeros((rows * th, cols * 64), bool)
    pad[:dh, :dw] = mask
    return pad.reshape(rows, th, cols, 64).any(axis=(1, 3))


def census(params, dw, dh, sw, sh, th, nan_behind=False):
    """-> dict: tiles, truly dead tiles, tiles the rule calls dead, wrongly dead tiles, tiles cut by the source edge (live and outside
    pixels both)."""
    live = live_pixels(params, dw, dh, sw, sh, nan_behind)
    any_live, any_out = tiles_any(live, th), tiles_any(~live, th)
    r = rule(params, dw, dh, sw, sh, th, nan_behind)
    return dict(tiles=int(r.size), truly_dead=int((~any_live).sum()), ruled_dead=int(r.sum()), wrong=int((r & any_live).sum()),
                cut=int((any_live & any_out).sum()))
