"""Expected records and a CPU model of the fetch-ahead decisions of the LK tracker's multi-pair launches (k_lk_track,
video-annotator_amd/csrc/vstab_lk.hip).  Test infrastructure only (a plain module, imported by the tests).

Records.  A launch tracks every slot through a SEGMENT of frame pairs; a chained launch starts from the device records of its
parent's last pair.  expected() chains oracle.pyr_lk over the slots that survive: a slot lost in pair i reports status 0 there (at
the position it was dropped at), then status 2 at (0, 0) for the rest of its segment and in every launch chained behind it.  A
launch handed a wrong parent tag reports status 3 for all its pairs, and so does every launch behind it (a status-3 parent stays 3).

Fetch ahead.  During the last level (0) of pair fi, for pair fi + 1 of the same launch, waves 1 - 3 fetch
  neighbourhoods  per level l: a 32 x 32 block of the current next image around e0 = 2 x (level 1's estimate), origin
                  floor(e0 / 2^l - 10) - 5, if that position passes the range test and the block lies inside the image
                  (blocks fetched ahead are loaded without border handling) -- otherwise none;
  top block       the top level's 32 x 32 block of pair fi + 1's next image around p0 = e0 + (e0 - this pair's start point),
                  origin floor(p0 / 2^top - 10) - 5, under the same two conditions.
Pair fi + 1 then, per level l, with ipx = floor(pp / 2^l - 10) of its start point pp:
  skipped      ipx outside [-21, w_l) (the level loop skips the level; nothing is loaded);
  served       0 <= ipx - 1 - origin <= 8 in both axes (the 24 x 24 neighbourhood lies in the block: +-4 px of slack);
  missed       a block was fetched but does not hold the neighbourhood: loaded again;
  not_fetched  no block (pair 0 of a launch, a block across the border, a one-level pyramid): loaded.
and for the top level's next-image block: served if the block holds the window with 2 px to spare on every side (ipx - 2 >= bx,
ipx + 24 <= bx + 32), else missed or not_fetched (or skipped with the level).  The integer tests are the kernel's, on the same
float32 values: the oracle's per-level estimates are bit for bit the kernel's (the GPU tests assert the final ones).
A slot that reached pair fi + 1 survived pair fi, whose level-0 final-position test is the level-0 range test of pair fi + 1: at fi > 0
level 0 is never skipped, and no coarser level either (floor(x / 2^l - 10) stays inside [-21, w_l) when floor(x - 10) does), so
`skipped` is reached only by start points of a launch's first pair."""
import functools

import numpy as np

import lk_def as L
import oracle
from lk_def import _floor_i, level_sizes  # noqa: F401  (level_sizes(w, h, W=21): the pyramid's sizes, defined once)

LKW, LKR, LKJR, LKJM, SLACK = 21, 24, 32, 5, 4      # lk_def.geometry(21), by hand
NONE = None
HALF = np.float32(10.0)
CATS = ("served", "missed", "not_fetched", "skipped")


def expected(frames, pts, segs, bad_parent=-1, W=None):
    """frames: K + 1 (h, w) uint8; pts (n, 2); segs: launch lengths (sum K); W: None chains oracle.pyr_lk_trace (window 21), a window
    chains the definition lk_def.track(..., W) in its place.  -> dict with, per pair k (axis 0) and slot (axis 1):
    status (K, n) uint8, xy (K, n, 2) float32 (the record's x, y), start (K, n, 2) float32 (the pair's start point; NaN where the
    slot is not tracked), levels (K, n, 4, 2) float32 (oracle per-level estimates; NaN where not tracked), fi (K,) index of the pair in
    its launch, launch (K,) index of the launch, nl (pyramid levels)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n, K = pts.shape[0], int(sum(segs))
    status = np.zeros((K, n), np.uint8)
    xy = np.zeros((K, n, 2), np.float32)
    start = np.full((K, n, 2), np.nan, np.float32)
    lv = np.full((K, n, 4, 2), np.nan, np.float32)
    fi = np.concatenate([np.arange(s) for s in segs])
    launch = np.concatenate([np.full(s, i) for i, s in enumerate(segs)])
    cur = pts.copy()
    alive = np.ones(n, bool)      # tracked into the next pair
    chain3 = False                # a launch with a wrong parent tag (and every launch behind it): status 3
    nl = level_sizes(frames[0].shape[1], frames[0].shape[0], 21 if W is None else W)[0]
    for k in range(K):
        if fi[k] == 0 and launch[k] == bad_parent:
            chain3 = True
        if chain3:
            status[k] = 3
            continue
        status[k] = np.where(alive, 0, 2)
        idx = np.flatnonzero(alive)
        if idx.size:
            if W is None:
                nxt, st, lvl, nl = oracle.pyr_lk_trace(frames[k], frames[k + 1], cur[idx])
            else:
                r = L.track(frames[k], frames[k + 1], cur[idx], W)
                nxt, st, lvl = r["xy"], r["status"], r["levels"]
            start[k, idx] = cur[idx]
            lv[k, idx] = lvl
            status[k, idx] = st
            xy[k, idx] = nxt
            cur[idx] = nxt
            alive[idx[st == 0]] = False
    return {"status": status, "xy": xy, "start": start, "levels": lv, "fi": fi, "launch": launch, "nl": nl}


def _ahead_origin(c, size, off, W=21):
    """the kernel's range test and interior test of a block fetched ahead: c = (cx, cy) float32 positions (window corner at the level),
    off = the block's margin (1 + SLACK for a neighbourhood, LKJM for the top block) -> (ox, oy) int64, valid bool."""
    w, h = size
    jr = L.geometry(W)["LKJR"]
    cx, cy = c[..., 0], c[..., 1]
    ok = (cx > np.float32(-(W + 1))) & (cx < np.float32(w)) & (cy > np.float32(-(W + 1))) & (cy < np.float32(h))
    with np.errstate(invalid="ignore"):
        ox, oy = _floor_i(np.where(ok, cx, 0)) - off, _floor_i(np.where(ok, cy, 0)) - off
    ok &= (ox >= 0) & (oy >= 0) & (ox + jr <= w) & (oy + jr <= h)
    return ox, oy, ok


def fetch_ahead(exp, w, h, W=21):
    """-> (neigh, top): neigh (K, n, 4) object array of CATS (None: the slot is not tracked in that pair, or the level is absent),
    top (K, n) the same for the top level's next-image block.  For a window W the module docstring's numbers become lk_def.geometry(W)'s:
    half(W) for 10, LKJR for 32, 1 + SLACK and LKJM for the margins, 2 SLACK for 8, LKT + 2 for 24."""
    G = L.geometry(W)
    HALF, SLACK, LKJM, LKJR, LKT = L.half(W), G["SLACK"], G["LKJM"], G["LKJR"], G["LKT"]
    nl, sizes = level_sizes(w, h, W)
    K, n = exp["status"].shape
    neigh = np.full((K, n, 4), None, object)
    top = np.full((K, n), None, object)
    tl = nl - 1
    for k in range(K):
        tracked = ~np.isnan(exp["start"][k, :, 0])
        if not tracked.any():
            continue
        pp = exp["start"][k]
        # what the previous pair of the launch fetched (only if this is not the launch's first pair and there is a level 1)
        have_prev = exp["fi"][k] > 0 and nl >= 2
        if have_prev:
            e0 = exp["levels"][k - 1, :, 1] * np.float32(2.0)
            p0 = e0 + (e0 - exp["start"][k - 1])
        for l in range(nl):
            ls = np.float32(2.0 ** -l)
            ip = _floor_i(np.where(tracked[:, None], pp, 0) * ls - HALF)
            wl, hl = sizes[l]
            skipped = (ip[:, 0] < -W) | (ip[:, 0] >= wl) | (ip[:, 1] < -W) | (ip[:, 1] >= hl)
            cat = np.full(n, "not_fetched", object)
            if have_prev:
                with np.errstate(invalid="ignore"):
                    ox, oy, ok = _ahead_origin(np.where(np.isnan(e0), 0, e0) * ls - HALF, sizes[l], 1 + SLACK, W)
                dx, dy = ip[:, 0] - 1 - ox, ip[:, 1] - 1 - oy
                hit = ok & (dx >= 0) & (dx <= 2 * SLACK) & (dy >= 0) & (dy <= 2 * SLACK)
                cat = np.where(ok, np.where(hit, "served", "missed"), "not_fetched")
            cat = np.where(skipped, "skipped", cat)
            neigh[k, tracked, l] = cat[tracked]
            if l == tl:
                tc = np.full(n, "not_fetched", object)
                if have_prev:
                    with np.errstate(invalid="ignore"):
                        bx, by, ok = _ahead_origin(np.where(np.isnan(p0), 0, p0) * ls - HALF, sizes[l], LKJM, W)
                    hit = ok & (ip[:, 0] - 2 >= bx) & (ip[:, 1] - 2 >= by) & (ip[:, 0] + LKT + 2 <= bx + LKJR) & (ip[:, 1] + LKT + 2 <= by + LKJR)
                    tc = np.where(ok, np.where(hit, "served", "missed"), "not_fetched")
                tc = np.where(skipped, "skipped", tc)
                top[k, tracked] = tc[tracked]
    return neigh, top


def reached(neigh, top, fi, nl):
    """-> {("neigh", level, cat) | ("top", cat): count} over pairs with fi > 0 (and ("first", level, cat) for fi == 0)."""
    out = {}
    for k in range(neigh.shape[0]):
        tag = "neigh" if fi[k] > 0 else "first"
        for l in range(nl):
            for c in neigh[k, :, l]:
                if c is not None:
                    out[(tag, l, c)] = out.get((tag, l, c), 0) + 1
        for c in top[k]:
            if c is not None:
                key = ("top", c) if fi[k] > 0 else ("first_top", c)
                out[key] = out.get(key, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# scripted clips: crops of a larger texture at subpixel offsets (content moves by minus the offset step)
# ---------------------------------------------------------------------------------------------------------------------------------
def texture(seed, tw, th, kind="noise"):
    """tw x th float64.  noise: value noise + bright / dark rectangles (synth.luma's recipe); smooth: a gaussian-filtered random field
    (edge_leaving_pair's), whose wide basins let a feature be carried out of the image by its last Gauss-Newton step; coarse_blind:
    a cosine of period 256 along x plus a square wave of period 4 along y.  pyrDown turns the period-4 rows into period-2 rows
    (level 1; REFLECT_101 keeps the parity) and then into constant ones, and Scharr's central difference sees nothing in period-2
    rows, so every level above 0 has no vertical gradient at all: D = 0, the level is rejected and the tracker reaches level 0 at
    the start point -- level 0 alone carries the whole motion, tens of pixels in a few iterations on the wide cosine."""
    import synth
    if kind == "smooth":
        from scipy.ndimage import gaussian_filter
        rng = np.random.default_rng(1000 + seed)
        base = rng.integers(0, 256, (th // 4 + 2, tw // 4 + 2)).astype(np.float64)
        return gaussian_filter(np.kron(base, np.ones((4, 4)))[:th, :tw], 1.5)
    if kind == "coarse_blind":
        x, y = np.arange(tw, dtype=np.float64), np.arange(th)
        return 128 + 90 * np.cos(2 * np.pi * x / 256 + seed)[None, :] + 14 * np.where(y % 4 < 2, 1.0, -1.0)[:, None]
    from scipy.ndimage import gaussian_filter   # (rounded edges: a bilinear crop of a hard edge is not a pure subpixel shift)
    return gaussian_filter(synth.luma(seed, tw, th, rects=max(40, tw * th // 6000)).astype(np.float64), 1.0)


def crop(tex, ox, oy, w, h):
    """bilinear crop: frame(x, y) = tex(x + ox, y + oy), rounded to u8."""
    x0, y0 = int(np.floor(ox)), int(np.floor(oy))
    fx, fy = ox - x0, oy - y0
    t = tex[y0:y0 + h + 1, x0:x0 + w + 1]
    v = (t[:-1, :-1] * (1 - fx) + t[:-1, 1:] * fx) * (1 - fy) + (t[1:, :-1] * (1 - fx) + t[1:, 1:] * fx) * fy
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def clip(steps, w, h, seed, kind="noise", flat=None):
    """frames of a w x h window sliding over a texture by `steps` (per-frame (dx, dy) of the window; the content moves by minus them),
    starting at a subpixel offset.  flat: (x0, y0, x1, y1, k0) -- from frame k0 on, a constant-grey patch in FRAME coordinates (the
    scene there goes flat: a slot whose window lies in it has nothing to track).  -> (frames list of (h, w) u8, offsets (K + 1, 2))."""
    steps = np.asarray(steps, np.float64).reshape(-1, 2)
    off = np.concatenate([[[0.0, 0.0]], np.cumsum(steps, 0)])
    off -= off.min(0)
    off += [40.37, 30.61]
    span = off.max(0) + [w + 81, h + 81]
    tex = texture(seed, int(span[0]), int(span[1]), kind)
    frames = [crop(tex, ox, oy, w, h) for ox, oy in off]
    if flat is not None:
        x0, y0, x1, y1, k0 = flat
        for f in frames[k0:]:
            f[y0:y1, x0:x1] = 128
    return frames, off


def grid_points(w, h, n, margin=3.0, seed=0):
    """n points spread over the frame (margin px inside it), jittered."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, w - 1 - margin, n), rng.uniform(margin, h - 1 - margin, n)], 1).astype(np.float32)


def start_points(frame, n, seed=0):
    """oracle corners of the first frame (minimum distance 8) topped up with spread points to n."""
    c = oracle.good_features(frame, max_corners=n, quality=0.01, min_distance=8.0)
    h, w = frame.shape
    if c.shape[0] < n:
        c = np.concatenate([c, grid_points(w, h, n - c.shape[0], seed=seed)])
    return c[:n].astype(np.float32)


# name -> (w, h, per-frame window steps, texture seed, texture kind, flat patch)
STEADY = [(2.37, -1.13)] * 8
JUMP = [(14.7, 6.2)] * 3 + [(-26.3, -11.9)] * 2 + [(29.6, 4.1), (-3.2, 27.4), (2.1, -26.7)]   # top-level motion changes by 3 - 7 px
DRIFT = [(-3.1, 0.7)] * 4 + [(3.3, -0.6)] * 4   # content moves right (features leave on the right), then back
DRIFT_Y = [(0.4, 3.2)] * 4 + [(-0.3, -3.4)] * 4  # content moves up, then back down
LEAVE = [(-15.7, 0.4)] * 8                       # content moves right fast: features leave the right edge, two by their last step
BLIND = [(5.3, 0.0), (11.6, 0.0), (-21.7, 0.0), (38.4, 0.0), (-42.1, 0.0), (6.2, 0.0), (35.7, 0.0), (-12.9, 0.0)]
SETS = {
    "steady_640": (640, 360, STEADY, 11, "noise", None),
    "jump_640": (640, 360, JUMP, 12, "noise", None),
    "blind_640": (640, 360, BLIND, 0, "coarse_blind", None),
    "drift_240": (240, 144, DRIFT, 13, "noise", None),
    "drift_y_333": (333, 181, DRIFT_Y, 14, "noise", None),
    "flat_200": (200, 120, [(1.1, 0.2)] * 8, 15, "noise", (110, 20, 196, 100, 4)),
    "leave_200": (200, 120, LEAVE, 16, "noise", None),
    "jump_130": (130, 80, [(2.6, 1.4), (2.6, 1.4), (-5.2, -2.7), (4.4, 0.3)] * 2, 17, "noise", None),
    "steady_40": (40, 30, [(0.8, -0.45)] * 8, 18, "noise", None),
    "long_240": (240, 144, [(1.7 * np.cos(k / 3.0), 1.3 * np.sin(k / 2.0)) for k in range(18)], 19, "noise", None),
}
TRANSLATION = ("steady_640", "jump_640", "blind_640", "drift_240", "drift_y_333", "jump_130", "steady_40", "long_240")


def make_set(name, n=None):
    """-> (frames, pts, offsets): the scripted clip and its start points (n of them; default 200, 60 for the smallest frames).  A few
    start points of steady_640 lie so far outside the frame that every level of the first pair is skipped."""
    w, h, steps, seed, kind, flat = SETS[name]
    frames, off = clip(steps, w, h, seed, kind, flat)
    if n is None:
        n = 200 if w * h >= 20000 else 60
    rng = np.random.default_rng(seed)
    if name == "leave_200":      # the band along the edge the content leaves by (edge_leaving_pair)
        pts = np.stack([rng.uniform(w - 40, w - 1, n), rng.uniform(5, h - 5, n)], 1)
    elif name == "flat_200":     # half of them where the scene goes flat at frame 4
        pts = np.concatenate([start_points(frames[0], n // 2, seed), np.stack([rng.uniform(130, 175, n - n // 2), rng.uniform(32, 86, n - n // 2)], 1)])
    elif name == "blind_640":    # (corners of a cosine and a square wave are rows of equal strength: spread points instead)
        pts = grid_points(w, h, n, margin=12.0, seed=seed)
    else:
        pts = start_points(frames[0], n, seed)
        if name == "steady_640":
            pts[-3:] = [(-120.0, 50.0), (700.0, -130.0), (320.0, 480.0)]
    return frames, np.asarray(pts, np.float32), off


# the clips the window's segment tests run on: the steady and the jump clip, and the coarse-blind one -- the only one on which level 0
# carries a feature further than the slack, i.e. a neighbourhood fetched ahead is `missed` (test_lk_window_cpu.py asserts the reach)
SEGMENT_CLIPS = ("steady_640", "jump_640", "blind_640")
SEGMENT_POINTS = 100
SEGMENTATIONS = ((8,), (3, 3, 2))


@functools.lru_cache(maxsize=None)
def segment_case(name, W):
    """-> (frames, pts, {segs: expected dict}) of a segment clip at window W, computed once per process (the definition is slow)"""
    frames, pts, _ = make_set(name, n=SEGMENT_POINTS)
    return frames, pts, {segs: expected(frames, pts, segs, W=W) for segs in SEGMENTATIONS}
