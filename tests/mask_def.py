"""The detection mask (include/vstab.h, "Detection mask") restated in numpy on top of oracle.min_eig: OpenCV 4.5's
goodFeaturesToTrack(gray, corners, max_corners, quality, min_distance, mask, 3, false, 0.04) on its CPU path, and the one-pass detector
under a mask (k_corners_fused_masked, then k_filter_keys) restated per tile as corner_tiles.Model restates k_corners_fused.  No GPU here.

    1  the eigenvalue map is that of the whole image: the mask plays no part in it
    2  maxVal = the maximum of the map over the pixels with mask != 0; none: no corner
    3  threshold (float)((double)maxVal * quality), strict >, for every pixel
    4  the 3 x 3 maximum test runs over all pixels: a masked-out neighbour competes
    5  a candidate is an interior pixel that passes 3 and 4 and has mask != 0
    6  order (value descending, ties: later raster index first), the min_distance grid and max_corners as without a mask

What a tile's own maximum runs over: the pixels with mask != 0 among the in-image part of the 66 x 33 eigenvalues around the tile -- the
region k_corners_fused takes it over, restricted by the mask.  A tile with no such pixel returns early (`early`): it computes nothing,
publishes no maximum and reports a count of 0."""
import functools

import numpy as np

import corner_tiles as C
import oracle
import synth

TW, TH, SLOTS = C.TW, C.TH, C.SLOTS


def _is_max(e):
    """interior pixels that equal the maximum of their 3 x 3 neighbourhood (every neighbour of an interior pixel is in the image)"""
    h, w = e.shape
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = e
    m = e.copy()
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, pad[dy:dy + h, dx:dx + w])
    inner = np.zeros((h, w), bool)
    inner[1:h - 1, 1:w - 1] = True
    return inner & (e == m)


def candidates(gray, mask, quality=0.01):
    """steps 1-5: (eigenvalue map, boolean map of the candidates, maxVal or None)"""
    gray = np.ascontiguousarray(gray, np.uint8)
    e = oracle.min_eig(gray)
    sel = np.asarray(mask) != 0
    assert sel.shape == e.shape
    if not sel.any():
        return e, np.zeros(e.shape, bool), None
    maxv = e[sel].max()
    thr = np.float32(np.float64(maxv) * quality)
    # (OpenCV sets what fails the threshold to zero and dilates that map: a pixel above a non-negative threshold that equals the maximum of
    #  the thresholded map equals the maximum of the raw one, and the other way round, since zeroed neighbours lie below it either way)
    return e, _is_max(e) & (e > thr) & sel, maxv


def select(e, cand, max_corners, min_distance):
    """step 6, as vo_good_features and select_corners (vstab_hostlogic.hpp) run it: keys descending, the grid of cells of round(min_distance) px"""
    h, w = e.shape
    ys, xs = np.nonzero(cand)
    keys = (e[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64)
    order = np.argsort(keys)[::-1]
    xs, ys = xs[order], ys[order]
    cell = int(np.rint(min_distance))
    if cell < 1:
        n = len(xs) if max_corners <= 0 else min(len(xs), max_corners)
        return np.stack([xs[:n], ys[:n]], 1).astype(np.float32).reshape(-1, 2)
    gw, gh = -(-w // cell), -(-h // cell)
    grid = [[] for _ in range(gw * gh)]
    md2 = min_distance * min_distance
    out = []
    for x, y in zip(xs.tolist(), ys.tolist()):
        xc, yc = x // cell, y // cell
        good = True
        for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
            for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                for (a, b) in grid[yy * gw + xx]:
                    if (x - a) * (x - a) + (y - b) * (y - b) < md2:   # (whole numbers below 2^24: exact in the float the detectors use)
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid[yc * gw + xc].append((x, y))
            out.append((x, y))
            if max_corners > 0 and len(out) == max_corners:
                break
    return np.array(out, np.float32).reshape(-1, 2)


def good_features(gray, mask, max_corners=200, quality=0.01, min_distance=30.0):
    """goodFeaturesToTrack(gray, max_corners, quality, min_distance, mask): (n, 2) float32 (x, y) in acceptance order"""
    e, cand, _ = candidates(gray, mask, quality)
    return select(e, cand, max_corners, min_distance)


class Model:
    """corner_tiles.Model under a mask: `final`, `keys`, and per tile `early`, `lo` and `hi` -- the count k_corners_fused_masked reports lies
    between the survivors under the final threshold quality * maxVal and those under quality * the tile's own masked maximum."""

    def __init__(self, img, mask, quality=0.01):
        img = np.ascontiguousarray(img, np.uint8)
        self.img, self.mask, self.quality = img, np.ascontiguousarray(mask, np.uint8), quality
        h, w = img.shape
        self.w, self.h = w, h
        e, self.final, maxv = candidates(img, mask, quality)
        self.eig = e
        sel = self.sel = self.mask != 0
        bits = e.view(np.int32)
        if maxv is not None:
            fmax = int(bits[sel].max())
            assert fmax >= 0 and np.int32(fmax).view(np.float32) == maxv, "a negative masked maximum: outside the definition"
        self.frame_max = maxv
        is_max = _is_max(e) & sel
        ys, xs = np.nonzero(self.final)
        self.keys = np.sort((e[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64))
        self.n = len(self.keys)
        self.tiles_x, self.tiles_y = -(-w // TW), -(-h // TH)
        shape = (self.tiles_y, self.tiles_x)
        self.lo, self.hi = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        self.early = np.zeros(shape, bool)
        for ty in range(self.tiles_y):
            for tx in range(self.tiles_x):
                oy, ox = ty * TH, tx * TW
                around = (slice(max(oy - 1, 0), min(oy + TH + 1, h)), slice(max(ox - 1, 0), min(ox + TW + 1, w)))
                if not sel[around].any():
                    self.early[ty, tx] = True
                    continue
                own = int(bits[around][sel[around]].max())
                assert own >= 0, "a tile whose masked maximum is negative"
                thr_own = np.float32(np.float64(np.int32(own).view(np.float32)) * quality)
                sl = (slice(oy, min(oy + TH, h)), slice(ox, min(ox + TW, w)))
                self.lo[ty, tx] = int(self.final[sl].sum())
                self.hi[ty, tx] = int((is_max[sl] & (e[sl] > thr_own)).sum())
        self.spills = self.lo > SLOTS
        self.timing = (self.lo <= SLOTS) & (self.hi > SLOTS)
        self.keyed = self.hi <= SLOTS
        self.full = (self.lo == SLOTS) & (self.hi == SLOTS)

    def spilled_range(self):
        return int(self.spills.sum()), int((self.hi > SLOTS).sum())

    def corners(self, max_corners, min_distance):
        return select(self.eig, self.final, max_corners, min_distance)


# ---- masks -------------------------------------------------------------------------------------------------------------------------
def full(h, w, value=255):
    return np.full((h, w), value, np.uint8)


def overlay_box(h, w):
    """everything but a box in the lower left, the shape of a burnt-in overlay"""
    m = full(h, w, 1)
    m[h * 5 // 8:h - 4, 5:w * 2 // 5] = 0
    return m


def roi(h, w):
    """one tile's worth of ones, across tile seams"""
    m = np.zeros((h, w), np.uint8)
    m[max(h // 2 - 15, 0):h // 2 + 16, max(w // 2 - 32, 0):w // 2 + 32] = 200
    return m


def checkerboard(h, w, py, px, oy=0, ox=0):
    return ((((np.arange(h)[:, None] + oy) // py + (np.arange(w)[None, :] + ox) // px) % 2) * 255).astype(np.uint8)


def rows_from(h, w, y0):
    m = np.zeros((h, w), np.uint8)
    m[y0:] = 7
    return m


# ---- the separating cases of the definition -------------------------------------------------------------------------------------------
def case_filter_afterwards():
    """timing_frame with the mask on rows >= 64: the masked maximum is 1.4 % of the frame's, so filtering the unmasked result afterwards
    finds 8 of 89 candidates where the definition has 5,154"""
    g = C.timing_frame()
    return g, rows_from(*g.shape, 64)


def case_neighbours_compete():
    """synth.luma(7, 320, 124) with exactly its unmasked candidates masked out: their masked-in neighbours lose the 3 x 3 test to them"""
    g = synth.luma(7, 320, 124)
    m = full(*g.shape, 1)
    ys, xs = np.nonzero(C.Model(g).final)
    m[ys, xs] = 0
    return g, m


# ---- the named raw-detector sets of the GPU test (test_detection_mask_cpu.py asserts what they reach) -----------------------------------
def _tiles_off(name, off):
    """the frame of corner_tiles set `name` with the whole tiles `off` (tile numbers, tile rows first) masked out"""
    g = C.make(name)
    h, w = g.shape
    m = full(h, w)
    tx = -(-w // TW)
    for t in off:
        y, x = divmod(t, tx)
        m[y * TH:(y + 1) * TH, x * TW:(x + 1) * TW] = 0
    return g, m


def _margin_off(g, m, tiles, tx):
    """the mask bytes around the switched-off tiles as well (one pixel: the ring their 66 x 33 regions share with their neighbours)"""
    for t in tiles:
        y, x = divmod(t, tx)
        m[max(y * TH - 1, 0):(y + 1) * TH + 1, max(x * TW - 1, 0):(x + 1) * TW + 1] = 0
    return g, m


def _half_plateaus(name):
    """the right half of every tile column masked out: plateau tiles are cut in half, patch tiles lose their right patches"""
    g = C.make(name)
    h, w = g.shape
    m = full(h, w)
    for x0 in range(32, w, TW):
        m[:, x0:x0 + 32] = 0
    return g, m


def _survivors(name, tile, n):
    """the frame of corner_tiles set `name` with the mask of its plateau tile `tile` zero but for n of the tile's candidates: exactly n survivors"""
    g = C.make(name)
    h, w = g.shape
    m = full(h, w)
    y, x = divmod(tile, -(-w // TW))
    own = (slice(y * TH, (y + 1) * TH), slice(x * TW, (x + 1) * TW))
    ys, xs = np.nonzero(C.model(name).final[own])
    assert len(ys) >= n
    m[own] = 0
    m[own][ys[-n:], xs[-n:]] = 1
    return g, m


def _raw_sets():
    s = {}
    s["grid_5x3_tiles_off"] = lambda: _tiles_off("grid_5x3", (0, 4, 7, 11))
    s["grid_7x5_tiles_off"] = lambda: (lambda g, m: _margin_off(g, m, (1, 2, 8, 9, 17, 30, 34), 7))(*_tiles_off("grid_7x5", (1, 2, 8, 9, 17, 30, 34)))
    s["mixed_wave_half"] = lambda: _half_plateaus("mixed_wave")
    s["grid_7x5_half"] = lambda: _half_plateaus("grid_7x5")
    s["full_16_tiles_off"] = lambda: (lambda g, m: _margin_off(g, m, (5, 6, 9, 10), 4))(*_tiles_off("full_16", (5, 6, 9, 10)))
    s["mixed_wave_256"] = lambda: _survivors("mixed_wave", 2, 256)
    s["grid_5x3_257"] = lambda: _survivors("grid_5x3", 2, 257)
    s["timing_top_off"] = lambda: (C.timing_frame(), rows_from(*C.timing_frame().shape, TH + 1))   # tile row 0 returns early; rows 2, 3 hold `timing` tiles
    s["timing_rows"] = case_filter_afterwards
    return s


RAW_SETS = _raw_sets()


@functools.lru_cache(maxsize=None)
def raw_model(name):
    """the masked model of a named raw set, computed once per process and shared"""
    g, m = RAW_SETS[name]()
    return Model(g, m)


# ---- the clips of the pipeline tests ----------------------------------------------------------------------------------------------------
OVERLAY_BOX = (250, 340, 20, 260)   # rows, columns of the overlay in the 640 x 360 clip
OVERLAY_MARGIN = 16                  # LK's 21 x 21 window reaches 10 px from a corner on level 0, and a corner drifts a few px between key frames


def overlay_clip(w=640, h=360, n=40, seed=3):
    """(K, clean NV12 frames, frames with the overlay, ground-truth rotations, mask): synth.shaky_clip with synth.luma(99) pasted unmoved
    into OVERLAY_BOX of every frame, and the mask that is zero on the box grown by OVERLAY_MARGIN"""
    K = oracle.get_preset_camera(4, w, h)
    frames, rots = synth.shaky_clip(seed, K, w, h, n, sigma=0.004)
    hud = synth.luma(99, w, h)
    y0, y1, x0, x1 = OVERLAY_BOX
    with_overlay = []
    for f in frames:
        g = f.copy()
        g[y0:y1, x0:x1] = hud[y0:y1, x0:x1]
        with_overlay.append(g)
    mask = full(h, w)
    k = OVERLAY_MARGIN
    mask[max(y0 - k, 0):min(y1 + k, h), max(x0 - k, 0):min(x1 + k, w)] = 0
    return K, frames, with_overlay, rots, mask


def planned_key_clip():
    """((w, h), frames, mask) of the planned-key-frame clip: corner_tiles.pipeline_clip("under_spec_cap") with the mask zero on rows < 70"""
    (w, h), frames = C.pipeline_clip("under_spec_cap")
    m = full(h, w, 1)
    m[:70] = 0
    return (w, h), frames, m


def run_state_machine(frames, K, w, h, r, seed, find):
    """the oracle state machine over a clip with the detector `find`: (state machine, frames it emits, (n_corners, n_tracked) per frame,
    rotations handed to the warp)"""
    Ko, _ = oracle.get_output_camera(K, w, h)
    rng = oracle.Pcg32(seed)
    counts, warp_rots = [], []

    def track(prev, cur, corners):
        if len(corners) == 0:
            counts.append((0, 0))
            return corners, corners
        nxt, st = oracle.pyr_lk(prev, cur, corners)
        counts.append((len(corners), int((st > 0).sum())))
        return corners[st > 0], nxt[st > 0]

    sm = oracle.WarpStateMachine(frames, r, find, track, lambda pp, cp: oracle.estimate_rotation(pp, cp, K, Ko, rng), lambda f, R: (warp_rots.append(R), f)[1])
    exp = []
    while True:
        o = sm.pull_frame()
        if o is None:
            break
        exp.append(o)
    return sm, exp, counts, warp_rots
