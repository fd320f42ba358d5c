"""Masks, masked cases and clips for the detector tests (include/vstab.h, "Detection mask").  The definition of the
detector under a mask is corner_def's (candidates, select, Model); this module holds what the tests feed it: mask shapes, the cases that
separate the definition from its near misses, the named raw-detector sets, and the clips and state machine of the pipeline tests.  No GPU
here.  A plain module, imported by corner_def and the tests."""
import numpy as np

import corner_tiles as C
import oracle
import synth

TW, TH, SLOTS = C.TW, C.TH, C.SLOTS


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


# ---- the named raw-detector sets of the GPU test (corner_def.raw_masked_model; test_detection_mask_cpu.py asserts what they reach) -----------------------------------
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
