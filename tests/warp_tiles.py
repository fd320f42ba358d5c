"""CPU model of the tiles of the warp kernels whose source box is exact, not probed -- k_warp_cubic / k_warp_lanczos4 and their _rs forms,
k_warp_border, k_warp_cubic_border / k_warp_lanczos4_border, k_warp_keep (video-annotator_amd/csrc/vstab_warp_cubic.hip,
vstab_warp_lanczos4.hip, vstab_warp_border.hip, vstab_warp_keep.hip over vstab_resample.hpp) --, restated from exact map planes.  Test
infrastructure only (a plain module).

Per 64 x 16 output tile and plane:
  samples   luma / BGR: every pixel of the tile, those right of / below the image evaluated at the last column / row (min(x, dw - 1),
            min(y, dh - 1)), quantised (warp_def.quantise).  chroma: the even lanes (even x) of the even rows of the tile, quantised from
            0.5f * map and held against the (sw / 2) x (sh / 2) chroma plane
  rule      which samples count towards the box (kernel_rule says which kernel has which):
              every     all of them, in virtual (not border-interpolated) coordinates: a tile far outside stages reflected picture
              clamp     all of them, X first clamped to [-2, w] and Y to [-2, h] (k_warp_border under BORDER_CONSTANT)
              touching  those whose K x K footprint touches the source: X - LO + K - 1 >= 0, X - LO < w, and the same for Y
              written   those inside the image that the keep-edge warp writes (warp_def.inlier): the box always lies inside the plane
  box       columns min X - LO .. max X - LO + K - 1 of the counted samples, rows likewise; a tile with none has no box
  path      no box, staged (w * h <= budget) or gathered from global memory (over the budget)
  budgets   6144 BGRx dwords, 12288 luma bytes, 6144 chroma pairs (24 KiB of LDS; the plane-wise kernels give luma and chroma half each)

The kernels' boxes are exact and their maps are bit for bit oracle.create_map_ex for modes 0..4 (what warp_def.maps gives), so the model
needs no margin: it predicts the path of every tile."""
import numpy as np

import oracle
import warp_def as wd

TW, TH = 64, 16
BUDGET = {"bgr": 6144, "luma": 12288, "chroma": 6144}
RULES = ("every", "clamp", "touching", "written")
BORDER_STATES = ("staged", "gathered", "at_budget", "outside_staged", "cross_l", "cross_r", "cross_t", "cross_b", "odd_w", "even_w")
KEEP_STATES = ("all_kept", "all_written", "mixed", "staged", "gathered", "ragged_mixed", "staged_mixed", "gathered_mixed")


def kernel_rule(resampler, border_mode):
    """The rule of the kernel a launch of (resampler, border mode) runs.  linear + CONSTANT has no exact-box kernel (the bilinear kernels
    probe their box: tests/layouts.py), so `clamp` is reached by running k_warp_border under BORDER_CONSTANT only."""
    assert not (resampler == "linear" and border_mode == wd.CONSTANT)
    if border_mode == wd.TRANSPARENT:
        return "written"
    return "touching" if border_mode == wd.CONSTANT else "every"


def _tiled(a, ty, tx, rh, rw):
    """(ty * rh, tx * rw) -> (ty, tx, rh * rw)"""
    return a.reshape(ty, rh, tx, rw).transpose(0, 2, 1, 3).reshape(ty, tx, rh * rw)


def sample_grids(mapx, mapy):
    """Exact map planes (dh, dw) -> {plane: (X, Y, real)}, each (tile rows, tile columns, samples of a tile): the quantised samples of the
    frame padded to whole tiles at the edge value, and which of them lie inside the image."""
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    dh, dw = mapx.shape
    ty, tx = -(-dh // TH), -(-dw // TW)
    pad = ((0, ty * TH - dh), (0, tx * TW - dw))
    mx, my = np.pad(mapx, pad, mode="edge"), np.pad(mapy, pad, mode="edge")   # the clamped coordinates of the kernels' step 1
    real = np.pad(np.ones((dh, dw), bool), pad)
    X, Y, _ = wd.quantise(mx, my)
    cx, cy, _ = wd.quantise(mx[::2, ::2] * np.float32(0.5), my[::2, ::2] * np.float32(0.5))
    full = tuple(_tiled(a, ty, tx, TH, TW) for a in (X, Y, real))
    return {"bgr": full, "luma": full, "chroma": tuple(_tiled(a, ty, tx, TH // 2, TW // 2) for a in (cx, cy, real[::2, ::2]))}


def plane_size(plane, sw, sh):
    return (sw >> 1, sh >> 1) if plane == "chroma" else (sw, sh)


def _counted(X, Y, real, w, h, K, LO, rule):
    """The samples of each tile that count towards its box, and their positions."""
    if rule == "clamp":
        X, Y = np.clip(X, -2, w), np.clip(Y, -2, h)
    if rule == "touching":
        return X, Y, (X - LO + K - 1 >= 0) & (X - LO < w) & (Y - LO + K - 1 >= 0) & (Y - LO < h)
    if rule == "written":
        return X, Y, real & wd.inlier(X, Y, w, h)
    return X, Y, np.ones(X.shape, bool)


def _tiles(mapx, mapy, sw, sh, resampler, rule):
    """-> {plane: (x0, y0, bw, bh, have, counted, real)}: tile_boxes' boxes, and per sample what counted and what lies inside the image."""
    assert rule in RULES, rule
    K, LO = wd.FOOTPRINT[resampler]
    big = np.int64(1) << 40
    out = {}
    for plane, (X, Y, real) in sample_grids(mapx, mapy).items():
        X, Y, t = _counted(X, Y, real, *plane_size(plane, sw, sh), K, LO, rule)
        have = t.any(-1)
        x0, y0 = np.where(t, X, big).min(-1) - LO, np.where(t, Y, big).min(-1) - LO
        bw = np.where(have, np.where(t, X, -big).max(-1) - LO + K - x0, 0)
        bh = np.where(have, np.where(t, Y, -big).max(-1) - LO + K - y0, 0)
        out[plane] = (x0, y0, bw, bh, have, t, real)
    return out


def tile_boxes(mapx, mapy, sw, sh, resampler, rule):
    """Exact map planes (dh, dw) of a warp from a sw x sh source -> {plane: (x0, y0, bw, bh, have)} with arrays of shape (tile rows, tile
    columns), planes 'bgr' / 'luma' (the same box: both are the map's footprints against the full-size source) and 'chroma'."""
    return {plane: v[:5] for plane, v in _tiles(mapx, mapy, sw, sh, resampler, rule).items()}


def tile_states(mapx, mapy, sw, sh, resampler, rule):
    """-> {plane: {state: count of tiles}}:
      none / all_kept      no box (no sample counts); all_written: every sample inside the image counts; mixed: some do
      staged, gathered     boxes within / over the budget; at_budget, over_by_one: boxes of exactly the budget and one element over it;
                           least_over: the least element count over the budget of any gathered box (None when nothing gathers)
      odd_w, even_w        staged boxes of odd and even width
      partial_staged       staged tiles that the right or bottom edge of the output cuts (dw % 64, dh % 16)
      outside_staged       staged boxes wholly outside the plane; cross_l / _r / _t / _b: staged boxes across its left, right, top, bottom edge
      staged_mixed, gathered_mixed, ragged_mixed   mixed tiles by path, and mixed tiles with fewer samples inside the image than a whole tile"""
    dh, dw = np.asarray(mapx).shape
    out = {}
    for plane, (x0, y0, bw, bh, have, t, real) in _tiles(mapx, mapy, sw, sh, resampler, rule).items():
        w, h = plane_size(plane, sw, sh)
        t = t & real
        cap = BUDGET[plane]
        area = bw * bh
        staged, gathered = have & (area <= cap), have & (area > cap)
        mixed = have & (t.sum(-1) < real.sum(-1))
        ragged = real.sum(-1) < real.shape[-1]
        partial = np.zeros(have.shape, bool)
        partial[:, -1] |= dw % TW != 0
        partial[-1, :] |= dh % TH != 0
        outside = (x0 + bw <= 0) | (x0 >= w) | (y0 + bh <= 0) | (y0 >= h)
        masks = {
            "none": ~have, "all_kept": ~have, "all_written": have & ~mixed, "mixed": mixed, "staged": staged, "gathered": gathered,
            "at_budget": have & (area == cap), "over_by_one": have & (area == cap + 1),
            "odd_w": staged & (bw % 2 == 1), "even_w": staged & (bw % 2 == 0), "partial_staged": staged & partial,
            "outside_staged": staged & outside,
            "cross_l": staged & (x0 < 0) & (x0 + bw > 0), "cross_r": staged & (x0 < w) & (x0 + bw > w),
            "cross_t": staged & (y0 < 0) & (y0 + bh > 0), "cross_b": staged & (y0 < h) & (y0 + bh > h),
            "staged_mixed": staged & mixed, "gathered_mixed": gathered & mixed, "ragged_mixed": mixed & ragged,
        }
        out[plane] = {k: int(v.sum()) for k, v in masks.items()}
        out[plane]["least_over"] = int((area[gathered] - cap).min()) if gathered.any() else None
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the parameter sets of the tests
# ---------------------------------------------------------------------------------------------------------------------
def anamorphic(sw, sh, dw, dh, sx, sy, roll):
    """Source focal lengths 100 sx / 100 sy against an output camera of focal length 100, both principal points centred, rolled about the
    optical axis: the source box of a 64 x 16 tile is about 64 sx wide and 16 sy tall, and an output larger than the source over sx, sy
    reaches beyond every edge."""
    Ki = np.array([[100.0 * sx, 0, sw / 2], [0, 100.0 * sy, sh / 2], [0, 0, 1]])
    Ko = np.array([[100.0, 0, dw / 2], [0, 100.0, dh / 2], [0, 0, 1]])
    return oracle.map_params(Ki, Ko, oracle.rodrigues((0.0, 0.0, roll)))


# kernel: (resampler, the border mode its sets are committed under)
KERNELS = {"cubic": ("cubic", wd.CONSTANT), "lanczos4": ("lanczos4", wd.CONSTANT), "border": ("linear", wd.REFLECT_101),
           "cubic_border": ("cubic", wd.REFLECT_101), "lanczos4_border": ("lanczos4", wd.REFLECT_101), "keep": ("linear", wd.TRANSPARENT)}
_M0, _M3 = 0, oracle.MAP_RECT_TO_RECT
_EDGES = {"outside_staged": 8, "cross_l": 1, "cross_r": 1, "cross_t": 1, "cross_b": 1, "odd_w": 1, "even_w": 1}
# kernel: {name: (sw, sh, dw, dh, sx, sy, roll, map mode, {plane: {state: count}})} -- anamorphic's pinhole maps.  The counts are what each
# set is committed to reach: exactly for "cubic" and "lanczos4", at least for the others (the *_tiles_cpu tests, test_resample_border_cpu.py
# and test_keep_tiles_cpu.py check them; the GPU tests of each kernel run the sets).
TILE_SETS = {
    # k_warp_cubic
    #   (a) BGR gathered               bgr_at_budget, luma_gathers, all_states, all_gather
    #   (b) luma gathered, chroma staged in the same launch              luma_at_budget, luma_gathers
    #   (c) luma and chroma gathered                                     all_states, all_gather
    #   (d) a box of exactly the budget: bgr_at_budget(_m0), luma_at_budget(_m0), chroma_at_budget; one element over it:
    #       bgr_over_by_one, chroma_over_by_one.  Luma's budget + 1 = 12289 is prime and a box is at least 4 x 4, so no box has it:
    #       luma_least_over has 12290 (5 x 2458), the least element count over the budget a box can have
    #   (e) no-box, staged and gathered tiles in one launch, every plane  all_states
    #   (f) partial right / bottom tiles (odd dw and dh) that stage       luma_gathers, all_states
    #   (g) odd and even staged widths, luma and chroma                   luma_gathers, all_states
    "cubic": {
        "bgr_at_budget": (4096, 256, 192, 48, 4.0, 1.3, 0.003, _M3,
                          {"bgr": {"at_budget": 5, "staged": 7, "gathered": 2}, "luma": {"gathered": 0}, "chroma": {"gathered": 0}}),
        "bgr_at_budget_m0": (4096, 256, 192, 48, 4.13, 1.3, 0.003, _M0, {"bgr": {"at_budget": 1, "gathered": 0}}),
        "luma_at_budget": (4096, 256, 192, 48, 8.07, 1.3, 0.003, _M3,
                           {"bgr": {"gathered": 9}, "luma": {"at_budget": 2, "staged": 4, "gathered": 5}, "chroma": {"staged": 9, "gathered": 0}}),
        "luma_at_budget_m0": (4096, 256, 192, 48, 8.33, 1.3, 0.003, _M0, {"bgr": {"gathered": 9}, "luma": {"at_budget": 1, "gathered": 0}}),
        "luma_gathers": (4096, 256, 767, 47, 12.0, 1.3, 0.003, _M0,
                         {"bgr": {"staged": 24, "gathered": 12}, "luma": {"staged": 30, "gathered": 6, "partial_staged": 12, "odd_w": 11, "even_w": 19},
                          "chroma": {"staged": 36, "gathered": 0, "partial_staged": 14, "odd_w": 21, "even_w": 15}}),
        "all_states": (4096, 256, 1023, 47, 16.0, 2.0, 0.003, _M0,
                       {"bgr": {"none": 12, "staged": 18, "gathered": 18, "partial_staged": 6},
                        "luma": {"none": 12, "staged": 24, "gathered": 12, "partial_staged": 8, "odd_w": 11, "even_w": 13},
                        "chroma": {"none": 12, "staged": 30, "gathered": 6, "partial_staged": 10, "odd_w": 10, "even_w": 20}}),
        "all_gather": (4096, 256, 192, 48, 16.0, 3.0, 0.003, _M0, {"bgr": {"gathered": 9}, "luma": {"gathered": 9}, "chroma": {"gathered": 9}}),
        "chroma_at_budget": (64, 4096, 64, 32, 0.26, 72.9, 0.0, _M0, {"luma": {"gathered": 2}, "chroma": {"at_budget": 1, "staged": 2}}),
        "bgr_over_by_one": (64, 4096, 64, 32, 0.02, 82.25, 0.0, _M0, {"bgr": {"over_by_one": 1, "staged": 1, "gathered": 1}, "luma": {"staged": 2}}),
        "luma_least_over": (64, 8192, 64, 32, 0.02, 164.85, 0.0, _M0, {"luma": {"gathered": 2, "least_over": 2}, "chroma": {"staged": 2}}),
        "chroma_over_by_one": (64, 8192, 64, 32, 0.02, 175.9, 0.0, _M0, {"chroma": {"over_by_one": 1, "staged": 1, "gathered": 1}}),
        # the gathered set of the 4 GiB tests (their 640 x 540 frame)
        "gather_540": (640, 540, 256, 160, 4.0, 8.0, 0.003, _M0,
                       {"bgr": {"none": 16, "staged": 0, "gathered": 24}, "luma": {"none": 16, "staged": 15, "gathered": 9},
                        "chroma": {"none": 16, "staged": 16, "gathered": 8}}),
    },
    # k_warp_lanczos4
    #   (a) staged and gathered tiles on every plane                      luma_gathers, all_states, gather_540
    #   (b) luma gathered while chroma stages                              luma_gathers, luma_over_one_row
    #   (c) no-box, staged and gathered tiles in one launch, every plane  all_states
    #   (d) boxes of exactly the budget, and a box one footprint row over it in the same launch: *_at_budget, *_over_one_row.  A box
    #       one element over the budget does not exist here: a Lanczos box is at least 8 x 8, 6145 = 5 x 1229 and 12289 is prime.  The
    #       vertical sets have boxes 24 (BGR, luma) and 16 (chroma) wide, so one row over is 24 / 16 elements over.
    #   (e) partial right / bottom tiles (odd dw and dh) that stage       luma_gathers, all_states
    "lanczos4": {
        "luma_gathers": (4096, 256, 767, 47, 12.0, 1.3, 0.003, _M0,
                         {"bgr": {"staged": 24, "gathered": 12, "partial_staged": 10},
                          "luma": {"staged": 30, "gathered": 6, "partial_staged": 12}, "chroma": {"staged": 36, "gathered": 0, "partial_staged": 14}}),
        "all_states": (4096, 256, 1023, 47, 16.0, 2.0, 0.003, _M0,
                       {"bgr": {"none": 12, "staged": 18, "gathered": 18, "partial_staged": 6},
                        "luma": {"none": 12, "staged": 24, "gathered": 12, "partial_staged": 8},
                        "chroma": {"none": 12, "staged": 30, "gathered": 6, "partial_staged": 10}}),
        "all_gather": (4096, 256, 192, 48, 16.0, 3.0, 0.003, _M0, {"bgr": {"gathered": 9}, "luma": {"gathered": 9}, "chroma": {"gathered": 9}}),
        "bgr_at_budget": (64, 4096, 64, 32, 0.26, 16.66, 0.0, _M0, {"bgr": {"at_budget": 2, "staged": 2}, "luma": {"staged": 2}, "chroma": {"staged": 2}}),
        "bgr_over_one_row": (64, 4096, 64, 32, 0.26, 16.71, 0.0, _M0,
                             {"bgr": {"at_budget": 1, "staged": 1, "gathered": 1, "least_over": 24}, "luma": {"staged": 2}}),
        "luma_at_budget": (64, 4096, 64, 32, 0.26, 33.785, 0.0, _M0, {"bgr": {"gathered": 2}, "luma": {"at_budget": 1, "staged": 2}, "chroma": {"staged": 2}}),
        "luma_over_one_row": (64, 4096, 64, 32, 0.26, 33.85, 0.0, _M0,
                              {"luma": {"at_budget": 1, "staged": 1, "gathered": 1, "least_over": 24}, "chroma": {"staged": 2, "gathered": 0}}),
        "chroma_at_budget": (64, 4096, 64, 32, 0.26, 54.0, 0.0, _M0, {"luma": {"gathered": 2}, "chroma": {"at_budget": 1, "staged": 2}}),
        "chroma_over_one_row": (64, 4096, 64, 32, 0.26, 54.1, 0.0, _M0, {"chroma": {"at_budget": 1, "staged": 1, "gathered": 1, "least_over": 16}}),
        # the gathered set of the 4 GiB tests (their 640 x 540 frame; test_cubic_paths_gpu.frames_4g)
        "gather_540": (640, 540, 256, 160, 4.0, 8.0, 0.003, _M0,
                       {"bgr": {"none": 16, "staged": 0, "gathered": 24}, "luma": {"none": 16, "staged": 10, "gathered": 14},
                        "chroma": {"none": 16, "staged": 16, "gathered": 8}}),
    },
    # k_warp_border
    "border": {
        # a small source seen from far away: tiles wholly outside on every side (they stage reflected picture), boxes across all four edges
        "zoomed_out": (96, 64, 512, 256, 0.25, 0.25, 0.1, _M3, {p: dict(_EDGES) for p in ("bgr", "chroma")}),
        # strong minification: every plane's boxes over the budget
        "gathers": (4096, 256, 192, 48, 16.0, 3.0, 0.003, _M3, {"bgr": {"gathered": 9}, "luma": {"gathered": 9}, "chroma": {"gathered": 9}}),
        # boxes of exactly the budget: BGR (6144 dwords), luma (12288 bytes) with BGR gathered in the same frame, chroma (6144 pairs)
        "bgr_at_budget": (4096, 256, 192, 48, 4.02, 1.4, 0.003, _M3, {"bgr": {"at_budget": 2, "staged": 9}}),
        "luma_at_budget": (4096, 256, 192, 48, 8.08, 1.4, 0.003, _M3, {"bgr": {"gathered": 9}, "luma": {"at_budget": 1, "staged": 9}}),
        "chroma_at_budget": (4096, 256, 192, 48, 16.43, 1.3, 0.003, _M3, {"chroma": {"at_budget": 1, "staged": 9}, "luma": {"gathered": 1}}),
    },
    # k_warp_cubic_border / k_warp_lanczos4_border: the at-budget sets were found by scanning sx and sy against this model
    "cubic_border": {
        "zoomed_out": (96, 64, 512, 256, 0.4, 0.4, 0.1, _M3, {p: dict(_EDGES) for p in ("bgr", "chroma")}),
        "gathers": (4096, 256, 192, 48, 16.0, 3.0, 0.003, _M3, {p: {"gathered": 9} for p in ("bgr", "luma", "chroma")}),
        "bgr_at_budget": (4096, 256, 192, 48, 3.99, 1.3, 0.003, _M3, {"bgr": {"at_budget": 2, "staged": 9}}),
        "luma_at_budget": (4096, 256, 192, 48, 8.05, 1.3, 0.003, _M3, {"bgr": {"gathered": 9}, "luma": {"at_budget": 3, "staged": 9}}),
        "chroma_at_budget": (4096, 256, 192, 48, 16.345, 1.1, 0.003, _M3, {"chroma": {"at_budget": 1, "staged": 9}, "luma": {"gathered": 9}}),
    },
    "lanczos4_border": {
        "zoomed_out": (96, 64, 512, 256, 0.4, 0.4, 0.1, _M3, {p: dict(_EDGES) for p in ("bgr", "chroma")}),
        "gathers": (4096, 256, 192, 48, 16.0, 3.0, 0.003, _M3, {p: {"gathered": 9} for p in ("bgr", "luma", "chroma")}),
        "bgr_at_budget": (4096, 256, 192, 48, 3.935, 1.1, 0.003, _M3, {"bgr": {"at_budget": 1, "staged": 1, "gathered": 8}}),
        "luma_at_budget": (4096, 256, 192, 48, 7.995, 1.1, 0.003, _M3, {"bgr": {"gathered": 9}, "luma": {"at_budget": 1, "staged": 1}}),
        "chroma_at_budget": (4096, 256, 192, 48, 12.1, 1.1, 0.003, _M3, {"chroma": {"at_budget": 2, "staged": 9}, "luma": {"gathered": 9}}),
    },
    # k_warp_keep
    "keep": {
        # a small source seen from far away: tiles wholly outside on every side, wholly inside in the middle, mixed around the picture
        "zoomed_out": (96, 64, 512, 256, 0.25, 0.25, 0.1, _M3,
                       {p: {"all_kept": 8, "all_written": 8, "mixed": 8, "staged_mixed": 8} for p in ("bgr", "luma", "chroma")}),
        # the same with an image that ends inside its last tile column and row: mixed tiles with ragged edges
        "zoomed_out_ragged": (96, 64, 500, 250, 0.25, 0.25, 0.1, _M3, {p: {"ragged_mixed": 1, "all_kept": 8} for p in ("bgr", "luma", "chroma")}),
        # strong minification over the source's edges: mixed tiles whose box is over the budget
        "gathers_edge": (2048, 128, 192, 48, 16.0, 3.0, 0.003, _M3,
                         {"bgr": {"gathered_mixed": 2}, "luma": {"gathered_mixed": 2}, "chroma": {"gathered_mixed": 2, "staged_mixed": 2}}),
        # and well inside it: every tile gathered, every sample written
        "gathers_in": (4096, 256, 192, 48, 16.0, 3.0, 0.003, _M3, {p: {"gathered": 9, "all_written": 9} for p in ("bgr", "luma", "chroma")}),
    },
}


def set_params(kernel, name):
    """-> (params, sw, sh, dw, dh, mode) of a TILE_SETS entry."""
    sw, sh, dw, dh, sx, sy, roll, mode, _ = TILE_SETS[kernel][name]
    return anamorphic(sw, sh, dw, dh, sx, sy, roll), sw, sh, dw, dh, mode


def states_of(kernel, name, rule=None):
    """tile_states of a TILE_SETS entry under its kernel's rule (or another rule of the same kernel)."""
    params, sw, sh, dw, dh, mode = set_params(kernel, name)
    resampler, border_mode = KERNELS[kernel]
    return tile_states(*wd.maps(params, dw, dh, mode), sw, sh, resampler, rule or kernel_rule(resampler, border_mode))
