"""CPU model of the tiled warp kernels' XCD band / tile schedule (layouts.tile_schedule, layouts.block_tiles: vstab_warp_tile.hpp
tile_schedule and the block -> tile prologue of k_warp_fused / k_warp_planar) and of the three launchers' choices of tile height, LDS
and tail (layouts.fused_launch, fused10_launch, planar_schedule_launch).  It proves, for every output size of a dense sweep and the
shapes of test_shapes_gpu.py, that the grid covers each 64-column tile row exactly once and that no live workgroup starts below the
image; that the GPU shapes between them reach every launcher branch; and it pins the launcher constants the model copies against the
sources, so that a change to a launcher has to update the model (and with it the claims above)."""
import os
import re

import numpy as np
import pytest

import layouts
import oracle
from test_shapes_gpu import SHAPES, STATELESS_OUTPUTS, warp_output

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-annotator_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def launches(dw, dh):
    """-> {launcher: (rwb, lds_kb, tail_rounds)} for an output of dw x dh."""
    return {"fused": layouts.fused_launch(dw, dh), "fused10": layouts.fused10_launch(dw, dh),
            "planar8": layouts.planar_schedule_launch(dw, dh, 8), "planar10": layouts.planar_schedule_launch(dw, dh, 10)}


def check_schedule(dw, dh, rwb, lds_kb, tail):
    """Every 64-column tile row of the output covered exactly once (by a tall tile or by half-height tiles), no live workgroup at
    ys >= dh, tall tiles inside their band, grid == 8 max(share)."""
    s = layouts.tile_schedule(dw, dh, rwb, lds_kb, tail)
    assert s["grid"] == 8 * max(s["shares"])
    assert s["band_y"][0] == 0 and s["band_y"][8] == dh and all(a <= b for a, b in zip(s["band_y"], s["band_y"][1:]))
    ts = 2 * rwb
    half_rows = -(-dh // ts)
    live, idle = layouts.block_tiles(s, rwb)
    assert len(live) + idle == s["grid"]
    b, x0, ys, rows = (np.array(v, np.int64) for v in zip(*live))
    assert (ys < dh).all() and (ys >= 0).all() and (x0 < dw).all() and (x0 % 64 == 0).all() and (ys % ts == 0).all()
    k = b & 7
    band_lo, band_hi = np.array(s["band_y"])[k], np.array(s["band_y"])[k + 1]
    assert (ys >= band_lo).all() and (ys < band_hi).all()
    tall = rows == 2 * ts
    assert (ys[tall] + rows[tall] <= band_hi[tall]).all()          # a tall tile never reaches into the next XCD's band
    cover = np.zeros((half_rows, s["tiles_x"]), np.int64)
    for n in (1, 2):                                               # the half-height rows a tile covers
        sel = rows >= n * ts
        np.add.at(cover, (ys[sel] // ts + n - 1, x0[sel] // 64), 1)
    assert cover.min() == 1 and cover.max() == 1, (dw, dh, rwb, lds_kb, tail, int((cover != 1).sum()))
    return s, live


_seen = {}


def _check_cached(dw, dh, rwb, lds_kb, tail):
    key = (-(-dw // 64), dh, rwb, lds_kb, tail)   # the schedule depends on dw only through the tile columns
    if key not in _seen:
        s, _ = check_schedule(((dw + 63) // 64) * 64, dh, rwb, lds_kb, tail)
        _seen[key] = s["grid"]
    return _seen[key]


def test_dense_sweep_of_small_outputs_every_launcher():
    """1..300 x 1..300 with each launcher's own choice, plus every tail the launchers use (0.25, 0.5) and a full round of half-height
    tiles, so that the tail arithmetic (lround(tail_rounds * slots / tiles_x) tall rows per band) is covered on small grids as well."""
    for dh in range(1, 301):
        for dw in range(1, 301):
            for rwb, lds_kb, tail in launches(dw, dh).values():
                _check_cached(dw, dh, rwb, lds_kb, tail)
        for dw in (1, 64, 65, 128, 300):
            for rwb, lds_kb in ((4, 14), (4, 20), (4, 28), (8, 24), (8, 40)):
                for tail in (0.25, 0.5, 1.0, 4.0):
                    _check_cached(dw, dh, rwb, lds_kb, tail)


def _all_outputs():
    out = [(dw, dh) for name in SHAPES for dw, dh in [warp_output(name)]]
    out += [(w, h) for name, (w, h, _) in SHAPES.items()] + list(STATELESS_OUTPUTS)
    return out + [(32767, 1), (1, 32767), (32767, 32767)]


@pytest.mark.parametrize("dw,dh", _all_outputs())
def test_gpu_shapes_and_the_largest_outputs(dw, dh):
    for what, (rwb, lds_kb, tail) in launches(dw, dh).items():
        check_schedule(dw, dh, rwb, lds_kb, tail)


def test_flat_output_leaves_bands_empty_and_the_last_band_cut_by_dh():
    """dw = 4000, dh = 40 (a stateless warp of test_shapes_gpu.py): 5 half-tile rows (64 x 8) for 8 XCDs -- three bands are empty and
    their workgroups all return at once; the last band ends at dh, inside its half-height row."""
    rwb, lds_kb, tail = layouts.fused_launch(4000, 40)
    assert (rwb, tail) == (4, 0.0)
    s, live = check_schedule(4000, 40, rwb, lds_kb, tail)
    rows = np.diff(s["band_y"])
    assert (rows == 0).sum() >= 3 and rows[-1] > 0
    assert {b & 7 for b, _, _, _ in live} != set(range(8))
    s, _ = check_schedule(4000, 37, rwb, lds_kb, tail)
    assert s["band_y"][8] - s["band_y"][7] == 5      # the last half-height row cut to 5 rows by dh


def test_portrait_bands_are_half_tail():
    """portrait1080 through the fused launcher: 18 tile columns and 64 x 16 tiles, half a round of half-height tiles -- lround(128 / 18)
    = 7 tall rows' worth at the end of every band, of the 15 a band of 248 rows holds: each band is about half tail."""
    dw, dh = warp_output("portrait1080")
    rwb, lds_kb, tail = layouts.fused_launch(dw, dh)
    assert (rwb, tail) == (4, 0.5)
    s, _ = check_schedule(dw, dh, rwb, lds_kb, tail)
    assert s["tiles_x"] == 18
    assert all(hi - sp >= 7 * 4 * rwb and sp > lo for lo, sp, hi in zip(s["band_y"], s["split_y"], s["band_y"][1:]))


def test_gpu_shapes_reach_every_launcher_branch():
    """The warp outputs test_shapes_gpu.py runs reach both tile heights of the fused 8-bit launcher with its tail on and off, the fused
    10-bit launcher's tail on and off, and the plane-wise launcher's quarter-round tail and no tail, at 8 and 10 bits."""
    reached = {k: set() for k in ("fused", "fused10", "planar8", "planar10")}
    for name in SHAPES:
        for k, v in launches(*warp_output(name)).items():
            reached[k].add(v)
    for dw, dh in STATELESS_OUTPUTS:
        for k, v in launches(dw, dh).items():
            reached[k].add(v)
    # (fused: 64 x 32 tiles need tiles32 >= 1536 > 256 x 4, so their tail is always on)
    assert {(r, t) for r, _, t in reached["fused"]} == {(4, 0.0), (4, 0.5), (8, 0.5)}, reached["fused"]
    assert {t for _, _, t in reached["fused10"]} == {0.0, 0.5}, reached["fused10"]
    for k in ("planar8", "planar10"):
        assert {(r, t) for r, _, t in reached[k]} >= {(4, 0.0), (4, 0.25), (8, 0.25)}, (k, reached[k])
    # the 4K headline output for comparison: the same branches as the past-4K shapes
    K = oracle.get_preset_camera(4, 3840, 2160)
    _, (cw, ch) = oracle.get_output_camera(K, 3840, 2160)
    assert launches(cw, ch)["fused"] == (8, 40, 0.5)


def test_launcher_constants_are_the_models():
    """The model's constants, as they stand in the launchers and in tile_schedule: change one there and this fails."""
    fused, planar, tile = _src("vstab_warp_fused.hip"), _src("vstab_warp_planar.hip"), _src("vstab_warp_tile.hpp")
    T = layouts.TILES32_RWB8
    assert f"int rwb = tiles32 < {T} ? 4 : 8, lds_kb = rwb == 4 ? {layouts.FUSED_LDS_KB[4]} : {layouts.FUSED_LDS_KB[8]};" in fused
    assert (f"double tail_rounds = (double)div_up(a.dw, 64) * div_up(a.dh, 4 * rwb) > {layouts.TAIL_SLOTS_PER_RESIDENT} * "
            f"({layouts.LDS_BUDGET_KB} / lds_kb) ? 0.5 : 0.0;") in fused
    assert f"const int lds_kb = {layouts.FUSED10_LDS_KB};" in fused and f"const int rwb = {layouts.FUSED10_RWB};" in fused
    assert f"tile_schedule(ta, rwb, lds_kb, tiles > {layouts.FUSED10_TAIL_TILES} ? 0.5 : 0.0)" in fused
    assert f"int rwb = tiles32 < {T} ? 4 : 8;" in planar
    assert "int lds_kb = rwb == 8 ? (bps == 2 ? 40 : 24) : 14 * bps;" in planar
    assert layouts.planar_launch(4000, 4000, 8)[1] == 24 and layouts.planar_launch(4000, 4000, 10)[1] == 40
    assert layouts.planar_launch(64, 64, 8)[1] == 14 and layouts.planar_launch(64, 64, 10)[1] == 28
    assert f"const int resident = std::min({{{layouts.LDS_BUDGET_KB} / lds_kb, rwb == 8 ? 7 : 8, 8}});" in planar
    assert f"> {layouts.TAIL_SLOTS_PER_RESIDENT} * resident ? 0.25 : 0.0;" in planar
    assert f"const int slots = {layouts.SLOTS_PER_WG_PER_CU} * std::max(1, std::min(8, (int)({layouts.LDS_BUDGET_KB} / lds_kb)));" in tile
    for line in ("ta.tiles_x = (int)div_up(a.dw, 64);", "const int th = 4 * rwb, ts = th / 2;", "const int half_rows = (int)div_up(a.dh, ts);",
                 "ta.band_y[k] = std::min(a.dh, (int)((long)k * half_rows / 8) * ts);", "ta.band_y[8] = a.dh;",
                 "const int tall_rows_max = rows / th;",
                 "const int tail_tall_rows = (int)std::min<long>(tall_rows_max, std::lround(tail_rounds * slots / ta.tiles_x));",
                 "ta.split_y[k] = ta.band_y[k] + tall_rows * th;",
                 "const int n = tall_rows * ta.tiles_x + (int)div_up(ta.band_y[k + 1] - ta.split_y[k], ts) * ta.tiles_x;",
                 "return 8u * (unsigned)share;"):
        assert line in tile, line
    for src in (fused, planar):                                   # the prologue block_tiles restates, in both kernels
        for line in ("const int k = (int)(blockIdx.x & 7u);", "const int n_tall = ((y_sp - y_lo) / TH) * ta.tiles_x;",
                     "const int idx = (int)(blockIdx.x >> 3);", "x0 = (idx - row * ta.tiles_x) * 64, ys = y_lo + row * TH;",
                     "x0 = (i2 - row * ta.tiles_x) * 64, ys = y_sp + row * TS, n_half = 1;", "if (ys >= y_hi) return;"):
            assert line in src, line
