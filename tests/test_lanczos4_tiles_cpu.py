"""CPU model of the Lanczos warp's tile boxes (tests/lanczos4_tiles.py: k_warp_lanczos4's box restated on the oracle's exact map).  It
proves that the parameter sets of the GPU tests (test_lanczos4_gpu.py) reach every path of the kernel: BGR / luma / chroma tiles with
no box, staged in LDS and gathered from global memory, all three in one launch, and boxes of exactly the LDS budget and one footprint
row over it.  The model is exact (no margin): the counts below are what the kernel does, tile for tile."""
import pytest

import lanczos4_tiles
from test_cubic_tiles_cpu import anamorphic

# name: (sw, sh, dw, dh, sx, sy, roll, map mode, {plane: {state: count}}) -- the counts each set is committed to reach.
#   (a) staged and gathered tiles on every plane                      luma_gathers, all_states, gather_540
#   (b) luma gathered while chroma stages                              luma_gathers, luma_over_one_row
#   (c) no-box, staged and gathered tiles in one launch, every plane  all_states
#   (d) boxes of exactly the budget, and a box one footprint row over it in the same launch: *_at_budget, *_over_one_row.  A box
#       one element over the budget does not exist here: a Lanczos box is at least 8 x 8, 6145 = 5 x 1229 and 12289 is prime.  The
#       vertical sets have boxes 24 (BGR, luma) and 16 (chroma) wide, so one row over is 24 / 16 elements over.
#   (e) partial right / bottom tiles (odd dw and dh) that stage       luma_gathers, all_states
TILE_SETS = {
    "luma_gathers": (4096, 256, 767, 47, 12.0, 1.3, 0.003, 0,
                     {"bgr": {"staged": 24, "gathered": 12, "partial_staged": 10},
                      "luma": {"staged": 30, "gathered": 6, "partial_staged": 12}, "chroma": {"staged": 36, "gathered": 0, "partial_staged": 14}}),
    "all_states": (4096, 256, 1023, 47, 16.0, 2.0, 0.003, 0,
                   {"bgr": {"none": 12, "staged": 18, "gathered": 18, "partial_staged": 6},
                    "luma": {"none": 12, "staged": 24, "gathered": 12, "partial_staged": 8},
                    "chroma": {"none": 12, "staged": 30, "gathered": 6, "partial_staged": 10}}),
    "all_gather": (4096, 256, 192, 48, 16.0, 3.0, 0.003, 0, {"bgr": {"gathered": 9}, "luma": {"gathered": 9}, "chroma": {"gathered": 9}}),
    "bgr_at_budget": (64, 4096, 64, 32, 0.26, 16.66, 0.0, 0, {"bgr": {"at_budget": 2, "staged": 2}, "luma": {"staged": 2}, "chroma": {"staged": 2}}),
    "bgr_over_one_row": (64, 4096, 64, 32, 0.26, 16.71, 0.0, 0,
                         {"bgr": {"at_budget": 1, "staged": 1, "gathered": 1, "least_over": 24}, "luma": {"staged": 2}}),
    "luma_at_budget": (64, 4096, 64, 32, 0.26, 33.785, 0.0, 0, {"bgr": {"gathered": 2}, "luma": {"at_budget": 1, "staged": 2}, "chroma": {"staged": 2}}),
    "luma_over_one_row": (64, 4096, 64, 32, 0.26, 33.85, 0.0, 0,
                          {"luma": {"at_budget": 1, "staged": 1, "gathered": 1, "least_over": 24}, "chroma": {"staged": 2, "gathered": 0}}),
    "chroma_at_budget": (64, 4096, 64, 32, 0.26, 54.0, 0.0, 0, {"luma": {"gathered": 2}, "chroma": {"at_budget": 1, "staged": 2}}),
    "chroma_over_one_row": (64, 4096, 64, 32, 0.26, 54.1, 0.0, 0, {"chroma": {"at_budget": 1, "staged": 1, "gathered": 1, "least_over": 16}}),
    # the gathered set of the 4 GiB tests (their 640 x 540 frame; test_cubic_paths_gpu.frames_4g)
    "gather_540": (640, 540, 256, 160, 4.0, 8.0, 0.003, 0,
                   {"bgr": {"none": 16, "staged": 0, "gathered": 24}, "luma": {"none": 16, "staged": 10, "gathered": 14},
                    "chroma": {"none": 16, "staged": 16, "gathered": 8}}),
}


def set_params(name):
    """-> (params, sw, sh, dw, dh, mode) of a TILE_SETS entry."""
    sw, sh, dw, dh, sx, sy, roll, mode, _ = TILE_SETS[name]
    return anamorphic(sw, sh, dw, dh, sx, sy, roll), sw, sh, dw, dh, mode


def states(name):
    p, sw, sh, dw, dh, mode = set_params(name)
    return lanczos4_tiles.states_of(p, dw, dh, sw, sh, mode)


@pytest.mark.parametrize("name", sorted(TILE_SETS))
def test_tile_set_reaches_its_states(name):
    s = states(name)
    for plane, want in TILE_SETS[name][8].items():
        for k, v in want.items():
            assert s[plane][k] == v, (name, plane, k, s[plane])


def test_tile_sets_reach_every_state_between_them():
    """(a) .. (e) of the table's legend, recomputed from the model rather than read from the table."""
    S = {n: states(n) for n in TILE_SETS}
    for plane in ("bgr", "luma", "chroma"):
        assert any(s[plane]["staged"] for s in S.values()) and any(s[plane]["gathered"] for s in S.values()), plane   # (a)
        assert any(s[plane]["none"] and s[plane]["staged"] and s[plane]["gathered"] for s in S.values()), plane         # (c)
        assert any(s[plane]["at_budget"] and s[plane]["gathered"] for s in S.values()), plane                          # (d)
    assert any(s["luma"]["gathered"] and s["chroma"]["staged"] and not s["chroma"]["gathered"] for s in S.values())    # (b)
    assert any(s["bgr"]["least_over"] == 24 for s in S.values()) and any(s["luma"]["least_over"] == 24 for s in S.values())
    assert any(s["chroma"]["least_over"] == 16 for s in S.values())
    assert any(s["luma"]["partial_staged"] and s["chroma"]["partial_staged"] for s in S.values())                      # (e)


def test_budget_plus_one_has_no_box():
    """Every Lanczos box is at least 8 x 8: 6145 = 5 x 1229 (1229 prime) and 12289 (prime) are no box's element count."""
    def boxes(n):
        return [(d, n // d) for d in range(8, n // 8 + 1) if n % d == 0]
    assert boxes(lanczos4_tiles.BUDGET["bgr"] + 1) == [] and boxes(lanczos4_tiles.BUDGET["luma"] + 1) == []


def test_model_box_is_the_footprint_extremes():
    """One tile, every pixel at X = 10.5 except one at (40.25, 7.0) -> luma box columns 7 .. 44, rows 4 .. 11; chroma from 0.5 * map."""
    import numpy as np
    mx = np.full((16, 70), 10.5, np.float32)
    my = np.full((16, 70), 7.0, np.float32)
    mx[5, 3], my[5, 3] = 40.25, 7.0          # odd column: luma only
    x0, y0, bw, bh, have = (a[0, 0] for a in lanczos4_tiles.tile_boxes(mx, my, 100, 100)["luma"])
    assert have and (x0, y0, bw, bh) == (7, 4, 38, 8)
    x0, y0, bw, bh, have = (a[0, 0] for a in lanczos4_tiles.tile_boxes(mx, my, 100, 100)["chroma"])
    assert have and (x0, y0, bw, bh) == (2, 0, 8, 8)    # (5, 3) after quantisation, X - 3 .. X + 4
    mx[:, 64:] = 1e6
    s = lanczos4_tiles.tile_states(mx, my, 100, 100)
    assert s["luma"]["none"] == 1 and s["luma"]["staged"] == 1
