"""CPU model of the Lanczos warp's tile boxes (tests/warp_tiles.py, rule `touching`: k_warp_lanczos4's box restated on the oracle's exact
map).  It proves that the parameter sets of the GPU tests (test_lanczos4_gpu.py) reach every path of the kernel: BGR / luma / chroma tiles with
no box, staged in LDS and gathered from global memory, all three in one launch, and boxes of exactly the LDS budget and one footprint
row over it.  The model is exact (no margin): the counts below are what the kernel does, tile for tile."""
import pytest

import warp_tiles as wt

TILE_SETS = wt.TILE_SETS["lanczos4"]


def states(name):
    return wt.states_of("lanczos4", name)


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
    assert boxes(wt.BUDGET["bgr"] + 1) == [] and boxes(wt.BUDGET["luma"] + 1) == []


def test_model_box_is_the_footprint_extremes():
    """One tile, every pixel at X = 10.5 except one at (40.25, 7.0) -> luma box columns 7 .. 44, rows 4 .. 11; chroma from 0.5 * map."""
    import numpy as np
    mx = np.full((16, 70), 10.5, np.float32)
    my = np.full((16, 70), 7.0, np.float32)
    mx[5, 3], my[5, 3] = 40.25, 7.0          # odd column: luma only
    x0, y0, bw, bh, have = (a[0, 0] for a in wt.tile_boxes(mx, my, 100, 100, "lanczos4", "touching")["luma"])
    assert have and (x0, y0, bw, bh) == (7, 4, 38, 8)
    x0, y0, bw, bh, have = (a[0, 0] for a in wt.tile_boxes(mx, my, 100, 100, "lanczos4", "touching")["chroma"])
    assert have and (x0, y0, bw, bh) == (2, 0, 8, 8)    # (5, 3) after quantisation, X - 3 .. X + 4
    mx[:, 64:] = 1e6
    s = wt.tile_states(mx, my, 100, 100, "lanczos4", "touching")
    assert s["luma"]["none"] == 1 and s["luma"]["staged"] == 1
