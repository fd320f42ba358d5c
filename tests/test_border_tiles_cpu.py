"""CPU model of the border warp's tile boxes (tests/border_tiles.py: k_warp_border's box restated on the oracle's exact map).  It proves that
the parameter sets of the GPU tests (test_border_gpu.py) reach every path of the kernel on BGR, luma and chroma: staged tiles, tiles over
the LDS budget, boxes of exactly the budget, tiles wholly outside the source (never read under BORDER_CONSTANT, reflected picture here),
boxes across each of the four edges, and staged boxes of odd and even width."""
import numpy as np
import pytest

import border_def
import border_tiles
import cubic_def


@pytest.mark.parametrize("name", sorted(border_tiles.TILE_SETS))
def test_set_reaches_its_committed_states(name):
    got = border_tiles.states_of(name)
    for plane, want in border_tiles.TILE_SETS[name][-1].items():
        for state, least in want.items():
            assert got[plane][state] >= least, (name, plane, state, got[plane])


def test_sets_cover_every_path_of_every_plane():
    total = {p: {} for p in ("bgr", "luma", "chroma")}
    for name in border_tiles.TILE_SETS:
        for plane, counts in border_tiles.states_of(name).items():
            for k, v in counts.items():
                total[plane][k] = total[plane].get(k, 0) + v
    for plane, counts in total.items():
        for state in ("staged", "gathered", "at_budget", "outside_staged", "cross_l", "cross_r", "cross_t", "cross_b", "odd_w", "even_w"):
            assert counts[state] > 0, (plane, state, counts)


def test_constant_border_keeps_boxes_near_the_source():
    """Under BORDER_CONSTANT the kernel clamps X to [-2, w] and Y to [-2, h] before the box: every box lies in [-2, w + 1] x [-2, h + 1], so
    the zoomed-out set's outside tiles stage a few border positions instead of reflected picture."""
    params, sw, sh, dw, dh, mode = border_tiles.set_params("zoomed_out")
    mx, my = cubic_def.maps(params, dw, dh, mode)
    for plane, (x0, y0, bw, bh) in border_tiles.tile_boxes(mx, my, sw, sh, border_def.CONSTANT).items():
        w, h = (sw, sh) if plane != "chroma" else (sw >> 1, sh >> 1)
        assert (x0 >= -2).all() and (x0 + bw <= w + 2).all() and (y0 >= -2).all() and (y0 + bh <= h + 2).all(), plane


def test_axis_pixel_stretches_one_box():
    """Map mode 0's 0/0 axis pixel quantises to X = Y = -32768: the tile holding it is gathered under a reflected border, staged under the
    constant one."""
    mx = np.full((16, 64), 10.0, np.float32)
    my = np.full((16, 64), 10.0, np.float32)
    mx[5, 7] = my[5, 7] = np.nan
    x0, y0, bw, bh = border_tiles.tile_boxes(mx, my, 64, 32, border_def.REFLECT_101)["bgr"]
    assert x0[0, 0] == -32768 and bw[0, 0] * bh[0, 0] > border_tiles.BUDGET["bgr"]
    x0, y0, bw, bh = border_tiles.tile_boxes(mx, my, 64, 32, border_def.CONSTANT)["bgr"]
    assert x0[0, 0] == -2 and bw[0, 0] * bh[0, 0] <= border_tiles.BUDGET["bgr"]
