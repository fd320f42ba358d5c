"""CPU model of the border warp's tile boxes (tests/warp_tiles.py, rules `every` and `clamp`: k_warp_border's box restated on the oracle's
exact map).  It proves that the parameter sets of the GPU tests (test_border_gpu.py) reach every path of the kernel on BGR, luma and chroma: staged tiles, tiles over
the LDS budget, boxes of exactly the budget, tiles wholly outside the source (never read under BORDER_CONSTANT, reflected picture here),
boxes across each of the four edges, and staged boxes of odd and even width."""
import numpy as np
import pytest

import warp_def as wd
import warp_tiles as wt


@pytest.mark.parametrize("name", sorted(wt.TILE_SETS["border"]))
def test_set_reaches_its_committed_states(name):
    got = wt.states_of("border", name)
    for plane, want in wt.TILE_SETS["border"][name][-1].items():
        for state, least in want.items():
            assert got[plane][state] >= least, (name, plane, state, got[plane])


def test_sets_cover_every_path_of_every_plane():
    total = {p: dict.fromkeys(wt.BORDER_STATES, 0) for p in ("bgr", "luma", "chroma")}
    for name in wt.TILE_SETS["border"]:
        for plane, counts in wt.states_of("border", name).items():
            for k in wt.BORDER_STATES:
                total[plane][k] += counts[k]
    for plane, counts in total.items():
        for state in wt.BORDER_STATES:
            assert counts[state] > 0, (plane, state, counts)


def test_constant_border_keeps_boxes_near_the_source():
    """Under BORDER_CONSTANT the kernel clamps X to [-2, w] and Y to [-2, h] before the box: every box lies in [-2, w + 1] x [-2, h + 1], so
    the zoomed-out set's outside tiles stage a few border positions instead of reflected picture."""
    params, sw, sh, dw, dh, mode = wt.set_params("border", "zoomed_out")
    mx, my = wd.maps(params, dw, dh, mode)
    for plane, (x0, y0, bw, bh, _) in wt.tile_boxes(mx, my, sw, sh, "linear", "clamp").items():
        w, h = (sw, sh) if plane != "chroma" else (sw >> 1, sh >> 1)
        assert (x0 >= -2).all() and (x0 + bw <= w + 2).all() and (y0 >= -2).all() and (y0 + bh <= h + 2).all(), plane


def test_axis_pixel_stretches_one_box():
    """Map mode 0's 0/0 axis pixel quantises to X = Y = -32768: the tile holding it is gathered under a reflected border, staged under the
    constant one."""
    mx = np.full((16, 64), 10.0, np.float32)
    my = np.full((16, 64), 10.0, np.float32)
    mx[5, 7] = my[5, 7] = np.nan
    x0, y0, bw, bh, _ = wt.tile_boxes(mx, my, 64, 32, "linear", "every")["bgr"]
    assert x0[0, 0] == -32768 and bw[0, 0] * bh[0, 0] > wt.BUDGET["bgr"]
    x0, y0, bw, bh, _ = wt.tile_boxes(mx, my, 64, 32, "linear", "clamp")["bgr"]
    assert x0[0, 0] == -2 and bw[0, 0] * bh[0, 0] <= wt.BUDGET["bgr"]
