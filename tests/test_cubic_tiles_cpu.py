"""CPU model of the cubic warp's tile boxes (tests/warp_tiles.py, rule `touching`: k_warp_cubic's box restated on the oracle's exact map).  It proves
that the parameter sets of the GPU tests (test_cubic_paths_gpu.py) reach every path of the kernel: luma / chroma / BGR tiles with no
box, staged in LDS and gathered from global memory, boxes of exactly the LDS budget and just over it, partial tiles that stage, and
staged boxes of odd and even width.  The model is exact (no margin): the counts below are what the kernel does, tile for tile."""
import numpy as np
import pytest

import oracle
import warp_def as wd
import warp_tiles as wt


TILE_SETS = wt.TILE_SETS["cubic"]


def states(name):
    return wt.states_of("cubic", name)


def states_of(params, dw, dh, sw, sh, mode):
    return wt.tile_states(*wd.maps(params, dw, dh, mode), sw, sh, "cubic", "touching")


@pytest.mark.parametrize("name", sorted(TILE_SETS))
def test_tile_set_reaches_its_states(name):
    s = states(name)
    for plane, want in TILE_SETS[name][8].items():
        for k, v in want.items():
            assert s[plane][k] == v, (name, plane, k, s[plane])


def test_tile_sets_reach_every_state_between_them():
    """(a) .. (g) of the table's legend, recomputed from the model rather than read from the table."""
    S = {n: states(n) for n in TILE_SETS}
    sets = TILE_SETS.values()
    assert any(s["bgr"]["gathered"] for s in S.values())                                                       # (a)
    assert any(s["luma"]["gathered"] and s["chroma"]["staged"] and not s["chroma"]["gathered"] for s in S.values())   # (b)
    assert any(s["luma"]["gathered"] and s["chroma"]["gathered"] for s in S.values())                         # (c)
    for plane in ("bgr", "luma", "chroma"):                                                                    # (d)
        assert any(s[plane]["at_budget"] for s in S.values()), plane
    assert any(s["bgr"]["over_by_one"] for s in S.values()) and any(s["chroma"]["over_by_one"] for s in S.values())
    assert any(s["luma"]["least_over"] == 2 for s in S.values())
    for plane in ("bgr", "luma", "chroma"):                                                                    # (e)
        assert any(s[plane]["none"] and s[plane]["staged"] and s[plane]["gathered"] for s in S.values()), plane
    assert any(s["luma"]["partial_staged"] and s["chroma"]["partial_staged"] and dw % 2 and dh % 2       # (f)
               for s, (_, _, dw, dh, *_) in zip(S.values(), sets))
    for plane in ("luma", "chroma"):                                                                           # (g)
        assert any(s[plane]["odd_w"] for s in S.values()) and any(s[plane]["even_w"] for s in S.values()), plane


def test_preset_camera_of_the_4_gib_frame_stages_every_tile():
    """The staged set of the 4 GiB tests: the preset camera on their 640 x 540 frame gathers no tile."""
    K = oracle.get_preset_camera(4, 640, 540)
    Ko, (dw, dh) = oracle.get_output_camera(K, 640, 540)
    s = states_of(oracle.map_params(K, Ko, oracle.rodrigues((0.02, -0.03, 0.01))), dw, dh, 640, 540, 0)
    assert all(s[p]["gathered"] == 0 and s[p]["staged"] > 0 for p in s), s


def test_luma_budget_plus_one_has_no_box():
    """12289 elements: prime, so only a 1-wide or 1-tall box could have it; every box is at least 4 x 4."""
    n = wt.BUDGET["luma"] + 1
    assert all(n % d for d in range(2, int(n ** 0.5) + 1))


def test_model_counts_of_the_existing_gpu_tests():
    """What test_cubic_gpu.py's warps reach: the RECT -> FISH 300 degree pair of test_warp_cubic_every_projection_pair is the one
    existing test whose plane-wise tiles gather (luma for every rotation, chroma for one); the extreme box shapes gather BGR tiles
    only (the docstring of test_warp_cubic_extreme_box_shapes)."""
    w, h, dw, dh = 640, 360, 481, 271
    Kin, Kout = oracle.lens_camera(oracle.PROJ_RECT, 100.0, w, h), oracle.lens_camera(oracle.PROJ_FISH, 300.0, dw, dh)
    mode = oracle.map_mode(oracle.PROJ_RECT, oracle.PROJ_FISH)
    got = []
    for rv in [(0.02, -0.03, 0.01), (-0.15, 0.1, 0.3), (0.0, 1.2, 0.0)]:
        s = states_of(oracle.map_params(Kin, Kout, oracle.rodrigues(rv)), dw, dh, w, h, mode)
        got.append((s["luma"]["gathered"], s["chroma"]["gathered"]))
    assert got == [(11, 0), (18, 6), (11, 0)], got
    for sw, sh, dw, dh, sx, sy, bgr_gathers in [(2048, 32, 128, 64, 15.0, 0.25, 8), (64, 1024, 128, 64, 0.125, 15.0, 0),
                                                 (4096, 64, 200, 70, 15.5, 0.3, 12)]:
        Ki = np.array([[100.0 * sx, 0, sw / 2], [0, 100.0 * sy, sh / 2], [0, 0, 1]])
        Ko = np.array([[100.0, 0, dw / 2], [0, 100.0, dh / 2], [0, 0, 1]])
        for rot in [(0.0, 0.0, 0.0), (0.0, 0.0, 0.002)]:
            s = states_of(oracle.map_params(Ki, Ko, oracle.rodrigues(rot)), dw, dh, sw, sh, oracle.MAP_RECT_TO_RECT)
            assert s["bgr"]["gathered"] == bgr_gathers and s["luma"]["gathered"] == 0 and s["chroma"]["gathered"] == 0, (sw, sh, rot, s)


def test_model_box_is_the_footprint_extremes():
    """The model's own sanity on a hand-made map: one tile, every pixel at X = 10.5 except one at (40.25, 7.0) -> box columns
    9 .. 42, rows 6 .. 9 (luma); a pixel right of a 70-wide output's last column never counts; chroma only from even rows / columns."""
    mx = np.full((16, 70), 10.5, np.float32)
    my = np.full((16, 70), 7.0, np.float32)
    mx[5, 3], my[5, 3] = 40.25, 7.0          # odd column: luma only
    x0, y0, bw, bh, have = (a[0, 0] for a in wt.tile_boxes(mx, my, 100, 100, "cubic", "touching")["luma"])
    assert have and (x0, y0, bw, bh) == (9, 6, 34, 4)
    x0, y0, bw, bh, have = (a[0, 0] for a in wt.tile_boxes(mx, my, 100, 100, "cubic", "touching")["chroma"])
    assert have and (x0, y0, bw, bh) == (4, 2, 4, 4)    # 0.5 * (10.5, 7.0) -> (5, 3) after quantisation, X - 1 .. X + 2
    mx[:, 64:] = 1e6                         # the second tile column holds x = 64 .. 69: all outside
    s = wt.tile_states(mx, my, 100, 100, "cubic", "touching")
    assert s["luma"]["none"] == 1 and s["luma"]["staged"] == 1 and s["luma"]["partial_staged"] == 0
