"""CPU model of the tiled warp kernels' source boxes (layouts.tile_boxes: probe_tile restated on the oracle's exact map).  It proves
that the parameter sets of the wide-box GPU tests (test_layouts_gpu.py) reach the tile states they are meant to reach: boxes that
fit the plane-wise kernel's LDS budget while a box row has more than 64 16-byte chunks -- one LDS-DMA instruction stages
floor(64 / chunks) rows, zero for such a box, so before probe_tile's `fits` bounded the chunks per row these tiles read stale LDS --
and boxes over the budget (the split tile).  A margin of a few pixels stands for the device probe's approximate arithmetic."""
import numpy as np
import pytest

import layouts
import oracle

W, H = 1920, 1080


def anamorphic(sx, sy, rvec, dw, dh, w=W, h=H):
    """Output camera squeezing x by sx and stretching y by 1 / sy against the source's focal lengths, principal point half a tile
    right of the centre (a tile column then straddles the optical axis); -> (params, K, Ko)."""
    K = oracle.get_preset_camera(4, w, h)
    Ko = np.array([[K[0, 0] / sx, 0.0, dw / 2 + 32], [0.0, K[1, 1] / sy, dh / 2], [0.0, 0.0, 1.0]])
    return oracle.map_params(K, Ko, oracle.rodrigues(rvec)), K, Ko


# (depth, dw, dh, sx, sy, rotation, least number of wide staged boxes): 10 bits with 64 x 16 tiles (rwb = 4), 8 bits with an output
# large enough for 64 x 32 tiles (rwb = 8); rotations about x put whole tiles above the source (clamped to hb = 8)
WIDE_SETS = [
    (10, 256, 720, 12.0, 0.25, (-0.7, 0.0, 0.0), 1),
    (10, 256, 720, 9.0, 0.25, (0.6, 0.0, 0.0), 20),
    (8, 512, 6144, 16.0, 0.16, (0.6, 0.0, 0.0), 10),
    (8, 512, 6144, 20.0, 0.16, (0.3, 0.0, 0.0), 10),
]


def test_planar_launch_capacity_matches_the_launcher():
    """The LDS capacities named in the launcher's comments: 14314 px (8 bits, 64 x 32), 7498 / 11594 px (10 bits, 64 x 16 / 64 x 32)."""
    assert layouts.planar_launch(512, 6144, 8) == (8, 24, 14314)
    assert layouts.planar_launch(256, 720, 10) == (4, 28, 7498)
    assert layouts.planar_launch(3840, 2160, 10) == (8, 40, 11594)
    assert layouts.planar_launch(256, 720, 8)[0] == 4


@pytest.mark.parametrize("depth,dw,dh,sx,sy,rv,least", WIDE_SETS)
def test_wide_box_parameter_sets_reach_the_wide_staged_state(depth, dw, dh, sx, sy, rv, least):
    p, _, _ = anamorphic(sx, sy, rv, dw, dh)
    mx, my = oracle.create_map_ex(p, dw, dh, 0)
    counts, rwb, cap = layouts.planar_tile_states(mx, my, W, H, depth, margin=4)
    assert rwb == (8 if depth == 8 else 4)
    assert counts["wide"] >= least, counts     # tiles that, without the bound on chunks per row, were staged with rpi = 0
    assert counts["split"] > 0, counts         # and tiles over the LDS budget: the split tile / the gather path


def test_wide_boxes_are_the_rows_over_64_chunks_only():
    """The model's own sanity: a tile straddling the axis of a strongly squeezed camera has a box row of more than 64 chunks, and
    the boxes of the plain preset camera never do."""
    p, _, _ = anamorphic(9.0, 0.25, (0.6, 0.0, 0.0), 256, 720)
    mx, my = oracle.create_map_ex(p, 256, 720, 0)
    boxes = layouts.tile_boxes(mx, my, W, H, 16, True, 8)
    assert max(b[2] for b in boxes.values() if b[4]) > 64 * 8
    K = oracle.get_preset_camera(4, W, H)
    Ko, (dw, dh) = oracle.get_output_camera(K, W, H)
    mx, my = oracle.create_map_ex(oracle.map_params(K, Ko, oracle.rodrigues((0.02, -0.03, 0.01))), dw, dh, 0)
    for depth in (8, 10):
        counts, _, _ = layouts.planar_tile_states(mx, my, W, H, depth)
        assert counts["wide"] == 0 and counts["split"] == 0, (depth, counts)


def test_layout_specs_keep_the_promised_alignment():
    for rb, h in ((640, 540), (1280, 360), (3840, 2160)):
        for name in layouts.LAYOUTS:
            py, pu, how, oy, ou = layouts.layout_spec(name, rb, h)
            assert py >= rb and pu >= rb
            aligned = all(v % 16 == 0 for v in (py, pu, oy, ou))
            assert aligned == (name != "unaligned"), name
            if how == "one":   # the two planes of one buffer never overlap
                assert oy + py * h <= ou or ou + pu * (h // 2) <= oy, name
        assert layouts.layout_spec("uv_wider", rb, h)[1] > layouts.layout_spec("uv_wider", rb, h)[0]
        assert layouts.layout_spec("uv_narrower", rb, h)[1] < layouts.layout_spec("uv_narrower", rb, h)[0]
        py, _, _, _, ou = layouts.layout_spec("decoder", rb, h)
        assert py > rb and ou == py * ((h + 31) // 32 * 32)
