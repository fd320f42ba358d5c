"""The dead-tile rule of the fused warp kernels (tile_dead_rule, vstab_warp_tile.hpp), restated in numpy (dead_tiles.py) and judged against
the exact fp64 map at EVERY pixel: a tile the rule calls dead must not hold one pixel with a tap inside the source -- over the cameras of
test_shapes_gpu.py, random rotations up to 30 degrees, a source width that is no multiple of 8, a 16 x 16 source whose whole image falls
inside one output tile, and rotations that put the wz = 0 line through a tile.  And the rule must not be so cautious that it does
nothing: at the 4K headline shape it has to recognise at least 85 % of the truly dead tiles (the exact count with a margin of 8 source
pixels is 96 %).  The constants are pinned against the kernel source."""
import os
import re

import numpy as np
import pytest

import dead_tiles as D
import oracle
from test_shapes_gpu import SHAPES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-annotator_amd", "csrc")
TILE_HEIGHTS = (8, 16, 32)      # the tall and half-height tiles of the 64 x 16 and the 64 x 32 kernels


def random_rotation(rng, max_deg=30.0):
    v = rng.normal(size=3)
    return oracle.rodrigues(v / np.linalg.norm(v) * np.deg2rad(rng.uniform(0.0, max_deg)))


def check(params, dw, dh, sw, sh, nan_behind=False, what=""):
    """No wrongly dead tile at any tile height.  -> {th: (truly dead, ruled dead, cut)}"""
    live = D.live_pixels(params, dw, dh, sw, sh, nan_behind)
    out = {}
    for th in TILE_HEIGHTS:
        any_live = D.tiles_any(live, th)
        r = D.rule(params, dw, dh, sw, sh, th, nan_behind)
        wrong = int((r & any_live).sum())
        assert wrong == 0, (what, th, wrong, np.argwhere(r & any_live)[:4].tolist())
        out[th] = (int((~any_live).sum()), int(r.sum()), int((any_live & D.tiles_any(~live, th)).sum()))
    return out


def test_stretch_constant_bounds_the_radial_factor():
    r = np.concatenate([np.linspace(1e-6, 10.0, 2_000_001), np.logspace(1, 9, 100_000)])
    h = (1.0 + r) * np.arctan(r) / r
    assert h.max() < D.STRETCH and abs(r[h.argmax()] - 2.7) < 0.1 and h.max() > 1.666


def test_constants_are_the_kernels():
    with open(os.path.join(CSRC, "vstab_warp_tile.hpp")) as f:
        src = re.sub(r"\s+", " ", f.read())
    assert f"constexpr int DEAD_MARGIN = {D.MARGIN};" in src
    assert "constexpr int DEAD_GUARD = 3 * DEAD_MARGIN / 4;" in src and D.GUARD == 3 * D.MARGIN // 4
    assert f"__builtin_fabsf(ax) < {D.BIG:.1f}f" in src
    for line in ("const float lo = -32.0f * (1 + DEAD_MARGIN), hx = 32.0f * (float)(sw + DEAD_MARGIN), hy = 32.0f * (float)(sh + DEAD_MARGIN);",
                 "__builtin_amdgcn_ballot_w64(ax < lo) == all || __builtin_amdgcn_ballot_w64(ax >= hx) == all",
                 "__builtin_amdgcn_ballot_w64(ay < lo) == all || __builtin_amdgcn_ballot_w64(ay >= hy) == all",
                 "__builtin_fabsf(ax - pax) < 32.0f * DEAD_GUARD && __builtin_fabsf(ay - pay) < 32.0f * DEAD_GUARD",
                 "2.0f * DEAD_STRETCH * slope32 * rz <= 32.0f * (DEAD_MARGIN - 1);", f"constexpr float DEAD_STRETCH = {D.STRETCH}f;",
                 "__builtin_fmaxf(ta.p32.ifx32, ta.p32.ify32) * __builtin_fmaxf(rfx, rfy), a.sw, a.sh);"):
        assert line in src, line
    # the perimeter the model samples is probe_tile's
    for line in ("const int l16 = lane & 15, side = (l16 * (TH - 1) + 7) / 15;", "if (lane < 16) px = 4 * l16, py = 0;",
                 "else if (lane < 32) px = 4 * l16 + 3, py = TH - 1;", "else if (lane < 48) px = 0, py = side;", "else px = 63, py = side;"):
        assert line in src, line


@pytest.mark.parametrize("name", list(SHAPES))
def test_no_wrongly_dead_tile_cameras_of_the_shapes(name):
    """Each camera at its own output, random rotations up to 30 degrees (two for the frames up to 4K, one past it), both forms of the
    map behind the camera."""
    w, h, preset = SHAPES[name]
    K = oracle.get_preset_camera(preset, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    rng = np.random.default_rng(list(SHAPES).index(name) + 40)
    for i in range(2 if w * h <= 3840 * 2160 else 1):
        p = oracle.map_params(K, Ko, random_rotation(rng))
        got = check(p, cw, ch, w, h, nan_behind=bool(i), what=(name, i))
        # (a camera whose slope bound fails even at wz = 1 -- the strip, whose output camera comes out with a focal length near zero -- has no dead tiles by the rule)
        gives_up = 2.0 * D.STRETCH * max(p[2], p[3]) * max(1.0 / p[6], 1.0 / p[7]) > D.MARGIN - 1
        assert got[16][1] > 0 or gives_up, (name, i, "no dead tile found at all")


def test_headline_share_of_the_dead_tiles_recognised():
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, 3840, 2160)
    Ko, (cw, ch) = oracle.get_output_camera(K, 3840, 2160)
    assert (cw, ch) == (3524, 1999)
    for rv in ((0.0, 0.0, 0.0), (0.02, 0.015, 0.01), (-0.02, -0.015, -0.01)):
        got = check(oracle.map_params(K, Ko, oracle.rodrigues(rv)), cw, ch, 3840, 2160, what=rv)
        for th in (16, 32):
            truly, ruled, _ = got[th]
            print(f"rotation {rv} tile height {th}: truly dead {truly}, recognised {ruled} ({100.0 * ruled / truly:.1f} %)")
            assert ruled >= 0.85 * truly, (rv, th, truly, ruled)
        assert 2350 <= got[16][0] <= 2450      # a third of the 7,000 half-tiles


@pytest.mark.parametrize("w,h", [(250, 141), (256, 144), (1918, 1080)])
def test_small_sources_and_widths_that_are_no_multiple_of_8(w, h):
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    rng = np.random.default_rng(w)
    for i in range(8):
        check(oracle.map_params(K, Ko, random_rotation(rng)), cw, ch, w, h, nan_behind=bool(i & 1), what=(w, h, i))


def test_source_smaller_than_a_tile_inside_one_tile():
    """A 16 x 16 source seen at the centre of tile (1, 1) of a 192 x 96 output: every perimeter sample of that tile is outside the source,
    on all four sides -- the tile is live and the rule must say so; every other tile is truly dead."""
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, 16, 16)
    Ko = np.eye(3)
    Ko[0, 0] = Ko[1, 1] = K[0, 0] * 0.75
    Ko[0, 2], Ko[1, 2] = 96.0, 48.0
    p = oracle.map_params(K, Ko, np.eye(3))
    live = D.live_pixels(p, 192, 96, 16, 16)
    ys, xs = np.nonzero(live)
    assert len(xs) and xs.min() > 64 and xs.max() < 127 and ys.min() > 32 and ys.max() < 63, (xs.min(), xs.max(), ys.min(), ys.max())
    r = D.rule(p, 192, 96, 16, 16, 32)
    assert not r[1, 1]
    check(p, 192, 96, 16, 16, what="tiny")
    for dx, dy in ((0.0, 0.0), (13.0, -7.0), (-30.0, 14.0)):   # the image moved about inside and across the tile's edges
        Ko[0, 2], Ko[1, 2] = 96.0 + dx, 48.0 + dy
        check(oracle.map_params(K, Ko, np.eye(3)), 192, 96, 16, 16, what=("tiny", dx, dy))


@pytest.mark.parametrize("nan_behind", [False, True])
def test_rays_behind_the_camera_inside_a_tile(nan_behind):
    """Rotations of 60 to 120 degrees about axes near the image plane put the wz = 0 line through the output: tiles on it hold rays with
    wz <= 0 (mapped mirrored by createMap.cl's arithmetic, nowhere by the fish -> rect form) next to rays whose map runs off to infinity."""
    w, h = 640, 360
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    rng = np.random.default_rng(9)
    crossed = 0
    for i in range(12):
        axis = np.array([np.cos(0.5 * i), np.sin(0.5 * i), 0.15 * rng.normal()])
        R = oracle.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(rng.uniform(60.0, 120.0)))
        p = oracle.map_params(K, Ko, R)
        _, _, wz, _ = D.exact_map(p, np.arange(cw)[None, :], np.arange(ch)[:, None])
        crossed += int((wz > 0).any() and (wz <= 0).any())
        check(p, cw, ch, w, h, nan_behind=nan_behind, what=("behind", i))
    assert crossed >= 8
