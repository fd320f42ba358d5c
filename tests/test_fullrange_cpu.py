"""Full-range 10-bit content and maximum-contrast tracking, on the CPU (tests/fullrange.py).

1. Reach: the exact count, on the oracle's map, of the decisions each GPU parameter set (fullrange.SETS) hands the 10-bit kernels --
   saturating conversions, dark taps, binary16 accumulators at 1023.5 and above -- is committed as a lower bound; the older synthetic
   content (test_p010_cpu.p010_frame) reaches neither the saturating add, nor dark luma, nor the plane-wise clamp on the same maps.
2. The oracle's 10-bit chains against the independent numpy statements (test_p010_cpu, test_planar_cpu) on full-range frames.
3. The LK sums: the largest magnitudes the older LK inputs reach (pinned), and the maximum-contrast pairs that pass 2^31."""
import numpy as np
import pytest

import fullrange as F
import lk_segments as M
import oracle
import synth
from test_p010_cpu import np_bgr10, np_remap10, p010_frame
from test_planar_cpu import np_warp_planar

# name: lower bounds of (BGR16 saturating conversions, dark taps, fp16 clamps; plane-wise fp16 clamps luma, chroma).  The model is
# exact: these are the counts of the committed content (plane-wise: mode 0 sets only, the modes vstab_warp_p010_planar tiles).
REACH = {
    "m0_640": (82376, 96828, 15034, 3271, 2096),
    "m0_640_rs": (94374, 99083, 15610, 3792, 2256),
    "m1_320": (24730, 34227, 6119, None, None),
    "m1_320_rs": (35454, 41512, 6277, None, None),
    "split_1280": (22519, 25755, 3966, 874, 624),
    "split_roll_1280": (212702, 266820, 39414, 7792, 5731),
    "m2_320": (30579, 34615, 5136, None, None),
    "m3_320": (46096, 32466, 6778, None, None),
    "m4_320": (4623, 4967, 835, None, None),
}


@pytest.mark.parametrize("name", list(F.SETS))
def test_gpu_sets_reach_every_value_range_branch(name):
    y16, uv16, y10, uv10, p, rb, dw, dh, mode = F.set_params(name)
    mx, my = F.set_map(name)
    sat, dark, clamp, clamp_y, clamp_c = REACH[name]
    r = F.reach_bgr(y10, uv10, mx, my)
    assert r["sat"] >= sat > 0 and r["dark"] >= dark > 0 and r["clamp"] >= clamp > 0, r
    if clamp_y is not None:
        q = F.reach_planar(y10, uv10, mx, my)
        assert q["clamp_y"] >= clamp_y > 0 and q["clamp_c"] >= clamp_c > 0, q
    # the older content on the same map (luma ~120..906, chroma ~272..758) reaches neither the saturating add, nor dark luma, nor
    # the plane-wise clamp (its BGR taps do reach 1023: sat10 clips strong blue)
    _, _, oy, ouv = p010_frame(7, y10.shape[1], y10.shape[0])
    r = F.reach_bgr(oy, ouv, mx, my)
    assert r["sat"] == 0 and r["dark"] == 0, r
    assert F.reach_planar(oy, ouv, mx, my) == {"clamp_y": 0, "clamp_c": 0}


def test_extreme_frame_has_every_kind_of_content():
    y16, uv16, y10, uv10 = F.p010_extreme_frame(3, 192, 64)
    assert (y16 >> 6 == y10).all() and (uv16 >> 6 == uv10).all() and (y16 & 63).any()
    assert y10.min() == 0 and y10.max() == 1023 and uv10.min() == 0 and uv10.max() == 1023
    U, V = uv10[:, 0::2], uv10[:, 1::2]
    Ys = y10[0::2, 0::2]   # the luma of one pixel per chroma site
    assert ((Ys >= 950) & (U >= 980)).sum() >= 64
    for u, v in ((0, 0), (0, 1023), (1023, 0), (1023, 1023)):
        hit = (U == u) & (V == v)
        assert any(hit[r:r + 4, c:c + 4].all() for r in range(hit.shape[0] - 3) for c in range(hit.shape[1] - 3)), (u, v)
    for lo, hi in ((0, 63), (1023, 1023), (1021, 1022)):
        hit = (y10 >= lo) & (y10 <= hi)
        assert any(hit[r:r + 8, c:c + 8].all() for r in range(0, 57, 8) for c in range(0, 185, 8)), (lo, hi)


def test_conversion_at_the_extremes_matches_numpy():
    """The oracle's 64-bit conversion on every (luma, U, V) corner and on full-range frames: the numpy statement; blue of luma 1023 on
    U >= 973 and of luma 938 on U = 1023 saturates (the sums that need the 33rd bit)."""
    for seed, (w, h) in ((1, (64, 36)), (2, (130, 66))):
        y, uv, y10, uv10 = F.p010_extreme_frame(seed, w, h, block=8)
        assert np.array_equal(oracle.cvt_p010_bgr10(y, uv), np_bgr10(y10, uv10))
    ys = np.array([0, 1, 63, 64, 65, 938, 939, 940, 1021, 1022, 1023], np.uint16)
    cs = np.array([0, 1, 511, 512, 973, 1022, 1023], np.uint16)
    yy, uu, vv = np.meshgrid(ys, cs, cs, indexing="ij")
    y10 = np.repeat(np.repeat(yy.reshape(-1, 1), 2, 0), 2, 1)
    uv10 = np.stack([uu.reshape(-1), vv.reshape(-1)], 1)
    got = oracle.cvt_p010_bgr10((y10 << 6) | 37, (uv10 << 6) | 21)
    assert np.array_equal(got, np_bgr10(y10, uv10))
    blue = got[0::2, 0, 0].reshape(yy.shape)
    assert (blue[list(ys).index(1023), list(cs).index(973):] == 1023).all() and (blue[list(ys).index(938), list(cs).index(1023)] == 1023).all()
    assert (blue[:list(ys).index(64) + 1] == blue[list(ys).index(64)]).all()   # luma 0 .. 64 is black


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_p010_chain_matches_numpy_on_full_range_frames(seed):
    w, h = 48, 28
    y, uv, y10, uv10 = F.p010_extreme_frame(seed, w, h, block=8)
    K = oracle.get_preset_camera(4, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    p = oracle.map_params(K, Ko, oracle.rodrigues((0.03, -0.02, 0.05)))
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.05, -0.01, 0.02)))[8:]
    bgr = np_bgr10(y10, uv10)
    for rot_bottom, (mx, my) in ((None, oracle.create_map(p, cw, ch)), (rb, oracle.create_map_rs(p, rb, cw, ch))):
        r = F.reach_bgr(y10, uv10, mx, my)
        assert r["sat"] > 0 and r["dark"] > 0 and r["clamp"] > 0, r
        for blend in (0, 1):
            got = oracle.warp_p010(y, uv, p, cw, ch, rot_bottom, 0, blend)
            assert np.array_equal(got, np_remap10(bgr, mx, my, blend)), (rot_bottom is not None, blend)
    for mode in (1, 2, 3, 4):
        mx, my = oracle.create_map_ex(p, 40, 24, mode)
        for blend in (0, 1):
            assert np.array_equal(oracle.warp_p010(y, uv, p, 40, 24, None, mode, blend), np_remap10(bgr, mx, my, blend)), (mode, blend)


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_p010_planar_matches_numpy_on_full_range_frames(seed):
    w, h = 48, 28
    y, uv, y10, uv10 = F.p010_extreme_frame(seed + 10, w, h, block=8)
    K = oracle.get_preset_camera(4, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    p = oracle.map_params(K, Ko, oracle.rodrigues((0.03, -0.02, 0.05)))
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.05, -0.01, 0.02)))[8:]
    for rot_bottom in (None, rb):
        mx, my = oracle.create_map_rs(p, rb, cw, ch) if rot_bottom is not None else oracle.create_map_ex(p, cw, ch, 0)
        q = F.reach_planar(y10, uv10, mx, my)
        assert q["clamp_y"] > 0 and q["clamp_c"] > 0, q
        for blend in (0, 1):
            gy, guv = oracle.warp_p010_planar(y, uv, p, cw, ch, 0, rot_bottom, blend)
            ey, euv = np_warp_planar(y, uv, mx, my, 10, blend)
            assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (rot_bottom is not None, blend)


def test_stretched_clip_spans_the_range_and_keeps_its_corners():
    W, H = 640, 360
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = F.stretched_clip(3, K, W, H, 3)
    f = frames[1] >> 6
    assert f[:H].min() == 0 and f[:H].max() == 1023 and f[H:].min() == 0 and f[H:].max() == 1023
    mx, my = oracle.create_map_ex(oracle.map_params(K, oracle.get_output_camera(K, W, H)[0], np.eye(3)), 583, 331, 0)
    r = F.reach_bgr(f[:H], f[H:], mx, my)
    assert r["sat"] > 0 and r["dark"] > 0 and r["clamp"] > 0, r
    assert len(oracle.good_features((frames[0][:H] >> 8).astype(np.uint8))) >= 60


# ---- LK sums ---------------------------------------------------------------------------------------------------------------------
def _old_lk_inputs():
    """The frame pairs and points of the older LK tests (test_track_gpu, test_lk_segments_gpu's first pairs)."""
    from test_oracle_cpu import LK_EDGE_SEEDS
    for w, h, shift in ((640, 360, (3.3, -1.2)), (1920, 1080, (-7.6, 4.1)), (200, 120, (0.4, 0.7))):
        g0 = synth.luma(31, w, h)
        yield g0, synth.shifted(g0, *shift), oracle.good_features(g0, 200, 0.01, 15.0)
    g0 = synth.luma(41, 3840, 2160, rects=400)
    yield g0, synth.shifted(g0, 2.6, -1.9), oracle.good_features(g0)
    for seed in LK_EDGE_SEEDS:
        yield synth.edge_leaving_pair(seed)
    for name in M.SETS:
        frames, pts, _ = M.make_set(name)
        yield frames[0], frames[1], pts


# (w, h, seed, shift) of the maximum-contrast pairs (test_fullrange_gpu.py)
CONTRAST_PAIRS = [(160, 120, 1, (0.37, -0.61)), (97, 71, 2, (-1.3, 0.8))]


def test_lk_sums_of_the_older_inputs_stay_below_2_31():
    """The measurement the int32 arguments of k_lk_track lacked: the older LK inputs reach 0.29 x 2^31 (|sum Iy^2|, the 4K pair) and
    0.11 x 2^31 (|sum diff Ix|) -- summing the wave totals in plain int32 would pass them all."""
    m = np.max([oracle.pyr_lk_sums(*args)[2].max(0) for args in _old_lk_inputs()], 0)
    assert (m == [546892200, 42422394, 617069700, 234067812, 188043104]).all(), m.tolist()
    assert m.max() < 2 ** 30


def test_lk_sums_of_the_contrast_pairs_pass_2_31():
    """0 / 255 checkerboards of 2 - 4 px cells and hard steps: |sum Ix^2|, |sum Iy^2| pass 2^31 for tracked features, and so do
    |sum diff Ix|, |sum diff Iy| (3 and 4 px cells); the 1 px checkerboard has no Scharr gradient at all (no corners, nothing tracked)."""
    over = {}
    for kind in F.CONTRAST:
        for w, h, seed, shift in CONTRAST_PAIRS:
            prev, nxt, pts = F.contrast_pair(kind, w, h, seed, shift)
            _, st, s = oracle.pyr_lk_sums(prev, nxt, pts)
            o = over.setdefault(kind, np.zeros(5, int))
            o += ((s >= 2 ** 31) & (st[:, None] > 0)).sum(0)
            if kind == "checker1":
                assert (s == 0).all() and (st == 0).all()
    assert (over["checker4"] >= [25, 0, 37, 4, 4]).all() and (over["checker3"] >= [17, 0, 17, 2, 4]).all(), over
    assert (over["steps"] >= [16, 0, 28, 0, 0]).all() and (over["checker2"] >= [2, 0, 2, 0, 0]).all(), over
