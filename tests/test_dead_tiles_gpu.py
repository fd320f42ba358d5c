"""Tiles wholly outside the source (state 3 of the fused kernels' probe: zeros stored, nothing mapped or sampled) against the oracle, bit
for bit, into canaried planes: both tile shapes of the 8-bit kernel, every mode the rule is enabled for (0, 1, 5), BGR and NV12 out,
the gather path (unaligned source planes) and the byte stores (odd output pitch), the 10-bit kernel with both blends and both outputs.
For every case the CPU model of the rule (dead_tiles.py) must report at least one dead tile and at least one tile cut by the source
edge, so the path is known to have run next to the tiles that must not take it.
(The sources are 256 x 144 and 250 x 142: NV12 has no odd height, 250 is the width that is no multiple of the 8-pixel staging block.)"""
import numpy as np
import pytest

import dead_tiles as D
import layouts
import oracle
import synth
from test_p010_cpu import p010_frame

pytestmark = pytest.mark.gpu

PRESET = oracle.GOPRO_H4B_WIDE169_MEASURED
# eight rotations from none to 30 degrees
ROTATIONS = [(0.0, 0.0, 0.0), (0.02, -0.01, 0.03), (-0.05, 0.04, 0.0), (0.0, 0.12, -0.05), (0.15, 0.0, 0.1), (-0.2, -0.15, 0.05), (0.1, -0.3, -0.2),
             (0.3, 0.3, 0.3)]


def setup(w, h):
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    return K, Ko, cw, ch


def model_ran(p, dw, dh, sw, sh, heights, nan_behind, what):
    """The CPU model: at one of the kernel's tile heights at least one dead tile, and at least one tile cut by the source edge."""
    live = D.live_pixels(p, dw, dh, sw, sh, nan_behind)
    dead = sum(int(D.rule(p, dw, dh, sw, sh, th, nan_behind).sum()) for th in heights)
    cut = sum(int((D.tiles_any(live, th) & D.tiles_any(~live, th)).sum()) for th in heights)
    assert dead >= 1 and cut >= 1, (what, dead, cut)


def expected8(frame, p, dw, dh, mode, nv12):
    if mode == 5:
        bgr = oracle.warp_nv12_ref_gfx950(frame, p, dw, dh)
        return oracle.cvt_bgr_nv12(bgr) if nv12 else bgr
    return oracle.warp_nv12_ex(frame, p, dw, dh, mode, 1 if nv12 else 0)


@pytest.fixture(scope="module")
def small_frames():
    return {(w, h): synth.nv12(70 + w, w, h) for w, h in ((256, 144), (250, 142))}


@pytest.mark.parametrize("mode", [0, 1, 5])
@pytest.mark.parametrize("w,h", [(256, 144), (250, 142)])
def test_small_outputs_64x16_tiles(vs, cuda, small_frames, w, h, mode):
    f = small_frames[(w, h)]
    K, Ko, cw, ch = setup(w, h)
    assert layouts.fused_launch(cw, ch)[0] == 4
    src = layouts.place(f[:h], f[h:], "decoder", cuda)
    for rv in ROTATIONS:
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        model_ran(p, cw, ch, w, h, (16, 8), mode == 1, (w, h, mode, rv))
        exp = expected8(f, p, cw, ch, mode, False)
        got = layouts.warp_nv12(vs, src, p, cw, ch, mode, vs.OUT_BGR8, cuda)
        assert np.array_equal(got, exp), (w, h, mode, rv, int((got != exp).any(axis=2).sum()))
        ey, euv = expected8(f, p, cw, ch, mode, True)
        gy, guv = layouts.warp_nv12(vs, src, p, cw, ch, mode, vs.OUT_NV12, cuda)
        assert np.array_equal(gy, ey) and np.array_equal(guv, euv.reshape(guv.shape)), (w, h, mode, rv, "nv12")


@pytest.mark.parametrize("mode", [0, 5])
def test_gather_path_and_byte_stores(vs, cuda, small_frames, mode):
    """Source planes at 4-byte aligned bases and pitches (nothing is staged: every live pixel is gathered from global memory) and an output
    of odd pitch (byte stores, dst_vec_ok == 0): the dead tiles go through the same store code."""
    w, h = 256, 144
    f = small_frames[(w, h)]
    K, Ko, cw, ch = setup(w, h)
    rv = ROTATIONS[4]
    p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
    pp = np.ascontiguousarray(p, np.float32)
    model_ran(p, cw, ch, w, h, (16, 8), False, ("unaligned", mode))
    exp = expected8(f, p, cw, ch, mode, False)
    src = layouts.place(f[:h], f[h:], "unaligned", cuda)
    got = layouts.warp_nv12(vs, src, p, cw, ch, mode, vs.OUT_BGR8, cuda)
    assert np.array_equal(got, exp), ("unaligned source", mode)
    src = layouts.place(f[:h], f[h:], "packed", cuda)
    o = layouts.Plane(ch, 3 * cw, cuda, pad=49)
    assert o.pitch % 2 == 1
    layouts._call(vs, "vstab_warp_nv12_ex", src.y, src.pitch_y, src.uv, src.pitch_uv, w, h, layouts._f(pp)[1], mode, int(vs.OUT_BGR8), o.ptr, o.pitch,
                  None, 0, cw, ch, vs._stream())
    assert np.array_equal(o.host(shape=(ch, cw, 3)), exp), ("odd pitch_dst", mode)
    ey, euv = expected8(f, p, cw, ch, mode, True)
    oy, ou = layouts.Plane(ch, cw, cuda, pad=49), layouts.Plane((ch + 1) // 2, 2 * ((cw + 1) // 2), cuda, pad=50)
    layouts._call(vs, "vstab_warp_nv12_ex", src.y, src.pitch_y, src.uv, src.pitch_uv, w, h, layouts._f(pp)[1], mode, int(vs.OUT_NV12), oy.ptr, oy.pitch,
                  ou.ptr, ou.pitch, cw, ch, vs._stream())
    assert np.array_equal(oy.host(), ey) and np.array_equal(ou.host(), euv.reshape(ou.rows, ou.rb)), ("odd pitch_dst nv12", mode)


@pytest.fixture(scope="module")
def hd_frame():
    return synth.nv12(77, 1920, 1080)


@pytest.mark.parametrize("rv", [(0.01, -0.02, 0.005), (0.12, 0.2, -0.1)])
def test_64x32_tiles_tall_split_and_tail_meet_dead_tiles(vs, cuda, hd_frame, rv):
    """A stateless 3072 x 1024 output (1,536 tiles of 64 x 32: the smallest that selects that kernel, with its half-height tail) looking
    at a 1920 x 1080 source with 0.9 of the output camera's focal length, so that the boxes of the image centre are over the LDS budget
    (SPLIT: done as two half-height tiles) while the rim is dead."""
    w, h, dw, dh = 1920, 1080, 3072, 1024
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, _ = oracle.get_output_camera(K, w, h)
    Ko = Ko.copy()
    Ko[0, 0], Ko[1, 1] = 0.9 * Ko[0, 0], 0.9 * Ko[1, 1]
    Ko[0, 2], Ko[1, 2] = (dw - 1) / 2, (dh - 1) / 2
    assert layouts.fused_launch(dw, dh) == (8, 40, 0.5)
    p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
    model_ran(p, dw, dh, w, h, (32, 16), False, (dw, dh, rv))
    mx, my, _, _ = D.exact_map(p, np.arange(dw)[None, :], np.arange(dh)[:, None])
    boxes = layouts.tile_boxes(mx, my, w, h, 32, planar=False, block_w=8)
    assert sum(1 for b in boxes.values() if b[4] and b[2] * b[3] > 40 * 256 - 8) >= 20, "no tall tile over the LDS budget"
    s = layouts.tile_schedule(dw, dh, 8, 40, 0.5)
    assert all(sp < hi for sp, hi in zip(s["split_y"], s["band_y"][1:]))       # every band ends in half-height tiles
    r16 = D.rule(p, dw, dh, w, h, 16)
    assert any(r16[sp // 16:hi // 16].any() for sp, hi in zip(s["split_y"], s["band_y"][1:])), "no dead tile in any band's tail"
    src = layouts.place(hd_frame[:h], hd_frame[h:], "packed", cuda)
    for mode in (0, 5):
        exp = expected8(hd_frame, p, dw, dh, mode, False)
        got = layouts.warp_nv12(vs, src, p, dw, dh, mode, vs.OUT_BGR8, cuda)
        assert np.array_equal(got, exp), (rv, mode, int((got != exp).any(axis=2).sum()))


@pytest.mark.parametrize("blend", [0, 1])
def test_10_bit_both_outputs(vs, cuda, blend):
    w, h = 256, 144
    K, Ko, cw, ch = setup(w, h)
    y, uv, _, _ = p010_frame(31, w, h)
    src = layouts.place(y, uv, "packed", cuda)
    for rv in (ROTATIONS[2], ROTATIONS[5], ROTATIONS[7]):   # (each with dead 64 x 32 tiles at this size: model_ran)
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        model_ran(p, cw, ch, w, h, (32, 16), False, ("p010", rv))
        exp = oracle.warp_p010(y, uv, p, cw, ch, None, 0, blend)
        got = layouts.warp_p010(vs, src, p, cw, ch, 0, blend, cuda)
        assert np.array_equal(got, exp), (blend, rv, "bgr16")
        ey, euv = oracle.cvt_bgr10_p010(exp)
        gy, guv = layouts.warp_p010_planes(vs, src, p, cw, ch, 0, blend, cuda)
        assert np.array_equal(gy, ey) and np.array_equal(guv, euv.reshape(guv.shape)), (blend, rv, "p010")


def test_weighted_bands_across_cache_entries(vs, cuda, hd_frame):
    """The 3072 x 1024 output again (several rounds of tiles: the launcher weighs its XCD bands by cost and keeps them in a cache keyed on
    everything but the rotation): a sequence of rotations that computes an entry, reuses it for a rotation one degree away, computes
    another for one four degrees away and returns to the first -- placement must never change a pixel."""
    w, h, dw, dh = 1920, 1080, 3072, 1024
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, _ = oracle.get_output_camera(K, w, h)
    Ko = Ko.copy()
    Ko[0, 2], Ko[1, 2] = (dw - 1) / 2 + 40.0, (dh - 1) / 2 - 25.0
    src = layouts.place(hd_frame[:h], hd_frame[h:], "packed", cuda)
    d = np.deg2rad
    for rv in ((0.0, 0.0, 0.0), (d(1.0), 0.0, 0.0), (d(4.0), d(-2.0), 0.0), (0.0, 0.0, 0.0)):
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        exp = expected8(hd_frame, p, dw, dh, 5, False)
        got = layouts.warp_nv12(vs, src, p, dw, dh, 5, vs.OUT_BGR8, cuda)
        assert np.array_equal(got, exp), (rv, int((got != exp).any(axis=2).sum()))


def test_pipeline_1080p_changing_rotations(vs, cuda):
    """64 frames at 1080p through pull_into, every emitted frame against the oracle's warp of its input under the rotation the pipeline
    chose for it: the dead tiles move with the rotation from frame to frame.  The clip is one rendered frame rolled by a random walk of
    even pixel offsets (cheap to make; the tracker sees a pan and the rotation estimate follows it)."""
    import torch
    w, h, n = 1920, 1080, 65
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    base = synth.shaky_clip(21, K, w, h, 1)[0][0]
    rng = np.random.default_rng(8)
    pos = np.cumsum(2 * rng.integers(-4, 5, (n, 2)), axis=0)
    frames = []
    for dx, dy in pos:
        f = np.empty_like(base)
        f[:h] = np.roll(base[:h], (int(dy), int(dx)), axis=(0, 1))
        f[h:] = np.roll(base[h:], (int(dy) // 2, int(dx)), axis=(0, 1))
        frames.append(f)
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=n, smooth_radius=2, seed=4)
    out = torch.empty((ch, cw, 3), dtype=torch.uint8, device=cuda)
    angles = []
    for i in range(n - 1):
        assert stab.pull_into(out)
        R = stab.warp_rotation(i)
        angles.append(oracle.rotation_angle(R))
        exp = oracle.warp_nv12_ref_gfx950(frames[i + 1], oracle.map_params(K, Ko, R), cw, ch)
        assert np.array_equal(out.cpu().numpy(), exp), i
    assert not stab.pull_into(out)
    assert max(angles) - min(angles) > np.deg2rad(0.1), "the rotation never changed"
