"""GPU parity of the border modes (cv::remap borderMode; include/vstab.h "Border modes") through the C ABI and the pipeline object:
vstab_remap_bilinear_border, vstab_warp_nv12_border (BGR8 and plane-wise NV12, with and without a rotation per output row) and
vstab_set_border_mode.  Bar: every byte equals the numpy definition (tests/warp_def.py) fed by the oracle's maps -- the reference kernel's own
map, run on this GPU, for VSTAB_MAP_CREATEMAP_CL_OPENCL -- and every output plane is guarded by canary bytes (tests/layouts.py).  Under
BORDER_CONSTANT the new entry points give the bytes of the pinned ones (vstab_warp_nv12_ex / _rs, vstab_remap_bilinear)."""
import ctypes

import numpy as np
import pytest

import expect
import layouts
import oracle
import synth
import warp_def as wd
import warp_tiles as wt
from test_layouts_gpu import PITCH_UV_4G

pytestmark = pytest.mark.gpu

MODES = wd.MODES
ROT = (0.02, -0.03, 0.01)
PAST = (0.35, -0.25, 0.2)   # looks past the source: wide border areas, tiles wholly outside


def cams(w, h, rvec=ROT, preset=4):
    K = oracle.get_preset_camera(preset, w, h)
    Ko, (dw, dh) = oracle.get_output_camera(K, w, h)
    return oracle.map_params(K, Ko, oracle.rodrigues(rvec)), dw, dh, K, Ko


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp).reshape(np.asarray(got).shape)
    assert np.array_equal(got, exp), (what, int((got != exp).sum()))


def map_modes():
    """Map modes 0..4, and 5 (the reference kernel's map, run on this GPU) where its code object is built."""
    return list(range(5)) + ([5] if oracle.ref_gfx950_available() else [])


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- the C ABI with separate, canaried planes ---------------------------------------------------------------------------------------
def warp_border(vs, s, params, dw, dh, mode, out_format, border_mode, cuda, rot_bottom=None, out=None):
    """vstab_warp_nv12_border on layouts.Src s -> BGR (dh, dw, 3), or (y, uv) plane-wise NV12, read back after the canary check."""
    p, pp = layouts._f(params)
    rb, rbp = layouts._f(np.asarray(rot_bottom).reshape(9)) if rot_bottom is not None else (None, None)
    if out_format == vs.OUT_BGR8:
        o = out or layouts.Plane(dh, 3 * dw, cuda)
        layouts._call(vs, "vstab_warp_nv12_border", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, rbp, int(mode), int(out_format), int(border_mode),
                      o.ptr, o.pitch, None, 0, dw, dh, vs._stream())
        return o.host(shape=(dh, dw, 3))
    oy, ou = out or layouts.out_nv12(dw, dh, cuda)
    layouts._call(vs, "vstab_warp_nv12_border", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, rbp, int(mode), int(out_format), int(border_mode),
                  oy.ptr, oy.pitch, ou.ptr, ou.pitch, dw, dh, vs._stream())
    return oy.host(), ou.host()


def remap_border(vs, cuda, src, mx, my, border_mode):
    """vstab_remap_bilinear_border into a canaried Plane -> (dh, dw[, cn]) uint8."""
    s = dev(src, cuda)
    cn = 1 if src.ndim == 2 else src.shape[2]
    dh, dw = mx.shape
    mxt, myt = dev(mx, cuda), dev(my, cuda)
    o = layouts.Plane(dh, dw * cn, cuda)
    layouts._call(vs, "vstab_remap_bilinear_border", s.data_ptr(), s.stride(0), src.shape[1], src.shape[0], cn, mxt.data_ptr(), mxt.stride(0) * 4,
                  myt.data_ptr(), myt.stride(0) * 4, int(border_mode), o.ptr, o.pitch, dw, dh, vs._stream())
    return o.host(shape=(dh, dw, cn) if cn > 1 else (dh, dw))


def check_warp(vs, cuda, s, f, p, dw, dh, mode, border_mode, what, rot_bottom=None, outs=None):
    """BGR and plane-wise border warps of Src s (packed NV12 f on the host) against the definition."""
    ob, op = outs if outs else (None, None)
    eq(warp_border(vs, s, p, dw, dh, mode, vs.OUT_BGR8, border_mode, cuda, rot_bottom, ob),
       wd.bgr(f, *wd.maps(p, dw, dh, mode, rot_bottom), "linear", border_mode), (what, "bgr", mode, border_mode))
    gy, guv = warp_border(vs, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, border_mode, cuda, rot_bottom, op)
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, mode, rot_bottom), "linear", border_mode)
    eq(gy, ey, (what, "luma", mode, border_mode)), eq(guv, euv, (what, "chroma", mode, border_mode))


# ---- the stateless remap ------------------------------------------------------------------------------------------------------------
def test_remap_border_golden_vectors(vs, cuda):
    import test_border_cpu
    n = 0
    for k, src, mx, my, mode, out in test_border_cpu.golden_cases():
        eq(remap_border(vs, cuda, src, mx, my, mode), out, k)
        n += 1
    assert n >= 27


def test_remap_border_random_maps_every_channel_count(vs, cuda):
    rng = np.random.default_rng(11)
    for sw, sh in ((1, 1), (2, 3), (3, 2), (37, 21), (300, 170)):
        for cn in (1, 2, 3):
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            dw, dh = (71, 33) if sw < 100 else (333, 190)
            mx = rng.uniform(-3.0 * sw - 5, 4.0 * sw + 5, (dh, dw)).astype(np.float32)
            my = rng.uniform(-3.0 * sh - 5, 4.0 * sh + 5, (dh, dw)).astype(np.float32)
            special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 32768.0, -32768.0, -0.0], np.float32)
            for m in (mx, my):
                pick = rng.random((dh, dw)) < 0.05
                m[pick] = rng.choice(special, int(pick.sum()))
            for mode in MODES:
                eq(remap_border(vs, cuda, src, mx, my, mode), wd.remap(src, mx, my, "linear", mode), (sw, sh, cn, mode))


@pytest.mark.parametrize("sw", [1, 2, 3, 5, 1920, 32767])
def test_remap_border_sweeps_every_position(vs, cuda, sw):
    """X over all of [-32768, 32767] (four rows of 16384), fx = 13 / 32 and a fixed row: every position borderInterpolate can see."""
    rng = np.random.default_rng(sw)
    sh = 3
    src = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    X = np.arange(-32768, 32768, dtype=np.int64).reshape(4, 16384)
    mx = ((X * 32 + 13) / 32.0).astype(np.float32)
    my = np.full(mx.shape, 1.25, np.float32)
    fx = 13
    for mode in MODES:
        x0, x1 = wd.border_interpolate(X, sw, mode), wd.border_interpolate(X + 1, sw, mode)
        row = src[1].astype(np.int64)   # my = 1.25: taps on rows 1 and 2, fy = 8
        row2 = src[2].astype(np.int64)
        acc = 512 + (32 - fx) * 24 * row[x0] + fx * 24 * row[x1] + (32 - fx) * 8 * row2[x0] + fx * 8 * row2[x1]
        exp = (acc >> 10).astype(np.uint8)
        eq(remap_border(vs, cuda, src, mx, my, mode), exp, (sw, mode))


def test_remap_border_constant_equals_remap_bilinear(vs, cuda):
    rng = np.random.default_rng(12)
    for cn in (1, 3):
        src = rng.integers(0, 256, (41, 57, cn) if cn > 1 else (41, 57), dtype=np.uint8)
        mx = rng.uniform(-70, 130, (45, 77)).astype(np.float32)
        my = rng.uniform(-50, 90, (45, 77)).astype(np.float32)
        mx[0, :5] = [np.nan, np.inf, -1e30, 32768.0, -32768.0]
        ref = vs.remap_bilinear(dev(src, cuda), dev(mx, cuda), dev(my, cuda)).cpu().numpy()
        eq(remap_border(vs, cuda, src, mx, my, vs.BORDER_CONSTANT), ref, cn)
        eq(vs.remap_bilinear_border(dev(src, cuda), dev(mx, cuda), dev(my, cuda), vs.BORDER_CONSTANT).cpu().numpy(), ref, ("binding", cn))


# ---- the warp: every map mode, both formats, every border mode, with and without a rotation per row -------------------------------
@pytest.mark.parametrize("rv", [ROT, PAST])
def test_warp_border_every_map_mode(vs, cuda, rv):
    w, h = 320, 180
    f = synth.nv12(31, w, h, full_range=True)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    p, dw, dh, K, Ko = cams(w, h, rv)
    for mode in map_modes():
        for bm in MODES:
            check_warp(vs, cuda, s, f, p, dw - 3, dh - 1, mode, bm, ("modes", rv))


def test_warp_border_rotation_per_row(vs, cuda):
    w, h = 320, 180
    f = synth.nv12(32, w, h)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    p, dw, dh, K, Ko = cams(w, h, PAST)
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.38, -0.2, 0.26)))[8:]
    for mode in [m for m in map_modes() if m in (0, 1, 5)]:
        for bm in MODES:
            check_warp(vs, cuda, s, f, p, dw, dh, mode, bm, "rs", rot_bottom=rb)
    for mode in (2, 3, 4):
        with pytest.raises(vs.VstabError):
            warp_border(vs, s, p, dw, dh, mode, vs.OUT_BGR8, vs.BORDER_REFLECT_101, cuda, rb)


def test_warp_border_constant_equals_pinned_warps(vs, cuda):
    """BORDER_CONSTANT through vstab_warp_nv12_border gives the bytes of vstab_warp_nv12_ex (every map mode, both formats) and
    vstab_warp_nv12_rs (modes 0, 1, 5): the new kernel tied to the pinned ones."""
    w, h = 320, 180
    f = synth.nv12(33, w, h, full_range=True)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    for rv in (ROT, PAST):
        p, dw, dh, K, Ko = cams(w, h, rv)
        rb = oracle.map_params(K, Ko, oracle.rodrigues((rv[0] + 0.02, rv[1], rv[2] + 0.03)))[8:]
        for mode in range(6):
            for fmt in (vs.OUT_BGR8, vs.OUT_NV12_PLANAR):
                for r in ((None, rb) if mode in (0, 1, 5) else (None,)):
                    got = warp_border(vs, s, p, dw, dh, mode, fmt, vs.BORDER_CONSTANT, cuda, r)
                    ref = layouts.warp_nv12(vs, s, p, dw, dh, mode, fmt, cuda, r)
                    if fmt == vs.OUT_BGR8:
                        eq(got, ref, (rv, mode, r is None))
                    else:
                        eq(got[0], ref[0], (rv, mode, "y", r is None)), eq(got[1], ref[1], (rv, mode, "uv", r is None))


def test_warp_border_binding(vs, cuda):
    w, h = 128, 72
    f = synth.nv12(34, w, h)
    p, dw, dh, K, Ko = cams(w, h, PAST)
    got = vs.warp_nv12_border(dev(f, cuda), p, dw, dh, 0, vs.OUT_BGR8, vs.BORDER_REPLICATE).cpu().numpy()
    eq(got, wd.bgr(f, *wd.maps(p, dw, dh, 0), "linear", vs.BORDER_REPLICATE), "binding bgr")
    y, uv = vs.warp_nv12_border(dev(f, cuda), p, dw, dh, 1, vs.OUT_NV12_PLANAR, vs.BORDER_REFLECT, rot_bottom=p[8:])
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, 1, p[8:]), "linear", vs.BORDER_REFLECT)
    eq(y.cpu().numpy(), ey, "binding y"), eq(uv.cpu().numpy(), euv, "binding uv")


# ---- tile and layout paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wt.TILE_SETS["border"]))
def test_border_tile_sets(vs, cuda, name):
    """The sets of tests/warp_tiles.py for k_warp_border: staged, gathered, exactly-the-budget, wholly-outside and edge-crossing tiles on every
    plane."""
    p, sw, sh, dw, dh, mode = wt.set_params("border", name)
    f = synth.nv12(sum(map(ord, name)), sw, sh, full_range=True)
    s = layouts.place(f[:sh], f[sh:], "packed", cuda)
    for bm in MODES:
        check_warp(vs, cuda, s, f, p, dw, dh, mode, bm, name)
    got = warp_border(vs, s, p, dw, dh, mode, vs.OUT_BGR8, vs.BORDER_CONSTANT, cuda)
    eq(got, layouts.warp_nv12(vs, s, p, dw, dh, mode, vs.OUT_BGR8, cuda), (name, "constant"))


def test_border_axis_pixel_tile_gathers(vs, cuda):
    """Map mode 0 with the identity rotation and the principal point on a pixel: that pixel's 0/0 quantises to X = Y = -32768, which
    stretches its tile's box over the budget (the gather path); under a reflected border it is interpolated like any position."""
    w, h = 256, 144
    f = synth.nv12(35, w, h)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    K = oracle.get_preset_camera(4, w, h)
    Ko = np.array([[100.0, 0, 64.0], [0, 100.0, 40.0], [0, 0, 1]])
    p = oracle.map_params(K, Ko, np.eye(3))
    mx, my = oracle.create_map_ex(p, 130, 70, 0)
    assert np.isnan(mx[40, 64]), "the axis pixel must be 0/0 in map mode 0"
    for bm in MODES:
        check_warp(vs, cuda, s, f, p, 130, 70, 0, bm, "axis")


@pytest.mark.parametrize("name", layouts.LAYOUTS)
def test_border_every_layout(vs, cuda, name):
    w, h = 640, 360
    p, dw, dh, _, _ = cams(w, h, PAST)
    f = synth.nv12(36, w, h)
    s = layouts.place(f[:h], f[h:], name, cuda)
    for bm in (vs.BORDER_REFLECT_101, vs.BORDER_REPLICATE):
        check_warp(vs, cuda, s, f, p, dw, dh, 0, bm, name)


def test_border_odd_luma_address_and_pitch(vs, cuda):
    """Luma at an odd address with an odd pitch (bytes are read one at a time), chroma 2-byte aligned with a pitch of its own."""
    w, h = 320, 180
    p, dw, dh, _, _ = cams(w, h, PAST)
    f = synth.nv12(37, w, h)
    s = layouts.place(f[:h], f[h:], None, cuda, spec=(w + 3, w + 6, "two", 1, 2))
    assert s.y % 2 == 1 and s.pitch_y % 2 == 1 and s.uv % 2 == 0
    for bm in MODES:
        check_warp(vs, cuda, s, f, p, dw, dh, 0, bm, "odd")


def test_border_chroma_plane_past_4_gib(vs, cuda):
    """A 640 x 540 frame whose chroma rows from 257 on start past 2^32 bytes (one 4.5 GB allocation): chroma differs row by row."""
    import torch
    w, h = 640, 540
    f = synth.nv12(17, w, h)
    rows = np.arange(h // 2, dtype=np.uint16)[:, None]
    f[h:] = ((f[h:].astype(np.uint16) + 37 * rows) % 256).astype(np.uint8)
    assert PITCH_UV_4G * (h // 2 - 1) >= 1 << 32
    p, dw, dh, K, Ko = cams(w, h, PAST)
    s = layouts.place(f[:h], f[h:], None, cuda, spec=(w, PITCH_UV_4G, "one", 0, w * h))
    try:
        check_warp(vs, cuda, s, f, p, dw, dh, 0, vs.BORDER_REFLECT_101, "chroma 4g")
        check_warp(vs, cuda, s, f, p, dw, dh, 1, vs.BORDER_REPLICATE, "chroma 4g", rot_bottom=p[8:])
    finally:
        del s
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", [0, 5])
def test_border_4k_config3_shape(vs, cuda, mode):
    if mode == 5 and not oracle.ref_gfx950_available():
        pytest.skip("oracle/_ref/createMap.gfx950.co not built")
    w, h = 3840, 2160
    f = synth.nv12(77, w, h)
    p, dw, dh, _, _ = cams(w, h, (0.01, -0.02, 0.015))
    assert (dw, dh) == (3524, 1999)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    check_warp(vs, cuda, s, f, p, dw, dh, mode, vs.BORDER_REFLECT_101, "4k")


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
W, H = 640, 360


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = synth.shaky_clip(5, K, W, H, 10, sigma=0.02)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    return K, Ko, cw, ch, frames


def pulls(vs, cuda, frames, how, border_mode=None, **cfg):
    """A Stabilizer over device frames, pulled to the end with `how` ('pull', 'frames', 'host', 'peek', 'planar') -> (stabilizer, outputs)."""
    import torch
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), border_mode=border_mode, **cfg)
    cw, ch = stab.out_size
    outs = []
    if how == "frames":
        ring = [torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda) for _ in range(3)]
        while True:
            n = stab.pull_frames_into(ring, len(outs), 3)
            outs += [ring[(len(outs) + i) % 3].cpu().numpy() for i in range(n)]
            if n < 3:
                break
        return stab, outs
    while True:
        if how == "peek":
            o = layouts.Plane(ch, 3 * cw, cuda)
            st = vs.lib.vstab_peek_frame(stab._h, o.ptr, o.pitch)
            if st == vs.EOF:
                break
            assert st == vs.OK, vs.lib.vstab_last_error()
            outs.append(o.host(shape=(ch, cw, 3)))
            continue
        o = {"pull": stab.pull, "host": stab.pull_host, "planar": lambda: stab.pull_nv12(planar=True)}[how]()
        if o is None:
            break
        outs.append(tuple(x.cpu().numpy() for x in o) if how == "planar" else o if how == "host" else o.cpu().numpy())
    return stab, outs


def expect_frame(vs, f, K, Ko, R, cw, ch, out, how, map_mode=0, border_mode=wd.REFLECT_101, rot_bottom=None, what=None):
    p = oracle.map_params(K, Ko, R)
    if how == "planar":
        ey, euv = wd.planar(f, *wd.maps(p, cw, ch, map_mode, rot_bottom), "linear", border_mode)
        eq(out[0], ey, (what, "y")), eq(out[1], euv, (what, "uv"))
    else:
        eq(out, wd.bgr(f, *wd.maps(p, cw, ch, map_mode, rot_bottom), "linear", border_mode), what)


@pytest.mark.parametrize("tracking", [1, 0])
@pytest.mark.parametrize("how", ["pull", "frames", "host", "peek", "planar"])
def test_pipeline_border_pulls(vs, cuda, clip, how, tracking):
    """A REFLECT_101 handle: each pull is the border warp of its frame under the handle's own rotation.  Tracking off repeats the
    parameters frame after frame -- where a constant-border handle would serve its BGR pulls from the cached quantised map."""
    K, Ko, cw, ch, frames = clip
    stab, outs = pulls(vs, cuda, frames, how, vs.BORDER_REFLECT_101, smooth_radius=2, tracking=tracking, map_precision=expect.IEEE)
    assert len(outs) == len(frames) - 1
    for i, o in enumerate(outs):
        expect_frame(vs, frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, o, how, what=(how, tracking, i))
    if tracking == 0 and how == "pull":   # the constant border's cached map would have given black edges
        p = oracle.map_params(K, Ko, stab.warp_rotation(len(outs) - 1))
        assert not np.array_equal(outs[-1], expect.warp(frames[len(outs)], p, cw, ch, expect.IEEE))
    stab.close()


def test_pipeline_border_default_precision(vs, cuda, clip):
    """The handle's default map arithmetic (the reference kernel's, map mode 5)."""
    if not oracle.ref_gfx950_available():
        pytest.skip("oracle/_ref/createMap.gfx950.co not built")
    K, Ko, cw, ch, frames = clip
    for how in ("pull", "planar"):
        stab, outs = pulls(vs, cuda, frames[:6], how, vs.BORDER_REFLECT_101, smooth_radius=2)
        for i, o in enumerate(outs):
            expect_frame(vs, frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, o, how, map_mode=5, what=(how, i))
        stab.close()


def test_pipeline_border_lens_mode(vs, cuda, clip):
    """lens_mode 1, fisheye -> fisheye (map mode 2)."""
    K, Ko, cw, ch, frames = clip
    cfg = dict(lens_mode=1, in_projection=1, out_projection=1, in_dfov=150.0, out_dfov=120.0, out_width=480, out_height=270, smooth_radius=2)
    Kout = oracle.lens_camera(oracle.PROJ_FISH, 120.0, 480, 270)
    for how in ("pull", "planar"):
        stab, outs = pulls(vs, cuda, frames[:8], how, vs.BORDER_REFLECT_101, **cfg)
        for i, o in enumerate(outs):
            p = oracle.map_params(stab.K_in, Kout, stab.warp_rotation(i))
            if how == "planar":
                ey, euv = wd.planar(frames[i + 1], *wd.maps(p, 480, 270, oracle.MAP_FISH_TO_FISH), "linear", wd.REFLECT_101)
                eq(o[0], ey, ("lens y", i)), eq(o[1], euv, ("lens uv", i))
            else:
                eq(o, wd.bgr(frames[i + 1], *wd.maps(p, 480, 270, oracle.MAP_FISH_TO_FISH), "linear", wd.REFLECT_101), ("lens", i))
        stab.close()


def test_pipeline_border_readout_rotations(vs, cuda, clip):
    """Frames with read-out rotations (map mode 0): the border warp takes the rotation of the last output row, readout * W."""
    import torch
    K, Ko, cw, ch, frames = clip
    ro = [oracle.rodrigues((0.002 * (k % 3), -0.003, 0.001 * k)) for k in range(6)]
    for how in ("pull", "planar"):
        stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames[:6]], total=6, smooth_radius=1, tracking=0, readouts=ro,
                             map_precision=expect.IEEE, border_mode=vs.BORDER_REFLECT_101)
        for i in range(5):
            o = stab.pull() if how == "pull" else stab.pull_nv12(planar=True)
            o = o.cpu().numpy() if how == "pull" else tuple(x.cpu().numpy() for x in o)
            W_rot = stab.warp_rotation(i)
            rb = oracle.map_params(K, Ko, ro[i + 1] @ W_rot)[8:]
            expect_frame(vs, frames[i + 1], K, Ko, W_rot, cw, ch, o, how, rot_bottom=rb, what=("readout", how, i))
        stab.close()


def test_pipeline_border_switches_mid_stream(vs, cuda, clip):
    """CONSTANT <-> REFLECT_101 between pulls: each frame is warped with the mode in force when it is pulled.  Tracking off, so the
    constant frames come from the cached map from the second one on, and the reflected ones must not."""
    K, Ko, cw, ch, frames = clip
    seq = [0, 0, 4, 4, 0, 4, 1, 0, 2]
    import torch
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), smooth_radius=2, tracking=0, map_precision=expect.IEEE)
    for i, bm in enumerate(seq):
        stab.set_border_mode(bm)
        planar = i % 3 == 2
        o = stab.pull_nv12(planar=True) if planar else stab.pull()
        o = tuple(x.cpu().numpy() for x in o) if planar else o.cpu().numpy()
        R = stab.warp_rotation(i)
        if bm == 0:
            p = oracle.map_params(K, Ko, R)
            if planar:
                ey, euv = expect.warp_planar(frames[i + 1], p, cw, ch, expect.IEEE)
                eq(o[0], ey, ("switch y", i)), eq(o[1], euv, ("switch uv", i))
            else:
                eq(o, expect.warp(frames[i + 1], p, cw, ch, expect.IEEE), ("switch", i))
        else:
            expect_frame(vs, frames[i + 1], K, Ko, R, cw, ch, o, "planar" if planar else "pull", border_mode=bm, what=("switch", bm, i))
    stab.close()


def test_pipeline_border_refusals(vs, cuda, clip):
    import torch
    K, Ko, cw, ch, frames = clip
    fr = [torch.from_numpy(f).to(cuda) for f in frames[:5]]
    stab = vs.Stabilizer(fr, total=5, smooth_radius=1, border_mode=vs.BORDER_REFLECT_101)
    with pytest.raises(vs.VstabError, match="NV12 through BGR"):
        stab.pull_nv12(planar=False)                  # refused before a frame is taken
    for bad in (3, 5, -1, 8):
        assert vs.lib.vstab_set_border_mode(stab._h, bad) == vs.ERR_INVALID
    n = 0
    while stab.pull() is not None:                     # the handle keeps working and no frame was lost
        n += 1
    assert n == 4
    stab.close()
    for cfg in (dict(interpolation=0), dict(resample=vs.RESAMPLE_CUBIC), dict(resample=vs.RESAMPLE_LANCZOS4)):
        stab = vs.Stabilizer(fr, total=5, smooth_radius=1, **cfg)
        for bm in MODES:
            assert vs.lib.vstab_set_border_mode(stab._h, bm) == vs.ERR_UNSUPPORTED, cfg
            assert b"VSTAB_BORDER_CONSTANT" in vs.lib.vstab_last_error()
        assert vs.lib.vstab_set_border_mode(stab._h, vs.BORDER_CONSTANT) == vs.OK
        stab.close()
    p16 = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in frames[:5]]
    stab = vs.Stabilizer(p16, total=5, smooth_radius=1, bit_depth=10, pixel_depth=10)
    assert vs.lib.vstab_set_border_mode(stab._h, vs.BORDER_REPLICATE) == vs.ERR_UNSUPPORTED
    stab.close()
    with pytest.raises(vs.VstabError):
        vs.Stabilizer(fr, total=5, smooth_radius=1, interpolation=0, border_mode=vs.BORDER_REFLECT)
