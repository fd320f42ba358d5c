"""GPU parity of the colour matrix and range (include/vstab.h "Colour matrix and range") through the C ABI and the pipeline object:
vstab_cvt_nv12_bgr_colour, vstab_cvt_bgr_nv12_colour, vstab_warp_nv12_colour and vstab_set_colour.  Bar: every byte equals the numpy
definition (tests/colour_def.py) -- for the warps, the oracle's remap of the converted frame under the oracle's maps (the reference
kernel's own map, run on this GPU, for map mode 5) -- and every output plane is guarded by canary bytes (tests/layouts.py).  Under
(CVTCOLOR, LIMITED) the new entry points give the bytes of vstab_cvt_nv12_bgr and vstab_warp_nv12_ex."""
import ctypes
import functools
import os

import numpy as np
import pytest

import colour_def as C
import expect
import layouts
import oracle
import synth
import warp_def as wd

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [C.NAMES[s] for s in C.SPECS]
BT709L, BT601F = (C.BT709, C.LIMITED), (C.BT601, C.FULL)
ROT = (0.02, -0.03, 0.01)
PAST = (0.35, -0.25, 0.2)   # looks past the source: edge waves, dead tiles
SIZES = [(2, 2), (66, 34), (258, 130)]


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp).reshape(np.asarray(got).shape)
    assert np.array_equal(got, exp), (what, int((got != exp).sum()))


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def map_modes():
    return list(range(5)) + ([5] if oracle.ref_gfx950_available() else [])


# ---- the C ABI with separate, canaried planes ---------------------------------------------------------------------------------------
def cvt_fwd(vs, cuda, f, spec, layout="decoder"):
    h = f.shape[0] * 2 // 3
    s = layouts.place(f[:h], f[h:], layout, cuda)
    o = layouts.Plane(s.h, 3 * s.w, cuda)
    layouts._call(vs, "vstab_cvt_nv12_bgr_colour", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, o.ptr, o.pitch, spec[0], spec[1], vs._stream())
    return o.host(shape=(s.h, s.w, 3))


def cvt_inv(vs, cuda, bgr, spec):
    """vstab_cvt_bgr_nv12_colour from a padded source pitch into canaried planes -> (y (h, w), uv (h / 2, w))"""
    import torch
    h, w = bgr.shape[:2]
    pitch = (3 * w + 15) // 16 * 16 + 32
    src = torch.full((h, pitch), layouts.FILL, dtype=torch.uint8, device=cuda)
    src[:, :3 * w] = dev(bgr.reshape(h, 3 * w), cuda)
    oy, ou = layouts.Plane(h, w, cuda), layouts.Plane(h // 2, w, cuda)
    layouts._call(vs, "vstab_cvt_bgr_nv12_colour", src.data_ptr(), pitch, w, h, oy.ptr, oy.pitch, ou.ptr, ou.pitch, spec[0], spec[1], vs._stream())
    return oy.host(), ou.host()


def warp_colour(vs, cuda, s, params, dw, dh, mode, out_format, spec):
    """vstab_warp_nv12_colour on layouts.Src s -> BGR (dh, dw, 3), or (y, uv) NV12 planes, read back after the canary check"""
    p, pp = layouts._f(params)
    if out_format == vs.OUT_BGR8:
        o = layouts.Plane(dh, 3 * dw, cuda)
        layouts._call(vs, "vstab_warp_nv12_colour", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), o.ptr, o.pitch, None, 0, dw, dh,
                      spec[0], spec[1], vs._stream())
        return o.host(shape=(dh, dw, 3))
    oy, ou = layouts.out_nv12(dw, dh, cuda)
    layouts._call(vs, "vstab_warp_nv12_colour", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), oy.ptr, oy.pitch, ou.ptr, ou.pitch,
                  dw, dh, spec[0], spec[1], vs._stream())
    return oy.host(), ou.host()


def expected_bgr(f, maps, spec):
    return oracle.remap_bilinear(C.nv12_to_bgr(f, spec), *maps)


def check_warp(vs, cuda, s, f, p, dw, dh, mode, spec, maps, what, formats=(0, 1)):
    exp = expected_bgr(f, maps, spec)
    if 0 in formats:
        eq(warp_colour(vs, cuda, s, p, dw, dh, mode, vs.OUT_BGR8, spec), exp, (what, "bgr", mode, spec))
    if 1 in formats:
        gy, guv = warp_colour(vs, cuda, s, p, dw, dh, mode, vs.OUT_NV12, spec)
        ey, euv = C.bgr_to_nv12(exp, spec)
        eq(gy, ey, (what, "luma", mode, spec)), eq(guv, euv, (what, "chroma", mode, spec))


# ---- the stateless converters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_converters_every_spec(vs, cuda, spec):
    """full-range content and a frame of extremes at 2 x 2, 66 x 34 and 258 x 130 with padded pitches (vector and byte paths)"""
    rng = np.random.default_rng(3)
    for w, h in SIZES:
        for f in (synth.nv12(21, w, h, full_range=True), C.extremes_frame(w, h)):
            for layout in ("decoder", "unaligned"):
                eq(cvt_fwd(vs, cuda, f, spec, layout), C.nv12_to_bgr(f, spec), ("fwd", w, h, layout))
        for bgr in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), C.nv12_to_bgr(C.extremes_frame(w, h), spec)):
            gy, guv = cvt_inv(vs, cuda, bgr, spec)
            ey, euv = C.bgr_to_nv12(bgr, spec)
            eq(gy, ey, ("inv y", w, h)), eq(guv, euv, ("inv uv", w, h))


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_converters_golden_vectors_and_cube_corners(vs, cuda, spec):
    kat = np.load(os.path.join(HERE, "golden", "colour_kat.npz"))
    name = C.NAMES[spec]
    for k in range(4):
        eq(cvt_fwd(vs, cuda, kat[f"nv12_{k}"], spec), kat[f"fwd_{k}_{name}"], ("kat fwd", k))
        bgr = kat[f"bgr_{k}"]
        gy, guv = cvt_inv(vs, cuda, bgr, spec)
        eq(np.concatenate([gy, guv]), kat[f"inv_{k}_{name}"], ("kat inv", k))
    gy, guv = cvt_inv(vs, cuda, C.cube_corner_frame(), spec)
    ey, euv = C.bgr_to_nv12(C.cube_corner_frame(), spec)
    eq(gy, ey, "corners y"), eq(guv, euv, "corners uv")
    if spec[1] == C.FULL:   # the saturating case: pure blue's U and pure red's V are 256 before sat8
        assert C.bgr_to_yuv_unsaturated(C.CUBE_CORNERS, spec)[:, 1:].max() == 256 and guv[0, 8] == 255 and guv[0, 3] == 255


# ---- the default spec is the pinned entry points ------------------------------------------------------------------------------------
def test_default_spec_gives_the_pinned_bytes(vs, cuda):
    spec = (C.CVTCOLOR, C.LIMITED)
    for w, h in SIZES:
        f = synth.nv12(22, w, h, full_range=True)
        s = layouts.place(f[:h], f[h:], "decoder", cuda)
        eq(cvt_fwd(vs, cuda, f, spec), layouts.cvt_nv12_bgr(vs, s, cuda), ("cvt", w, h))
    w, h, dw, dh = 256, 144, 230, 131
    f = synth.nv12(23, w, h, full_range=True)
    s = layouts.place(f[:h], f[h:], "decoder", cuda)
    K = oracle.get_preset_camera(4, w, h)
    Ko, _ = oracle.get_output_camera(K, w, h)
    for mode in (0, 1, 3):
        for rv in (ROT, PAST):
            p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
            eq(warp_colour(vs, cuda, s, p, dw, dh, mode, vs.OUT_BGR8, spec), layouts.warp_nv12(vs, s, p, dw, dh, mode, vs.OUT_BGR8, cuda), ("bgr", mode, rv))
            gy, guv = warp_colour(vs, cuda, s, p, dw, dh, mode, vs.OUT_NV12, spec)
            ey, euv = layouts.warp_nv12(vs, s, p, dw, dh, mode, vs.OUT_NV12, cuda)
            eq(gy, ey, ("y", mode, rv)), eq(guv, euv, ("uv", mode, rv))


# ---- the fused warp -----------------------------------------------------------------------------------------------------------------
SW, SH, DW, DH = 256, 144, 230, 131


@functools.lru_cache(maxsize=None)
def small_case(rv, mode):
    K = oracle.get_preset_camera(4, SW, SH)
    Ko, _ = oracle.get_output_camera(K, SW, SH)
    p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
    return p, wd.maps(p, DW, DH, mode)


@functools.lru_cache(maxsize=None)
def small_frame():
    return synth.nv12(24, SW, SH, full_range=True)


@pytest.mark.parametrize("rv", [ROT, PAST], ids=["near", "past"])
@pytest.mark.parametrize("mode", range(6))
def test_warp_every_map_mode(vs, cuda, mode, rv):
    if mode == 5 and not oracle.ref_gfx950_available():
        pytest.skip("oracle/_ref/createMap.gfx950.co not built")
    f = small_frame()
    s = layouts.place(f[:SH], f[SH:], "decoder", cuda)
    p, maps = small_case(rv, mode)
    check_warp(vs, cuda, s, f, p, DW, DH, mode, BT709L, maps, "modes")


@pytest.mark.parametrize("rv", [ROT, PAST], ids=["near", "past"])
@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_warp_every_spec(vs, cuda, spec, rv):
    f = small_frame()
    s = layouts.place(f[:SH], f[SH:], "uv_wider", cuda)
    p, maps = small_case(rv, 0)
    check_warp(vs, cuda, s, f, p, DW, DH, 0, spec, maps, "specs")


@functools.lru_cache(maxsize=None)
def tall_case():
    w, h, dw, dh = 1280, 256, 4096, 768
    assert ((dw + 63) // 64) * ((dh + 31) // 32) == 1536
    f = synth.nv12(8, w, h, full_range=True)
    K = oracle.get_preset_camera(4, w, h)
    Ko = K.copy()
    Ko[0, 0] *= 0.8 * dw / w
    Ko[1, 1] *= 0.8 * dh / h
    Ko[0, 2], Ko[1, 2] = dw / 2.0, dh / 2.0
    p = oracle.map_params(K, Ko, oracle.rodrigues(ROT))
    return f, p, wd.maps(p, dw, dh, 0)


@pytest.mark.parametrize("spec", [BT709L, BT601F], ids=["bt709_limited", "bt601_full"])
def test_warp_smallest_output_of_the_64x32_tile_kernels(vs, cuda, spec):
    """4096 x 768 is 64 x 24 = 1536 tiles of 32 rows: the smallest count at which the launcher chooses the 64 x 32-tile kernels"""
    f, p, maps = tall_case()
    s = layouts.place(f[:256], f[256:], "packed", cuda)
    check_warp(vs, cuda, s, f, p, 4096, 768, 0, spec, maps, "64x32")


def test_warp_gather_path(vs, cuda):
    """source planes at 4-byte aligned addresses and pitches only: nothing is staged, every pixel goes through gather_pixel"""
    f = small_frame()
    s = layouts.place(f[:SH], f[SH:], "unaligned", cuda)
    for rv in (ROT, PAST):
        p, maps = small_case(rv, 0)
        check_warp(vs, cuda, s, f, p, DW, DH, 0, BT601F, maps, "gather")


def test_warp_refusals_on_the_device(vs, cuda):
    """what the CPU table cannot reach: nothing is written by a refused call"""
    f = small_frame()
    s = layouts.place(f[:SH], f[SH:], "decoder", cuda)
    p, _ = small_case(ROT, 0)
    _, pp = layouts._f(p)
    oy, ou = layouts.out_nv12(DW, DH, cuda)
    st = vs.lib.vstab_warp_nv12_colour(s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, 0, vs.OUT_NV12_PLANAR, oy.ptr, oy.pitch, ou.ptr, ou.pitch, DW, DH,
                                       C.BT709, C.LIMITED, vs._stream())
    assert st == vs.ERR_INVALID and b"VSTAB_OUT_NV12_PLANAR converts nothing" in vs.lib.vstab_last_error()
    st = vs.lib.vstab_warp_nv12_colour(s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, 0, vs.OUT_BGR8, oy.ptr, oy.pitch, None, 0, DW // 3, DH, C.CVTCOLOR, C.FULL,
                                       vs._stream())
    assert st == vs.ERR_INVALID
    assert np.all(oy.host() == layouts.CANARY) and np.all(ou.host() == layouts.CANARY)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
W, H = 640, 360


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = synth.shaky_clip(5, K, W, H, 12, sigma=0.02)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    return K, Ko, cw, ch, frames


def stabilizer(vs, cuda, frames, **cfg):
    import torch
    return vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), **cfg)


def expect_pull(f, K, Ko, R, cw, ch, spec):
    p = oracle.map_params(K, Ko, R)
    return expected_bgr(f, wd.maps(p, cw, ch, 0), spec)


def test_pipeline_pulls_and_a_switch_mid_stream(vs, cuda, clip):
    """every converting pull under (BT709, LIMITED), from the handle's logged rotation; the spec switched between pulls; the plane-wise pull as ever"""
    import torch
    K, Ko, cw, ch, frames = clip
    stab = stabilizer(vs, cuda, frames, smooth_radius=2, map_precision=expect.IEEE)
    stab.set_colour(vs.COLOUR_BT709, vs.RANGE_LIMITED)
    plan = [("pull", BT709L), ("host", BT709L), ("nv12", BT709L), ("planar", BT709L), ("peek", BT709L), ("frames", BT709L), ("pull", BT601F), ("nv12", BT601F),
            ("pull", (C.CVTCOLOR, C.LIMITED)), ("nv12", (C.BT2020, C.LIMITED)), ("pull", BT709L)]
    assert len(plan) == len(frames) - 1
    for i, (how, spec) in enumerate(plan):
        stab.set_colour(*spec)
        f = frames[i + 1]
        if how == "pull":
            out = stab.pull().cpu().numpy()
        elif how == "host":
            out = stab.pull_host()
        elif how == "peek":
            o = layouts.Plane(ch, 3 * cw, cuda)
            assert vs.lib.vstab_peek_frame(stab._h, o.ptr, o.pitch) == vs.OK, vs.lib.vstab_last_error()
            out = o.host(shape=(ch, cw, 3))
        elif how == "frames":
            ring = [torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda)]
            assert stab.pull_frames_into(ring, 0, 1) == 1
            out = ring[0].cpu().numpy()
        else:
            out = tuple(x.cpu().numpy() for x in stab.pull_nv12(planar=how == "planar"))
        R = stab.warp_rotation(i)
        if how == "planar":   # converts nothing: the plane-wise warp of a handle without a spec
            ey, euv = expect.warp_planar(f, oracle.map_params(K, Ko, R), cw, ch, expect.IEEE)
            eq(out[0], ey, ("planar y", i)), eq(out[1], euv, ("planar uv", i))
            continue
        exp = expect_pull(f, K, Ko, R, cw, ch, spec)
        if how == "nv12":
            ey, euv = C.bgr_to_nv12(exp, spec)
            eq(out[0], ey, ("nv12 y", i, spec)), eq(out[1], euv, ("nv12 uv", i, spec))
        else:
            eq(out, exp, (how, i, spec))
            if spec == (C.CVTCOLOR, C.LIMITED):
                eq(out, expect.warp(f, oracle.map_params(K, Ko, R), cw, ch, expect.IEEE), ("default", i))
    assert stab.pull() is None
    stab.close()


def test_pipeline_cache_steps_aside_and_planar_is_unchanged(vs, cuda, clip):
    """stab = fixed without tracking repeats the parameters frame after frame: a plain handle serves its BGR pulls from the quantised map from
    the second frame on; with a spec set the counter does not move, and the plane-wise pull equals the plain handle's"""
    K, Ko, cw, ch, frames = clip
    cfg = dict(smooth_radius=1, tracking=0, smoother=vs.SMOOTHER_FIXED, map_precision=expect.IEEE)
    plain, col = stabilizer(vs, cuda, frames[:8], **cfg), stabilizer(vs, cuda, frames[:8], **cfg)
    col.set_colour(vs.COLOUR_BT709, vs.RANGE_LIMITED)
    for i in range(7):
        if i == 5:
            col.set_colour(vs.COLOUR_CVTCOLOR, vs.RANGE_LIMITED)   # back to the default: the cache serves again
        if i == 3:
            a, b = plain.pull_nv12(planar=True), col.pull_nv12(planar=True)
            eq(b[0].cpu().numpy(), a[0].cpu().numpy(), "planar y"), eq(b[1].cpu().numpy(), a[1].cpu().numpy(), "planar uv")
            continue
        a, b = plain.pull().cpu().numpy(), col.pull().cpu().numpy()
        spec = BT709L if i < 5 else (C.CVTCOLOR, C.LIMITED)
        eq(b, expect_pull(frames[i + 1], K, Ko, col.warp_rotation(i), cw, ch, spec), ("fixed", i))
        if i >= 5:
            eq(b, a, ("default again", i))
        else:
            assert col.warps_from_cache() == 0
    assert plain.warps_from_cache() >= 4 and col.warps_from_cache() >= 1
    plain.close(), col.close()


def test_pipeline_refusals_leave_the_handle_unchanged(vs, cuda, clip):
    import torch
    K, Ko, cw, ch, frames = clip
    UNS, INV = vs.ERR_UNSUPPORTED, vs.ERR_INVALID
    set_colour = vs.lib.vstab_set_colour
    # handles whose warp has no colour form: refused, the default spec still accepted, and they go on as they were
    lens = dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=cw, out_height=ch)
    rect = dict(lens_mode=1, in_projection=0, out_projection=0, in_dfov=100.0, out_dfov=80.0, out_width=cw, out_height=ch)
    for cfg in (dict(interpolation=0), dict(resample=vs.RESAMPLE_CUBIC), dict(resample=vs.RESAMPLE_LANCZOS4), dict(border_mode=vs.BORDER_REFLECT_101),
                dict(lens, calibration=(None, (0.01, 0.0, 0.0, 0.0))), dict(lens, calibration_ex=(None, (0.01, 0.0, 0.0, 0.0))),
                dict(rect, pinhole=(None, (0.01, 0.0, 0.0, 0.0, 0.0)))):
        ref, stab = stabilizer(vs, cuda, frames[:4], smooth_radius=1, tracking=0, **cfg), stabilizer(vs, cuda, frames[:4], smooth_radius=1, tracking=0, **cfg)
        for spec in C.SPECS[1:]:
            assert set_colour(stab._h, *spec) == UNS, (cfg, spec)
            assert b"vstab_set_colour: a colour spec other than" in vs.lib.vstab_last_error()
        assert set_colour(stab._h, 7, 0) == INV and set_colour(stab._h, C.CVTCOLOR, C.FULL) == INV
        assert set_colour(stab._h, C.CVTCOLOR, C.LIMITED) == vs.OK
        eq(stab.pull().cpu().numpy(), ref.pull().cpu().numpy(), ("unchanged", tuple(cfg)))
        ref.close(), stab.close()
    p16 = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in frames[:4]]
    stab = vs.Stabilizer(p16, total=4, smooth_radius=1, bit_depth=10, pixel_depth=10)
    assert set_colour(stab._h, C.BT2020, C.LIMITED) == UNS and set_colour(stab._h, C.CVTCOLOR, C.LIMITED) == vs.OK
    stab.close()

    # with a spec set: border modes, calibrations and keep pulls are refused; the spec and the constant border stay in force
    stab = stabilizer(vs, cuda, frames[:6], smooth_radius=1, map_precision=expect.IEEE)
    stab.set_colour(vs.COLOUR_BT709, vs.RANGE_LIMITED)
    assert set_colour(stab._h, 4, 0) == INV and set_colour(stab._h, 2, 2) == INV and set_colour(stab._h, C.CVTCOLOR, C.FULL) == INV
    for bm in (vs.BORDER_REPLICATE, vs.BORDER_REFLECT, vs.BORDER_REFLECT_101):
        assert vs.lib.vstab_set_border_mode(stab._h, bm) == UNS and vs.lib.vstab_set_border_mode_ex(stab._h, bm) == UNS
        assert b"a colour spec is set (vstab_set_colour)" in vs.lib.vstab_last_error()
    assert vs.lib.vstab_set_border_mode(stab._h, vs.BORDER_CONSTANT) == vs.OK
    out, prev = torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda), torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda)
    assert vs.lib.vstab_pull_frame_keep(stab._h, out.data_ptr(), out.stride(0), prev.data_ptr(), prev.stride(0)) == UNS
    y, uv = vs.nv12_out_planes(cw, ch)
    assert vs.lib.vstab_pull_frame_nv12_planar_keep(stab._h, y.data_ptr(), y.stride(0), uv.data_ptr(), uv.stride(0), y.data_ptr(), y.stride(0), uv.data_ptr(),
                                                    uv.stride(0)) == UNS
    assert int(out.max()) == 0
    for i in range(5):   # no frame was taken by a refused call, and the spec is still BT709 limited
        eq(stab.pull().cpu().numpy(), expect_pull(frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, BT709L), ("after refusals", i))
    assert stab.pull() is None
    stab.close()
    D4, D5 = (ctypes.c_double * 4)(0.01, 0, 0, 0), (ctypes.c_double * 5)(0.01, 0, 0, 0, 0)
    for cfg, fn, d in ((lens, "vstab_set_input_calibration", D4), (lens, "vstab_set_input_calibration_ex", D4), (rect, "vstab_set_input_pinhole", D5)):
        stab = stabilizer(vs, cuda, frames[:4], smooth_radius=1, tracking=0, **cfg)
        stab.set_colour(vs.COLOUR_BT601, vs.RANGE_FULL)
        assert getattr(vs.lib, fn)(stab._h, None, d) == UNS, fn
        assert b"a colour spec is set (vstab_set_colour)" in vs.lib.vstab_last_error()
        stab.set_colour(vs.COLOUR_CVTCOLOR, vs.RANGE_LIMITED)
        assert getattr(vs.lib, fn)(stab._h, None, d) == vs.OK, fn   # (and not calibrated by the refused call: the setter still works)
        stab.close()

    # a frame that carries a read-out rotation is refused and consumed by the converting pulls; the plane-wise pull warps it
    ro = [oracle.rodrigues((0.002 * (k % 3), -0.003, 0.001 * k)) for k in range(5)]
    stab = stabilizer(vs, cuda, frames[:5], smooth_radius=1, tracking=0, readouts=ro, map_precision=expect.IEEE)
    stab.set_colour(vs.COLOUR_BT709, vs.RANGE_LIMITED)
    with pytest.raises(vs.VstabError, match="colour spec"):
        stab.pull()
    assert stab.pull_nv12(planar=True) is not None
    with pytest.raises(vs.VstabError, match="colour spec"):
        stab.pull_nv12(planar=False)
    assert stab.pull_nv12(planar=True) is not None and stab.pull() is None   # four frames: two refused and consumed, two warped
    stab.close()
