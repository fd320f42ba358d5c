"""GPU parity of the colour matrix and range at 10 bits (include/vstab.h "Colour matrix and range at 10 bits") through the C ABI and the
pipeline object: vstab_cvt_p010_bgr16_colour, vstab_cvt_bgr16_p010_colour, vstab_warp_p010_colour, vstab_warp_p010_planes_colour and
vstab_set_colour10.  Bar: every 16-bit sample equals the numpy definition (tests/colour10_def.py) -- for the warps, the oracle's 10-bit
remap of the converted frame under the oracle's maps (the reference kernel's own map, run on this GPU, for map mode 5) -- and every output
plane is guarded by canary bytes (tests/layouts.py).  Under (CVTCOLOR, LIMITED) the new entry points give the bytes of their twins."""
import ctypes
import functools
import os

import numpy as np
import pytest

import colour10_def as C
import expect
import layouts
import oracle
import synth
import warp_def as wd

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [C.NAMES[s] for s in C.SPECS]
BT2020L, BT709F = (C.BT2020, C.LIMITED), (C.BT709, C.FULL)
ROT = (0.02, -0.03, 0.01)
PAST = (0.35, -0.25, 0.2)   # looks past the source: edge waves, dead tiles
FAR = (0.0, 2.6, 0.0)       # far and dead pixels
EXACT, FP16 = 0, 1


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp).reshape(np.asarray(got).shape)
    assert np.array_equal(got, exp), (what, int((got != exp).sum()))


@functools.lru_cache(maxsize=None)
def picture(seed, w, h):
    """a colourful full-range picture widened to P010 words, two more bits of detail and junk in the low six -> (y, uv)"""
    f = synth.nv12(seed, w, h, full_range=True).astype(np.uint16)
    rng = np.random.default_rng(seed)
    wide = (f << 8) | (rng.integers(0, 4, f.shape).astype(np.uint16) << 6) | rng.integers(0, 64, f.shape).astype(np.uint16)
    return wide[:h], wide[h:]


@functools.lru_cache(maxsize=None)
def converted(seed, w, h, spec):
    return C.p010_to_bgr10(*picture(seed, w, h), spec)


# ---- the C ABI with separate, canaried planes ---------------------------------------------------------------------------------------
def cvt_fwd(vs, cuda, y, uv, spec, layout="decoder", shift=0):
    """vstab_cvt_p010_bgr16_colour; shift 2: rows that are 2-byte and not 4-byte aligned (the 2-byte stores), the two bytes in front untouched"""
    s = layouts.place(y, uv, layout, cuda)
    o = layouts.Plane(s.h, 6 * s.w + shift, cuda)
    layouts._call(vs, "vstab_cvt_p010_bgr16_colour", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, o.ptr + shift, o.pitch, spec[0], spec[1], vs._stream())
    out = o.host(np.uint16)
    assert np.all(out[:, :shift // 2] == layouts.CANARY * 0x101)
    return out[:, shift // 2:].reshape(s.h, s.w, 3)


def cvt_inv(vs, cuda, bgr, spec, fn="vstab_cvt_bgr16_p010_colour"):
    """from a padded source pitch into canaried planes -> (y (h, w), uv (ceil(h / 2), 2 ceil(w / 2))) uint16"""
    import torch
    h, w = bgr.shape[:2]
    pitch = (6 * w + 15) // 16 * 16 + 34
    src = torch.full((h, pitch), layouts.FILL, dtype=torch.uint8, device=cuda)
    src[:, :6 * w] = torch.from_numpy(np.ascontiguousarray(bgr, np.uint16).view(np.uint8).reshape(h, 6 * w)).to(cuda)
    oy, ou = layouts.out_p010(w, h, cuda)
    tail = (spec[0], spec[1], vs._stream()) if fn.endswith("_colour") else (vs._stream(),)
    layouts._call(vs, fn, src.data_ptr(), pitch, w, h, oy.ptr, oy.pitch, ou.ptr, ou.pitch, *tail)
    return oy.host(np.uint16), ou.host(np.uint16)


def _rb(rot_bottom):
    return layouts._f(np.asarray(rot_bottom).reshape(9))[1] if rot_bottom is not None else None


def warp_bgr16(vs, cuda, s, params, dw, dh, mode, blend, spec, rot_bottom=None):
    """vstab_warp_p010_colour -> (dh, dw, 3) uint16"""
    o = layouts.Plane(dh, 6 * dw, cuda)
    layouts._call(vs, "vstab_warp_p010_colour", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, layouts._f(params)[1], _rb(rot_bottom), int(mode), int(blend), o.ptr,
                  o.pitch, dw, dh, spec[0], spec[1], vs._stream())
    return o.host(np.uint16, (dh, dw, 3))


def warp_planes(vs, cuda, s, params, dw, dh, mode, blend, spec, rot_bottom=None, shift=False):
    """vstab_warp_p010_planes_colour -> (y, uv) uint16; shift: planes that are not 8-byte aligned (the kernel's non-vector stores)"""
    sy, su = (2, 4) if shift else (0, 0)
    oy, ou = layouts.Plane(dh, 2 * dw + sy, cuda), layouts.Plane((dh + 1) // 2, 4 * ((dw + 1) // 2) + su, cuda)
    layouts._call(vs, "vstab_warp_p010_planes_colour", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, layouts._f(params)[1], _rb(rot_bottom), int(mode), int(blend),
                  oy.ptr + sy, oy.pitch, ou.ptr + su, ou.pitch, dw, dh, spec[0], spec[1], vs._stream())
    gy, gu = oy.host(np.uint16), ou.host(np.uint16)
    assert np.all(gy[:, :sy // 2] == layouts.CANARY * 0x101) and np.all(gu[:, :su // 2] == layouts.CANARY * 0x101)
    return gy[:, sy // 2:], gu[:, su // 2:]


def expected(seed, w, h, spec, maps, blend):
    return oracle.remap_bilinear10(converted(seed, w, h, spec), *maps, blend)


# ---- the stateless converters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_converters_every_spec(vs, cuda, spec):
    """a picture and a frame of extremes (junk in the low six bits) at 2 x 2, 66 x 34 and 258 x 130, aligned and 2-byte aligned rows; the
    inverse also at the odd sizes 323 x 181 and 1 x 1"""
    rng = np.random.default_rng(3)
    for w, h in [(2, 2), (66, 34), (258, 130)]:
        for y, uv in (picture(21, w, h), C.extremes_frame(w, h)):
            for layout, shift in (("decoder", 0), ("unaligned", 2)):
                eq(cvt_fwd(vs, cuda, y, uv, spec, layout, shift), C.p010_to_bgr10(y, uv, spec), ("fwd", w, h, layout))
    for w, h in [(2, 2), (66, 34), (258, 130), (323, 181), (1, 1)]:
        imgs = [rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)]
        if not (w & 1 or h & 1):
            imgs.append(C.p010_to_bgr10(*C.extremes_frame(w, h), spec))
        for bgr in imgs:
            gy, guv = cvt_inv(vs, cuda, bgr, spec)
            ey, euv = C.bgr10_to_p010(bgr, spec)
            eq(gy, ey, ("inv y", w, h)), eq(guv, euv, ("inv uv", w, h))


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_converters_golden_vectors_and_cube_corners(vs, cuda, spec):
    kat = np.load(os.path.join(HERE, "golden", "colour10_kat.npz"))
    name = C.NAMES[spec]
    for k in range(2):
        eq(cvt_fwd(vs, cuda, kat[f"y_{k}"], kat[f"uv_{k}"], spec), kat[f"fwd_{k}_{name}"], ("kat fwd", k))
        gy, guv = cvt_inv(vs, cuda, kat[f"bgr_{k}"], spec)
        eq(gy, kat[f"invy_{k}_{name}"], ("kat inv y", k)), eq(guv, kat[f"invuv_{k}_{name}"], ("kat inv uv", k))
    gy, guv = cvt_inv(vs, cuda, C.cube_corner_frame(), spec)
    ey, euv = C.bgr10_to_p010(C.cube_corner_frame(), spec)
    eq(gy, ey, "corners y"), eq(guv, euv, "corners uv")
    if spec[1] == C.FULL:   # the saturating case: pure blue's U and pure red's V are 1024 before sat10
        assert C.bgr10_to_yuv_unsaturated(C.CUBE_CORNERS, spec)[:, 1:].max() == 1024 and guv[0, 8] == 1023 << 6 and guv[0, 3] == 1023 << 6


def test_default_spec_converters_are_the_pinned_ones(vs, cuda):
    rng = np.random.default_rng(4)
    for w, h in [(2, 2), (66, 34), (258, 130), (323, 181), (1, 1)]:
        bgr = rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)
        a, b = cvt_inv(vs, cuda, bgr, C.DEFAULT), cvt_inv(vs, cuda, bgr, None, "vstab_cvt_bgr16_p010")
        eq(a[0], b[0], ("y", w, h)), eq(a[1], b[1], ("uv", w, h))
    y, uv = picture(22, 66, 34)
    eq(cvt_fwd(vs, cuda, y, uv, C.DEFAULT), oracle.cvt_p010_bgr10(y, uv), "forward")


# ---- the direct-gather kernel -------------------------------------------------------------------------------------------------------
GW, GH, GDW, GDH = 66, 34, 61, 33
LENSES = {1: (1, 150.0, 0, 110.0), 2: (1, 150.0, 1, 165.0), 3: (0, 100.0, 0, 80.0), 4: (0, 100.0, 1, 300.0)}


@functools.lru_cache(maxsize=None)
def gather_case(mode, per_row):
    if mode in LENSES:
        ip, ifov, op, ofov = LENSES[mode]
        Ki, Ko = oracle.lens_camera(ip, ifov, GW, GH), oracle.lens_camera(op, ofov, GDW, GDH)
    else:
        Ki = oracle.get_preset_camera(4, GW, GH)
        Ko, _ = oracle.get_output_camera(Ki, GW, GH)
    p = oracle.map_params(Ki, Ko, oracle.rodrigues((0.05, -0.1, 0.2)))
    rb = oracle.map_params(Ki, Ko, oracle.rodrigues((0.07, -0.09, 0.18)))[8:] if per_row else None
    return p, rb, wd.maps(p, GDW, GDH, mode, rb)


def gather_modes():
    return list(range(5)) + ([5] if oracle.ref_gfx950_available() else [])


@pytest.mark.parametrize("per_row", [False, True], ids=["frame", "per_row"])
@pytest.mark.parametrize("blend", [EXACT, FP16], ids=["exact", "fp16"])
def test_direct_kernel_every_mode_and_every_spec(vs, cuda, blend, per_row):
    """66 x 34 -> 61 x 33 from planes whose pitches are no multiple of 16: every map mode at BT2020 limited, every spec at mode 0"""
    y, uv = picture(25, GW, GH)
    s = layouts.place(y, uv, "unaligned", cuda)
    assert s.pitch_y % 16 and s.pitch_uv % 16
    for mode, spec in [(m, BT2020L) for m in gather_modes()] + [(0, sp) for sp in C.SPECS]:
        p, rb, maps = gather_case(mode, per_row)
        eq(warp_bgr16(vs, cuda, s, p, GDW, GDH, mode, blend, spec, rb), expected(25, GW, GH, spec, maps, blend), ("direct", mode, spec))


# ---- the tiled kernel ---------------------------------------------------------------------------------------------------------------
SW, SH, DW, DH = 256, 144, 230, 131


@functools.lru_cache(maxsize=None)
def small_case(rv, mode, per_row):
    K = oracle.get_preset_camera(4, SW, SH)
    Ko, _ = oracle.get_output_camera(K, SW, SH)
    p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
    rb = oracle.map_params(K, Ko, oracle.rodrigues(tuple(v + d for v, d in zip(rv, (0.02, 0.01, -0.02)))))[8:] if per_row else None
    return p, rb, wd.maps(p, DW, DH, mode, rb)


def check_tiled(vs, cuda, s, seed, w, h, p, rb, maps, dw, dh, mode, blend, spec, what, shift=False):
    """FMT 2 (16-bit BGR) and FMT 3 (P010 planes) of one warp against one expected frame"""
    exp = expected(seed, w, h, spec, maps, blend)
    eq(warp_bgr16(vs, cuda, s, p, dw, dh, mode, blend, spec, rb), exp, (what, "bgr16", mode, blend, spec))
    gy, guv = warp_planes(vs, cuda, s, p, dw, dh, mode, blend, spec, rb, shift)
    ey, euv = C.bgr10_to_p010(exp, spec)
    eq(gy, ey, (what, "luma", mode, blend, spec)), eq(guv, euv, (what, "chroma", mode, blend, spec))


@pytest.mark.parametrize("per_row", [False, True], ids=["frame", "per_row"])
@pytest.mark.parametrize("blend", [EXACT, FP16], ids=["exact", "fp16"])
@pytest.mark.parametrize("mode", [0, 1, 5])
def test_tiled_kernel_modes_blends_and_formats(vs, cuda, mode, blend, per_row):
    """256 x 144 -> 230 x 131 (an output width that is no multiple of 4: the scalar tails of the planes), near and past the source"""
    if mode == 5 and not oracle.ref_gfx950_available():
        pytest.skip("oracle/_ref/createMap.gfx950.co not built")
    s = layouts.place(*picture(24, SW, SH), "decoder", cuda)
    for rv in (ROT, PAST):
        p, rb, maps = small_case(rv, mode, per_row)
        for spec in (BT2020L, BT709F):
            check_tiled(vs, cuda, s, 24, SW, SH, p, rb, maps, DW, DH, mode, blend, spec, ("tiled", rv))


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_tiled_kernel_every_spec(vs, cuda, spec):
    s = layouts.place(*picture(24, SW, SH), "uv_wider", cuda)
    for rv, blend in ((ROT, EXACT), (PAST, FP16), (FAR, EXACT)):
        p, rb, maps = small_case(rv, 0, False)
        check_tiled(vs, cuda, s, 24, SW, SH, p, rb, maps, DW, DH, 0, blend, spec, ("specs", rv))


def test_tiled_kernel_far_and_dead_pixels_and_unaligned_planes(vs, cuda):
    """rotation (0, 2.6, 0); planes out that are not 8-byte aligned take the kernel's non-vector stores"""
    s = layouts.place(*picture(24, SW, SH), "decoder", cuda)
    for per_row in (False, True):
        p, rb, maps = small_case(FAR, 0, per_row)
        for blend in (EXACT, FP16):
            check_tiled(vs, cuda, s, 24, SW, SH, p, rb, maps, DW, DH, 0, blend, BT2020L, "far", shift=True)
    p, rb, maps = small_case(ROT, 1, True)
    check_tiled(vs, cuda, s, 24, SW, SH, p, rb, maps, DW, DH, 1, FP16, BT709F, "shifted planes", shift=True)


def test_tiled_kernel_split_tiles_at_640x360(vs, cuda):
    """the shape and tilts of test_p010_warp_bit_exact_vs_oracle under the fp16 blend, whose 8-byte LDS pixels put boxes past half the LDS
    capacity: the SPLIT halves run"""
    w, h = 640, 360
    K = oracle.get_preset_camera(4, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    s = layouts.place(*picture(31, w, h), "decoder", cuda)
    for rot in [(0.0, 0.0, 0.0), (0.02, -0.03, 0.01), (-0.15, 0.1, 0.3), (0.0, 2.6, 0.0)]:
        p = oracle.map_params(K, Ko, oracle.rodrigues(rot))
        check_tiled(vs, cuda, s, 31, w, h, p, None, wd.maps(p, cw, ch, 0), cw, ch, 0, FP16, BT2020L, ("640", rot))
    p = oracle.map_params(K, Ko, oracle.rodrigues((0.01, -0.02, 0.005)))
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.03, -0.01, -0.01)))[8:]
    check_tiled(vs, cuda, s, 31, w, h, p, rb, wd.maps(p, cw, ch, 1, rb), cw, ch, 1, FP16, BT709F, "640 per row")


def test_planes_out_is_warp_then_inverse_converter(vs, cuda):
    s = layouts.place(*picture(24, SW, SH), "decoder", cuda)
    p, rb, _ = small_case(PAST, 0, True)
    for spec, blend in ((BT2020L, FP16), (BT709F, EXACT)):
        bgr = warp_bgr16(vs, cuda, s, p, DW, DH, 0, blend, spec, rb)
        ey, euv = cvt_inv(vs, cuda, bgr, spec)
        gy, guv = warp_planes(vs, cuda, s, p, DW, DH, 0, blend, spec, rb)
        eq(gy, ey, ("y", spec)), eq(guv, euv, ("uv", spec))


# ---- cross-checks -------------------------------------------------------------------------------------------------------------------
def test_both_routes_equal_the_definition_and_specs_differ(vs, cuda):
    """one frame as aligned planes (the tiled route) and as views at a 2-byte / 4-byte offset into wider buffers (the direct route)"""
    y, uv = picture(24, SW, SH)
    tiled = layouts.place(y, uv, "decoder", cuda)
    direct = layouts.place(y, uv, None, cuda, spec=(2 * SW + 32, 2 * SW + 64, "two", 2, 4))
    assert direct.y % 4 == 2 and direct.uv % 16 == 4
    p, rb, maps = small_case(ROT, 0, False)
    outs = {}
    for spec in (BT2020L, BT709F, C.DEFAULT):
        for blend in (EXACT, FP16):
            exp = expected(24, SW, SH, spec, maps, blend)
            a, b = warp_bgr16(vs, cuda, tiled, p, DW, DH, 0, blend, spec), warp_bgr16(vs, cuda, direct, p, DW, DH, 0, blend, spec)
            eq(a, exp, ("tiled route", spec, blend)), eq(b, exp, ("direct route", spec, blend))
            outs[spec, blend] = a
    # (CVTCOLOR, LIMITED) is vstab_warp_p010 itself, byte for byte, on both routes and with planes out
    for s in (tiled, direct):
        for blend in (EXACT, FP16):
            eq(outs[C.DEFAULT, blend], layouts.warp_p010(vs, s, p, DW, DH, 0, blend, cuda), ("default", blend))
    gy, guv = warp_planes(vs, cuda, tiled, p, DW, DH, 0, EXACT, C.DEFAULT)
    ey, euv = layouts.warp_p010_planes(vs, tiled, p, DW, DH, 0, EXACT, cuda)
    eq(gy, ey, "default planes y"), eq(guv, euv, "default planes uv")
    # the specs are not one arithmetic under three names: on a colourful frame they differ in many samples
    for a, b in ((BT2020L, BT709F), (BT2020L, C.DEFAULT), (BT709F, C.DEFAULT)):
        assert int((outs[a, EXACT] != outs[b, EXACT]).sum()) > outs[a, EXACT].size // 4, (a, b)


def test_refusals_on_the_device_write_nothing(vs, cuda):
    s = layouts.place(*picture(24, SW, SH), "unaligned", cuda)
    p, _, _ = small_case(ROT, 0, False)
    pp = layouts._f(p)[1]
    oy, ou = layouts.out_p010(DW, DH, cuda)
    o = layouts.Plane(DH, 6 * DW, cuda)
    L = vs.lib
    # planes that do not allow the tiled kernel: VSTAB_ERR_UNSUPPORTED from _planes_colour, as from its twin
    assert L.vstab_warp_p010_planes_colour(s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, None, 0, 0, oy.ptr, oy.pitch, ou.ptr, ou.pitch, DW, DH, C.BT2020, C.LIMITED,
                                           vs._stream()) == vs.ERR_UNSUPPORTED
    assert L.vstab_last_error().decode() == "vstab_warp_p010_planes_colour: needs 16-byte aligned source planes and a fisheye -> pinhole map"
    assert L.vstab_warp_p010_colour(s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, None, 0, 0, o.ptr, o.pitch, DW, DH, C.CVTCOLOR, C.FULL, vs._stream()) == vs.ERR_INVALID
    assert L.vstab_cvt_p010_bgr16_colour(s.y, s.pitch_y, s.uv, s.pitch_uv, DW - 1, DH - 1, o.ptr, o.pitch, 9, 0, vs._stream()) == vs.ERR_INVALID
    assert np.all(oy.host() == layouts.CANARY) and np.all(ou.host() == layouts.CANARY) and np.all(o.host() == layouts.CANARY)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
W, H, N = 640, 360, 12


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames8, _ = synth.shaky_clip(3, K, W, H, N, sigma=0.004)
    rng = np.random.default_rng(9)
    wide = [((f.astype(np.uint16) << 8) | (rng.integers(0, 4, f.shape, dtype=np.uint16) << 6) | rng.integers(0, 64, f.shape, dtype=np.uint16)) for f in frames8]
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    return K, Ko, cw, ch, wide


def stabilizer(vs, cuda, wide, aligned=True, **cfg):
    """aligned: frames whose planes allow the tiled kernel; else views into buffers two samples wider, whose pitch is no multiple of 16:
    vstab_pull_frame_p010 then takes its fallback through the handle's 16-bit BGR buffer"""
    import torch
    dev = []
    for x in wide:
        t = torch.from_numpy(x.view(np.int16)).to(cuda)
        if not aligned:
            buf = torch.zeros((x.shape[0], x.shape[1] + 2), dtype=torch.int16, device=cuda)
            buf[:, :x.shape[1]] = t
            t = buf[:, :x.shape[1]]
            assert (t.stride(0) * 2) % 16
        dev.append(t)
    return vs.Stabilizer(dev, total=len(dev), bit_depth=10, pixel_depth=10, smooth_radius=3, seed=5, map_precision=expect.IEEE, **cfg)


@pytest.mark.parametrize("blend", [EXACT, FP16], ids=["exact", "fp16"])
def test_pipeline_pulls_and_a_switch_mid_stream(vs, cuda, clip, blend):
    """set_colour10 before the first pull and between pulls; 16-bit BGR and P010 pulls on both routes against the definition and against
    the stateless colour warp under the frame's rotation; the plane-wise pull as ever"""
    import torch
    K, Ko, cw, ch, wide = clip
    fused, fallback = stabilizer(vs, cuda, wide, True, blend=blend), stabilizer(vs, cuda, wide, False, blend=blend)
    plan = [("bgr16", BT2020L), ("p010", BT2020L), ("planar", BT2020L), ("p010", BT709F), ("bgr16", BT709F), ("bgr16", C.DEFAULT), ("p010", C.DEFAULT),
            ("p010", (C.BT601, C.LIMITED)), ("bgr16", (C.BT2020, C.FULL)), ("planar", BT709F), ("p010", BT2020L)]
    assert len(plan) == N - 1
    fused.set_colour10(*BT2020L), fallback.set_colour10(*BT2020L)
    for i, (how, spec) in enumerate(plan):
        y, uv = wide[i + 1][:H], wide[i + 1][H:]
        got = []
        for stab in (fused, fallback):
            stab.set_colour10(*spec)
            if how == "bgr16":
                o = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
                assert stab.pull_bgr16_into(o)
                got.append((o.cpu().numpy().view(np.uint16),))
            else:
                oy, ou = layouts.out_p010(cw, ch, cuda)
                fn = vs.lib.vstab_pull_frame_p010_planar if how == "planar" else vs.lib.vstab_pull_frame_p010
                assert fn(stab._h, oy.ptr, oy.pitch, ou.ptr, ou.pitch) == vs.OK, vs.lib.vstab_last_error()
                got.append((oy.host(np.uint16), ou.host(np.uint16)))
        R = fused.warp_rotation(i)
        assert np.array_equal(R, fallback.warp_rotation(i))
        p = oracle.map_params(K, Ko, R)
        for a, b in zip(*got):   # the two routes give the same bytes
            eq(b, a, ("routes", how, i, spec))
        if how == "planar":      # converts nothing: the plane-wise warp of a handle without a spec
            ey, euv = expect.warp_p010_planar(y, uv, p, cw, ch, None, blend, expect.IEEE)
            eq(got[0][0], ey, ("planar y", i)), eq(got[0][1], euv, ("planar uv", i))
            continue
        exp = oracle.remap_bilinear10(C.p010_to_bgr10(y, uv, spec), *wd.maps(p, cw, ch, 0), blend)
        s = layouts.place(y, uv, "decoder", cuda)
        eq(warp_bgr16(vs, cuda, s, p, cw, ch, 0, blend, spec), exp, ("stateless", i, spec))
        if how == "bgr16":
            eq(got[0][0], exp, ("bgr16", i, spec))
            if spec == C.DEFAULT:
                eq(got[0][0], oracle.warp_p010(y, uv, p, cw, ch, None, 0, blend), ("default", i))
        else:
            ey, euv = C.bgr10_to_p010(exp, spec)
            eq(got[0][0], ey, ("p010 y", i, spec)), eq(got[0][1], euv, ("p010 uv", i, spec))
    o = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
    assert not fused.pull_bgr16_into(o) and not fallback.pull_bgr16_into(o)
    fused.close(), fallback.close()


def test_pipeline_readout_rotations_are_warped_per_row(vs, cuda, clip):
    import torch
    K, Ko, cw, ch, wide = clip
    ro = [oracle.rodrigues(np.array([0.003 * np.sin(k), -0.002 * np.cos(k), 0.004 * np.sin(2 * k + 1)])) for k in range(5)]
    stab = stabilizer(vs, cuda, wide[:5], True, blend=FP16, readouts=ro)
    stab.set_colour10(*BT2020L)
    for i, how in enumerate(("bgr16", "p010", "bgr16", "p010")):
        y, uv = wide[i + 1][:H], wide[i + 1][H:]
        if how == "bgr16":
            o = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
            assert stab.pull_bgr16_into(o)
        else:
            oy, ou = layouts.out_p010(cw, ch, cuda)
            assert vs.lib.vstab_pull_frame_p010(stab._h, oy.ptr, oy.pitch, ou.ptr, ou.pitch) == vs.OK, vs.lib.vstab_last_error()
        Wr = stab.warp_rotation(i)
        p = oracle.map_params(K, Ko, Wr)
        rb = oracle.map_params(K, Ko, ro[i + 1] @ Wr)[8:]
        exp = C.warp_p010(y, uv, p, cw, ch, BT2020L, rb, 0, FP16)
        if how == "bgr16":
            eq(o.cpu().numpy().view(np.uint16), exp, ("per row bgr16", i))
        else:
            ey, euv = C.bgr10_to_p010(exp, BT2020L)
            eq(oy.host(np.uint16), ey, ("per row y", i)), eq(ou.host(np.uint16), euv, ("per row uv", i))
    stab.close()


def test_pipeline_refusals_leave_the_handle_unchanged(vs, cuda, clip):
    import torch
    K, Ko, cw, ch, wide = clip
    UNS, INV = vs.ERR_UNSUPPORTED, vs.ERR_INVALID
    set10 = vs.lib.vstab_set_colour10
    stab = stabilizer(vs, cuda, wide[:5], True)
    stab.set_colour10(*BT709F)
    for m, r in ((-1, 0), (4, 0), (2, 2), (1, -1), (C.CVTCOLOR, C.FULL)):
        assert set10(stab._h, m, r) == INV and vs.lib.vstab_last_error().decode().startswith("vstab_set_colour10: ")
    assert set10(None, C.BT709, C.LIMITED) == INV
    # vstab_set_colour keeps refusing a 10-bit handle, and changes nothing
    assert vs.lib.vstab_set_colour(stab._h, C.BT2020, C.LIMITED) == UNS and b"a pixel_depth 10 handle" in vs.lib.vstab_last_error()
    for i in range(4):   # the spec is still BT709 full
        o = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
        assert stab.pull_bgr16_into(o)
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        eq(o.cpu().numpy().view(np.uint16), C.warp_p010(wide[i + 1][:H], wide[i + 1][H:], p, cw, ch, BT709F), ("after refusals", i))
    stab.close()
    # an 8-bit handle is vstab_set_colour's
    frames8 = [torch.from_numpy((x >> 8).astype(np.uint8)).to(cuda) for x in wide[:4]]
    ref, st8 = (vs.Stabilizer(frames8, total=4, smooth_radius=1, tracking=0) for _ in range(2))
    for spec in C.SPECS:
        assert set10(st8._h, *spec) == UNS
        assert vs.lib.vstab_last_error().decode() == "vstab_set_colour10: served for pixel_depth 10 handles; the colour spec of an 8-bit handle is set with vstab_set_colour"
    assert set10(st8._h, 7, 0) == INV
    eq(st8.pull().cpu().numpy(), ref.pull().cpu().numpy(), "8-bit handle unchanged")
    ref.close(), st8.close()
