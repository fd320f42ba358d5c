"""The colour matrix and range of the 10-bit path, without a device (include/vstab.h "Colour matrix and range at 10 bits";
tests/colour10_def.py).

1. vstab_colour_coefficients10 against the seven rows as literals and against colour10_def's derivation with fractions.Fraction.
2. The overflow argument of the header and of channel10 (csrc/vstab_device10.hpp), recomputed from the table.
3. colour10_def at (CVTCOLOR, LIMITED) against the oracle: both converters and the warp, both blends.
4. End points of every spec: the range ends, grey, the cube corners through the inverse with the unsaturated 1024 reached.
5. Every refusal that is made before a device is touched (the pointers are a dummy address a refused call never dereferences).
6. The known-answer vectors of tests/golden/colour10_kat.npz."""
import ctypes
import os

import numpy as np
import pytest

import colour10_def as C
import oracle
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
P = 4096  # a non-null dummy address, 16-byte aligned

# CY, CUB, CUG, CVG, CVR, yoff, CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV
TABLE = {
    (C.CVTCOLOR, C.LIMITED): (1220542, 2116026, -409993, -852492, 1673527, 64, 269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448),
    (C.BT601, C.LIMITED): (1224536, 2121442, -412001, -854966, 1678478, 64, 268472, 527068, 102361, -154967, -304233, 459200, -384523, -74677),
    (C.BT601, C.FULL): (1048576, 1858077, -360853, -748826, 1470104, 0, 313524, 615514, 119538, -176932, -347356, 524288, -439026, -85262),
    (C.BT709, C.LIMITED): (1224536, 2221529, -224265, -560439, 1885354, 64, 190894, 642179, 64828, -105223, -353977, 459200, -417094, -42106),
    (C.BT709, C.FULL): (1048576, 1945738, -196424, -490864, 1651297, 0, 222927, 749942, 75707, -120138, -404150, 524288, -476214, -48074),
    (C.BT2020, C.LIMITED): (1224536, 2252416, -197003, -684025, 1765394, 64, 235879, 608777, 53246, -128236, -330964, 459200, -422268, -36933),
    (C.BT2020, C.FULL): (1048576, 1972791, -172546, -599107, 1546230, 0, 275461, 710935, 62181, -146413, -377875, 524288, -482120, -42168),
}
IDS = [C.NAMES[s] for s in C.SPECS]


# ---- 1. the coefficient table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_coefficients10_equal_the_table(vs, spec):
    assert tuple(int(v) for v in vs.colour_coefficients10(*spec)) == TABLE[spec]


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_coefficients10_equal_the_fraction_derivation(vs, spec):
    assert tuple(int(v) for v in vs.colour_coefficients10(*spec)) == tuple(C.coefficients(*spec))


def test_default_row_is_the_8bit_cvtcolor_row_with_yoff_64(vs):
    a, b = [int(v) for v in vs.colour_coefficients(C.CVTCOLOR, C.LIMITED)], [int(v) for v in vs.colour_coefficients10(C.CVTCOLOR, C.LIMITED)]
    assert a[5] == 16 and b[5] == 64 and a[:5] == b[:5] and a[6:] == b[6:]


def test_the_8bit_table_is_unchanged(vs):
    import colour_def
    for spec in colour_def.SPECS:
        assert tuple(int(v) for v in vs.colour_coefficients(*spec)) == tuple(colour_def.coefficients(*spec))


# ---- 2. the overflow argument -----------------------------------------------------------------------------------------------------
def test_overflow_bounds(vs):
    """The header's figures, from the library's own table: coefficients below 2^23; the luma term and every folded chroma term in int32;
    their sum past 2^31 only where the channel saturates; inverse sums at most 2^30."""
    i32 = (1 << 31) - 1
    luma_max, lo, hi, plain_max, sum_max, sum_min, inv_max, inv_min = 0, 0, 0, 0, 0, 0, 0, 1 << 40
    for spec in C.SPECS:
        k = [int(v) for v in vs.colour_coefficients10(*spec)]
        cy, cub, cug, cvg, cvr, yoff, cry, cgy, cby, cru, cgu, cbu, cgv, cbv = k
        assert all(abs(v) < (1 << 23) for v in k), spec
        K = (1 << 19) - yoff * cy
        luma_max = max(luma_max, 1023 * cy)
        for u in (-512, 511):
            for v in (-512, 511):
                plain = ((1 << 19) + cvr * v, (1 << 19) + cvg * v + cug * u, (1 << 19) + cub * u)
                folded = (K + cvr * v, K + cvg * v + cug * u, K + cub * u)
                lo, hi, plain_max = min(lo, *folded), max(hi, *folded), max(plain_max, *(abs(t) for t in plain))
                # the largest luma term beside each chroma term (folded: max(y, yoff) * CY; plain: max(y - yoff, 0) * CY: the same sums)
                sum_max = max(sum_max, *(1023 * cy + t for t in folded))
                sum_min = min(sum_min, *(yoff * cy + t for t in folded))
        inv_max = max(inv_max, 1023 * (cry + cgy + cby) + (1 << 19) + (yoff << 20), 1023 * cbu + (1 << 19) + (512 << 20))
        inv_min = min(inv_min, 1023 * (cru + cgu) + (1 << 19) + (512 << 20), 1023 * (cgv + cbv) + (1 << 19) + (512 << 20), (1 << 19) + (yoff << 20))
    assert max(abs(v) for row in TABLE.values() for v in row) == 2252416
    assert luma_max == 1252700328 and luma_max <= 1.2527e9 + 1e5 and luma_max <= i32
    assert lo == -1231083008 and hi == 1073138560 and -i32 - 1 <= lo and hi <= i32       # the folded terms: [-1.2311e9, 1.0732e9]
    assert plain_max <= 1.1538e9 and plain_max <= i32                                      # the unfolded ones of the direct-gather kernel: 2^19 + C uv
    assert sum_max == 2325838888 and sum_max > i32                                         # 2.3259e9, BT2020 limited: the one sum past 2^31
    assert (i32 + 1) >> 20 == 2048 and i32 >> 20 == 2047                                   # a sum past INT_MAX is a channel >= 2048; the saturated add gives 2047: both -> 1023
    assert sum_min >= -1.24e9 and sum_min >= -i32 - 1
    assert inv_max == 1 << 30 and inv_min >= 0


# ---- 3. the default spec is the oracle's 10-bit path -----------------------------------------------------------------------------
def _p010(seed, w, h):
    """a picture (synth.nv12, full range) widened to P010 words, with two more bits of detail and junk in the low six"""
    f = synth.nv12(seed, w, h, full_range=True).astype(np.uint16)
    rng = np.random.default_rng(seed)
    wide = (f << 8) | (rng.integers(0, 4, f.shape).astype(np.uint16) << 6) | rng.integers(0, 64, f.shape).astype(np.uint16)
    return wide[:h], wide[h:]


def test_default_spec_is_the_oracle_converters():
    w, h = 66, 34
    for y, uv in (_p010(3, w, h), C.extremes_frame(w, h)):
        bgr = oracle.cvt_p010_bgr10(y, uv)
        assert np.array_equal(C.p010_to_bgr10(y, uv, C.DEFAULT), bgr)
        rnd = np.random.default_rng(5).integers(0, 1024, (h, w, 3)).astype(np.uint16)
        for img in (bgr, rnd, rnd[:33, :65]):
            ey, euv = oracle.cvt_bgr10_p010(img)
            gy, guv = C.bgr10_to_p010(img, C.DEFAULT)
            assert np.array_equal(gy, ey) and np.array_equal(guv, euv)


@pytest.mark.parametrize("blend", [0, 1], ids=["exact", "fp16"])
def test_default_spec_is_the_oracle_warp(blend):
    w, h = 66, 34
    y, uv = _p010(4, w, h)
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, w, h)
    Ko, (dw, dh) = oracle.get_output_camera(K, w, h)
    p = oracle.map_params(K, Ko, oracle.rodrigues([0.02, -0.03, 0.01]))
    rb = np.asarray(oracle.rodrigues([0.03, -0.02, 0.02]), np.float32).reshape(9)
    for mode in (0, 2):
        assert np.array_equal(C.warp_p010(y, uv, p, dw, dh, C.DEFAULT, mode=mode, blend=blend), oracle.warp_p010(y, uv, p, dw, dh, mode=mode, blend=blend))
    assert np.array_equal(C.warp_p010(y, uv, p, dw, dh, C.DEFAULT, rot_bottom=rb, blend=blend), oracle.warp_p010(y, uv, p, dw, dh, rot_bottom=rb, blend=blend))


# ---- 4. end points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_grey_and_range_end_points(spec):
    Y = np.arange(1024)
    bgr = C.yuv10_to_bgr10(Y, np.full(1024, 512), np.full(1024, 512), spec)
    assert np.array_equal(bgr[:, 0], bgr[:, 1]) and np.array_equal(bgr[:, 1], bgr[:, 2])   # neutral chroma: B = G = R
    if spec[1] == C.FULL:
        assert bgr[0, 0] == 0 and bgr[1023, 0] == 1023 and np.array_equal(bgr[:, 0], Y)      # full range: grey Y maps to itself
    elif spec == C.DEFAULT:
        assert bgr[64, 0] == 0 and bgr[940, 0] == 1020                                      # the 8-bit constants: white lands on 1020 (the issue's second bullet)
    else:
        assert bgr[64, 0] == 0 and bgr[940, 0] == 1023 and np.all(bgr[:64] == 0) and np.all(bgr[940:] == 1023)
        assert bgr[939, 0] == 1022


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_cube_corners_through_the_inverse(spec):
    raw = C.bgr10_to_yuv_unsaturated(C.CUBE_CORNERS, spec)
    y, uv = C.bgr10_to_p010(C.cube_corner_frame(), spec)
    assert np.array_equal(y[0, ::2], np.clip(raw[:, 0], 0, 1023) << 6) and np.array_equal(uv[0].reshape(8, 2), np.clip(raw[:, 1:], 0, 1023) << 6)
    assert tuple(raw[0, 1:]) == (512, 512) and tuple(raw[7, 1:]) == (512, 512)             # black and white are neutral
    if spec[1] == C.FULL:
        # pure blue (B = 1023, G = R = 0) has U = 512 + 1023 / 2 -> 1024 before the saturation, pure red V likewise: the saturation acts
        assert raw[0, 0] == 0 and raw[7, 0] == 1023
        assert raw[4, 1] == 1024 and raw[1, 2] == 1024 and raw[:, 1:].max() == 1024
        assert uv[0, 8] == 1023 << 6 and uv[0, 3] == 1023 << 6
    elif spec != C.DEFAULT:
        assert raw[0, 0] == 64 and raw[7, 0] == 940 and raw.min() >= 0 and raw.max() <= 1023
        assert raw[4, 1] == 960 and raw[1, 2] == 960                                         # limited range: chroma ends at 960
    else:
        assert raw[0, 0] == 64 and raw.min() >= 0 and raw.max() <= 1023


# ---- 5. refusals without a device -------------------------------------------------------------------------------------------------
M = "matrix must be VSTAB_COLOUR_CVTCOLOR (0), _BT601 (1), _BT709 (2) or _BT2020 (3)"
R = "range must be VSTAB_RANGE_LIMITED (0) or VSTAB_RANGE_FULL (1)"
BAD_SPECS = [(-1, 0, M), (4, 0, M), (4, 7, M), (2, 2, R), (1, -1, R),
             (0, 1, "VSTAB_COLOUR_CVTCOLOR is cvtColor's limited-range arithmetic; full range needs a matrix (BT601, BT709, BT2020)")]


def _refused(vs, fn, args, status, text):
    st = getattr(vs.lib, fn)(*args)
    assert st == status, (fn, st, vs.lib.vstab_last_error().decode())
    assert vs.lib.vstab_last_error().decode() == text


def _fp():
    return np.zeros(17, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _warp(**change):  # vstab_warp_p010_colour: 64 x 32 -> 32 x 16
    good = dict(y=P, pitch_y=128, uv=P, pitch_uv=128, sw=64, sh=32, params=_fp(), rot_bottom=None, map_mode=0, blend=0, dst=P, pitch_dst=192, dw=32, dh=16,
                matrix=C.BT2020, rng=C.LIMITED, stream=None)
    return tuple(dict(good, **change).values())


def _planes(**change):  # vstab_warp_p010_planes_colour
    good = dict(y=P, pitch_y=128, uv=P, pitch_uv=128, sw=64, sh=32, params=_fp(), rot_bottom=None, map_mode=0, blend=0, dst_y=P, pitch_dst_y=64, dst_uv=P,
                pitch_dst_uv=64, dw=32, dh=16, matrix=C.BT2020, rng=C.LIMITED, stream=None)
    return tuple(dict(good, **change).values())


FWD = dict(y=P, pitch_y=128, uv=P, pitch_uv=128, w=64, h=32, dst=P, pitch_dst=384, matrix=C.BT709, rng=C.LIMITED, stream=None)
INV = dict(src=P, pitch=384, w=64, h=32, dst_y=P, pitch_y=128, dst_uv=P, pitch_uv=128, matrix=C.BT709, rng=C.FULL, stream=None)


@pytest.mark.parametrize("matrix,rng,what", BAD_SPECS)
def test_bad_spec_is_refused_everywhere(vs, matrix, rng, what):
    out = (ctypes.c_int32 * 14)(*([7] * 14))
    _refused(vs, "vstab_colour_coefficients10", (matrix, rng, out), vs.ERR_INVALID, "vstab_colour_coefficients10: " + what)
    assert list(out) == [7] * 14
    for fn, args in (("vstab_warp_p010_colour", _warp(matrix=matrix, rng=rng)), ("vstab_warp_p010_planes_colour", _planes(matrix=matrix, rng=rng)),
                     ("vstab_cvt_p010_bgr16_colour", tuple(dict(FWD, matrix=matrix, rng=rng).values())),
                     ("vstab_cvt_bgr16_p010_colour", tuple(dict(INV, matrix=matrix, rng=rng).values()))):
        _refused(vs, fn, args, vs.ERR_INVALID, fn + ": " + what)
    _refused(vs, "vstab_set_colour10", (None, matrix, rng), vs.ERR_INVALID, "vstab_set_colour10: null handle")


def test_null_pointer_and_null_handle(vs):
    _refused(vs, "vstab_colour_coefficients10", (C.BT709, C.LIMITED, None), vs.ERR_INVALID, "vstab_colour_coefficients10: null pointer")
    _refused(vs, "vstab_set_colour10", (None, C.BT709, C.LIMITED), vs.ERR_INVALID, "vstab_set_colour10: null handle")


def test_warp_refusals_are_the_twins_under_the_own_name(vs):
    n = "vstab_warp_p010_colour: "
    bad = "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"
    rows = [(dict(y=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(sw=63), "sizes must be in [1, 32767], source even and at least 4 x 2"),
            (dict(dw=0), "sizes must be in [1, 32767], source even and at least 4 x 2"), (dict(pitch_y=126), bad), (dict(uv=P + 2), bad), (dict(pitch_dst=190), bad),
            (dict(map_mode=9), "unknown map mode"), (dict(blend=5), "unknown blend"),
            (dict(blend=5, matrix=9), "unknown blend"), (dict(pitch_y=126, rng=4), bad)]   # the spec is checked behind them
    for change, text in rows:
        _refused(vs, "vstab_warp_p010_colour", _warp(**change), vs.ERR_INVALID, n + text)
    n = "vstab_warp_p010_planes_colour: "
    out_bad = "bad output pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"
    rows = [(dict(dst_uv=None), vs.ERR_INVALID, "null pointer"), (dict(sw=6), vs.ERR_INVALID, "sizes must be in [1, 32767], source even and at least 8 x 2"),
            (dict(pitch_dst_y=62), vs.ERR_INVALID, out_bad), (dict(dst_uv=P + 2), vs.ERR_INVALID, out_bad), (dict(blend=2), vs.ERR_INVALID, "unknown blend"),
            # what the tiled kernel cannot take is VSTAB_ERR_UNSUPPORTED, as from the twin, and in front of the spec
            (dict(y=P + 2), vs.ERR_UNSUPPORTED, "needs 16-byte aligned source planes and a fisheye -> pinhole map"),
            (dict(pitch_uv=132), vs.ERR_UNSUPPORTED, "needs 16-byte aligned source planes and a fisheye -> pinhole map"),
            (dict(map_mode=2), vs.ERR_UNSUPPORTED, "needs 16-byte aligned source planes and a fisheye -> pinhole map"),
            (dict(map_mode=2, matrix=7), vs.ERR_UNSUPPORTED, "needs 16-byte aligned source planes and a fisheye -> pinhole map")]
    for change, status, text in rows:
        _refused(vs, "vstab_warp_p010_planes_colour", _planes(**change), status, n + text)
    # the twins themselves say the same under their names
    _refused(vs, "vstab_warp_p010_planes", _planes(map_mode=2)[:-3] + (None,), vs.ERR_UNSUPPORTED, "vstab_warp_p010_planes: needs 16-byte aligned source planes and a fisheye -> pinhole map")
    _refused(vs, "vstab_warp_p010", _warp(blend=5)[:-3] + (None,), vs.ERR_INVALID, "vstab_warp_p010: unknown blend")


@pytest.mark.parametrize("fn,good,change,what", [
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(y=None), "null pointer"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(uv=None), "null pointer"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(dst=None, w=63), "null pointer"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(w=63), "sizes must be even and in [2, 32767]"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(h=0), "sizes must be even and in [2, 32767]"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(w=32768), "sizes must be even and in [2, 32767]"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(pitch_y=126), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(pitch_uv=130), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(uv=P + 2), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(y=P + 1), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(pitch_dst=382), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_p010_bgr16_colour", FWD, dict(dst=P + 1), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(src=None), "null pointer"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(dst_uv=None, w=0), "null pointer"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(w=0), "sizes must be in [1, 32767]"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(h=32768), "sizes must be in [1, 32767]"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(pitch=382), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(pitch_uv=126), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(dst_uv=P + 2), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
    ("vstab_cvt_bgr16_p010_colour", INV, dict(pitch_y=126, matrix=11), "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"),
])
def test_converter_refusals(vs, fn, good, change, what):
    _refused(vs, fn, tuple(dict(good, **change).values()), vs.ERR_INVALID, fn + ": " + what)


# ---- 6. known answers ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "colour10_kat.npz"))


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_known_answers(kat, spec):
    name = C.NAMES[spec]
    for k in range(2):
        assert np.array_equal(C.p010_to_bgr10(kat[f"y_{k}"], kat[f"uv_{k}"], spec), kat[f"fwd_{k}_{name}"]), (name, "forward", k)
        y, uv = C.bgr10_to_p010(kat[f"bgr_{k}"], spec)
        assert np.array_equal(y, kat[f"invy_{k}_{name}"]) and np.array_equal(uv, kat[f"invuv_{k}_{name}"]), (name, "inverse", k)
