"""The colour matrix and range of the BGR path, without a device (include/vstab.h "Colour matrix and range"; tests/colour_def.py).

1. vstab_colour_coefficients against the table of the issue (literals below), against colour_def's derivation with fractions.Fraction,
   and its cvtColor row against the constants of csrc/vstab_device.hpp.
2. colour_def at (CVTCOLOR, LIMITED) against the oracle's cvtColor restatements, bit for bit, on full-range frames.
3. Invariants of every spec: grey, the range end points, the cube corners through the inverse with the saturating case reached.
4. Every refusal that is made before a device is touched (the pointers are a dummy address a refused call never dereferences).
5. The known-answer vectors of tests/golden/colour_kat.npz."""
import ctypes
import os
import re

import numpy as np
import pytest

import colour_def as C
import oracle
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
P = 4096  # a non-null dummy address, 16-byte aligned

# forward CY, CUB, CUG, CVG, CVR; inverse CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV
TABLE = {
    (C.BT601, C.LIMITED): ((1220945, 2115221, -410793, -852458, 1673555), (269262, 528618, 102662, -155423, -305128, 460551, -385654, -74897)),
    (C.BT601, C.FULL): ((1048576, 1858077, -360853, -748826, 1470104), (313524, 615514, 119538, -176932, -347356, 524288, -439026, -85262)),
    (C.BT709, C.LIMITED): ((1220945, 2215014, -223607, -558796, 1879825), (191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230)),
    (C.BT709, C.FULL): ((1048576, 1945738, -196424, -490864, 1651297), (222927, 749942, 75707, -120138, -404150, 524288, -476214, -48074)),
    (C.BT2020, C.LIMITED): ((1220945, 2245811, -196426, -682019, 1760217), (236572, 610567, 53402, -128614, -331937, 460551, -423510, -37041)),
    (C.BT2020, C.FULL): ((1048576, 1972791, -172546, -599107, 1546230), (275461, 710935, 62181, -146413, -377875, 524288, -482120, -42168)),
}
DERIVED = sorted(TABLE)
IDS = [C.NAMES[s] for s in C.SPECS]


# ---- 1. the coefficient table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", DERIVED, ids=[C.NAMES[s] for s in DERIVED])
def test_coefficients_equal_the_table(vs, spec):
    got = [int(v) for v in vs.colour_coefficients(*spec)]
    fwd, inv = TABLE[spec]
    assert tuple(got[:5]) == fwd and got[5] == (16 if spec[1] == C.LIMITED else 0) and tuple(got[6:]) == inv


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_coefficients_equal_the_fraction_derivation(vs, spec):
    assert tuple(int(v) for v in vs.colour_coefficients(*spec)) == tuple(C.coefficients(*spec))


def test_cvtcolor_row_is_the_header_constants(vs):
    text = open(os.path.join(os.path.dirname(HERE), "video-annotator_amd", "csrc", "vstab_device.hpp")).read()
    consts = {}
    for line in re.findall(r"^constexpr int (C[A-Z]+ = [^;]+);", text, re.M):
        for name, val in re.findall(r"(C[A-Z]+) = (-?\d+)", line):
            consts[name] = int(val)
    names = ("CY", "CUB", "CUG", "CVG", "CVR", None, "CRY", "CGY", "CBY", "CRU", "CGU", "CBU", "CGV", "CBV")
    got = [int(v) for v in vs.colour_coefficients(C.CVTCOLOR, C.LIMITED)]
    assert got[5] == 16
    assert [got[i] for i, n in enumerate(names) if n] == [consts[n] for n in names if n]
    assert tuple(got) == C.CVTCOLOR_ROW


def test_bounds_hold_for_every_spec():
    """int32 forward sums below 5.8e8, coefficients below 2^23 (the kernels' 24-bit multiplies)"""
    for spec in C.SPECS:
        k = C.coefficients(*spec)
        cy, cub, cug, cvg, cvr, yoff = k[:6]
        assert all(abs(v) < (1 << 23) for v in k)
        luma = (255 - yoff) * cy + (1 << 19)
        worst = max(luma + 128 * abs(cub), luma + 128 * abs(cvr), luma + 128 * (abs(cvg) + abs(cug)), 128 * abs(cub), 128 * abs(cvr))
        assert worst < 5.8e8, (spec, worst)


# ---- 2. the default spec is the oracle's cvtColor ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(2, 2), (66, 34), (258, 130)])
def test_default_spec_is_the_oracle(w, h):
    f = synth.nv12(11, w, h, full_range=True)
    bgr = oracle.cvt_nv12_bgr(f)
    assert np.array_equal(C.nv12_to_bgr(f, (C.CVTCOLOR, C.LIMITED)), bgr)
    rnd = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for img in (bgr, rnd):
        y, uv = oracle.cvt_bgr_nv12(img)
        gy, guv = C.bgr_to_nv12(img, (C.CVTCOLOR, C.LIMITED))
        assert np.array_equal(gy, y) and np.array_equal(guv, uv)


# ---- 3. invariants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_grey_and_range_end_points(spec):
    Y = np.arange(256)
    bgr = C.yuv_to_bgr(Y, np.full(256, 128), np.full(256, 128), spec)
    assert np.array_equal(bgr[:, 0], bgr[:, 1]) and np.array_equal(bgr[:, 1], bgr[:, 2])   # U = V = 128: B = G = R
    if spec[1] == C.FULL:
        assert np.array_equal(bgr[:, 0], Y)                                                  # full range: grey Y maps to itself
    else:
        assert bgr[16, 0] == 0 and bgr[235, 0] == 255 and np.all(bgr[:16] == 0) and np.all(bgr[235:] == 255)


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_cube_corners_through_the_inverse(spec):
    raw = C.bgr_to_yuv_unsaturated(C.CUBE_CORNERS, spec)
    y, uv = C.bgr_to_nv12(C.cube_corner_frame(), spec)
    assert np.array_equal(y[0, ::2], np.clip(raw[:, 0], 0, 255)) and np.array_equal(uv[0], np.clip(raw[:, 1:], 0, 255))
    lo, hi = (16, 235) if spec[1] == C.LIMITED else (0, 255)
    assert raw[0, 0] == lo and raw[7, 0] == hi and tuple(raw[0, 1:]) == (128, 128) and tuple(raw[7, 1:]) == (128, 128)   # black, white
    if spec[1] == C.FULL:
        # pure blue (B = 255, G = R = 0) has U = 128 + 255 / 2 -> 256 before the saturation, pure red V likewise: the saturation acts
        assert raw[4, 1] == 256 and raw[1, 2] == 256 and raw[:, 1:].max() == 256
        assert uv[0, 4, 0] == 255 and uv[0, 1, 1] == 255
    else:
        assert raw.min() >= 0 and raw.max() <= 255
        assert raw[4, 1] == 240 and raw[1, 2] == 240                                         # limited range: chroma ends at 240


# ---- 4. refusals without a device -------------------------------------------------------------------------------------------------
BAD_SPECS = [(-1, 0, "matrix must be VSTAB_COLOUR_CVTCOLOR (0), _BT601 (1), _BT709 (2) or _BT2020 (3)"),
             (4, 0, "matrix must be VSTAB_COLOUR_CVTCOLOR (0), _BT601 (1), _BT709 (2) or _BT2020 (3)"),
             (4, 7, "matrix must be VSTAB_COLOUR_CVTCOLOR (0), _BT601 (1), _BT709 (2) or _BT2020 (3)"),
             (2, 2, "range must be VSTAB_RANGE_LIMITED (0) or VSTAB_RANGE_FULL (1)"),
             (1, -1, "range must be VSTAB_RANGE_LIMITED (0) or VSTAB_RANGE_FULL (1)"),
             (0, 1, "VSTAB_COLOUR_CVTCOLOR is cvtColor's limited-range arithmetic; full range needs a matrix (BT601, BT709, BT2020)")]


def _refused(vs, fn, args, status, text):
    st = getattr(vs.lib, fn)(*args)
    assert st == status, (fn, st, vs.lib.vstab_last_error().decode())
    assert vs.lib.vstab_last_error().decode() == text


@pytest.mark.parametrize("matrix,rng,what", BAD_SPECS)
def test_bad_spec_is_refused_everywhere(vs, matrix, rng, what):
    out = (ctypes.c_int32 * 14)(*([7] * 14))
    _refused(vs, "vstab_colour_coefficients", (matrix, rng, out), vs.ERR_INVALID, "vstab_colour_coefficients: " + what)
    assert list(out) == [7] * 14
    _refused(vs, "vstab_cvt_nv12_bgr_colour", (P, 64, P, 64, 64, 32, P, 192, matrix, rng, None), vs.ERR_INVALID, "vstab_cvt_nv12_bgr_colour: " + what)
    _refused(vs, "vstab_cvt_bgr_nv12_colour", (P, 192, 64, 32, P, 64, P, 64, matrix, rng, None), vs.ERR_INVALID, "vstab_cvt_bgr_nv12_colour: " + what)
    fp = np.zeros(17, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    _refused(vs, "vstab_warp_nv12_colour", (P, 64, P, 64, 64, 32, fp, 0, 0, P, 192, None, 0, 32, 16, matrix, rng, None), vs.ERR_INVALID,
             "vstab_warp_nv12_colour: " + what)
    _refused(vs, "vstab_set_colour", (None, matrix, rng), vs.ERR_INVALID, "vstab_set_colour: null handle")


def test_coefficients_null_pointer(vs):
    _refused(vs, "vstab_colour_coefficients", (C.BT709, C.LIMITED, None), vs.ERR_INVALID, "vstab_colour_coefficients: null pointer")


def test_set_colour_null_handle(vs):
    _refused(vs, "vstab_set_colour", (None, C.BT709, C.LIMITED), vs.ERR_INVALID, "vstab_set_colour: null handle")


CVT_FWD = dict(y=P, pitch_y=64, uv=P, pitch_uv=64, w=64, h=32, dst=P, pitch_dst=192, matrix=C.BT709, rng=C.LIMITED, stream=None)
CVT_INV = dict(src=P, pitch=192, w=64, h=32, dst_y=P, pitch_y=64, dst_uv=P, pitch_uv=64, matrix=C.BT709, rng=C.FULL, stream=None)


@pytest.mark.parametrize("fn,good,change,what", [
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(y=None), "null pointer"),
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(uv=None), "null pointer"),
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(dst=None, w=63), "null pointer"),
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(w=63), "width and height must be even"),
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(h=0), "width and height must be even"),
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(pitch_y=63), "pitch smaller than row"),
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(pitch_uv=62), "pitch smaller than row"),
    ("vstab_cvt_nv12_bgr_colour", CVT_FWD, dict(pitch_dst=191), "pitch smaller than row"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(src=None), "null pointer"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(dst_y=None), "null pointer"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(dst_uv=None, h=31), "null pointer"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(h=31), "width and height must be even"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(w=-2), "width and height must be even"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(pitch=191), "pitch smaller than row"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(pitch_y=63), "pitch smaller than row"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(pitch_uv=62, dst_uv=P + 1), "pitch smaller than row"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(dst_uv=P + 1), "chroma plane must be 2-B aligned"),
    ("vstab_cvt_bgr_nv12_colour", CVT_INV, dict(pitch_uv=65), "chroma plane must be 2-B aligned"),
])
def test_converter_refusals(vs, fn, good, change, what):
    _refused(vs, fn, tuple(dict(good, **change).values()), vs.ERR_INVALID, fn + ": " + what)


def _warp_args(**change):
    fp = np.zeros(17, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    good = dict(y=P, pitch_y=64, uv=P, pitch_uv=64, sw=64, sh=32, params=fp, map_mode=0, out_format=0, dst=P, pitch_dst=192, dst_uv=None, pitch_dst_uv=0,
                dw=32, dh=16, matrix=C.BT709, rng=C.LIMITED, stream=None)
    return tuple(dict(good, **change).values())


def test_warp_refusals(vs):
    n, c = "vstab_warp_nv12: ", "vstab_warp_nv12_colour: "
    planar = dict(out_format=2, pitch_dst=32, dst_uv=P, pitch_dst_uv=32)
    rows = [
        (dict(y=None), vs.ERR_INVALID, n + "null pointer"),                        # the bilinear entry points' checks, under their name
        (dict(sw=63), vs.ERR_INVALID, n + "source must be even-sized and <= 32767"),
        (dict(map_mode=6), vs.ERR_INVALID, n + "unknown map mode"),
        (dict(out_format=3), vs.ERR_INVALID, n + "unknown output format"),
        (dict(pitch_dst=95), vs.ERR_INVALID, n + "pitch smaller than row"),
        (dict(out_format=1, pitch_dst=32), vs.ERR_INVALID, n + "NV12 output needs a chroma plane of 2*ceil(width/2) bytes per row"),
        (dict(pitch_dst=95, matrix=9), vs.ERR_INVALID, n + "pitch smaller than row"),   # the spec is checked behind them
        (planar, vs.ERR_INVALID, c + "VSTAB_OUT_NV12_PLANAR converts nothing, a colour spec belongs to VSTAB_OUT_BGR8 and VSTAB_OUT_NV12"),
        (dict(planar, rng=C.FULL), vs.ERR_INVALID, c + "VSTAB_OUT_NV12_PLANAR converts nothing, a colour spec belongs to VSTAB_OUT_BGR8 and VSTAB_OUT_NV12"),
        # planes of 4 GiB and more (a pitch a 24-bit multiply cannot take; pitch * height past 2^32): the direct-gather kernel has cvtColor's constants
        (dict(pitch_y=1 << 24), vs.ERR_UNSUPPORTED, c + "source planes of 4 GiB and more are served with (VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED) only"),
        (dict(pitch_y=1 << 23, pitch_uv=1 << 23, sh=512, out_format=1, pitch_dst=32, dst_uv=P, pitch_dst_uv=32, matrix=C.BT601, rng=C.FULL), vs.ERR_UNSUPPORTED,
         c + "source planes of 4 GiB and more are served with (VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED) only"),
    ]
    for change, status, text in rows:
        _refused(vs, "vstab_warp_nv12_colour", _warp_args(**change), status, text)


# ---- 5. known answers ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "colour_kat.npz"))


@pytest.mark.parametrize("spec", C.SPECS, ids=IDS)
def test_known_answers(kat, spec):
    name = C.NAMES[spec]
    for k in range(4):
        assert np.array_equal(C.nv12_to_bgr(kat[f"nv12_{k}"], spec), kat[f"fwd_{k}_{name}"]), (name, "forward", k)
        assert np.array_equal(C.pack(*C.bgr_to_nv12(kat[f"bgr_{k}"], spec)), kat[f"inv_{k}_{name}"]), (name, "inverse", k)
