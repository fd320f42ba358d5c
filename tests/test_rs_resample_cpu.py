"""CPU tests of vstab_warp_nv12_rs_ex's definition (tests/warp_def.py) and of what the entry point decides before any device work:
the two anchors of the per-row distorted map, every refusal in its order with its whole message, the tile states the GPU cases are
committed to reach, and the known-answer file."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import distort_def as dd
import oracle
import warp_def as wd
import warp_tiles as wt

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the per-row distorted map against the two statements it must meet
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anchor():
    return wd.case_params(128, 72, 300, 170, 60.0, 40.0) + (300, 170)


def test_zero_distortion_is_the_oracles_per_row_map(anchor):
    p, rb, dw, dh = anchor
    got, exp = wd.maps(p, dw, dh, 1, rb, dd.D_0), oracle.create_map_rs(p, rb, dw, dh, 1)
    assert np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(bits(got[1]), bits(exp[1]))
    plain = oracle.create_map_ex(p, dw, dh, 1)
    assert not np.array_equal(bits(got[0]), bits(plain[0]))            # the rotation per row moves the map


def test_one_rotation_is_the_distorted_map(anchor):
    p, _, dw, dh = anchor
    got, exp = wd.maps(p, dw, dh, 1, np.asarray(p[8:], np.float32), dd.D_A), dd.maps(p, dw, dh, 1, dd.D_A)
    assert np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(bits(got[1]), bits(exp[1]))


def test_fma_rounds_once():
    F = np.float32
    a, b, c = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12), F(-1.0)              # a * b = 1 + 2^-11 + 2^-24: the last bit is lost to a rounded product
    assert wd.fma_f32(a, b, c) == F(2.0 ** -11 + 2.0 ** -24) != a * b + c
    # a tie that a sum rounded to double first would break the wrong way: 1 + 2^-24 + 2^-60 is above the halfway point
    assert wd.round_f32(1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)) == F(1 + 2.0 ** -23)
    assert wd.round_f32(1 + Fraction(1, 2 ** 24)) == F(1.0)        # the tie itself: to even
    m = wd.row_matrices(np.arange(17, dtype=F), np.arange(9, dtype=F) + 9, 1)
    assert np.array_equal(m[0], np.arange(8, 17, dtype=F))             # one row: t = 0, the first row's rotation


# ---------------------------------------------------------------------------------------------------------------------
# refusals: before any device work (dummy pointers), in their order, whole messages
# ---------------------------------------------------------------------------------------------------------------------
P = 4096
_params, _rot = np.zeros(17, np.float32), np.zeros(9, np.float32)
FP = _params.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
RB = _rot.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
_good_d, _bad_d, _nan_d = np.array(dd.D_A, np.float32), np.array([-0.5, 0, 0, 0], np.float32), np.array([np.nan, 0, 0, 0], np.float32)
DP, DBAD, DNAN = (d.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for d in (_good_d, _bad_d, _nan_d))
BGR8, NV12, PLANAR = 0, 1, 2
GOOD = dict(y=P, pitch_y=64, uv=P, pitch_uv=64, sw=64, sh=32, params=FP, rot_bottom=RB, dist=None, map_mode=1, resample=2, border_mode=0, out_format=BGR8,
            dst=P, pitch_dst=192, dst_uv=None, pitch_dst_uv=0, dw=32, dh=16, stream=None)
N = "vstab_warp_nv12_rs_ex: "
NULL, SRC, OUT, MODE = N + "null pointer", N + "source must be even-sized and <= 32767", N + "output size must be in [1, 32767]", N + "unknown map mode"
PER_ROW = N + "a rotation per output row (rot_bottom) is served for map modes 0, 1 and 5"
FORMAT = N + "the per-row warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)"
BORDER = N + "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)"
PITCH, CHROMA_PLANE = N + "pitch smaller than row", N + "plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row"
ALIGN = N + "chroma plane must be 2-B aligned"
RESAMPLE = N + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)"
FISH, THETA = N + "distortion belongs to a fisheye input (map modes 1 and 2)", N + "the distortion must keep theta_d increasing on [0, pi/2]"
_PL = dict(out_format=PLANAR, pitch_dst=32, dst_uv=P, pitch_dst_uv=32)
ROWS = [
    # 1. check_warp_nv12's checks, each alone and with a later one broken too
    (dict(y=None), NULL), (dict(uv=None), NULL), (dict(dst=None), NULL), (dict(params=None), NULL), (dict(dst=None, sw=63), NULL),
    (dict(sw=0), SRC), (dict(sw=63), SRC), (dict(sh=31), SRC), (dict(sh=32768), SRC), (dict(sw=62, sh=-2, dw=0), SRC),
    (dict(dw=0), OUT), (dict(dh=0), OUT), (dict(dw=32768, pitch_dst=98304), OUT), (dict(dh=32768, map_mode=9), OUT),
    (dict(map_mode=-1), MODE), (dict(map_mode=6), MODE), (dict(map_mode=6, out_format=NV12), MODE), (dict(map_mode=7, dist=DP), MODE),
    (dict(map_mode=2), PER_ROW), (dict(map_mode=3), PER_ROW), (dict(map_mode=4), PER_ROW), (dict(map_mode=2, out_format=NV12), PER_ROW),
    (dict(map_mode=2, dist=DP), PER_ROW), (dict(map_mode=2, dist=DBAD, resample=3), PER_ROW),      # dist + rot_bottom + mode 2
    (dict(out_format=NV12), FORMAT), (dict(out_format=3), FORMAT), (dict(out_format=-1, border_mode=3), FORMAT),
    (dict(border_mode=3), BORDER), (dict(border_mode=5), BORDER), (dict(border_mode=-1, pitch_y=63), BORDER),
    (dict(pitch_y=63), PITCH), (dict(pitch_uv=62), PITCH), (dict(pitch_dst=95), PITCH), (dict(_PL, pitch_dst=31, dst_uv=None), PITCH),
    (dict(_PL, dst_uv=None), CHROMA_PLANE), (dict(_PL, pitch_dst_uv=31), CHROMA_PLANE), (dict(_PL, pitch_dst_uv=30, uv=P + 1), CHROMA_PLANE),
    (dict(uv=P + 1), ALIGN), (dict(pitch_uv=65), ALIGN), (dict(uv=P + 1, resample=1), ALIGN),
    # 2. the resampler
    (dict(resample=1), RESAMPLE), (dict(resample=3), RESAMPLE), (dict(resample=-1), RESAMPLE), (dict(resample=5, dist=DBAD, map_mode=0), RESAMPLE),
    (dict(resample=1, rot_bottom=None, dist=DP, map_mode=3), RESAMPLE),
    # 3. with dist: the map mode, then the coefficients
    (dict(dist=DP, map_mode=0), FISH), (dict(dist=DP, map_mode=5), FISH), (dict(dist=DBAD, map_mode=0), FISH),
    (dict(dist=DP, map_mode=3, rot_bottom=None), FISH), (dict(dist=DP, map_mode=4, rot_bottom=None, resample=0), FISH),
    (dict(dist=DBAD), THETA), (dict(dist=DNAN), THETA), (dict(dist=DBAD, rot_bottom=None, map_mode=2, resample=0, border_mode=4), THETA),
    (dict(_PL, dist=DBAD, resample=4, border_mode=2), THETA),
]


def test_every_refusal_in_its_order_without_a_device(vs):
    L = vs.lib
    assert {text for _, text in ROWS} == {NULL, SRC, OUT, MODE, PER_ROW, FORMAT, BORDER, PITCH, CHROMA_PLANE, ALIGN, RESAMPLE, FISH, THETA}
    for bad, text in ROWS:
        assert bad and set(bad) <= set(GOOD), bad
        got = L.vstab_warp_nv12_rs_ex(*dict(GOOD, **bad).values())
        assert got == vs.ERR_INVALID, (bad, got, L.vstab_last_error())
        assert L.vstab_last_error() == text.encode(), (bad, L.vstab_last_error())


def test_set_readout_warp_refuses_a_null_handle_without_a_device(vs):
    assert vs.lib.vstab_set_readout_warp(None, vs.READOUT_PER_ROW) == vs.ERR_INVALID
    assert vs.lib.vstab_last_error() == b"vstab_set_readout_warp: null handle"
    assert (vs.READOUT_REFUSE, vs.READOUT_PER_ROW) == (0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the tile states the GPU cases reach (modes 0 and 1: the oracle's C statement; mode 5's map needs the GPU)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoomed_out():
    sw, sh, dw, dh, fi, fo = wd.ZOOMED_OUT
    p, rb = wd.case_params(sw, sh, dw, dh, fi, fo)
    return {mode: (wd.maps(p, dw, dh, mode, rb), wd.maps(p, dw, dh, mode, None)) for mode in (0, 1)}


@pytest.mark.parametrize("mode", [0, 1])
def test_zoomed_out_tile_states(zoomed_out, mode):
    sw, sh, dw, dh = wd.ZOOMED_OUT[:4]
    (mx, my), (zx, zy) = zoomed_out[mode]
    q, z = wd.quantise(mx, my), wd.quantise(zx, zy)
    assert int(((q[0] != z[0]) | (q[1] != z[1]) | (q[2] != z[2])).sum()) == 19738       # a kernel that ignores rot_bottom fails
    assert dw % 64 and dh % 16                                                          # partial tiles
    for resampler in ("cubic", "lanczos4"):
        st = wt.tile_states(mx, my, sw, sh, resampler, wt.kernel_rule(resampler, wd.REFLECT_101))
        recorded = wd.golden("warp_definitions_kat")[f"states_rs_zoomed_out_m{mode}_{resampler}_every"]     # the border kernels' model, as it was
        assert [[st[p][k] for k in wt.BORDER_STATES] for p in ("bgr", "luma", "chroma")] == recorded.tolist()
        for plane in ("bgr", "luma", "chroma"):
            s = st[plane]
            assert s["staged"] == 28 and s["gathered"] == 0, (resampler, plane, s)
            assert min(s["cross_l"], s["cross_r"], s["cross_t"], s["cross_b"], s["odd_w"], s["even_w"]) >= 1, (resampler, plane, s)
            assert (s["outside_staged"] >= 1) == (not (resampler == "lanczos4" and plane == "chroma")), (resampler, plane, s)
        # the constant border: the tiles wholly outside have no box, every other stages
        sc = wt.tile_states(mx, my, sw, sh, resampler, wt.kernel_rule(resampler, wd.CONSTANT))
        for plane in ("bgr", "luma", "chroma"):
            c = sc[plane]
            assert c["none"] == st[plane]["outside_staged"] and c["none"] + c["staged"] == 28 and c["gathered"] == 0, (resampler, plane, c)
            assert c["partial_staged"] >= 1 and c["odd_w"] >= 1 and c["even_w"] >= 1, (resampler, plane, c)


def test_the_constant_border_keeps_the_axis_pixel_of_mode_0_out_of_the_box():
    """Map mode 0 at the identity: the axis pixel's map is NaN (0 / 0), its tap at -32768.  Under a non-constant border its tile gathers;
    under the constant border that footprint does not touch the source and stays out of the box."""
    sw, sh, dw, dh = 64, 36, 65, 37
    p, rb = wd.case_params(sw, sh, dw, dh, 30.0, 30.0, r0=(0.0, 0.0, 0.0), r_bottom=(0.0, 0.0, 0.0))
    p[4], p[5] = 32.0, 16.0                                   # the output camera's centre on a pixel: that pixel looks along the axis
    mx, my = wd.maps(p, dw, dh, 0, rb)
    assert np.isnan(mx).sum() == 1
    for resampler in ("cubic", "lanczos4"):
        assert wt.tile_states(mx, my, sw, sh, resampler, wt.kernel_rule(resampler, wd.REPLICATE))["bgr"]["gathered"] == 1
        assert wt.tile_states(mx, my, sw, sh, resampler, wt.kernel_rule(resampler, wd.CONSTANT))["bgr"]["gathered"] == 0


def test_gathers_every_tile_over_the_budget():
    sw, sh, dw, dh, fi, fo = wd.GATHERS
    p, rb = wd.case_params(sw, sh, dw, dh, fi, fo, wd.GATHERS_R0, wd.GATHERS_R_BOTTOM)
    mx, my = wd.maps(p, dw, dh, 1, rb)
    for resampler in ("cubic", "lanczos4"):
        for border in (wd.CONSTANT, wd.REFLECT_101):
            for plane, s in wt.tile_states(mx, my, sw, sh, resampler, wt.kernel_rule(resampler, border)).items():
                assert s["staged"] == 0 and s["gathered"] == 4, (resampler, border, plane, s)


# ---------------------------------------------------------------------------------------------------------------------
# the known-answer file
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_file_reproduces_from_the_definition():
    sys.path.insert(0, GOLD)
    import make_rs_resample_golden as gen
    path = os.path.join(GOLD, "rs_resample_kat.npz")
    kat = np.load(path)
    fresh = gen.build()
    assert sorted(kat.files) == sorted(fresh)
    for key in kat.files:
        assert np.array_equal(kat[key], fresh[key]) and kat[key].dtype == fresh[key].dtype, key
    n = len(gen.CASES)
    assert {int(kat[f"case{k}_mode"]) for k in range(n)} == {0, 1} and {int(kat[f"case{k}_resample"]) for k in range(n)} == {0, 2, 4}
    assert any(f"case{k}_dist" in kat.files for k in range(n)) and not all(f"case{k}_dist" in kat.files for k in range(n))
    for k in range(n):
        assert kat[f"case{k}_bgr"].shape == (32, 64, 3) and kat[f"case{k}_luma"].shape == (32, 64) and kat[f"case{k}_chroma"].shape == (16, 64)
        assert (kat[f"case{k}_bgr"] != 0).mean() > 0.1
    assert os.path.getsize(path) < 400 * 1024
