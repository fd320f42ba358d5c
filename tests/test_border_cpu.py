"""Border modes (cv::remap borderMode) without a GPU: the numpy statement (tests/warp_def.py) against its golden vectors, OpenCV's
borderInterpolate loop against the closed form the kernels use, the constant border against the oracle's bilinear warp, and the argument
checks of the new entry points."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import synth
import warp_def as wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = np.arange(-32768, 32768, dtype=np.int64)


def golden_cases():
    return wd.golden_cases("border_kat", "src", "mapx", "mapy", "mode", "out")


def test_golden_remaps():
    n = 0
    seen = set()
    for k, src, mx, my, mode, out in golden_cases():
        got = wd.remap(src, mx, my, "linear", mode)
        assert np.array_equal(got, out), k
        seen.add((mode, 1 if src.ndim == 2 else src.shape[2]))
        seen.add(("w", src.shape[1]))
        seen.add(("h", src.shape[0]))
        n += 1
    assert n >= 27
    assert {(m, c) for m in wd.MODES for c in (1, 2, 3)} <= seen
    assert {("w", 1), ("w", 2), ("w", 3), ("h", 1), ("h", 2), ("h", 3)} <= seen


def test_golden_maps_hold_the_special_entries():
    specials = {"nan": False, "inf": False, "-inf": False, "1e30": False, "-1e30": False, "32768": False, "-32768": False, "tie": False, "far": False}
    for _, src, mx, my, _, _ in golden_cases():
        sh, sw = src.shape[:2]
        for m, n in ((mx, sw), (my, sh)):
            specials["nan"] |= bool(np.isnan(m).any())
            specials["inf"] |= bool(np.isposinf(m).any())
            specials["-inf"] |= bool(np.isneginf(m).any())
            specials["1e30"] |= bool((m == np.float32(1e30)).any())
            specials["-1e30"] |= bool((m == np.float32(-1e30)).any())
            specials["32768"] |= bool((m == 32768.0).any())
            specials["-32768"] |= bool((m == -32768.0).any())
            with np.errstate(invalid="ignore"):
                fin = m[np.isfinite(m) & (np.abs(m) < 1e6)]
                specials["tie"] |= bool(((fin * 64) % 2 == 1).any())
                specials["far"] |= bool(((fin < -3 * n) | (fin > 4 * n)).any())
    assert all(specials.values()), specials


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1919, 1920, 32767])
@pytest.mark.parametrize("mode", wd.MODES)
def test_closed_form_equals_opencv_loop(n, mode):
    """The kernels' borderInterpolate (fold by the period 2 len / 2 len - 2, clamp) equals OpenCV's do-while loop for every position in
    [-32768, 32767] (and the 32768 that X + 1 reaches)."""
    p = np.concatenate([SWEEP, [32768]])
    loop = wd.border_interpolate_loop(p, n, mode)
    assert ((loop >= 0) & (loop < n)).all()
    assert np.array_equal(wd.border_interpolate(p, n, mode), loop)


def test_loop_spot_values():
    L = wd.border_interpolate_loop
    # OpenCV's documentation: REPLICATE aaaaaa|abcdefgh|hhhhhhh, REFLECT fedcba|abcdefgh|hgfedcb, REFLECT_101 gfedcb|abcdefgh|gfedcba
    p = np.arange(-6, 15)
    assert list(L(p, 8, wd.REPLICATE)) == [0] * 6 + list(range(8)) + [7] * 7
    assert list(L(p, 8, wd.REFLECT)) == [5, 4, 3, 2, 1, 0] + list(range(8)) + [7, 6, 5, 4, 3, 2, 1]
    assert list(L(p, 8, wd.REFLECT_101)) == [6, 5, 4, 3, 2, 1] + list(range(8)) + [6, 5, 4, 3, 2, 1, 0]
    assert list(L(np.array([-5, -1, 1, 7]), 1, wd.REFLECT_101)) == [0, 0, 0, 0]


def test_constant_equals_oracle_bilinear():
    rng = np.random.default_rng(5)
    for cn in (1, 3):
        src = rng.integers(0, 256, (23, 31, cn) if cn > 1 else (23, 31), dtype=np.uint8)
        mx = rng.uniform(-40, 70, (17, 29)).astype(np.float32)
        my = rng.uniform(-30, 50, (17, 29)).astype(np.float32)
        mx[0, :4] = [np.nan, np.inf, -1e30, 32768.0]
        assert np.array_equal(wd.remap(src, mx, my, "linear", wd.CONSTANT), oracle.remap_bilinear(src, mx, my))


def test_constant_warp_equals_oracle_warps():
    w, h = 96, 64
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h, 1.3)
    frame = synth.nv12(3, w, h)
    R = oracle.rodrigues([0.05, -0.04, 0.1])
    p = oracle.map_params(K, Ko, R)
    rb = oracle.map_params(K, Ko, oracle.rodrigues([0.02, 0.03, 0.12]))[8:]
    def numpy_warps(mx, my):
        """The warps of wd.bgr / wd.planar from wd.remap itself: under linear + CONSTANT those two answer with the oracle."""
        y, uv = wd.planes_of(frame)
        ouv = wd.remap(uv, *oracle.chroma_maps(mx, my), "linear", wd.CONSTANT, (128, 128))
        bgr = wd.remap(oracle.cvt_nv12_bgr(frame), mx, my, "linear", wd.CONSTANT, 0)
        return bgr, wd.remap(y, mx, my, "linear", wd.CONSTANT, 16), ouv.reshape(ouv.shape[0], -1)

    for mode in range(5):
        bgr, y, uv = numpy_warps(*wd.maps(p, cw, ch, mode))
        assert np.array_equal(bgr, oracle.warp_nv12_ex(frame, p, cw, ch, mode, 0))
        ey, euv = oracle.warp_nv12_planar(frame, p, cw, ch, mode)
        assert np.array_equal(y, ey) and np.array_equal(uv, euv), mode
    for mode in (0, 1):
        bgr, y, uv = numpy_warps(*wd.maps(p, cw, ch, mode, rb))
        assert np.array_equal(bgr, oracle.warp_nv12_rs(frame, p, rb, cw, ch, mode, 0))
        ey, euv = oracle.warp_nv12_planar(frame, p, cw, ch, mode, rot_bottom=rb)
        assert np.array_equal(y, ey) and np.array_equal(uv, euv), mode


def test_replicate_inside_equals_constant():
    """A map whose four taps all stay inside the source reads no border at all: REPLICATE (and the reflections) equal the constant border."""
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    mx = rng.uniform(1.0, 28.0, (15, 25)).astype(np.float32)   # X in [1, 27], X + 1 <= 28 < 30
    my = rng.uniform(1.0, 18.0, (15, 25)).astype(np.float32)
    ref = wd.remap(src, mx, my, "linear", wd.CONSTANT)
    for mode in wd.MODES:
        assert np.array_equal(wd.remap(src, mx, my, "linear", mode), ref)


def test_reflect_far_outside_reads_picture():
    """A tile wholly outside the source (which the constant border leaves black) reads mirrored picture: the output at -x equals the output
    at x - 1 (REFLECT) or x (REFLECT_101) for integer positions."""
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (9, 12), dtype=np.uint8)
    xs = np.arange(0, 12, dtype=np.float32)
    mx, my = np.stack([-1 - xs, xs]), np.full((2, 12), 4.0, np.float32)
    out = wd.remap(src, mx, my, "linear", wd.REFLECT)
    assert np.array_equal(out[0], out[1])
    mx = np.stack([-xs, xs])
    out = wd.remap(src, mx, my, "linear", wd.REFLECT_101)
    assert np.array_equal(out[0], out[1])
    assert wd.remap(src, mx - 100, my, "linear", wd.CONSTANT).max() == 0


def test_border_matches_opencv_when_present():
    """cv2.remap with each border mode, where OpenCV is installed (skipped otherwise)."""
    cv2 = pytest.importorskip("cv2")
    for k, src, mx, my, mode, out in golden_cases():
        if not (np.isfinite(mx).all() and np.isfinite(my).all()):
            continue   # cv2's SIMD path may treat NaN / inf differently from its scalar one
        exp = cv2.remap(src, mx, my, cv2.INTER_LINEAR, borderMode=mode)
        assert np.array_equal(exp, out), k
    rng = np.random.default_rng(8)
    for cn in (1, 2, 3):
        src = rng.integers(0, 256, (13, 17, cn) if cn > 1 else (13, 17), dtype=np.uint8)
        mx = rng.uniform(-60, 80, (19, 23)).astype(np.float32)
        my = rng.uniform(-40, 60, (19, 23)).astype(np.float32)
        for mode in wd.MODES:
            assert np.array_equal(cv2.remap(src, mx, my, cv2.INTER_LINEAR, borderMode=mode), wd.remap(src, mx, my, "linear", mode)), (cn, mode)


def test_header_binding_and_opencv_values(vs):
    assert (vs.BORDER_CONSTANT, vs.BORDER_REPLICATE, vs.BORDER_REFLECT, vs.BORDER_REFLECT_101) == (0, 1, 2, 4)
    text = open(os.path.join(ROOT, "include", "vstab.h")).read()
    assert "VSTAB_BORDER_CONSTANT = 0, VSTAB_BORDER_REPLICATE = 1, VSTAB_BORDER_REFLECT = 2, VSTAB_BORDER_REFLECT_101 = 4" in text
    for name in ("vstab_remap_bilinear_border", "vstab_warp_nv12_border", "vstab_set_border_mode"):
        assert name in vs.SIGNATURES and hasattr(vs.lib, name)


def test_border_entry_points_refuse_bad_arguments_without_a_device(vs):
    """Argument checks come before any launch: null pointers, channel counts, sizes, pitches, border modes, output formats, map modes and
    rot_bottom outside modes 0 / 1 / 5.  The setter refuses a NULL handle."""
    P = 4096   # a non-null dummy address: never dereferenced, every call below is refused first
    L = vs.lib
    R = L.vstab_remap_bilinear_border
    assert R(P, 64, 8, 8, 1, P, 32, P, 32, 5, P, 8, 8, 8, None) == vs.ERR_INVALID   # TRANSPARENT
    assert b"border_mode" in L.vstab_last_error()
    for bad in (3, 5, -1, 16, 6):
        assert R(P, 64, 8, 8, 1, P, 32, P, 32, bad, P, 8, 8, 8, None) == vs.ERR_INVALID
    assert R(None, 64, 8, 8, 1, P, 32, P, 32, 1, P, 8, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 4, P, 32, P, 32, 1, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 0, P, 32, P, 32, 1, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 0, 8, 1, P, 32, P, 32, 1, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 32768, 8, 1, P, 32, P, 32, 1, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 1, P, 16, P, 32, 1, P, 32, 8, 8, None) == vs.ERR_INVALID   # map pitch < 4 * width
    assert R(P, 64, 8, 8, 1, P + 2, 32, P, 32, 1, P, 32, 8, 8, None) == vs.ERR_INVALID   # map plane not 4-byte aligned
    assert R(P, 64, 8, 8, 3, P, 32, P, 32, 1, P, 16, 8, 8, None) == vs.ERR_INVALID   # dst pitch < 3 * width
    p = np.zeros(17, np.float32)
    rb = np.zeros(9, np.float32)
    fp = p.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rbp = rb.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    W = L.vstab_warp_nv12_border
    B = vs.BORDER_REFLECT_101
    assert W(P, 64, P, 64, 64, 32, fp, None, 0, vs.OUT_NV12, B, P, 64, P, 64, 32, 16, None) == vs.ERR_INVALID
    assert b"VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR" in L.vstab_last_error()
    assert W(P, 64, P, 64, 64, 32, fp, None, 0, 7, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    for bad in (3, 5, -1, 8):
        assert W(P, 64, P, 64, 64, 32, fp, None, 0, vs.OUT_BGR8, bad, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
        assert b"border_mode" in L.vstab_last_error()
    assert W(P, 64, P, 64, 64, 32, fp, None, 6, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, None, -1, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    for mode in (2, 3, 4):   # a rotation per output row is served for map modes 0, 1 and 5
        assert W(P, 64, P, 64, 64, 32, fp, rbp, mode, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
        assert b"rot_bottom" in L.vstab_last_error()
    assert W(P, 64, P, 64, 63, 32, fp, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd source
    assert W(P, 64, P, 64, 64, 31, fp, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, None, 0, vs.OUT_BGR8, B, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # pitch < 3 * width
    assert W(P, 64, P, 64, 64, 32, fp, None, 0, vs.OUT_NV12_PLANAR, B, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # no chroma plane
    assert W(P, 64, P + 1, 64, 64, 32, fp, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd chroma address
    assert W(P, 64, P, 63, 64, 32, fp, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # pitch < width
    assert W(None, 64, P, 64, 64, 32, fp, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, None, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 0, 16, None) == vs.ERR_INVALID
    assert L.vstab_set_border_mode(None, B) == vs.ERR_INVALID
    assert L.vstab_set_border_mode(None, 0) == vs.ERR_INVALID
