"""The refusals of the lens-distortion entry points (include/vstab.h "Lens distortion"), as a table in the style of
test_warp_refusals_cpu.py: every distinct message of every entry point, calls that break two checks at once (the earlier check's message
wins: that pins the order -- the coefficients are always checked last), coefficients that are not finite or let theta_d fold, and the map
modes without a fisheye input.  Every call is refused before any device work: the device pointers are a dummy non-null address that is
never dereferenced, so the table runs without a GPU.  Each row: entry point, the arguments that differ from a good call, status, and the
whole vstab_last_error() text."""
import ctypes

import numpy as np
import pytest

P = 4096                       # a non-null dummy address, 16-byte aligned
BGR8, NV12, PLANAR = 0, 1, 2   # VSTAB_OUT_*
INVALID = "ERR_INVALID"
M16 = 1 << 24
_keep = []


def _arr(values, dtype, ctype):
    a = np.array(values, dtype)
    _keep.append(a)
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def f32(values):
    return _arr(values, np.float32, ctypes.c_float)


def f64(values):
    return _arr(values, np.float64, ctypes.c_double)


D_GOOD = (-0.02, 0.004, -0.001, 0.0002)
D_BAD = [(float("nan"), 0, 0, 0), (0, float("inf"), 0, 0), (0, 0, -float("inf"), 0), (0, 0, 0, float("nan")),   # not finite
         (-0.5, 0, 0, 0), (-0.14, 0, 0, 0), (0.1, -0.2, 0, 0), (0, 0, 0, -0.01)]                                 # theta_d folds below pi/2
FP, DF, DD = f32(np.zeros(17)), f32(D_GOOD), f64(D_GOOD)
K9 = f64([100, 0, 32, 0, 100, 16, 0, 0, 1])
PTS, OUT, R9, INL = f64(np.zeros(8)), f64(np.zeros(8)), f64(np.zeros(9)), (ctypes.c_int * 1)()
XY = f32(np.zeros(16))
FOLD = "the distortion must keep theta_d increasing on [0, pi/2]"
FISH = "distortion belongs to a fisheye input (map modes 1 and 2)"
OTHER_MODES = (0, 3, 4, 5, 6, -1)

# a good call of every entry point, arguments in the order of include/vstab.h
GOOD = {
    "vstab_fisheye_undistort_points_d": dict(pts=PTS, n=4, K=K9, D=DD, R=None, P=None, out=OUT),
    "vstab_estimate_rotation_d": dict(prev_xy=XY, cur_xy=XY, n=8, K_in=K9, K_out=K9, D=DD, seed=1, R=R9, inliers=INL),
    "vstab_create_map_dist": dict(map_x=P, pitch_x=128, map_y=P, pitch_y=128, cols=32, rows=16, params=FP, dist=DF, map_mode=1, stream=None),
    "vstab_quantised_map_dist": dict(qmap=P, dw=32, dh=16, params=FP, dist=DF, map_mode=1, stream=None),
    "vstab_warp_nv12_dist": dict(y=P, pitch_y=64, uv=P, pitch_uv=64, sw=64, sh=32, params=FP, dist=DF, map_mode=1, out_format=BGR8, dst=P, pitch_dst=192,
                                 dst_uv=None, pitch_dst_uv=0, dw=32, dh=16, stream=None),
    "vstab_set_input_calibration": dict(h=None, K=K9, D=DD),
}
_PLANAR_OUT = dict(out_format=PLANAR, pitch_dst=32, dst_uv=P, pitch_dst_uv=32)


def _rows():
    rows = []
    # ---- vstab_fisheye_undistort_points_d -----------------------------------------------------------------------------------------
    fn, n = "vstab_fisheye_undistort_points_d", "vstab_fisheye_undistort_points_d: "
    rows += [(fn, d, INVALID, n + "bad argument") for d in (dict(pts=None), dict(K=None), dict(D=None), dict(out=None), dict(n=-1),
                                                            dict(D=None, pts=None), dict(pts=None, D=f64(D_BAD[4])))]
    rows += [(fn, dict(D=f64(d)), INVALID, n + FOLD) for d in D_BAD]
    # ---- vstab_estimate_rotation_d ------------------------------------------------------------------------------------------------
    fn, n = "vstab_estimate_rotation_d", "vstab_estimate_rotation_d: "
    rows += [(fn, d, INVALID, n + "bad argument") for d in (dict(prev_xy=None), dict(cur_xy=None), dict(K_in=None), dict(K_out=None), dict(D=None),
                                                            dict(R=None), dict(inliers=None), dict(n=-1), dict(R=None, D=f64(D_BAD[0])))]
    rows += [(fn, dict(D=f64(d)), INVALID, n + FOLD) for d in D_BAD]
    # ---- vstab_create_map_dist ----------------------------------------------------------------------------------------------------
    fn, n = "vstab_create_map_dist", "vstab_create_map_dist: "
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("map_x", "map_y", "params", "dist")]
    rows += [(fn, dict(dist=None, cols=0), INVALID, n + "null pointer")]
    rows += [(fn, d, INVALID, n + "size must be in [1, 32767] (createMap.cl:10-11)") for d in (dict(cols=0), dict(rows=0), dict(cols=32768), dict(rows=32768),
                                                                                                dict(cols=0, pitch_x=2))]
    rows += [(fn, d, INVALID, n + "bad pitch") for d in (dict(pitch_x=124), dict(pitch_y=124), dict(pitch_x=130), dict(pitch_y=130),
                                                         dict(pitch_x=130, map_mode=6))]
    rows += [(fn, dict(map_mode=m), INVALID, n + FISH) for m in OTHER_MODES]
    rows += [(fn, dict(map_mode=0, dist=f32(D_BAD[4])), INVALID, n + FISH)]
    rows += [(fn, dict(dist=f32(d), map_mode=m), INVALID, n + FOLD) for d in D_BAD for m in (1, 2)]
    # ---- vstab_quantised_map_dist -------------------------------------------------------------------------------------------------
    fn, n = "vstab_quantised_map_dist", "vstab_quantised_map_dist: "
    rows += [(fn, d, INVALID, n + "bad argument") for d in (dict(qmap=None), dict(params=None), dict(dist=None), dict(dw=0), dict(dh=0), dict(dw=32768),
                                                            dict(dh=32768), dict(dw=0, map_mode=6), dict(qmap=None, map_mode=-1))]
    rows += [(fn, dict(map_mode=m), INVALID, n + FISH) for m in OTHER_MODES]
    rows += [(fn, dict(map_mode=6, qmap=P + 4), INVALID, n + FISH)]
    rows += [(fn, d, INVALID, n + "the buffer must be 16-byte aligned") for d in (dict(qmap=P + 4), dict(qmap=P + 8, map_mode=2),
                                                                                  dict(qmap=P + 8, dist=f32(D_BAD[4])))]
    rows += [(fn, dict(dist=f32(d), map_mode=m), INVALID, n + FOLD) for d in D_BAD for m in (1, 2)]
    # ---- vstab_warp_nv12_dist: check_warp_nv12's checks in its order, the map mode, the coefficients ------------------------------
    fn, n = "vstab_warp_nv12_dist", "vstab_warp_nv12_dist: "
    fmt = n + "the distorted-lens warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)"
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("y", "uv", "dst", "params", "dist")]
    rows += [(fn, dict(dst=None, sw=63), INVALID, n + "null pointer"), (fn, dict(dist=None, map_mode=0), INVALID, n + "null pointer")]
    rows += [(fn, d, INVALID, n + "source must be even-sized and <= 32767") for d in (
        dict(sw=0), dict(sw=63), dict(sh=31), dict(sw=32768, pitch_y=32768, pitch_uv=32768), dict(sh=32768), dict(sh=-2, dw=0))]
    rows += [(fn, d, INVALID, n + "output size must be in [1, 32767]") for d in (dict(dw=0), dict(dh=0), dict(dw=32768, pitch_dst=98304),
                                                                                  dict(dh=32768, out_format=7), dict(dw=0, map_mode=6))]
    rows += [(fn, d, INVALID, fmt) for d in (dict(out_format=NV12, pitch_dst=32, dst_uv=P, pitch_dst_uv=32), dict(out_format=3), dict(out_format=-1, pitch_y=63),
                                             dict(out_format=NV12, map_mode=0))]
    rows += [(fn, d, INVALID, n + "pitch smaller than row") for d in (dict(pitch_y=63), dict(pitch_uv=62), dict(pitch_dst=95), dict(_PLANAR_OUT, pitch_dst=31),
                                                                      dict(pitch_dst=95, dist=f32(D_BAD[4])))]
    rows += [(fn, d, INVALID, n + "plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row") for d in (
        dict(_PLANAR_OUT, dst_uv=None), dict(_PLANAR_OUT, pitch_dst_uv=31), dict(_PLANAR_OUT, pitch_dst_uv=30, uv=P + 1))]
    rows += [(fn, d, INVALID, n + "chroma plane must be 2-B aligned") for d in (dict(uv=P + 1), dict(pitch_uv=65), dict(uv=P + 1, map_mode=3))]
    rows += [(fn, dict(map_mode=m), INVALID, n + FISH) for m in OTHER_MODES]
    rows += [(fn, dict(map_mode=4, dist=f32(D_BAD[0])), INVALID, n + FISH), (fn, dict(_PLANAR_OUT, map_mode=5), INVALID, n + FISH)]
    rows += [(fn, dict(dist=f32(d), map_mode=m), INVALID, n + FOLD) for d in D_BAD for m in (1, 2)]
    rows += [(fn, dict(_PLANAR_OUT, dist=f32(D_BAD[5])), INVALID, n + FOLD), (fn, dict(dist=f32(D_BAD[5]), pitch_y=M16), INVALID, n + FOLD)]
    # (what vstab_warp_nv12_ex refuses behind its argument checks, under its own name)
    rows += [(fn, dict(pitch_y=M16), INVALID, "vstab_warp_nv12: source pitch too large for this mode"),
             (fn, dict(_PLANAR_OUT, sw=14), INVALID, "vstab_warp_nv12: the plane-wise warp needs a source of at least 16 x 2")]
    # ---- vstab_set_input_calibration (everything else needs a live handle: test_distort_gpu.py) -----------------------------------
    fn, n = "vstab_set_input_calibration", "vstab_set_input_calibration: "
    rows += [(fn, d, INVALID, n + "null argument") for d in (dict(h=None), dict(h=None, D=None), dict(h=None, D=f64(D_BAD[4])))]
    return rows


ROWS = _rows()


def test_the_table_names_every_entry_point():
    assert {fn for fn, _, _, _ in ROWS} == set(GOOD)
    for fn, bad, _, _ in ROWS:
        assert bad and set(bad) <= set(GOOD[fn]), (fn, bad)


@pytest.mark.parametrize("fn", sorted(GOOD))
def test_distortion_entry_points_refuse_bad_arguments_without_a_device(vs, fn):
    L = vs.lib
    for name, bad, status, text in ROWS:
        if name != fn:
            continue
        got = getattr(L, fn)(*dict(GOOD[fn], **bad).values())
        assert got == getattr(vs, status), (fn, bad, got, L.vstab_last_error())
        assert L.vstab_last_error() == text.encode(), (fn, bad, L.vstab_last_error())


def test_accepted_coefficients_are_the_documented_rule(vs):
    """1 + 3 k1 t^2 + 5 k2 t^4 + 7 k3 t^6 + 9 k4 t^8 > 0 at t = i (pi/2) / 1024, i = 0 .. 1024: coefficients on either side of the
    edge, through the one host entry point that runs to completion without a device."""
    import distort_def as dd
    pts = np.array([[40.0, 20.0]])
    K = np.array([[100.0, 0, 32], [0, 100.0, 16], [0, 0, 1]])
    for D in [(-0.135, 0, 0, 0), (-0.1351, 0, 0, 0), (0, -0.0328, 0, 0), (0, -0.0329, 0, 0), (0.3, -0.1, 0, 0), (0, 0, 0, -0.0029), (0, 0, 0, -0.0031),
              dd.D_A, dd.D_B, dd.D_C, dd.D_0]:
        ok = dd.min_derivative(D) > 0
        if ok:
            vs.fisheye_undistort_points(pts, K, D=D)
        else:
            with pytest.raises(vs.VstabError) as e:
                vs.fisheye_undistort_points(pts, K, D=D)
            assert e.value.status == vs.ERR_INVALID and FOLD in str(e.value)


def test_public_map_modes_beyond_5_stay_refused(vs):
    """The distorted maps are internal kernel modes (9, 10): no public entry point takes them as a map_mode."""
    L = vs.lib
    for m in (6, 7, 8, 9, 10):
        assert L.vstab_warp_nv12_ex(P, 64, P, 64, 64, 32, FP, m, BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
        assert L.vstab_last_error() == b"vstab_warp_nv12: unknown map mode"
        assert L.vstab_create_map_ex(P, 128, P, 128, 32, 16, FP, m, None) == vs.ERR_INVALID
        assert L.vstab_quantised_map(P, 32, 16, FP, m, None) == vs.ERR_INVALID
        assert L.vstab_warp_nv12_dist(P, 64, P, 64, 64, 32, FP, DF, m, BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
