"""CPU tests of the pinhole lens distortion (include/vstab.h, "Pinhole lens distortion"; tests/pinhole_def.py): the numpy definition against
the oracle's modes 3 / 4 at D = 0 and against the golden file, the C undistortion against the numpy one, the refusals of the stateless
entry points as a table in the style of test_distort_refusals_cpu.py (every call is refused before any device work: the device pointers
are a dummy address), the rotation estimate through a distorted lens, the tile states the GPU tests' shapes are there for (from the
committed CPU models of the kernels' boxes, imported), and the new kernels' private segments (from the built library's kernel metadata)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle
import pinhole_def as pd
import warp_def as wd
import warp_tiles as wt
from test_distort_refusals_cpu import BGR8, FP, INL, INVALID, K9, NV12, OUT, P, PLANAR, PTS, R9, XY, f32, f64
from test_lens_gpu import LENSES, ROTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEFAULT, CUBIC, LANCZOS4 = 0, 2, 4       # VSTAB_RESAMPLE_*
DS = {"D_P": pd.D_P, "D_Q": pd.D_Q, "D_M": pd.D_M}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cameras(w, h, dw, dh, mode, aniso=1.0):
    """test_lens_gpu.LENSES[2:]: rect 100 -> rect 80 (mode 3), rect 100 -> fish 300 (mode 4)."""
    ip, ifov, op, ofov = LENSES[mode - 1]
    assert ip == oracle.PROJ_RECT and op == (oracle.PROJ_RECT if mode == 3 else oracle.PROJ_FISH)
    Kin = oracle.lens_camera(ip, ifov, w, h)
    Kin[1, 1] *= aniso
    return Kin, oracle.lens_camera(op, ofov, dw, dh)


def shape_maps(w, h, dw, dh, mode, rv, D=pd.D_P):
    Kin, Kout = cameras(w, h, dw, dh, mode)
    return pd.maps(oracle.map_params(Kin, Kout, oracle.rodrigues(rv)), dw, dh, mode, D)


# ---------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_distortion_is_the_oracles_map_bit_for_bit():
    n = 0
    for mode in (3, 4):
        for (w, h, dw, dh) in [(128, 72, 130, 70), (640, 360, 333, 201), (320, 180, 97, 45), (1024, 576, 200, 72)]:
            for rv in ROTS[:4]:
                Kin, Kout = cameras(w, h, dw, dh, mode)
                p = oracle.map_params(Kin, Kout, oracle.rodrigues(rv))
                mx, my = pd.maps(p, dw, dh, mode, pd.D_0)
                ex, ey = oracle.create_map_ex(p, dw, dh, mode)
                nan = np.isnan(ex)
                assert np.array_equal(np.isnan(mx), nan) and np.array_equal(np.isnan(my), nan), (mode, dw, rv)
                assert np.array_equal(bits(mx)[~nan], bits(ex)[~nan]) and np.array_equal(bits(my)[~nan], bits(ey)[~nan]), (mode, dw, rv)
                n += 1
    assert n == 32


def test_distortion_moves_the_map():
    """The coefficient sets are not a no-op at the GPU tests' main shape: most quantised positions differ from the ideal lens's."""
    for mode in (3, 4):
        zx, zy = shape_maps(128, 72, 130, 70, mode, ROTS[1], pd.D_0)
        for D in DS.values():
            mx, my = shape_maps(128, 72, 130, 70, mode, ROTS[1], D)
            ok = ~np.isnan(zx)
            assert np.array_equal(np.isnan(mx), ~ok)
            with np.errstate(invalid="ignore"):
                moved = (np.rint(mx * 32) != np.rint(zx * 32)) | (np.rint(my * 32) != np.rint(zy * 32))
            assert moved[ok].mean() > 0.5, (mode, D)


def test_golden_file_reproduces_from_the_definition():
    sys.path.insert(0, GOLD)
    import make_pinhole_golden as gen
    path = os.path.join(GOLD, "pinhole_kat.npz")
    kat = np.load(path)
    fresh = gen.build()
    assert sorted(kat.files) == sorted(fresh)
    for key in kat.files:
        a, b = kat[key], fresh[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        if a.dtype.kind == "f" and a.dtype.itemsize == 4:
            nan = np.isnan(a)
            assert np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan]), key
        else:
            assert np.array_equal(a, b), key
    assert len(gen.MAPS) == 4 and {int(kat[f"map{k}_mode"]) for k in range(4)} == {3, 4}
    assert any(np.isnan(kat[f"map{k}_x"]).any() for k in range(4))
    largest = max(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if f.endswith("_kat.npz") and f != "pinhole_kat.npz")
    assert os.path.getsize(path) <= largest


# ---------------------------------------------------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------------------------------------------------
def test_c_undistortion_equals_the_numpy_one(vs):
    kat = np.load(os.path.join(GOLD, "pinhole_kat.npz"))
    K, pts, R, Pm = kat["pts_K"], kat["pts_in"], kat["pts_R"], kat["pts_P"]
    for j in range(4):
        D = kat[f"pts{j}_dist"]
        assert np.allclose(vs.undistort_points_pinhole(pts, K, D), kat[f"pts{j}_out"], rtol=1e-13, atol=1e-10), j
        assert np.allclose(vs.undistort_points_pinhole(pts, K, D, R, Pm), kat[f"pts{j}_out_rp"], rtol=1e-13, atol=1e-10), j
        assert np.allclose(vs.undistort_points_pinhole(pts, K, D, R, Pm), pd.undistort_points(pts, K, D, R, Pm), rtol=1e-13, atol=1e-10), j
    # D = 0 is the normalisation alone
    z = vs.undistort_points_pinhole(pts, K, pd.D_0)
    assert np.array_equal(z, np.stack([(pts[:, 0] - K[0, 2]) / K[0, 0], (pts[:, 1] - K[1, 2]) / K[1, 1]], -1))


def test_undistortion_inverts_the_forward_model_to_its_round_trip_residual():
    """What five steps leave, over the 640 x 360 image of the rect 100 camera: small for D_M (the set the rotation test uses), larger for D_P."""
    w, h = 640, 360
    K = oracle.lens_camera(oracle.PROJ_RECT, 100.0, w, h)
    ys, xs = np.meshgrid(np.r_[0:h:8, h - 1].astype(np.float64), np.r_[0:w:8, w - 1].astype(np.float64), indexing="ij")   # every eighth pixel and the far edges
    norm = np.stack([(xs.ravel() - K[0, 2]) / K[0, 0], (ys.ravel() - K[1, 2]) / K[1, 1]], -1)
    rm, rp = pd.round_trip_residual(K, pd.D_M, norm), pd.round_trip_residual(K, pd.D_P, norm)
    print("round-trip residual over the image: D_M %.3e, D_P %.3e (normalised coordinates)" % (rm, rp))
    assert rm < 1e-4 < 1e-3 < rp < 1e-2


def test_negative_radial_factor_returns_the_point(vs):
    """icdist < 0 on the first step: cv::undistortPoints gives the normalised point back."""
    K = np.array([[100.0, 0, 50], [0, 100.0, 40], [0, 0, 1]])
    D = (-2.0, 0.0, 0.0, 0.0, 0.0)
    pts = np.array([[150.0, 40.0], [50.0, 150.0]])          # r2 = 1, 1.21: 1 + k1 r2 < 0
    exp = pd.undistort_points(pts, K, D)
    assert np.array_equal(exp, [[1.0, 0.0], [0.0, 1.1]])
    assert np.array_equal(vs.undistort_points_pinhole(pts, K, D), exp)


def test_points_match_opencv_when_present(vs):
    cv2 = pytest.importorskip("cv2")
    kat = np.load(os.path.join(GOLD, "pinhole_kat.npz"))
    K, pts, R, Pm = kat["pts_K"], kat["pts_in"], kat["pts_R"], kat["pts_P"]
    for D in (pd.D_P, pd.D_Q, pd.D_M):
        ref = cv2.undistortPoints(pts.reshape(-1, 1, 2), K, np.array(D), R=R, P=Pm).reshape(-1, 2)
        assert np.allclose(vs.undistort_points_pinhole(pts, K, D, R, Pm), ref, rtol=1e-9, atol=1e-7), D


# ---------------------------------------------------------------------------------------------------------------------
# refusals of the stateless entry points
# ---------------------------------------------------------------------------------------------------------------------
D5 = (-0.12, 0.02, 0.0005, -0.0004, 0.0)
D5_BAD = [(float("nan"), 0, 0, 0, 0), (0, float("inf"), 0, 0, 0), (0, 0, -float("inf"), 0, 0), (0, 0, 0, float("nan"), 0), (0, 0, 0, 0, float("inf"))]
D5_BAD64 = D5_BAD + [(1e39, 0, 0, 0, 0), (0, 0, 0, 0, -1e300)]      # finite in fp64, not after the cast to fp32
DF5, DD5 = f32(D5), f64(D5)
FINITE = "the five distortion coefficients must be finite"
RECT = "pinhole distortion belongs to a rectilinear input (map modes 3 and 4)"
OTHER_MODES = (0, 1, 2, 5, 6, 12, -1)

GOOD = {
    "vstab_undistort_points_pinhole": dict(pts=PTS, n=4, K=K9, D=DD5, R=None, P=None, out=OUT),
    "vstab_estimate_rotation_pinhole": dict(prev_xy=XY, cur_xy=XY, n=8, K_in=K9, K_out=K9, D=DD5, seed=1, R=R9, inliers=INL),
    "vstab_create_map_pinhole": dict(map_x=P, pitch_x=128, map_y=P, pitch_y=128, cols=32, rows=16, params=FP, dist=DF5, map_mode=3, stream=None),
    "vstab_warp_nv12_pinhole": dict(y=P, pitch_y=64, uv=P, pitch_uv=64, sw=64, sh=32, params=FP, dist=DF5, map_mode=3, resample=CUBIC, border_mode=4,
                                    out_format=BGR8, dst=P, pitch_dst=192, dst_uv=None, pitch_dst_uv=0, dw=32, dh=16, stream=None),
}
_PLANAR_OUT = dict(out_format=PLANAR, pitch_dst=32, dst_uv=P, pitch_dst_uv=32)


def _rows():
    rows = []
    fn, n = "vstab_undistort_points_pinhole", "vstab_undistort_points_pinhole: "
    rows += [(fn, d, INVALID, n + "bad argument") for d in (dict(pts=None), dict(K=None), dict(D=None), dict(out=None), dict(n=-1), dict(D=None, n=-1),
                                                            dict(out=None, D=f64(D5_BAD64[0])))]
    rows += [(fn, dict(D=f64(d)), INVALID, n + FINITE) for d in D5_BAD64]
    fn, n = "vstab_estimate_rotation_pinhole", "vstab_estimate_rotation_pinhole: "
    rows += [(fn, d, INVALID, n + "bad argument") for d in (dict(prev_xy=None), dict(cur_xy=None), dict(n=-1), dict(K_in=None), dict(K_out=None), dict(D=None),
                                                            dict(R=None), dict(inliers=None), dict(R=None, D=f64(D5_BAD64[1])))]
    rows += [(fn, dict(D=f64(d)), INVALID, n + FINITE) for d in D5_BAD64]
    fn, n = "vstab_create_map_pinhole", "vstab_create_map_pinhole: "
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("map_x", "map_y", "params", "dist")]
    rows += [(fn, d, INVALID, n + "null pointer") for d in (dict(dist=None, cols=0), dict(dist=None, map_mode=1))]
    rows += [(fn, d, INVALID, n + "size must be in [1, 32767] (createMap.cl:10-11)") for d in (dict(cols=0), dict(rows=0), dict(cols=32768, pitch_x=1 << 20, pitch_y=1 << 20),
                                                                                               dict(rows=32768), dict(cols=0, pitch_x=2), dict(rows=-1, map_mode=1))]
    rows += [(fn, d, INVALID, n + "bad pitch") for d in (dict(pitch_x=127), dict(pitch_y=124), dict(pitch_x=130), dict(pitch_y=126, map_mode=0),
                                                         dict(pitch_x=127, dist=f32(D5_BAD[0])))]
    rows += [(fn, dict(map_mode=m), INVALID, n + RECT) for m in OTHER_MODES]
    rows += [(fn, dict(map_mode=1, dist=f32(D5_BAD[2])), INVALID, n + RECT)]
    rows += [(fn, dict(dist=f32(d), map_mode=m), INVALID, n + FINITE) for d in D5_BAD for m in (3, 4)]
    # ---- vstab_warp_nv12_pinhole: the documented order -----------------------------------------------------------------------------
    fn, n = "vstab_warp_nv12_pinhole", "vstab_warp_nv12_pinhole: "
    fmt = n + "the pinhole-lens warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)"
    bm = n + "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)"
    rs = n + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)"
    # 1. dist null, before everything; 2. check_warp_nv12's checks in its order
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("y", "uv", "dst", "params", "dist")]
    rows += [(fn, d, INVALID, n + "null pointer") for d in (dict(dst=None, sw=63), dict(dist=None, map_mode=0), dict(dist=None, sw=63), dict(dist=None, resample=1),
                                                            dict(dist=None, border_mode=3))]
    rows += [(fn, d, INVALID, n + "source must be even-sized and <= 32767") for d in (
        dict(sw=0), dict(sw=63), dict(sh=31), dict(sw=32768, pitch_y=32768, pitch_uv=32768), dict(sh=32768), dict(sh=-2, dw=0), dict(sw=63, resample=1))]
    rows += [(fn, d, INVALID, n + "output size must be in [1, 32767]") for d in (
        dict(dw=0), dict(dh=0), dict(dw=32768, pitch_dst=98304), dict(dh=32768, out_format=7), dict(dw=0, map_mode=6), dict(dw=0, resample=1),
        dict(dh=0, border_mode=3))]
    rows += [(fn, d, INVALID, fmt) for d in (dict(out_format=NV12, pitch_dst=32, dst_uv=P, pitch_dst_uv=32), dict(out_format=3), dict(out_format=-1, pitch_y=63),
                                             dict(out_format=NV12, map_mode=0), dict(out_format=3, border_mode=3), dict(out_format=NV12, resample=DEFAULT, border_mode=0))]
    rows += [(fn, dict(border_mode=b), INVALID, bm) for b in (3, 5, -1, 8, 16)]
    rows += [(fn, d, INVALID, bm) for d in (dict(border_mode=3, pitch_y=63), dict(border_mode=3, resample=1), dict(border_mode=3, map_mode=0),
                                            dict(border_mode=5, dist=f32(D5_BAD[4])))]
    rows += [(fn, d, INVALID, n + "pitch smaller than row") for d in (dict(pitch_y=63), dict(pitch_uv=62), dict(pitch_dst=95), dict(_PLANAR_OUT, pitch_dst=31),
                                                                      dict(pitch_dst=95, dist=f32(D5_BAD[4])), dict(pitch_dst=95, resample=1))]
    rows += [(fn, d, INVALID, n + "plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row") for d in (
        dict(_PLANAR_OUT, dst_uv=None), dict(_PLANAR_OUT, pitch_dst_uv=31), dict(_PLANAR_OUT, pitch_dst_uv=30, uv=P + 1))]
    rows += [(fn, d, INVALID, n + "chroma plane must be 2-B aligned") for d in (dict(uv=P + 1), dict(pitch_uv=65), dict(uv=P + 1, map_mode=1), dict(uv=P + 1, resample=3))]
    # 3. the resampler, before the map mode and the coefficients
    rows += [(fn, dict(resample=r), INVALID, rs) for r in (1, 3, 5, -1)]
    rows += [(fn, d, INVALID, rs) for d in (dict(resample=1, map_mode=0), dict(resample=3, dist=f32(D5_BAD[0])), dict(resample=5, map_mode=6, dist=f32(D5_BAD[4])),
                                            dict(_PLANAR_OUT, resample=-1), dict(resample=1, border_mode=0))]
    # 4. the map mode, before the coefficients
    rows += [(fn, dict(map_mode=m, resample=r), INVALID, n + RECT) for m in OTHER_MODES for r in (DEFAULT, CUBIC, LANCZOS4)]
    rows += [(fn, d, INVALID, n + RECT) for d in (dict(map_mode=2, dist=f32(D5_BAD[0])), dict(_PLANAR_OUT, map_mode=5), dict(map_mode=13, dist=f32(D5_BAD[3])))]
    # 5. the coefficients
    rows += [(fn, dict(dist=f32(d), map_mode=m), INVALID, n + FINITE) for d in D5_BAD for m in (3, 4)]
    rows += [(fn, dict(dist=f32(D5_BAD[1]), resample=r, border_mode=b), INVALID, n + FINITE) for r in (DEFAULT, CUBIC, LANCZOS4) for b in (0, 1, 2, 4)]
    rows += [(fn, dict(_PLANAR_OUT, dist=f32(D5_BAD[3])), INVALID, n + FINITE)]
    return rows


ROWS = _rows()


def test_the_table_names_every_entry_point_and_every_message():
    assert {fn for fn, _, _, _ in ROWS} == set(GOOD)
    for fn, bad, _, _ in ROWS:
        assert bad and set(bad) <= set(GOOD[fn]), (fn, bad)
    # every message include/vstab.h states for vstab_warp_nv12_pinhole is in the table
    text = " ".join(open(os.path.join(ROOT, "include", "vstab.h")).read().replace(" *", " ").split())
    doc = text[text.index("Every refusal is VSTAB_ERR_INVALID, made before any device work, in this order, each message behind \"vstab_warp_nv12_pinhole: \""):
               text.index("VSTAB_API vstab_status vstab_warp_nv12_pinhole")]
    stated = set(re.findall(r'"([^"]+)"', doc)) - {"vstab_warp_nv12_pinhole: "}
    tabled = {t.split(": ", 1)[1] for fn, _, _, t in ROWS if t.startswith("vstab_warp_nv12_pinhole: ")}
    assert len(stated) == 11 and stated == tabled, (stated ^ tabled)


@pytest.mark.parametrize("fn", sorted(GOOD))
def test_entry_points_refuse_bad_arguments_without_a_device(vs, fn):
    L = vs.lib
    n = 0
    for name, bad, status, text in ROWS:
        if name != fn:
            continue
        got = getattr(L, fn)(*dict(GOOD[fn], **bad).values())
        assert got == getattr(vs, status), (fn, bad, got, L.vstab_last_error())
        assert L.vstab_last_error() == text.encode(), (fn, bad, L.vstab_last_error())
        n += 1
    assert n >= 10


def test_older_entry_points_keep_refusing_the_internal_modes(vs):
    """The public enum still ends at 5: the kernels' MAP_RECTD_* values 12 / 13 are unknown map modes to every older entry point."""
    L = vs.lib
    for m in (12, 13):
        assert L.vstab_create_map_ex(P, 128, P, 128, 32, 16, FP, m, None) == vs.ERR_INVALID
        assert L.vstab_last_error() == b"vstab_create_map: unknown map mode"
        assert L.vstab_warp_nv12_cubic_border(P, 64, P, 64, 64, 32, FP, m, BGR8, 4, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
        assert L.vstab_last_error() == b"vstab_warp_nv12_cubic_border: unknown map mode"
        assert L.vstab_warp_nv12_border(P, 64, P, 64, 64, 32, FP, None, m, BGR8, 4, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
        assert L.vstab_warp_nv12_ex(P, 64, P, 64, 64, 32, FP, m, BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID


def test_abi_version_and_struct_sizes_are_unchanged(vs):
    assert vs.lib.vstab_abi_version() == 0x56534206 == vs.ABI_VERSION
    assert [vs.lib.vstab_struct_size(k) for k in range(5)] == [104, 24, 144, 168, 160]


# ---------------------------------------------------------------------------------------------------------------------
# rotation estimate
# ---------------------------------------------------------------------------------------------------------------------
def test_rotation_estimate_through_a_distorted_pinhole_lens(vs):
    """120 rays under a known 0.02-rad rotation, seen by the rect 100 camera at 640 x 360 through D_M and through D_0.  The estimate with
    D_M may be worse than the ideal lens's by what the undistortion itself leaves: twice the angle of its largest round-trip residual at
    these points (one residual for each of the two point sets).  Measured: error 3.0e-7 rad through D_M against 0 (to fp64's acos) through
    D_0, margin 3.6e-5 (residual 1.8e-5 at these points), 120 inliers of 120 each; the D_M points estimated without the coefficients: 1.6e-3."""
    w, h = 640, 360
    K = oracle.lens_camera(oracle.PROJ_RECT, 100.0, w, h)
    Ko = oracle.lens_camera(oracle.PROJ_RECT, 80.0, 480, 270)
    rng = np.random.default_rng(12)
    Rt = oracle.rodrigues(np.array([0.6, -0.64, 0.48]) * 0.02)
    ideal = rng.uniform([40, 40], [w - 40, h - 40], (120, 2))
    norm = np.stack([(ideal[:, 0] - K[0, 2]) / K[0, 0], (ideal[:, 1] - K[1, 2]) / K[1, 1]], -1)
    rays = np.concatenate([norm, np.ones((120, 1))], -1)
    moved = rays @ Rt.T
    err, inl = {}, {}
    for name, D in (("D_M", pd.D_M), ("D_0", pd.D_0)):
        p, c = pd.project(K, D, rays).astype(np.float32), pd.project(K, D, moved).astype(np.float32)
        R, inl[name] = vs.estimate_rotation_pinhole(p, c, K, Ko, D, seed=3)
        err[name] = oracle.rotation_angle(R @ Rt.T)
    both = np.concatenate([norm, moved[:, :2] / moved[:, 2:]])
    residual = pd.round_trip_residual(K, pd.D_M, both)
    margin = 2 * np.arctan(residual)
    p, c = pd.project(K, pd.D_M, rays).astype(np.float32), pd.project(K, pd.D_M, moved).astype(np.float32)
    Rn, inln = vs.estimate_rotation_pinhole(p, c, K, Ko, pd.D_0, seed=3)
    errn = oracle.rotation_angle(Rn @ Rt.T)
    print("rotation error through D_M %.3e (inliers %d), through D_0 %.3e (inliers %d), margin %.3e (residual %.3e); D_M points without D %.3e (inliers %d)"
          % (err["D_M"], inl["D_M"], err["D_0"], inl["D_0"], margin, residual, errn, inln))
    assert err["D_M"] <= err["D_0"] + margin
    assert inl["D_0"] >= 113 and inl["D_M"] >= 113 and errn > err["D_M"]


# ---------------------------------------------------------------------------------------------------------------------
# tile states of the shapes test_pinhole_gpu.py runs.  The kernels behind vstab_warp_nv12_pinhole: k_warp_border for INTER_LINEAR (every border
# mode: BORDER_CONSTANT is the rule `clamp` of tests/warp_tiles.py), k_warp_cubic_rs / k_warp_lanczos4_rs for the other two (wt.kernel_rule).
# ---------------------------------------------------------------------------------------------------------------------
KERNELS = [(r, b) for r in wd.RESAMPLERS for b in (wd.CONSTANT, wd.REFLECT_101)]
PLANES = ("bgr", "luma", "chroma")


def tile_states(resampler, mx, my, sw, sh, border):
    rule = "clamp" if (resampler, border) == ("linear", wd.CONSTANT) else wt.kernel_rule(resampler, border)
    return wt.tile_states(mx, my, sw, sh, resampler, rule)


def test_tile_states_640x360_staged_partial_crossing_and_mixed():
    w, h, dw, dh = 640, 360, 333, 201
    mx, my = shape_maps(w, h, dw, dh, 3, ROTS[1])
    for r, b in KERNELS:
        st = tile_states(r, mx, my, w, h, b)
        for pl in PLANES:
            s = st[pl]
            assert s["staged"] == 78 and s["gathered"] == 0 and s["odd_w"] > 0 and s["even_w"] > 0, (r, b, pl, s)
            if b == wd.CONSTANT and r != "linear":
                assert s["none"] == 0 and s["partial_staged"] == 18, (r, b, pl, s)      # the partial tiles at the right and bottom edge
    mx, my = shape_maps(w, h, dw, dh, 4, ROTS[1])                                        # staged and gathered tiles in one launch
    for r, b in KERNELS:
        st = tile_states(r, mx, my, w, h, b)
        for pl in PLANES:
            assert st[pl]["staged"] > 0 and st[pl]["gathered"] > 0, (r, b, pl, st[pl])
        if r != "linear" and b == wd.CONSTANT:
            assert st["bgr"]["none"] > 0, (r, st["bgr"])                                 # tiles with no box beside them
        else:
            assert st["bgr"]["outside_staged"] > 0, (r, b, st["bgr"])
        c = st["chroma"]
        if r == "linear" and b == wd.CONSTANT:                                          # clamped taps: boxes that cross every edge of the source
            assert min(c["cross_l"], c["cross_r"], c["cross_t"], c["cross_b"]) > 0 and min(st["bgr"][k] for k in ("cross_l", "cross_r", "cross_t", "cross_b")) > 0
        elif b != wd.CONSTANT:
            assert c["cross_r"] > 0 and c["cross_t"] > 0 and c["cross_b"] > 0, (r, c)


def test_tile_states_1024x576_staged_and_gathered_in_one_launch():
    w, h, dw, dh = 1024, 576, 200, 72
    mx, my = shape_maps(w, h, dw, dh, 3, ROTS[1])
    for r, b in KERNELS:
        st = tile_states(r, mx, my, w, h, b)
        assert st["bgr"]["staged"] == 5 and st["bgr"]["gathered"] == 15, (r, b, st["bgr"])
        assert st["chroma"]["staged"] == 20, (r, b, st["chroma"])
    mx, my = shape_maps(w, h, dw, dh, 4, ROTS[1])
    for r, b in KERNELS:
        st = tile_states(r, mx, my, w, h, b)
        assert st["bgr"]["gathered"] == 15, (r, b, st["bgr"])
        if r != "linear" and b == wd.CONSTANT:
            assert st["bgr"]["none"] == 5 and st["chroma"]["staged"] > 0, (r, st)
        else:
            assert st["bgr"]["outside_staged"] == 5, (r, b, st["bgr"])


def test_tile_states_every_box_over_the_lds_budget():
    """2048 x 1152 -> 256 x 128, mode 3: every BGR box is over the budget, but a few chroma boxes (and, INTER_LINEAR, luma boxes) still fit.
    The nearest shape at which every box of every plane is over it is 3072 x 1728 -> 256 x 128: the GPU test runs both.  Mode 4 has no such
    shape -- two fifths of its map is NaN, and a tile of NaN entries has no box (CONSTANT) or a small one far outside --, so there the
    shapes reach 'most tiles gathered' beside those."""
    dw, dh = 256, 128
    for r, b in KERNELS:
        mx, my = shape_maps(2048, 1152, dw, dh, 3, ROTS[1])
        st = tile_states(r, mx, my, 2048, 1152, b)
        assert st["bgr"]["gathered"] == 32 and st["bgr"]["staged"] == 0, (r, b, st["bgr"])
        mx, my = shape_maps(3072, 1728, dw, dh, 3, ROTS[1])
        st = tile_states(r, mx, my, 3072, 1728, b)
        for pl in PLANES:
            assert st[pl]["gathered"] == 32 and st[pl]["staged"] == 0 and st[pl].get("none", 0) == 0, (r, b, pl, st[pl])
        mx, my = shape_maps(2048, 1152, dw, dh, 4, ROTS[1])
        st = tile_states(r, mx, my, 2048, 1152, b)
        for pl in PLANES:
            assert st[pl]["gathered"] >= 19 and st[pl]["gathered"] + st[pl]["staged"] + st[pl].get("none", 0) == 32, (r, b, pl, st[pl])


def test_tile_states_a_quarter_of_the_map_behind_the_camera():
    w, h, dw, dh = 128, 72, 130, 70
    mx, my = shape_maps(w, h, dw, dh, 3, ROTS[3])
    nan = np.isnan(mx)
    assert 0.2 < nan.mean() < 0.3 and np.array_equal(nan, np.isnan(my))
    tiles = [nan[y:y + 16, x:x + 64] for y in range(0, dh, 16) for x in range(0, dw, 64)]
    mixed, all_nan = sum(bool(t.any() and not t.all()) for t in tiles), sum(bool(t.all()) for t in tiles)
    assert mixed > 0 and all_nan > 0
    for r, b in [(r, b) for r in wd.RESAMPLERS for b in (wd.CONSTANT, wd.REPLICATE)]:
        st = tile_states(r, mx, my, w, h, b)
        s = st["bgr"]
        if b == wd.CONSTANT and r != "linear":     # a NaN entry quantises to (-32768, -32768): it touches nothing and stays out of the box
            assert s["none"] >= all_nan and s["staged"] > 0, (r, s)
        elif b == wd.CONSTANT:                     # INTER_LINEAR clamps such a tap to (-2, -2): a tile of NaN entries stages a 2 x 2 box outside
            assert s["outside_staged"] >= all_nan and s["staged"] > 0, (r, s)
        else:                                       # every footprint counts: the box of a tile that holds a NaN entry beside a number reaches -32768
            assert s["gathered"] >= mixed and s["outside_staged"] >= all_nan, (r, s)


# ---------------------------------------------------------------------------------------------------------------------
# the new kernels' resources
# ---------------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch(tmp_path):
    """The 48 MAP_RECTD_* instantiations of the tile kernels (map modes 12 / 13 of the kernel templates) and the two map-plane kernels have
    a private segment of 0, from the kernel metadata of the library as built; k_warp_border's are compared with their siblings of mode 3 / 4."""
    lib = shutil.copy(os.path.join(ROOT, "video-annotator_amd", "lib", "libvstab.so"), tmp_path / "libvstab.so")
    subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "--offloading", str(lib)], check=True, capture_output=True)     # code objects beside the copy
    sizes = {}
    for obj in sorted(tmp_path.glob("libvstab.so.*gfx950")):
        notes = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            sizes[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    new = [n for n in sizes if re.match(r"_ZN5vstab\d+k_(warp_border|warp_cubic_rs|warp_lanczos4_rs|create_map_ex)ILi(12|13)E", n)]
    count = {}
    for n in new:
        fam = re.match(r"_ZN5vstab\d+(k_\w+?)ILi", n).group(1)
        count[fam] = count.get(fam, 0) + 1
        assert sizes[n] == 0, (n, sizes[n])
        if fam == "k_warp_border":
            sibling = n.replace("ILi12E", "ILi3E", 1).replace("ILi13E", "ILi4E", 1)
            assert sibling in sizes and sibling != n and sizes[sibling] == 0, n
    assert count == {"k_warp_border": 16, "k_warp_cubic_rs": 16, "k_warp_lanczos4_rs": 16, "k_create_map_ex": 2}, count
