"""GPU tests of the lens distortion (include/vstab.h "Lens distortion"): the map planes, the quantised map, the fused BGR and plane-wise
NV12 warps, and a calibrated handle, every float and byte against the numpy definition (tests/distort_def.py) and the golden vectors
(tests/golden/distort_kat.npz).  Shapes: the smallest that reach every path of the tiled kernels -- partial tiles right and below, more
than one workgroup, a source plane off its alignment (the gather path), boxes over the LDS budget, and the smallest output that selects
the 64 x 32-tile kernels."""
import ctypes
import os

import numpy as np
import pytest

import distort_def as dd
import layouts
import oracle
import synth
from test_lens_gpu import ROTS

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
INT_MIN = -(2 ** 31)


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cameras(w, h, dw, dh, mode, aniso=1.0):
    Kin = oracle.lens_camera(oracle.PROJ_FISH, 150.0, w, h)
    Kin[1, 1] *= aniso
    Kout = oracle.lens_camera(oracle.PROJ_RECT if mode == 1 else oracle.PROJ_FISH, 110.0 if mode == 1 else 165.0, dw, dh)
    return Kin, Kout


def same_map(got_x, got_y, ex, ey, what):
    nan = np.isnan(ex)
    assert np.array_equal(np.isnan(got_x), nan) and np.array_equal(np.isnan(got_y), nan), what
    assert np.array_equal(bits(got_x)[~nan], bits(ex)[~nan]) and np.array_equal(bits(got_y)[~nan], bits(ey)[~nan]), what


# ---------------------------------------------------------------------------------------------------------------------
# map planes and quantised map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("w,h,dw,dh", [(128, 72, 96, 64), (128, 72, 130, 70), (640, 360, 481, 271)])
def test_map_planes_and_quantised_map_bit_exact(vs, cuda, w, h, dw, dh, mode):
    Kin, Kout = cameras(w, h, dw, dh, mode)                 # lens_camera: the principal point is (dw / 2, dh / 2)
    for D in (dd.D_A, dd.D_B):
        for rv in ROTS:
            p = oracle.map_params(Kin, Kout, oracle.rodrigues(rv))
            ex, ey = dd.maps(p, dw, dh, mode, D)
            mx, my = vs.create_map_dist(p, D, dw, dh, mode)
            same_map(mx.cpu().numpy(), my.cpu().numpy(), ex, ey, (mode, D, rv))
            q = vs.quantised_map_dist(p, D, dw, dh, mode).cpu().numpy().view(np.int32).reshape(dh, -1, 2)[:, :dw]
            qx, qy, ok = dd.quantised(ex, ey)
            inr = ok & (np.abs(qx) < 2 ** 30) & (np.abs(qy) < 2 ** 30)
            assert np.array_equal(q[..., 0][inr], qx[inr]) and np.array_equal(q[..., 1][inr], qy[inr]), (mode, D, rv)
            assert (q[..., 0][~ok] == INT_MIN).all()
            if rv == ROTS[0] and dw % 2 == 0 and dh % 2 == 0:    # the axis pixel exists: correction factor 1, the input centre exactly
                assert ex[dh // 2, dw // 2] == np.float32(Kin[0, 2]) and ey[dh // 2, dw // 2] == np.float32(Kin[1, 2])
                assert float(mx[dh // 2, dw // 2]) == Kin[0, 2] and float(my[dh // 2, dw // 2]) == Kin[1, 2]
            if rv == ROTS[3]:
                assert np.isnan(ex).any() and not np.isnan(ex).all()      # part of the frame is behind the camera


# ---------------------------------------------------------------------------------------------------------------------
# warps
# ---------------------------------------------------------------------------------------------------------------------
class Expected:
    """The definition's frames for one (frame, parameters, size, mode, D), computed once; checked not to be black and to differ from the
    undistorted frame in at least half of the pixels."""

    def __init__(self, f, p, dw, dh, mode, D):
        mx, my = dd.maps(p, dw, dh, mode, D)
        zx, zy = oracle.create_map_ex(p, dw, dh, mode)
        src = oracle.cvt_nv12_bgr(f)
        h = f.shape[0] * 2 // 3
        self.bgr = oracle.remap_bilinear(src, mx, my)
        self.luma, self.chroma = oracle.warp_planar_mapped(f[:h], f[h:], mx, my)
        plain = oracle.remap_bilinear(src, zx, zy)
        assert (self.bgr != 0).mean() >= 0.1, "the expected frame is black"
        assert (self.bgr != plain).any(axis=-1).mean() >= 0.5, "the distortion moves too few pixels of this frame"


def check_bgr(vs, cuda, fd, p, D, dw, dh, mode, exp, pad=0):
    import torch
    out = torch.full((dh, dw * 3 + pad + 5), 7, dtype=torch.uint8, device=cuda)
    got = vs.warp_nv12_dist(fd, p, D, dw, dh, mode, vs.OUT_BGR8, out=out[:, pad:pad + dw * 3].unflatten(1, (dw, 3)))
    assert np.array_equal(got.cpu().numpy(), exp.bgr), ("bgr", mode, D, dw, dh, pad)
    assert bool((out[:, :pad] == 7).all()) and bool((out[:, pad + dw * 3:] == 7).all())      # guard bytes untouched


def check_planar(vs, cuda, fd, p, D, dw, dh, mode, exp, pad=0):
    import torch
    cw = (dw + 1) // 2
    yb = torch.full((dh, dw + pad + 8), 7, dtype=torch.uint8, device=cuda)
    cb = torch.full(((dh + 1) // 2, 2 * cw + pad + 8), 7, dtype=torch.uint8, device=cuda)
    y, c = vs.warp_nv12_dist(fd, p, D, dw, dh, mode, vs.OUT_NV12_PLANAR, out=(yb[:, pad:pad + dw], cb[:, pad:pad + 2 * cw]))
    assert np.array_equal(y.cpu().numpy(), exp.luma) and np.array_equal(c.cpu().numpy(), exp.chroma), ("planar", mode, D, dw, dh, pad)
    assert bool((yb[:, pad + dw:] == 7).all()) and bool((cb[:, pad + 2 * cw:] == 7).all())
    assert bool((yb[:, :pad] == 7).all()) and bool((cb[:, :pad] == 7).all())


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("w,h,dw,dh", [(128, 72, 96, 64), (128, 72, 130, 70), (640, 360, 333, 201)])
def test_warp_small_shapes_both_formats_and_the_mapped_warp(vs, cuda, w, h, dw, dh, mode):
    f = synth.nv12(dw + mode, w, h, full_range=True)
    fd = dev(f, cuda)
    Kin, Kout = cameras(w, h, dw, dh, mode)
    # (the third rotation puts a tenth to a fifth of the frame behind the camera -- ROTS[3] puts half of it there, and a frame that is
    #  half black cannot differ from the undistorted one in half of its pixels; the maps of ROTS[3] are checked above)
    for D, rv in ((dd.D_A, ROTS[1]), (dd.D_B, ROTS[2]), (dd.D_A, (0.0, 0.8, 0.0))):
        p = oracle.map_params(Kin, Kout, oracle.rodrigues(rv))
        exp = Expected(f, p, dw, dh, mode, D)
        assert rv != (0.0, 0.8, 0.0) or np.isnan(dd.maps(p, dw, dh, mode, D)[0]).mean() > 0.05
        check_bgr(vs, cuda, fd, p, D, dw, dh, mode, exp)
        check_planar(vs, cuda, fd, p, D, dw, dh, mode, exp)
        q = vs.quantised_map_dist(p, D, dw, dh, mode)           # what a calibrated handle warps a run of equal frames from
        assert np.array_equal(vs.warp_nv12_mapped(fd, q, dw, dh, vs.OUT_BGR8).cpu().numpy(), exp.bgr), (mode, D, rv)


@pytest.mark.parametrize("mode", [1, 2])
def test_warp_anisotropic_camera_and_unaligned_destinations(vs, cuda, mode):
    w, h = 320, 180
    f = synth.nv12(5, w, h, full_range=True)
    fd = dev(f, cuda)
    for (dw, dh, pad) in [(67, 35, 1), (130, 75, 3), (64, 32, 2)]:
        Kin, Kout = cameras(w, h, dw, dh, mode, aniso=1.2)          # fx != fy
        p = oracle.map_params(Kin, Kout, oracle.rodrigues((0.01, 0.02, -0.05)))
        exp = Expected(f, p, dw, dh, mode, dd.D_A)
        check_bgr(vs, cuda, fd, p, dd.D_A, dw, dh, mode, exp, pad=pad)
        check_planar(vs, cuda, fd, p, dd.D_A, dw, dh, mode, exp, pad=pad)


def raw_warp(vs, cuda, s, p, D, dw, dh, mode, fmt):
    """vstab_warp_nv12_dist with separate source planes (layouts.Src) into guarded output planes."""
    pp = np.ascontiguousarray(p, np.float32)
    d = np.ascontiguousarray(D, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    if fmt == vs.OUT_BGR8:
        o = layouts.Plane(dh, 3 * dw, cuda)
        args = (o.ptr, o.pitch, None, 0)
    else:
        oy, ou = layouts.out_nv12(dw, dh, cuda)
        args = (oy.ptr, oy.pitch, ou.ptr, ou.pitch)
    st = vs.lib.vstab_warp_nv12_dist(s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp.ctypes.data_as(fp), d.ctypes.data_as(fp), mode, fmt, *args, dw, dh,
                                     vs._stream())
    assert st == vs.OK, vs.lib.vstab_last_error()
    if fmt == vs.OUT_BGR8:
        return o.host(shape=(dh, dw, 3))
    return oy.host(), ou.host()


@pytest.mark.parametrize("mode", [1, 2])
def test_warp_source_plane_offset_by_one_byte_takes_the_gather_path(vs, cuda, mode):
    w, h, dw, dh = 128, 72, 130, 70
    f = synth.nv12(9, w, h, full_range=True)
    s = layouts.place(f[:h], f[h:], None, cuda, spec=(w + 24, w + 40, "two", 1, 2))     # luma at an odd address, chroma 2-byte aligned only
    assert s.y % 2 == 1 and s.uv % 4 == 2
    Kin, Kout = cameras(w, h, dw, dh, mode)
    p = oracle.map_params(Kin, Kout, oracle.rodrigues(ROTS[1]))
    exp = Expected(f, p, dw, dh, mode, dd.D_B)
    assert np.array_equal(raw_warp(vs, cuda, s, p, dd.D_B, dw, dh, mode, vs.OUT_BGR8), exp.bgr)
    y, c = raw_warp(vs, cuda, s, p, dd.D_B, dw, dh, mode, vs.OUT_NV12_PLANAR)
    assert np.array_equal(y, exp.luma) and np.array_equal(c, exp.chroma)


@pytest.mark.parametrize("mode", [1, 2])
def test_warp_compressing_geometry_with_boxes_over_the_lds_budget(vs, cuda, mode):
    """2048 x 1152 -> 256 x 128: a 64 x 16 tile reads a source box of about 512 x 144 pixels, far over 20 KB of LDS."""
    w, h, dw, dh = 2048, 1152, 256, 128
    f = synth.nv12(3, w, h, full_range=True)
    fd = dev(f, cuda)
    Kin, Kout = cameras(w, h, dw, dh, mode)
    p = oracle.map_params(Kin, Kout, oracle.rodrigues(ROTS[1]))
    exp = Expected(f, p, dw, dh, mode, dd.D_A)
    check_bgr(vs, cuda, fd, p, dd.D_A, dw, dh, mode, exp)
    check_planar(vs, cuda, fd, p, dd.D_A, dw, dh, mode, exp)


@pytest.mark.parametrize("mode", [1, 2])
def test_warp_smallest_output_of_the_64x32_tile_kernels(vs, cuda, mode):
    """4096 x 768 is 64 x 24 = 1536 tiles of 32 rows: the smallest count at which the launchers choose the 64 x 32-tile kernels."""
    w, h, dw, dh = 1280, 256, 4096, 768
    assert ((dw + 63) // 64) * ((dh + 31) // 32) == 1536
    f = synth.nv12(8, w, h, full_range=True)
    fd = dev(f, cuda)
    Kin, Kout = cameras(w, h, dw, dh, mode)
    p = oracle.map_params(Kin, Kout, oracle.rodrigues(ROTS[1]))
    exp = Expected(f, p, dw, dh, mode, dd.D_A)
    check_bgr(vs, cuda, fd, p, dd.D_A, dw, dh, mode, exp)
    check_planar(vs, cuda, fd, p, dd.D_A, dw, dh, mode, exp)


@pytest.mark.parametrize("mode", [1, 2])
def test_zero_distortion_is_the_plain_warp_byte_for_byte(vs, cuda, mode):
    for (w, h, dw, dh) in [(128, 72, 130, 70), (640, 360, 333, 201)]:
        f = synth.nv12(2, w, h)
        fd = dev(f, cuda)
        Kin, Kout = cameras(w, h, dw, dh, mode)
        p = oracle.map_params(Kin, Kout, oracle.rodrigues(ROTS[2]))
        a = vs.warp_nv12_dist(fd, p, dd.D_0, dw, dh, mode, vs.OUT_BGR8)
        b = vs.warp_nv12(fd, p, dw, dh, mode, vs.OUT_BGR8)
        assert bool((a == b).all()) and bool((b != 0).any())
        ya, ca = vs.warp_nv12_dist(fd, p, dd.D_0, dw, dh, mode, vs.OUT_NV12_PLANAR)
        yb, cb = vs.warp_nv12(fd, p, dw, dh, mode, vs.OUT_NV12_PLANAR)
        assert bool((ya == yb).all()) and bool((ca == cb).all())
        mx, my = vs.create_map_dist(p, dd.D_0, dw, dh, mode)
        ox, oy = vs.create_map(p, dw, dh, mode=mode)
        same_map(mx.cpu().numpy(), my.cpu().numpy(), ox.cpu().numpy(), oy.cpu().numpy(), mode)


def test_golden_vectors(vs, cuda):
    kat = np.load(os.path.join(GOLD, "distort_kat.npz"))
    k = 0
    while f"case{k}_src" in kat.files:
        f, p, D, mode = kat[f"case{k}_src"], kat[f"case{k}_params"], kat[f"case{k}_dist"], int(kat[f"case{k}_mode"])
        dw, dh = (int(v) for v in kat[f"case{k}_size"])
        fd = dev(f, cuda)
        assert np.array_equal(vs.warp_nv12_dist(fd, p, D, dw, dh, mode, vs.OUT_BGR8).cpu().numpy(), kat[f"case{k}_bgr"]), k
        y, c = vs.warp_nv12_dist(fd, p, D, dw, dh, mode, vs.OUT_NV12_PLANAR)
        assert np.array_equal(y.cpu().numpy(), kat[f"case{k}_luma"]) and np.array_equal(c.cpu().numpy(), kat[f"case{k}_chroma"]), k
        if f"case{k}_mapx" in kat.files:
            mx, my = vs.create_map_dist(p, D, dw, dh, mode)
            same_map(mx.cpu().numpy(), my.cpu().numpy(), kat[f"case{k}_mapx"], kat[f"case{k}_mapy"], k)
        k += 1
    assert k == 4


# ---------------------------------------------------------------------------------------------------------------------
# a calibrated handle
# ---------------------------------------------------------------------------------------------------------------------
W, H, OW, OH = 320, 180, 240, 136
LENS = dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=OW, out_height=OH)
K_CAL = np.array([[118.0, 0.0, 161.5], [0.0, 121.0, 88.0], [0.0, 0.0, 1.0]])     # a calibrated camera matrix: fx != fy, centre off the middle


def run(vs, cuda, frames, nv12=False, **cfg):
    import torch
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), **cfg)
    outs = []
    while True:
        o = stab.pull_nv12(planar=True) if nv12 else stab.pull()
        if o is None:
            break
        outs.append(tuple(t.cpu().numpy() for t in o) if nv12 else o.cpu().numpy())
    return stab, outs


@pytest.fixture(scope="module")
def still_clip():
    return [synth.nv12(60 + k, W, H) for k in range(8)]


def test_pipeline_tracking_off_warps_with_the_calibration(vs, cuda, still_clip):
    frames = still_clip
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, OW, OH)
    p = oracle.map_params(K_CAL, Kout, np.eye(3))
    cfg = dict(LENS, smooth_radius=2, tracking=0)
    stab, outs = run(vs, cuda, frames, calibration=(K_CAL, dd.D_A), **cfg)
    assert len(outs) == 7 and stab.out_size == (OW, OH) and np.array_equal(stab.K_in, K_CAL)
    for i, o in enumerate(outs):
        assert np.allclose(stab.warp_rotation(i), np.eye(3), atol=1e-12)
        assert np.array_equal(o, dd.warp_bgr(frames[i + 1], p, OW, OH, 1, dd.D_A)), i
    assert stab.warps_from_cache() == 6       # every frame but the first is warped from the quantised map written for the second
    plain = oracle.warp_nv12_ex(frames[1], p, OW, OH, oracle.MAP_FISH_TO_RECT, 0)
    assert (outs[0] != plain).any(axis=-1).mean() > 0.5
    # plane-wise pulls always evaluate the map
    stab, outs = run(vs, cuda, frames, nv12=True, calibration=(K_CAL, dd.D_A), **cfg)
    assert len(outs) == 7 and stab.warps_from_cache() == 0
    for i, (y, c) in enumerate(outs):
        ey, ec = dd.warp_planar(frames[i + 1], p, OW, OH, 1, dd.D_A)
        assert np.array_equal(y, ey) and np.array_equal(c, ec), i
    # zero coefficients and no matrix: the handle without the call
    _, zero = run(vs, cuda, frames, calibration=(None, 0), **cfg)
    _, none = run(vs, cuda, frames, **cfg)
    assert len(zero) == len(none) == 7 and all(np.array_equal(a, b) for a, b in zip(zero, none))


TW, TH, TN, TR = 640, 360, 40, 5      # size, length and shake of test_pipeline_gpu.test_rotation_estimates_follow_ground_truth_and_stabilise


@pytest.fixture(scope="module")
def shaky():
    K = oracle.get_preset_camera(4, TW, TH)
    frames, rots = dd.shaky_clip(3, K, dd.D_A, TW, TH, TN, sigma=0.004)
    return K, frames, rots


def rotation_errors(stab, rots):
    log = stab.frame_log()
    return [oracle.rotation_angle(lg["R"] @ (rots[k] @ rots[k - 1].T).T) for k, lg in enumerate(log, start=1)], log


def test_pipeline_tracking_through_a_distorted_lens(vs, cuda, shaky):
    """A clip rendered through a D_A lens: with the calibration the rotation estimates meet the bounds of the ideal-lens pipeline test (the
    model is exact in both), and beat the estimates made without it; pixels are the definition's warp with the handle's own rotation."""
    K, frames, rots = shaky
    cfg = dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=480, out_height=270, smooth_radius=TR, seed=5)
    stab, outs = run(vs, cuda, frames, calibration=(K, dd.D_A), **cfg)
    assert len(outs) == TN - 1
    errs, log = rotation_errors(stab, rots)
    assert all(lg["inliers"] >= 40 and not lg["fallback"] for lg in log)
    plain, _ = run(vs, cuda, frames, calibration=(K, 0), **cfg)
    errs0, _ = rotation_errors(plain, rots)
    print("rotation error, median / max: calibrated %.3e / %.3e, D left at zero %.3e / %.3e" % (np.median(errs), max(errs), np.median(errs0), max(errs0)))
    assert np.median(errs) < 1.5e-3 and max(errs) < 6e-3, (np.median(errs), max(errs))
    assert np.median(errs) < np.median(errs0)
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, 480, 270)
    for i in (0, 1, TR, TN - 2):
        p = oracle.map_params(K, Kout, stab.warp_rotation(i))
        assert np.array_equal(outs[i], dd.warp_bgr(frames[i + 1], p, 480, 270, 1, dd.D_A)), i


def to_output(pts, K, D, Kout, R):
    """Where the warp sends input pixels: pixel -> theta_d -> theta (Newton) -> ray -> R^T -> the pinhole output camera."""
    out = []
    for x, y in np.asarray(pts, np.float64):
        a, b = (x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]
        td = np.hypot(a, b)
        th, ok, _ = dd.undistort_theta(td, D) if td > 0 else (0.0, True, 0)
        s = np.sin(th) / td if td > 0 else 1.0
        o = R.T @ np.array([a * s, b * s, np.cos(th)])
        if ok and o[2] > 0:
            out.append((Kout[0, 2] + Kout[0, 0] * o[0] / o[2], Kout[1, 2] + Kout[1, 1] * o[1] / o[2]))
    return np.array(out)


def test_debug_markers_go_through_the_distorted_lens(vs, cuda, shaky):
    K, frames, _ = shaky
    cfg = dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=480, out_height=270, smooth_radius=1, seed=3)
    plain_stab, plain = run(vs, cuda, frames[:5], calibration=(K, dd.D_A), **cfg)
    dbg_stab, dbg = run(vs, cuda, frames[:5], calibration=(K, dd.D_A), debug=1, **cfg)
    R = dbg_stab.warp_rotation(0)
    assert np.array_equal(R, plain_stab.warp_rotation(0))
    corners = oracle.good_features(np.ascontiguousarray(frames[0][:TH]))
    nxt, st = oracle.pyr_lk(frames[0][:TH], frames[1][:TH], corners)
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, 480, 270)
    centres = to_output(nxt[st > 0], K, dd.D_A, Kout, R)
    ideal = to_output(nxt[st > 0], K, dd.D_0, Kout, R)
    assert len(centres) > 40 and np.abs(centres - ideal).max() > 2          # the undistorted projection would put markers elsewhere
    marked = (dbg[0] != plain[0]).any(axis=-1)
    green = (dbg[0] == (0, 255, 0)).all(axis=-1)
    assert marked.sum() > 20 * 49
    inside = [(x, y) for x, y in centres if 4 <= x < 480 - 4 and 4 <= y < 270 - 4]
    assert len(inside) > 30
    allowed = np.zeros_like(marked)
    for x, y in centres:
        cx, cy = int(np.rint(x)), int(np.rint(y))
        allowed[max(cy - 4, 0):cy + 5, max(cx - 4, 0):cx + 5] = True       # a 7 x 7 square within one pixel of the expected centre
    assert not (marked & ~allowed).any()
    for x, y in inside:                                                    # and every expected square is there
        cx, cy = int(np.rint(x)), int(np.rint(y))
        assert green[cy - 2:cy + 3, cx - 2:cx + 3].all(), (x, y)


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need a live handle: status, the whole message, and whether a frame was consumed
# ---------------------------------------------------------------------------------------------------------------------
SET = "vstab_set_input_calibration: "
SERVED = " emits 8-bit BGR or plane-wise NV12 frames (vstab_pull_frame / _frames / _host / vstab_peek_frame / vstab_pull_frame_nv12_planar), not NV12 through BGR"


def refused(vs, fn, *args):
    with pytest.raises(vs.VstabError) as e:
        fn(*args)
    return e.value.status, vs.lib.vstab_last_error().decode()


def test_calibration_refusals_on_live_handles(vs, cuda, still_clip):
    import torch
    frames = still_clip[:5]
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, OW, OH)
    p = oracle.map_params(K_CAL, Kout, np.eye(3))
    base = dict(LENS, smooth_radius=1, tracking=0)
    INV = vs.ERR_INVALID

    def handle(**kw):
        return vs.Stabilizer(devf, total=len(devf), **dict(base, **kw))

    # the kinds of handle that cannot be calibrated
    assert refused(vs, handle(resample=vs.RESAMPLE_CUBIC).set_input_calibration, K_CAL, dd.D_A) == (
        INV, SET + "the distorted-lens warp resamples with VSTAB_RESAMPLE_DEFAULT, this handle with VSTAB_RESAMPLE_CUBIC")
    wide = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in frames]
    h10 = vs.Stabilizer(wide, total=len(wide), bit_depth=10, pixel_depth=10, **base)
    assert refused(vs, h10.set_input_calibration, K_CAL, dd.D_A) == (INV, SET + "the distorted-lens warp takes 8-bit pixels, this is a pixel_depth 10 handle")
    assert refused(vs, handle(border_mode=vs.BORDER_REFLECT_101).set_input_calibration, K_CAL, dd.D_A) == (
        INV, SET + "the distorted-lens warp has the constant border, this handle has another border mode set (vstab_set_border_mode)")
    assert refused(vs, vs.Stabilizer(devf, total=len(devf), smooth_radius=1, tracking=0).set_input_calibration, K_CAL, dd.D_A) == (
        INV, SET + "a calibration belongs to lens_mode 1 (the preset path derives its output camera from the input's)")
    assert refused(vs, handle(in_projection=0, in_dfov=100.0).set_input_calibration, K_CAL, dd.D_A) == (
        INV, SET + "distortion belongs to a fisheye input (in_projection VSTAB_PROJ_FISH)")
    # bad arguments on a good handle: the handle stays uncalibrated
    s = handle()
    bad_K = K_CAL.copy()
    bad_K[0, 1] = 0.5
    assert refused(vs, s.set_input_calibration, bad_K, dd.D_A) == (INV, SET + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1")
    assert refused(vs, s.set_input_calibration, K_CAL, (-0.5, 0, 0, 0)) == (INV, "vstab_set_input_calibration: the distortion must keep theta_d increasing on [0, pi/2]")
    assert refused(vs, s.set_input_calibration, bad_K, (-0.5, 0, 0, 0))[1] == SET + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1"
    Kin = oracle.lens_camera(oracle.PROJ_FISH, 150.0, W, H)
    assert np.array_equal(s.pull().cpu().numpy(), oracle.warp_nv12_ex(frames[1], oracle.map_params(Kin, Kout, np.eye(3)), OW, OH, 1, 0))
    # ... and after the first pull it is too late
    assert refused(vs, s.set_input_calibration, K_CAL, dd.D_A) == (INV, SET + "the calibration must be set before the first pull")
    assert np.array_equal(s.pull().cpu().numpy(), oracle.warp_nv12_ex(frames[2], oracle.map_params(Kin, Kout, np.eye(3)), OW, OH, 1, 0))

    # a calibrated handle: no border mode, no NV12 through BGR (refused before a frame is taken)
    s = handle(calibration=(K_CAL, dd.D_A))
    for fn, name in ((s.set_border_mode, "vstab_set_border_mode"), (s.set_border_mode_ex, "vstab_set_border_mode_ex")):
        assert refused(vs, fn, vs.BORDER_REPLICATE) == (INV, name + ": a calibrated handle (vstab_set_input_calibration) warps with VSTAB_BORDER_CONSTANT")
    s.set_border_mode(vs.BORDER_CONSTANT)
    assert refused(vs, s.pull_nv12) == (INV, "vstab_pull_frame: a calibrated handle (vstab_set_input_calibration)" + SERVED)
    assert np.array_equal(s.pull().cpu().numpy(), dd.warp_bgr(frames[1], p, OW, OH, 1, dd.D_A))       # the first frame is still there
    o = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
    assert vs.lib.vstab_peek_frame(s._h, o.data_ptr(), o.stride(0)) == vs.OK                          # every served pull
    assert np.array_equal(o.cpu().numpy(), dd.warp_bgr(frames[2], p, OW, OH, 1, dd.D_A))
    assert np.array_equal(s.pull_host(), dd.warp_bgr(frames[3], p, OW, OH, 1, dd.D_A))
    assert s.pull_frames_into([o], 0, 1) == 1 and np.array_equal(o.cpu().numpy(), dd.warp_bgr(frames[4], p, OW, OH, 1, dd.D_A))
    assert s.pull() is None

    # a frame that carries a read-out rotation is refused and consumed: input frames 1 and 3 carry one, 2 and 4 are delivered
    ro = np.ascontiguousarray(oracle.rodrigues((0.002, -0.003, 0.001)), np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    state = {"i": 0}

    def fill(out, advance):
        i = state["i"]
        if i >= len(devf):
            return vs.EOF
        t, o = devf[i], out.contents
        o.y, o.uv = t.data_ptr(), t.data_ptr() + H * t.stride(0)
        o.pitch_y = o.pitch_uv = t.stride(0)
        o.width, o.height, o.mem, o.pts, o.hold, o.bit_depth = W, H, 0, i, 1 << 30, 8
        o.readout_rotation = ro.ctypes.data_as(dp) if i in (1, 3) else None
        if advance:
            state["i"] += 1
        return 0
    pull, peek = vs.PULL_FN(lambda u, o: fill(o, True)), vs.PULL_FN(lambda u, o: fill(o, False))
    src = vs.Source(pull, peek, None)
    cfg = vs.default_config(**base)
    h = ctypes.c_void_p()
    assert vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(src), ctypes.byref(h)) == vs.OK, vs.lib.vstab_last_error()
    try:
        Kc, Dc = np.ascontiguousarray(K_CAL.reshape(9)), np.array(dd.D_A, np.float64)
        assert vs.lib.vstab_set_input_calibration(h, Kc.ctypes.data_as(dp), Dc.ctypes.data_as(dp)) == vs.OK, vs.lib.vstab_last_error()
        for k in range(1, len(devf)):
            o = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
            st = vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0))
            if k in (1, 3):
                assert st == INV, k
                assert vs.lib.vstab_last_error() == b"a calibrated handle (vstab_set_input_calibration) warps frames without a read-out rotation"
            else:
                assert st == vs.OK, (k, vs.lib.vstab_last_error())
                assert np.array_equal(o.cpu().numpy(), dd.warp_bgr(frames[k], p, OW, OH, 1, dd.D_A)), k
        assert vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0)) == vs.EOF
    finally:
        vs.lib.vstab_destroy(h)
