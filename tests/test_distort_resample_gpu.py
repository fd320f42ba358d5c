"""GPU tests of the calibrated lens in the cubic, Lanczos and border warps (include/vstab.h, vstab_warp_nv12_dist_ex and
vstab_set_input_calibration_ex): every byte, BGR and plane-wise, against the numpy definition -- the distorted map (tests/distort_def.py)
fed to the resampler's own definition (tests/warp_def.py) --, against the entry points the new one must agree with, and
against the route it replaces (vstab_create_map_dist + a stateless vstab_remap_*).  Shapes: the smallest that reach the tile states
test_distort_resample_cpu.py asserts for them (all staged with partial tiles and edge crossings; staged and gathered in one launch; every
tile gathered; a third of the map NaN), a source plane off its alignment, a 16 x 2 source, and a calibrated handle through every pull."""
import ctypes
import os

import numpy as np
import pytest

import distort_def as dd
import layouts
import oracle
import synth
import warp_def as wd
from test_border_gpu import pulls
from test_distort_gpu import H, K_CAL, LENS, OH, OW, W, cameras, dev, refused
from test_lens_gpu import ROTS

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
RESAMPLERS, RESAMPLE, BORDERS = wd.RESAMPLERS, wd.RESAMPLE, wd.MODES
CONSTANT, REPLICATE, REFLECT, REFLECT_101 = wd.CONSTANT, wd.REPLICATE, wd.REFLECT, wd.REFLECT_101


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got != exp
    assert not bad.any(), (what, int(bad.sum()), "of", bad.size, "first at", tuple(int(v[0]) for v in np.nonzero(bad)))


class Case:
    """One frame, parameter set and size: the distorted map evaluated once, the definition's frames of any (resampler, border) from it."""

    def __init__(self, w, h, dw, dh, mode, rv, D=dd.D_A, aniso=1.0, seed=None, frame=None):
        self.w, self.h, self.dw, self.dh, self.mode, self.D = w, h, dw, dh, mode, D
        self.f = synth.nv12(dw + mode if seed is None else seed, w, h, full_range=True) if frame is None else frame
        Kin, Kout = cameras(w, h, dw, dh, mode, aniso)
        self.p = oracle.map_params(Kin, Kout, oracle.rodrigues(rv))
        self.mx, self.my = dd.maps(self.p, dw, dh, mode, D)

    def bgr(self, resampler, border):
        return wd.bgr(self.f, self.mx, self.my, resampler, border)

    def planar(self, resampler, border):
        return wd.planar(self.f, self.mx, self.my, resampler, border)

    def check(self, vs, fd, resampler, border, what=None):
        """Both output formats of vstab_warp_nv12_dist_ex (through the binding, packed source fd) against the definition."""
        what = (what, resampler, border, self.mode, self.dw, self.dh)
        got = vs.warp_nv12_dist_ex(fd, self.p, self.D, self.dw, self.dh, self.mode, RESAMPLE[resampler], border, vs.OUT_BGR8)
        eq(got.cpu().numpy(), self.bgr(resampler, border), what + ("bgr",))
        y, c = vs.warp_nv12_dist_ex(fd, self.p, self.D, self.dw, self.dh, self.mode, RESAMPLE[resampler], border, vs.OUT_NV12_PLANAR)
        ey, ec = self.planar(resampler, border)
        eq(y.cpu().numpy(), ey, what + ("luma",)), eq(c.cpu().numpy(), ec, what + ("chroma",))
        return got


def stateless_bgr(vs, fd, case, resampler, border):
    """The route the fused kernels replace: vstab_create_map_dist, then the stateless remap of the BGR conversion."""
    mx, my = vs.create_map_dist(case.p, case.D, case.dw, case.dh, case.mode)
    src = vs.cvt_nv12_bgr(fd)
    if resampler == "linear":
        return vs.remap_bilinear_border(src, mx, my, border)
    return (vs.remap_cubic_border if resampler == "cubic" else vs.remap_lanczos4_border)(src, mx, my, border, (0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------------
# every combination once
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_every_resampler_border_and_mode(vs, cuda, resampler, mode):
    w, h, dw, dh = 128, 72, 130, 70
    c = Case(w, h, dw, dh, mode, ROTS[1])
    fd = dev(c.f, cuda)
    zx, zy = dd.maps(c.p, dw, dh, mode, dd.D_0)
    for border in BORDERS:
        got = c.check(vs, fd, resampler, border, "all").cpu().numpy()
        plain = wd.bgr(c.f, zx, zy, resampler, border)                     # the D = 0 frame
        assert (got != 0).mean() >= 0.1, ("black", resampler, border, mode)
        assert (got != plain).any(axis=-1).mean() >= 0.5, ("the distortion moved too few pixels", resampler, border, mode)
        eq(stateless_bgr(vs, fd, c, resampler, border).cpu().numpy(), got, ("stateless route", resampler, border, mode))


# ---------------------------------------------------------------------------------------------------------------------
# the tile-state shapes (test_distort_resample_cpu.py asserts the states)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("resampler", RESAMPLERS)
@pytest.mark.parametrize("w,h,dw,dh", [(640, 360, 333, 201), (1024, 576, 200, 72)])
def test_staged_partial_crossing_and_mixed_tiles(vs, cuda, w, h, dw, dh, resampler, mode):
    c = Case(w, h, dw, dh, mode, ROTS[1])
    fd = dev(c.f, cuda)
    for border in (CONSTANT, REFLECT_101):
        c.check(vs, fd, resampler, border, "tiles")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("resampler,border", [("linear", REFLECT_101), ("cubic", CONSTANT), ("lanczos4", REPLICATE)])
def test_every_tile_over_the_lds_budget(vs, cuda, resampler, border, mode):
    """2048 x 1152 -> 256 x 128: every box is over the budget, every pixel is sampled from global memory."""
    c = Case(2048, 1152, 256, 128, mode, ROTS[1])
    c.check(vs, dev(c.f, cuda), resampler, border, "gathers")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_a_third_of_the_map_behind_the_camera(vs, cuda, resampler, mode):
    """ROTS[3]: about a third of the entries NaN; under a non-constant border the tiles that hold one beside a number gather (the box
    reaches -32768), a tile of NaN entries alone stages a small box far outside."""
    c = Case(128, 72, 130, 70, mode, ROTS[3])
    assert 0.3 < np.isnan(c.mx).mean() < 0.4
    fd = dev(c.f, cuda)
    for border in (REPLICATE, CONSTANT):
        c.check(vs, fd, resampler, border, "nan")


# ---------------------------------------------------------------------------------------------------------------------
# cameras, pitches, alignments, the smallest source
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_anisotropic_camera(vs, cuda, mode):
    c = Case(320, 180, 130, 75, mode, (0.01, 0.02, -0.05), aniso=1.07, seed=5)
    fd = dev(c.f, cuda)
    for resampler, border in (("linear", REFLECT), ("cubic", CONSTANT), ("cubic", REFLECT_101), ("lanczos4", CONSTANT), ("lanczos4", REPLICATE)):
        c.check(vs, fd, resampler, border, "aniso")


@pytest.mark.parametrize("mode", [1, 2])
def test_destinations_with_padded_pitches(vs, cuda, mode):
    """Output rows at odd offsets inside wider buffers: every byte outside the planes keeps its fill."""
    import torch
    c = Case(128, 72, 67, 35, mode, ROTS[2], D=dd.D_B, seed=7)
    fd = dev(c.f, cuda)
    dw, dh, cw = c.dw, c.dh, (c.dw + 1) // 2
    for k, (resampler, border) in enumerate((("linear", REPLICATE), ("cubic", CONSTANT), ("cubic", REFLECT), ("lanczos4", CONSTANT), ("lanczos4", REFLECT_101))):
        pad = 1 + 2 * (k % 2)
        out = torch.full((dh, dw * 3 + pad + 5), 7, dtype=torch.uint8, device=cuda)
        got = vs.warp_nv12_dist_ex(fd, c.p, c.D, dw, dh, mode, RESAMPLE[resampler], border, vs.OUT_BGR8, out=out[:, pad:pad + dw * 3].unflatten(1, (dw, 3)))
        eq(got.cpu().numpy(), c.bgr(resampler, border), ("pad bgr", resampler, border, mode))
        assert bool((out[:, :pad] == 7).all()) and bool((out[:, pad + dw * 3:] == 7).all())
        yb = torch.full((dh, dw + pad + 8), 7, dtype=torch.uint8, device=cuda)
        cb = torch.full(((dh + 1) // 2, 2 * cw + pad + 8), 7, dtype=torch.uint8, device=cuda)
        y, uv = vs.warp_nv12_dist_ex(fd, c.p, c.D, dw, dh, mode, RESAMPLE[resampler], border, vs.OUT_NV12_PLANAR, out=(yb[:, pad:pad + dw], cb[:, pad:pad + 2 * cw]))
        ey, ec = c.planar(resampler, border)
        eq(y.cpu().numpy(), ey, ("pad luma", resampler, border, mode)), eq(uv.cpu().numpy(), ec, ("pad chroma", resampler, border, mode))
        assert bool((yb[:, pad + dw:] == 7).all()) and bool((cb[:, pad + 2 * cw:] == 7).all())
        assert bool((yb[:, :pad] == 7).all()) and bool((cb[:, :pad] == 7).all())


def raw_warp(vs, cuda, s, p, D, dw, dh, mode, resampler, border, fmt):
    """vstab_warp_nv12_dist_ex with separate source planes (layouts.Src) into canaried output planes."""
    _, pp = layouts._f(p)
    _, d = layouts._f(D)
    if fmt == vs.OUT_BGR8:
        o = layouts.Plane(dh, 3 * dw, cuda)
        args = (o.ptr, o.pitch, None, 0)
    else:
        oy, ou = layouts.out_nv12(dw, dh, cuda)
        args = (oy.ptr, oy.pitch, ou.ptr, ou.pitch)
    st = vs.lib.vstab_warp_nv12_dist_ex(s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, d, mode, RESAMPLE[resampler], border, fmt, *args, dw, dh, vs._stream())
    assert st == vs.OK, vs.lib.vstab_last_error()
    if fmt == vs.OUT_BGR8:
        return o.host(shape=(dh, dw, 3))
    return oy.host(), ou.host()


def check_raw(vs, cuda, s, c, resampler, border, what):
    eq(raw_warp(vs, cuda, s, c.p, c.D, c.dw, c.dh, c.mode, resampler, border, vs.OUT_BGR8), c.bgr(resampler, border), (what, "bgr", resampler, border, c.mode))
    y, uv = raw_warp(vs, cuda, s, c.p, c.D, c.dw, c.dh, c.mode, resampler, border, vs.OUT_NV12_PLANAR)
    ey, ec = c.planar(resampler, border)
    eq(y, ey, (what, "luma", resampler, border, c.mode)), eq(uv, ec, (what, "chroma", resampler, border, c.mode))


@pytest.mark.parametrize("mode", [1, 2])
def test_source_plane_offset_by_one_byte(vs, cuda, mode):
    """Luma at an odd address, chroma 2-byte aligned only, pitches wider than the rows, planes in two allocations."""
    w, h = 128, 72
    c = Case(w, h, 130, 70, mode, ROTS[1], D=dd.D_B, seed=9)
    s = layouts.place(c.f[:h], c.f[h:], None, cuda, spec=(w + 24, w + 40, "two", 1, 2))
    assert s.y % 2 == 1 and s.uv % 4 == 2
    for resampler in RESAMPLERS:
        for border in (CONSTANT, REFLECT_101):
            check_raw(vs, cuda, s, c, resampler, border, "offset")


@pytest.mark.parametrize("mode", [1, 2])
def test_16x2_source(vs, cuda, mode):
    """Two luma rows and one chroma row: every footprint of every resampler leaves the source."""
    w, h = 16, 2
    f = np.random.default_rng(16 + mode).integers(0, 256, (3, w), dtype=np.uint8)
    c = Case(w, h, 70, 20, mode, (0.01, -0.02, 0.1), frame=f)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    for resampler in RESAMPLERS:
        for border in BORDERS:
            check_raw(vs, cuda, s, c, resampler, border, "16x2")


# ---------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_zero_distortion_is_the_undistorted_entry_point_byte_for_byte(vs, cuda, mode):
    for (w, h, dw, dh) in [(128, 72, 130, 70), (640, 360, 333, 201)]:
        f = synth.nv12(2, w, h)
        fd = dev(f, cuda)
        Kin, Kout = cameras(w, h, dw, dh, mode)
        p = oracle.map_params(Kin, Kout, oracle.rodrigues(ROTS[2]))
        for fmt in (vs.OUT_BGR8, vs.OUT_NV12_PLANAR):
            def same(a, b, what):
                a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
                for x, y in zip(a, b):
                    assert bool((x == y).all()) and bool((y != 0).any()), (what, mode, fmt, dw)
            for border in BORDERS:
                ex = lambda resample: vs.warp_nv12_dist_ex(fd, p, dd.D_0, dw, dh, mode, resample, border, fmt)       # noqa: E731
                same(ex(vs.RESAMPLE_CUBIC), vs.warp_nv12_cubic_border(fd, p, dw, dh, mode, fmt, border), ("cubic_border", border))
                same(ex(vs.RESAMPLE_LANCZOS4), vs.warp_nv12_lanczos4_border(fd, p, dw, dh, mode, fmt, border), ("lanczos4_border", border))
                if border != CONSTANT:
                    same(ex(vs.RESAMPLE_DEFAULT), vs.warp_nv12_border(fd, p, dw, dh, mode, fmt, border), ("border", border))
            ex = lambda resample: vs.warp_nv12_dist_ex(fd, p, dd.D_0, dw, dh, mode, resample, CONSTANT, fmt)         # noqa: E731
            same(ex(vs.RESAMPLE_CUBIC), vs.warp_nv12_cubic(fd, p, dw, dh, mode, fmt), "cubic")
            same(ex(vs.RESAMPLE_LANCZOS4), vs.warp_nv12_lanczos4(fd, p, dw, dh, mode, fmt), "lanczos4")
            same(ex(vs.RESAMPLE_DEFAULT), vs.warp_nv12(fd, p, dw, dh, mode, fmt), "plain")


@pytest.mark.parametrize("mode", [1, 2])
def test_inter_linear_with_the_constant_border_is_vstab_warp_nv12_dist(vs, cuda, mode):
    for (w, h, dw, dh, rv) in [(128, 72, 130, 70, ROTS[1]), (640, 360, 333, 201, ROTS[2]), (128, 72, 96, 64, ROTS[3])]:
        c = Case(w, h, dw, dh, mode, rv)
        fd = dev(c.f, cuda)
        a = vs.warp_nv12_dist_ex(fd, c.p, c.D, dw, dh, mode, vs.RESAMPLE_DEFAULT, CONSTANT, vs.OUT_BGR8)
        assert bool((a == vs.warp_nv12_dist(fd, c.p, c.D, dw, dh, mode, vs.OUT_BGR8)).all())
        eq(a.cpu().numpy(), c.bgr("linear", CONSTANT), ("linear constant", mode, dw))
        ya, ca = vs.warp_nv12_dist_ex(fd, c.p, c.D, dw, dh, mode, vs.RESAMPLE_DEFAULT, CONSTANT, vs.OUT_NV12_PLANAR)
        yb, cb = vs.warp_nv12_dist(fd, c.p, c.D, dw, dh, mode, vs.OUT_NV12_PLANAR)
        assert bool((ya == yb).all()) and bool((ca == cb).all())


def test_golden_vectors(vs, cuda):
    from test_distort_resample_cpu import golden_cases
    n = 0
    for k, c in golden_cases():
        dw, dh = (int(v) for v in c["size"])
        args = (dev(c["src"], cuda), c["params"], c["dist"], dw, dh, int(c["mode"]), int(c["resample"]), int(c["border"]))
        eq(vs.warp_nv12_dist_ex(*args, vs.OUT_BGR8).cpu().numpy(), c["bgr"], ("golden bgr", k))
        y, uv = vs.warp_nv12_dist_ex(*args, vs.OUT_NV12_PLANAR)
        eq(y.cpu().numpy(), c["luma"], ("golden luma", k)), eq(uv.cpu().numpy(), c["chroma"], ("golden chroma", k))
        n += 1
    assert n == 5


# ---------------------------------------------------------------------------------------------------------------------
# a handle calibrated with vstab_set_input_calibration_ex
# ---------------------------------------------------------------------------------------------------------------------
SETX = "vstab_set_input_calibration_ex: "
SERVED = " emits 8-bit BGR or plane-wise NV12 frames (vstab_pull_frame / _frames / _host / vstab_peek_frame / vstab_pull_frame_nv12_planar), not NV12 through BGR"
HANDLES = [("cubic", REFLECT_101), ("lanczos4", REFLECT_101), ("linear", REPLICATE)]
BASE = dict(LENS, smooth_radius=2, tracking=0)


@pytest.fixture(scope="module")
def still_clip():
    return [synth.nv12(60 + k, W, H) for k in range(8)]


@pytest.fixture(scope="module")
def still_maps():
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, OW, OH)
    p = oracle.map_params(K_CAL, Kout, np.eye(3))
    return dd.maps(p, OW, OH, 1, dd.D_A)


def expect_pull(still_maps, f, resampler, border, out, how, what):
    mx, my = still_maps
    if how == "planar":
        ey, ec = wd.planar(f, mx, my, resampler, border)
        eq(out[0], ey, (what, "luma")), eq(out[1], ec, (what, "chroma"))
    else:
        eq(out, wd.bgr(f, mx, my, resampler, border), what)


@pytest.mark.parametrize("how", ["pull", "frames", "host", "peek", "planar"])
@pytest.mark.parametrize("resampler,border", HANDLES)
def test_pipeline_pulls_of_a_calibrated_handle(vs, cuda, still_clip, still_maps, resampler, border, how):
    stab, outs = pulls(vs, cuda, still_clip, how, border, calibration_ex=(K_CAL, dd.D_A), resample=RESAMPLE[resampler], **BASE)
    assert len(outs) == len(still_clip) - 1 and stab.out_size == (OW, OH) and np.array_equal(stab.K_in, K_CAL)
    for i, o in enumerate(outs):
        assert np.allclose(stab.warp_rotation(i), np.eye(3), atol=1e-12)
        expect_pull(still_maps, still_clip[i + 1], resampler, border, o, how, (resampler, border, how, i))
    assert stab.warps_from_cache() == 0          # the quantised map serves INTER_LINEAR with the constant border only
    stab.close()


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_pipeline_border_mode_switches_between_pulls(vs, cuda, still_clip, still_maps, resampler):
    """The mode in force at a pull is the mode of its frame; a calibration set before or after the border mode; INTER_LINEAR with the
    constant border goes back to vstab_warp_nv12_dist and the quantised map."""
    import torch
    devf = [torch.from_numpy(f).to(cuda) for f in still_clip]
    stab = vs.Stabilizer(devf, total=len(devf), resample=RESAMPLE[resampler], **BASE)
    stab.set_input_calibration_ex(K_CAL, dd.D_A)
    setters = [stab.set_border_mode_ex] + ([stab.set_border_mode] if resampler == "linear" else [])
    if resampler != "linear":                    # vstab_set_border_mode behaves as on an uncalibrated handle: it serves INTER_LINEAR handles only
        assert refused(vs, stab.set_border_mode, REPLICATE)[0] == vs.ERR_UNSUPPORTED
    for bad in (3, 5, -1):
        assert vs.lib.vstab_set_border_mode_ex(stab._h, bad) == vs.ERR_INVALID
    seq = [REFLECT_101, CONSTANT, REPLICATE, REFLECT, CONSTANT, CONSTANT, REPLICATE]
    for i, bm in enumerate(seq):
        setters[i % len(setters)](bm)
        how = "planar" if i % 3 == 2 else "pull"
        o = stab.pull_nv12(planar=True) if how == "planar" else stab.pull()
        assert o is not None, i
        o = tuple(x.cpu().numpy() for x in o) if how == "planar" else o.cpu().numpy()
        expect_pull(still_maps, still_clip[i + 1], resampler, bm, o, how, ("switch", resampler, bm, i))
    assert stab.pull() is None
    assert stab.warps_from_cache() == (1 if resampler == "linear" else 0)        # pulls 1 and 4: the second BGR pull with CONSTANT writes the map down
    stab.close()


def test_pipeline_refusals_of_a_calibrated_handle(vs, cuda, still_clip, still_maps):
    import torch
    frames = still_clip[:5]
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    INV = vs.ERR_INVALID

    def handle(**kw):
        return vs.Stabilizer(devf, total=len(devf), **dict(BASE, smooth_radius=1, **kw))

    # NV12 through BGR is refused before a frame is taken, whatever refuses it first: the first frame is still there
    for kw, resampler, border, why in (
            (dict(resample=vs.RESAMPLE_CUBIC), "cubic", CONSTANT, "VSTAB_RESAMPLE_CUBIC"),
            (dict(resample=vs.RESAMPLE_LANCZOS4, border_mode=REFLECT), "lanczos4", REFLECT, "VSTAB_RESAMPLE_LANCZOS4"),
            (dict(border_mode=REPLICATE), "linear", REPLICATE, "a border mode other than VSTAB_BORDER_CONSTANT"),
            (dict(), "linear", CONSTANT, "a calibrated handle (vstab_set_input_calibration)")):
        s = handle(calibration_ex=(K_CAL, dd.D_A), **kw)
        assert refused(vs, s.pull_nv12) == (INV, "vstab_pull_frame: " + why + SERVED)
        expect_pull(still_maps, frames[1], resampler, border, s.pull().cpu().numpy(), "pull", ("after the refusal", resampler))
        s.close()

    # what vstab_set_input_calibration_ex keeps refusing, message for message; the handle stays uncalibrated
    assert refused(vs, vs.Stabilizer(devf, total=len(devf), smooth_radius=1, tracking=0).set_input_calibration_ex, K_CAL, dd.D_A) == (
        INV, SETX + "a calibration belongs to lens_mode 1 (the preset path derives its output camera from the input's)")
    assert refused(vs, handle(in_projection=0, in_dfov=100.0).set_input_calibration_ex, K_CAL, dd.D_A) == (
        INV, SETX + "distortion belongs to a fisheye input (in_projection VSTAB_PROJ_FISH)")
    wide = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in frames]
    h10 = vs.Stabilizer(wide, total=len(wide), bit_depth=10, pixel_depth=10, **dict(BASE, smooth_radius=1))
    assert refused(vs, h10.set_input_calibration_ex, K_CAL, dd.D_A) == (INV, SETX + "the distorted-lens warp takes 8-bit pixels, this is a pixel_depth 10 handle")
    s = handle(resample=vs.RESAMPLE_CUBIC, border_mode=REFLECT_101)
    bad_K = K_CAL.copy()
    bad_K[0, 1] = 0.5
    assert refused(vs, s.set_input_calibration_ex, bad_K, dd.D_A) == (INV, SETX + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1")
    assert refused(vs, s.set_input_calibration_ex, K_CAL, (-0.5, 0, 0, 0)) == (INV, SETX + "the distortion must keep theta_d increasing on [0, pi/2]")
    assert refused(vs, s.set_input_calibration_ex, bad_K, (-0.5, 0, 0, 0))[1] == SETX + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1"
    Kin = oracle.lens_camera(oracle.PROJ_FISH, 150.0, W, H)
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, OW, OH)
    plain = wd.bgr(frames[1], *wd.maps(oracle.map_params(Kin, Kout, np.eye(3)), OW, OH, 1), "cubic", REFLECT_101)
    eq(s.pull().cpu().numpy(), plain, "uncalibrated after the refusals")
    assert refused(vs, s.set_input_calibration_ex, K_CAL, dd.D_A) == (INV, SETX + "the calibration must be set before the first pull")
    s.close()

    # the plain call keeps its refusals, and a handle calibrated through it keeps refusing a border mode
    assert refused(vs, handle(resample=vs.RESAMPLE_CUBIC).set_input_calibration, K_CAL, dd.D_A) == (
        INV, "vstab_set_input_calibration: the distorted-lens warp resamples with VSTAB_RESAMPLE_DEFAULT, this handle with VSTAB_RESAMPLE_CUBIC")
    assert refused(vs, handle(border_mode=REFLECT_101).set_input_calibration, K_CAL, dd.D_A) == (
        INV, "vstab_set_input_calibration: the distorted-lens warp has the constant border, this handle has another border mode set (vstab_set_border_mode)")
    s = handle(calibration=(K_CAL, dd.D_A))
    for fn, name in ((s.set_border_mode, "vstab_set_border_mode"), (s.set_border_mode_ex, "vstab_set_border_mode_ex")):
        assert refused(vs, fn, REPLICATE) == (INV, name + ": a calibrated handle (vstab_set_input_calibration) warps with VSTAB_BORDER_CONSTANT")
    expect_pull(still_maps, frames[1], "linear", CONSTANT, s.pull().cpu().numpy(), "pull", "plain calibration")
    s.close()


@pytest.mark.parametrize("resampler,border", [("cubic", REFLECT_101), ("linear", REPLICATE)])
def test_pipeline_frame_with_a_readout_rotation_is_refused_and_consumed(vs, cuda, still_clip, still_maps, resampler, border):
    """Input frames 1 and 3 carry a read-out rotation: their pulls are refused and the frames are gone, 2 and 4 are delivered."""
    import torch
    frames = still_clip[:5]
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
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
    cfg = vs.default_config(**dict(BASE, smooth_radius=1, resample=RESAMPLE[resampler]))
    h = ctypes.c_void_p()
    assert vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(src), ctypes.byref(h)) == vs.OK, vs.lib.vstab_last_error()
    try:
        Kc, Dc = np.ascontiguousarray(K_CAL.reshape(9)), np.array(dd.D_A, np.float64)
        assert vs.lib.vstab_set_border_mode_ex(h, border) == vs.OK
        assert vs.lib.vstab_set_input_calibration_ex(h, Kc.ctypes.data_as(dp), Dc.ctypes.data_as(dp)) == vs.OK, vs.lib.vstab_last_error()
        for k in range(1, len(devf)):
            o = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
            st = vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0))
            if k in (1, 3):
                assert st == vs.ERR_INVALID, k
                assert vs.lib.vstab_last_error() == b"a calibrated handle (vstab_set_input_calibration) warps frames without a read-out rotation"
            else:
                assert st == vs.OK, (k, vs.lib.vstab_last_error())
                expect_pull(still_maps, frames[k], resampler, border, o.cpu().numpy(), "pull", ("readout", k))
        assert vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0)) == vs.EOF
    finally:
        vs.lib.vstab_destroy(h)


def test_pipeline_rotation_estimate_does_not_depend_on_the_resampler(vs, cuda):
    """The distorted shaky clip: a CUBIC handle calibrated with _ex reports exactly the warp rotations of an INTER_LINEAR handle calibrated
    with the plain call (same seed), and its frames are the cubic definition's with those rotations."""
    import torch
    w, h, n, ow, oh = 640, 360, 12, 480, 270
    K = oracle.get_preset_camera(4, w, h)
    frames, _ = dd.shaky_clip(3, K, dd.D_A, w, h, n, sigma=0.004)
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    cfg = dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=ow, out_height=oh, smooth_radius=3, seed=5)
    a = vs.Stabilizer(devf, total=n, calibration=(K, dd.D_A), **cfg)
    b = vs.Stabilizer(devf, total=n, calibration_ex=(K, dd.D_A), resample=vs.RESAMPLE_CUBIC, border_mode=REFLECT_101, **cfg)
    outs = []
    for i in range(n - 1):
        assert a.pull() is not None
        outs.append(b.pull().cpu().numpy())
    assert a.pull() is None and b.pull() is None
    moved = 0
    for i in range(n - 1):
        Ra, Rb = a.warp_rotation(i), b.warp_rotation(i)
        assert np.array_equal(Ra, Rb), i
        moved += not np.allclose(Ra, np.eye(3), atol=1e-6)
    assert moved > 0                                           # the clip shakes: the rotations are estimates, not the identity
    assert all(lg["inliers"] >= 40 for lg in b.frame_log())
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, ow, oh)
    for i in (0, n - 2):
        p = oracle.map_params(K, Kout, b.warp_rotation(i))
        eq(outs[i], wd.bgr(frames[i + 1], *wd.maps(p, ow, oh, 1, None, dd.D_A), "cubic", REFLECT_101), ("tracked frame", i))
    a.close(), b.close()
