"""GPU tests of the pinhole lens distortion (include/vstab.h, "Pinhole lens distortion"): every byte of vstab_warp_nv12_pinhole, BGR, luma and
chroma, against the numpy definition -- the distorted map (tests/pinhole_def.py) fed to the resamplers' existing definitions
(tests/warp_def.py: bgr / planar) --, against the older entry points it must agree with at D = 0, and against the
stateless route (vstab_create_map_pinhole + a vstab_remap_*_border).  Shapes: the smallest that reach the tile states test_pinhole_cpu.py
asserts for them, a source plane off its alignment, a 16 x 2 source, padded destinations, and a handle with vstab_set_input_pinhole through
every pull, its refusals, and a tracked clip."""
import ctypes

import numpy as np
import pytest

import layouts
import oracle
import pinhole_def as pd
import synth
import warp_def as wd
from test_border_gpu import pulls
from test_distort_gpu import dev, refused, same_map
from test_lens_gpu import ROTS
from test_pinhole_cpu import cameras

pytestmark = pytest.mark.gpu

RESAMPLERS, RESAMPLE, BORDERS = wd.RESAMPLERS, wd.RESAMPLE, wd.MODES
CONSTANT, REPLICATE, REFLECT, REFLECT_101 = wd.CONSTANT, wd.REPLICATE, wd.REFLECT, wd.REFLECT_101
MODES = [3, 4]


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got != exp
    assert not bad.any(), (what, int(bad.sum()), "of", bad.size, "first at", tuple(int(v[0]) for v in np.nonzero(bad)))


class Case:
    """One frame, parameter set and size: the distorted map evaluated once, the definition's frames of any (resampler, border) from it."""

    def __init__(self, w, h, dw, dh, mode, rv, D=pd.D_P, aniso=1.0, seed=None, frame=None):
        self.w, self.h, self.dw, self.dh, self.mode, self.D = w, h, dw, dh, mode, D
        self.f = synth.nv12(dw + mode if seed is None else seed, w, h, full_range=True) if frame is None else frame
        Kin, Kout = cameras(w, h, dw, dh, mode, aniso)
        self.p = oracle.map_params(Kin, Kout, oracle.rodrigues(rv))
        self.mx, self.my = pd.maps(self.p, dw, dh, mode, D)

    def bgr(self, resampler, border):
        return wd.bgr(self.f, self.mx, self.my, resampler, border)

    def planar(self, resampler, border):
        return wd.planar(self.f, self.mx, self.my, resampler, border)

    def check(self, vs, fd, resampler, border, what=None):
        """Both output formats of vstab_warp_nv12_pinhole (through the binding, packed source fd) against the definition."""
        what = (what, resampler, border, self.mode, self.dw, self.dh)
        got = vs.warp_nv12_pinhole(fd, self.p, self.D, self.dw, self.dh, self.mode, RESAMPLE[resampler], border, vs.OUT_BGR8)
        eq(got.cpu().numpy(), self.bgr(resampler, border), what + ("bgr",))
        y, c = vs.warp_nv12_pinhole(fd, self.p, self.D, self.dw, self.dh, self.mode, RESAMPLE[resampler], border, vs.OUT_NV12_PLANAR)
        ey, ec = self.planar(resampler, border)
        eq(y.cpu().numpy(), ey, what + ("luma",)), eq(c.cpu().numpy(), ec, what + ("chroma",))
        return got


def stateless_bgr(vs, fd, case, resampler, border):
    """vstab_create_map_pinhole, then the stateless remap of the BGR conversion."""
    mx, my = vs.create_map_pinhole(case.p, case.D, case.dw, case.dh, case.mode)
    src = vs.cvt_nv12_bgr(fd)
    if resampler == "linear":
        return vs.remap_bilinear_border(src, mx, my, border)
    return (vs.remap_cubic_border if resampler == "cubic" else vs.remap_lanczos4_border)(src, mx, my, border, (0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------------
# every combination once
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_every_resampler_border_and_mode(vs, cuda, resampler, mode):
    w, h, dw, dh = 128, 72, 130, 70
    c = Case(w, h, dw, dh, mode, ROTS[1])
    fd = dev(c.f, cuda)
    zx, zy = pd.maps(c.p, dw, dh, mode, pd.D_0)
    for border in BORDERS:
        got = c.check(vs, fd, resampler, border, "all").cpu().numpy()
        plain = wd.bgr(c.f, zx, zy, resampler, border)                     # the D = 0 frame
        assert (got != 0).mean() >= 0.1, ("black", resampler, border, mode)
        assert (got != plain).any(axis=-1).mean() >= 0.5, ("the distortion moved too few pixels", resampler, border, mode)
        eq(stateless_bgr(vs, fd, c, resampler, border).cpu().numpy(), got, ("stateless route", resampler, border, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [pd.D_Q, pd.D_M])
def test_other_coefficient_sets(vs, cuda, D, mode):
    c = Case(128, 72, 130, 70, mode, ROTS[2], D=D, seed=3)
    fd = dev(c.f, cuda)
    for resampler, border in (("linear", CONSTANT), ("cubic", REFLECT), ("lanczos4", REPLICATE)):
        c.check(vs, fd, resampler, border, "sets")


# ---------------------------------------------------------------------------------------------------------------------
# the tile-state shapes (test_pinhole_cpu.py asserts the states)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("resampler", RESAMPLERS)
@pytest.mark.parametrize("w,h,dw,dh", [(640, 360, 333, 201), (1024, 576, 200, 72)])
def test_staged_partial_crossing_and_mixed_tiles(vs, cuda, w, h, dw, dh, resampler, mode):
    c = Case(w, h, dw, dh, mode, ROTS[1])
    fd = dev(c.f, cuda)
    for border in (CONSTANT, REFLECT_101):
        c.check(vs, fd, resampler, border, "tiles")


@pytest.mark.parametrize("w,h,mode", [(2048, 1152, 3), (2048, 1152, 4), (3072, 1728, 3)])
@pytest.mark.parametrize("resampler,border", [("linear", REFLECT_101), ("cubic", CONSTANT), ("lanczos4", REPLICATE)])
def test_tiles_over_the_lds_budget(vs, cuda, resampler, border, w, h, mode):
    """-> 256 x 128.  2048 x 1152: every BGR box is over the budget (mode 3), most are (mode 4); 3072 x 1728, mode 3: every box of every
    plane (test_pinhole_cpu.py, test_tile_states_every_box_over_the_lds_budget).  Those pixels are sampled from global memory."""
    c = Case(w, h, 256, 128, mode, ROTS[1])
    c.check(vs, dev(c.f, cuda), resampler, border, "gathers")


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_a_quarter_of_the_map_behind_the_camera(vs, cuda, resampler):
    """ROTS[3], mode 3: about a quarter of the entries NaN; under a non-constant border the tiles that hold one beside a number gather (the
    box reaches -32768), a tile of NaN entries alone stages a small box far outside."""
    c = Case(128, 72, 130, 70, 3, ROTS[3])
    assert 0.2 < np.isnan(c.mx).mean() < 0.3
    fd = dev(c.f, cuda)
    for border in (REPLICATE, CONSTANT):
        c.check(vs, fd, resampler, border, "nan")


# ---------------------------------------------------------------------------------------------------------------------
# cameras, pitches, alignments, the smallest source
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_anisotropic_camera(vs, cuda, mode):
    c = Case(320, 180, 130, 75, mode, (0.01, 0.02, -0.05), aniso=1.07, seed=5)
    fd = dev(c.f, cuda)
    for resampler, border in (("linear", REFLECT), ("linear", CONSTANT), ("cubic", CONSTANT), ("cubic", REFLECT_101), ("lanczos4", CONSTANT), ("lanczos4", REPLICATE)):
        c.check(vs, fd, resampler, border, "aniso")


@pytest.mark.parametrize("mode", MODES)
def test_destinations_with_padded_pitches(vs, cuda, mode):
    """Output rows at odd offsets inside wider buffers: every byte outside the planes keeps its fill."""
    import torch
    c = Case(128, 72, 67, 35, mode, ROTS[2], D=pd.D_Q, seed=7)
    fd = dev(c.f, cuda)
    dw, dh, cw = c.dw, c.dh, (c.dw + 1) // 2
    for k, (resampler, border) in enumerate((("linear", REPLICATE), ("linear", CONSTANT), ("cubic", CONSTANT), ("cubic", REFLECT), ("lanczos4", CONSTANT),
                                             ("lanczos4", REFLECT_101))):
        pad = 1 + 2 * (k % 2)
        out = torch.full((dh + 2, dw * 3 + pad + 5), 7, dtype=torch.uint8, device=cuda)
        got = vs.warp_nv12_pinhole(fd, c.p, c.D, dw, dh, mode, RESAMPLE[resampler], border, vs.OUT_BGR8, out=out[1:dh + 1, pad:pad + dw * 3].unflatten(1, (dw, 3)))
        eq(got.cpu().numpy(), c.bgr(resampler, border), ("pad bgr", resampler, border, mode))
        assert bool((out[:, :pad] == 7).all()) and bool((out[:, pad + dw * 3:] == 7).all()) and bool((out[0] == 7).all()) and bool((out[dh + 1] == 7).all())
        yb = torch.full((dh + 2, dw + pad + 8), 7, dtype=torch.uint8, device=cuda)
        cb = torch.full(((dh + 1) // 2 + 2, 2 * cw + pad + 8), 7, dtype=torch.uint8, device=cuda)
        ch = (dh + 1) // 2
        y, uv = vs.warp_nv12_pinhole(fd, c.p, c.D, dw, dh, mode, RESAMPLE[resampler], border, vs.OUT_NV12_PLANAR,
                                     out=(yb[1:dh + 1, pad:pad + dw], cb[1:ch + 1, pad:pad + 2 * cw]))
        ey, ec = c.planar(resampler, border)
        eq(y.cpu().numpy(), ey, ("pad luma", resampler, border, mode)), eq(uv.cpu().numpy(), ec, ("pad chroma", resampler, border, mode))
        assert bool((yb[:, pad + dw:] == 7).all()) and bool((cb[:, pad + 2 * cw:] == 7).all())
        assert bool((yb[:, :pad] == 7).all()) and bool((cb[:, :pad] == 7).all())
        assert bool((yb[0] == 7).all()) and bool((yb[dh + 1] == 7).all()) and bool((cb[0] == 7).all()) and bool((cb[ch + 1] == 7).all())


def raw_warp(vs, cuda, s, p, D, dw, dh, mode, resampler, border, fmt):
    """vstab_warp_nv12_pinhole with separate source planes (layouts.Src) into canaried output planes."""
    _, pp = layouts._f(p)
    _, d = layouts._f(D)
    if fmt == vs.OUT_BGR8:
        o = layouts.Plane(dh, 3 * dw, cuda)
        args = (o.ptr, o.pitch, None, 0)
    else:
        oy, ou = layouts.out_nv12(dw, dh, cuda)
        args = (oy.ptr, oy.pitch, ou.ptr, ou.pitch)
    st = vs.lib.vstab_warp_nv12_pinhole(s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, d, mode, RESAMPLE[resampler], border, fmt, *args, dw, dh, vs._stream())
    assert st == vs.OK, vs.lib.vstab_last_error()
    if fmt == vs.OUT_BGR8:
        return o.host(shape=(dh, dw, 3))
    return oy.host(), ou.host()


def check_raw(vs, cuda, s, c, resampler, border, what):
    eq(raw_warp(vs, cuda, s, c.p, c.D, c.dw, c.dh, c.mode, resampler, border, vs.OUT_BGR8), c.bgr(resampler, border), (what, "bgr", resampler, border, c.mode))
    y, uv = raw_warp(vs, cuda, s, c.p, c.D, c.dw, c.dh, c.mode, resampler, border, vs.OUT_NV12_PLANAR)
    ey, ec = c.planar(resampler, border)
    eq(y, ey, (what, "luma", resampler, border, c.mode)), eq(uv, ec, (what, "chroma", resampler, border, c.mode))


@pytest.mark.parametrize("mode", MODES)
def test_source_plane_offset_by_one_byte(vs, cuda, mode):
    """Luma at an odd address, chroma 2-byte aligned only, pitches wider than the rows, planes in two allocations."""
    w, h = 128, 72
    c = Case(w, h, 130, 70, mode, ROTS[1], D=pd.D_Q, seed=9)
    s = layouts.place(c.f[:h], c.f[h:], None, cuda, spec=(w + 24, w + 40, "two", 1, 2))
    assert s.y % 2 == 1 and s.uv % 4 == 2
    for resampler in RESAMPLERS:
        for border in (CONSTANT, REFLECT_101):
            check_raw(vs, cuda, s, c, resampler, border, "offset")


@pytest.mark.parametrize("mode", MODES)
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
@pytest.mark.parametrize("mode", MODES)
def test_zero_distortion_is_the_older_entry_point_byte_for_byte(vs, cuda, mode):
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
                ex = lambda resample: vs.warp_nv12_pinhole(fd, p, pd.D_0, dw, dh, mode, resample, border, fmt)       # noqa: E731
                same(ex(vs.RESAMPLE_CUBIC), vs.warp_nv12_cubic_border(fd, p, dw, dh, mode, fmt, border), ("cubic_border", border))
                same(ex(vs.RESAMPLE_LANCZOS4), vs.warp_nv12_lanczos4_border(fd, p, dw, dh, mode, fmt, border), ("lanczos4_border", border))
                same(ex(vs.RESAMPLE_DEFAULT), vs.warp_nv12_border(fd, p, dw, dh, mode, fmt, border), ("border", border))
            ex = lambda resample: vs.warp_nv12_pinhole(fd, p, pd.D_0, dw, dh, mode, resample, CONSTANT, fmt)         # noqa: E731
            same(ex(vs.RESAMPLE_CUBIC), vs.warp_nv12_cubic(fd, p, dw, dh, mode, fmt), "cubic")
            same(ex(vs.RESAMPLE_LANCZOS4), vs.warp_nv12_lanczos4(fd, p, dw, dh, mode, fmt), "lanczos4")
            same(ex(vs.RESAMPLE_DEFAULT), vs.warp_nv12(fd, p, dw, dh, mode, fmt), "plain")


@pytest.mark.parametrize("mode", MODES)
def test_create_map_pinhole_is_the_definition_in_its_bits(vs, cuda, mode):
    for (w, h, dw, dh, rv, aniso) in [(640, 360, 481, 271, ROTS[1], 1.0), (128, 72, 130, 70, ROTS[3], 1.0), (320, 180, 97, 45, ROTS[2], 1.07), (128, 72, 67, 35, ROTS[4], 1.0)]:
        Kin, Kout = cameras(w, h, dw, dh, mode, aniso)
        p = oracle.map_params(Kin, Kout, oracle.rodrigues(rv))
        for D in (pd.D_P, pd.D_Q, pd.D_M, pd.D_0):
            mx, my = vs.create_map_pinhole(p, D, dw, dh, mode)
            ex, ey = pd.maps(p, dw, dh, mode, D)
            same_map(mx.cpu().numpy(), my.cpu().numpy(), ex, ey, (mode, dw, dh, rv, D))
        zx, zy = vs.create_map(p, dw, dh, mode=mode)                                # D = 0: vstab_create_map_ex's planes
        mx, my = vs.create_map_pinhole(p, pd.D_0, dw, dh, mode)
        same_map(mx.cpu().numpy(), my.cpu().numpy(), zx.cpu().numpy(), zy.cpu().numpy(), ("D_0 vs create_map_ex", mode, dw))


def test_create_map_pinhole_with_unaligned_planes(vs, cuda):
    """Planes at a 4-byte offset with a pitch that is no multiple of 16: the column-by-column store path, nothing written outside."""
    import torch
    dw, dh, mode = 67, 35, 3
    Kin, Kout = cameras(128, 72, dw, dh, mode)
    p = np.ascontiguousarray(oracle.map_params(Kin, Kout, oracle.rodrigues(ROTS[1])), np.float32)
    d = np.array(pd.D_P, np.float32)
    bx = torch.full((dh + 2, dw + 6), -7.0, dtype=torch.float32, device=cuda)
    by = torch.full((dh + 2, dw + 6), -7.0, dtype=torch.float32, device=cuda)
    st = vs.lib.vstab_create_map_pinhole(bx[1:, 1:].data_ptr(), bx.stride(0) * 4, by[1:, 1:].data_ptr(), by.stride(0) * 4, dw, dh, vs._fptr(p), vs._fptr(d), mode,
                                         vs._stream())
    assert st == vs.OK, vs.lib.vstab_last_error()
    ex, ey = pd.maps(p, dw, dh, mode, pd.D_P)
    hx, hy = bx.cpu().numpy(), by.cpu().numpy()
    same_map(hx[1:dh + 1, 1:dw + 1], hy[1:dh + 1, 1:dw + 1], ex, ey, "unaligned")
    for hb in (hx, hy):
        assert (hb[0] == -7).all() and (hb[dh + 1] == -7).all() and (hb[:, 0] == -7).all() and (hb[:, dw + 1:] == -7).all()


# ---------------------------------------------------------------------------------------------------------------------
# a handle with vstab_set_input_pinhole
# ---------------------------------------------------------------------------------------------------------------------
SETP = "vstab_set_input_pinhole: "
SERVED = " emits 8-bit BGR or plane-wise NV12 frames (vstab_pull_frame / _frames / _host / vstab_peek_frame / vstab_pull_frame_nv12_planar), not NV12 through BGR"
W, H, OW, OH = 320, 180, 240, 136
LENS = dict(lens_mode=1, in_projection=0, out_projection=0, in_dfov=100.0, out_dfov=80.0, out_width=OW, out_height=OH)
K_CAL = np.array([[151.0, 0.0, 161.5], [0.0, 156.0, 88.0], [0.0, 0.0, 1.0]])     # a calibrated camera matrix: fx != fy, centre off the middle
HANDLES = [("cubic", REFLECT_101), ("lanczos4", REFLECT_101), ("linear", REPLICATE)]
BASE = dict(LENS, smooth_radius=2, tracking=0)


@pytest.fixture(scope="module")
def still_clip():
    return [synth.nv12(60 + k, W, H) for k in range(8)]


@pytest.fixture(scope="module")
def still_maps():
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 80.0, OW, OH)
    return pd.maps(oracle.map_params(K_CAL, Kout, np.eye(3)), OW, OH, 3, pd.D_P)


def expect_pull(still_maps, f, resampler, border, out, how, what):
    mx, my = still_maps
    if how == "planar":
        ey, ec = wd.planar(f, mx, my, resampler, border)
        eq(out[0], ey, (what, "luma")), eq(out[1], ec, (what, "chroma"))
    else:
        eq(out, wd.bgr(f, mx, my, resampler, border), what)


@pytest.mark.parametrize("how", ["pull", "frames", "host", "peek", "planar"])
@pytest.mark.parametrize("resampler,border", HANDLES)
def test_pipeline_pulls_of_a_pinhole_handle(vs, cuda, still_clip, still_maps, resampler, border, how):
    stab, outs = pulls(vs, cuda, still_clip, how, border, pinhole=(K_CAL, pd.D_P), resample=RESAMPLE[resampler], **BASE)
    assert len(outs) == len(still_clip) - 1 and stab.out_size == (OW, OH) and np.array_equal(stab.K_in, K_CAL)
    for i, o in enumerate(outs):
        assert np.allclose(stab.warp_rotation(i), np.eye(3), atol=1e-12)
        expect_pull(still_maps, still_clip[i + 1], resampler, border, o, how, (resampler, border, how, i))
    assert stab.warps_from_cache() == 0          # the quantised map steps aside, the constant border included (below)
    stab.close()


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_pipeline_border_mode_switches_between_pulls(vs, cuda, still_clip, still_maps, resampler):
    """The mode in force at a pull is the mode of its frame; the lens set after a border mode, modes set after the lens; INTER_LINEAR with
    the constant border stays with vstab_warp_nv12_pinhole: no pull reads the quantised map."""
    import torch
    devf = [torch.from_numpy(f).to(cuda) for f in still_clip]
    stab = vs.Stabilizer(devf, total=len(devf), resample=RESAMPLE[resampler], border_mode=REFLECT, **BASE)
    stab.set_input_pinhole(K_CAL, pd.D_P)
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
    assert stab.warps_from_cache() == 0
    stab.close()


def test_pipeline_refusals_of_a_pinhole_handle(vs, cuda, still_clip, still_maps):
    """Status, whole message, and whether a frame was taken."""
    import torch
    frames = still_clip[:5]
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    INV, UNS = vs.ERR_INVALID, vs.ERR_UNSUPPORTED

    def handle(**kw):
        return vs.Stabilizer(devf, total=len(devf), **dict(BASE, smooth_radius=1, **kw))

    # NV12 through BGR and the keep-edge pulls are refused before a frame is taken, whatever refuses them first: the first frame is still there
    for kw, resampler, border, why, keep_why in (
            (dict(resample=vs.RESAMPLE_CUBIC), "cubic", CONSTANT, "VSTAB_RESAMPLE_CUBIC", "VSTAB_RESAMPLE_CUBIC has no keep-edge warp"),
            (dict(resample=vs.RESAMPLE_LANCZOS4, border_mode=REFLECT), "lanczos4", REFLECT, "VSTAB_RESAMPLE_LANCZOS4", "VSTAB_RESAMPLE_LANCZOS4 has no keep-edge warp"),
            (dict(border_mode=REPLICATE), "linear", REPLICATE, "a border mode other than VSTAB_BORDER_CONSTANT",
             "a border mode other than VSTAB_BORDER_CONSTANT is in force (vstab_set_border_mode)"),
            (dict(), "linear", CONSTANT, "a calibrated handle (vstab_set_input_pinhole)", "a calibrated handle (vstab_set_input_pinhole) has no keep-edge warp")):
        s = handle(pinhole=(K_CAL, pd.D_P), **kw)
        assert refused(vs, s.pull_nv12) == (INV, "vstab_pull_frame: " + why + SERVED)
        prev = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
        out = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
        assert refused(vs, s.pull_keep_into, out, prev) == (UNS, "vstab_pull_frame_keep: " + keep_why)
        y, uv = vs.nv12_out_planes(OW, OH, cuda)
        py, puv = vs.nv12_out_planes(OW, OH, cuda)
        assert refused(vs, s.pull_nv12_planar_keep_into, y, uv, py, puv) == (UNS, "vstab_pull_frame_nv12_planar_keep: " + keep_why)
        expect_pull(still_maps, frames[1], resampler, border, s.pull().cpu().numpy(), "pull", ("after the refusals", resampler))
        s.close()

    # what vstab_set_input_pinhole refuses, message for message; the handle stays as it was
    Kin = oracle.lens_camera(oracle.PROJ_RECT, 100.0, W, H)
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 80.0, OW, OH)
    assert refused(vs, vs.Stabilizer(devf, total=len(devf), smooth_radius=1, tracking=0).set_input_pinhole, K_CAL, pd.D_P) == (
        INV, SETP + "a calibration belongs to lens_mode 1 (the preset path derives its output camera from the input's)")
    assert refused(vs, handle(in_projection=1, in_dfov=150.0).set_input_pinhole, K_CAL, pd.D_P) == (
        INV, SETP + "pinhole distortion belongs to a rectilinear input (in_projection VSTAB_PROJ_RECT)")
    wide = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in frames]
    h10 = vs.Stabilizer(wide, total=len(wide), bit_depth=10, pixel_depth=10, **dict(BASE, smooth_radius=1))
    assert refused(vs, h10.set_input_pinhole, K_CAL, pd.D_P) == (INV, SETP + "the pinhole-lens warp takes 8-bit pixels, this is a pixel_depth 10 handle")
    dp = ctypes.POINTER(ctypes.c_double)
    d5 = np.array(pd.D_P, np.float64)
    assert vs.lib.vstab_set_input_pinhole(None, None, d5.ctypes.data_as(dp)) == INV and vs.lib.vstab_last_error() == (SETP + "null argument").encode()
    s = handle(resample=vs.RESAMPLE_CUBIC, border_mode=REFLECT_101)
    assert vs.lib.vstab_set_input_pinhole(s._h, None, None) == INV and vs.lib.vstab_last_error() == (SETP + "null argument").encode()
    bad_K = K_CAL.copy()
    bad_K[0, 1] = 0.5
    nan_D = (0.0, float("nan"), 0.0, 0.0, 0.0)
    assert refused(vs, s.set_input_pinhole, bad_K, pd.D_P) == (INV, SETP + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1")
    assert refused(vs, s.set_input_pinhole, K_CAL, nan_D) == (INV, SETP + "the five distortion coefficients must be finite")
    assert refused(vs, s.set_input_pinhole, K_CAL, (1e39, 0, 0, 0, 0)) == (INV, SETP + "the five distortion coefficients must be finite")
    assert refused(vs, s.set_input_pinhole, bad_K, nan_D)[1] == SETP + "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1"
    plain = wd.bgr(frames[1], *wd.maps(oracle.map_params(Kin, Kout, np.eye(3)), OW, OH, 3), "cubic", REFLECT_101)
    eq(s.pull().cpu().numpy(), plain, "uncalibrated after the refusals")
    assert refused(vs, s.set_input_pinhole, K_CAL, pd.D_P) == (INV, SETP + "the calibration must be set before the first pull")
    s.close()

    # vstab_set_input_calibration[_ex] keep refusing a rectilinear input with their present messages, on a plain and on a pinhole handle
    for s in (handle(), handle(pinhole=(K_CAL, pd.D_P))):
        for fn, name in ((s.set_input_calibration, "vstab_set_input_calibration"), (s.set_input_calibration_ex, "vstab_set_input_calibration_ex")):
            assert refused(vs, fn, K_CAL, (0.0, 0.0, 0.0, 0.0)) == (INV, name + ": distortion belongs to a fisheye input (in_projection VSTAB_PROJ_FISH)")
        s.close()

    # K = None keeps the camera of in_dfov; D = 0 is the uncalibrated handle's frame
    s = handle(pinhole=(None, pd.D_0), resample=vs.RESAMPLE_CUBIC, border_mode=REFLECT_101)
    assert np.allclose(s.K_in, Kin, rtol=1e-15, atol=0)
    eq(s.pull().cpu().numpy(), plain, "D_0, K from in_dfov")
    s.close()
    s = handle(pinhole=(None, pd.D_Q))
    mx, my = pd.maps(oracle.map_params(Kin, Kout, np.eye(3)), OW, OH, 3, pd.D_Q)
    eq(s.pull().cpu().numpy(), wd.bgr(frames[1], mx, my, "linear", CONSTANT), "K from in_dfov")
    s.close()


@pytest.mark.parametrize("readout_warp", [0, 1])
@pytest.mark.parametrize("resampler,border", [("cubic", REFLECT_101), ("linear", REPLICATE)])
def test_pipeline_frame_with_a_readout_rotation_is_refused_and_consumed(vs, cuda, still_clip, still_maps, resampler, border, readout_warp):
    """Input frames 1 and 3 carry a read-out rotation: two pulls are refused and the frames are gone, 2 and 4 are delivered -- whatever
    vstab_set_readout_warp says.  A rectilinear input has no rolling-shutter warp, so the refusal is the one every such handle makes when it
    takes the frame from upstream (with its present message), which may be a pull ahead of the frame's own turn."""
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
        Kc, Dc = np.ascontiguousarray(K_CAL.reshape(9)), np.array(pd.D_P, np.float64)
        assert vs.lib.vstab_set_border_mode_ex(h, border) == vs.OK
        assert vs.lib.vstab_set_input_pinhole(h, Kc.ctypes.data_as(dp), Dc.ctypes.data_as(dp)) == vs.OK, vs.lib.vstab_last_error()
        assert vs.lib.vstab_set_readout_warp(h, readout_warp) == vs.OK
        refusals, due = 0, [2, 4]
        for k in range(1, len(devf)):
            o = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
            st = vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0))
            if st == vs.ERR_INVALID:
                assert vs.lib.vstab_last_error() == b"vstab_frame.readout_rotation: the 8-bit rolling-shutter warp exists for the preset and fisheye -> rectilinear maps only"
                refusals += 1
            else:
                assert st == vs.OK and due, (k, st, vs.lib.vstab_last_error())
                expect_pull(still_maps, frames[due.pop(0)], resampler, border, o.cpu().numpy(), "pull", ("readout", k))
        assert refusals == 2 and not due
        assert vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0)) == vs.EOF
    finally:
        vs.lib.vstab_destroy(h)


def test_pipeline_tracked_clip_through_a_distorted_pinhole_lens(vs, cuda):
    """The shaky clip rendered through D_M: a CUBIC and an INTER_LINEAR pinhole handle with the same seed report identical warp rotations
    (the estimate does not depend on the resampler), not all the identity; frames 0 and n - 2 are the definition's frames with those
    rotations; and each frame keeps at least the inliers of the same clip rendered and run with D_0 on an uncalibrated handle, less 10 %
    (points the undistortion moves across the RANSAC threshold).  Inliers per frame, D_M handle / D_0 handle: printed below."""
    import torch
    w, h, n, ow, oh = 640, 360, 12, 480, 270
    K = oracle.lens_camera(oracle.PROJ_RECT, 100.0, w, h)
    cfg = dict(lens_mode=1, in_projection=0, out_projection=0, in_dfov=100.0, out_dfov=80.0, out_width=ow, out_height=oh, smooth_radius=3, seed=5)
    frames, _ = pd.shaky_clip(3, K, pd.D_M, w, h, n, sigma=0.004)
    ideal, _ = pd.shaky_clip(3, K, pd.D_0, w, h, n, sigma=0.004)
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    devi = [torch.from_numpy(f).to(cuda) for f in ideal]
    a = vs.Stabilizer(devf, total=n, pinhole=(K, pd.D_M), **cfg)
    b = vs.Stabilizer(devf, total=n, pinhole=(K, pd.D_M), resample=vs.RESAMPLE_CUBIC, border_mode=REFLECT_101, **cfg)
    z = vs.Stabilizer(devi, total=n, **cfg)
    outs_a, outs_b = [], []
    for i in range(n - 1):
        outs_a.append(a.pull().cpu().numpy())
        outs_b.append(b.pull().cpu().numpy())
        assert z.pull() is not None
    assert a.pull() is None and b.pull() is None and z.pull() is None
    moved = 0
    for i in range(n - 1):
        Ra, Rb = a.warp_rotation(i), b.warp_rotation(i)
        assert np.array_equal(Ra, Rb), i
        moved += not np.allclose(Ra, np.eye(3), atol=1e-6)
    assert moved > 0                                           # the clip shakes: the rotations are estimates, not the identity
    ia, ib, iz = ([lg["inliers"] for lg in s.frame_log()] for s in (a, b, z))
    print("inliers per frame through D_M:", ia, "ideal lens, uncalibrated handle:", iz)
    assert ia == ib and len(ia) == len(iz)
    assert all(x >= 0.9 * y for x, y in zip(ia, iz)), (ia, iz)
    assert a.warps_from_cache() == 0 and b.warps_from_cache() == 0
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 80.0, ow, oh)
    for i in (0, n - 2):
        mx, my = pd.maps(oracle.map_params(K, Kout, b.warp_rotation(i)), ow, oh, 3, pd.D_M)
        eq(outs_b[i], wd.bgr(frames[i + 1], mx, my, "cubic", REFLECT_101), ("tracked cubic frame", i))
        eq(outs_a[i], wd.bgr(frames[i + 1], mx, my, "linear", CONSTANT), ("tracked linear frame", i))
    a.close(), b.close(), z.close()


def test_pipeline_debug_markers_go_through_the_lens(vs, cuda):
    """`debug` markers on a tracked clip: with D_0 the lens's inverse is the identity, so a pinhole handle draws exactly the markers (and
    the frames) of an uncalibrated handle; through D_M the markers are there too -- the frames differ from the same handle's without
    `debug`, and only where a marker's colour stands."""
    import torch
    w, h, n, ow, oh = 640, 360, 6, 480, 270
    K = oracle.lens_camera(oracle.PROJ_RECT, 100.0, w, h)
    cfg = dict(lens_mode=1, in_projection=0, out_projection=0, in_dfov=100.0, out_dfov=80.0, out_width=ow, out_height=oh, smooth_radius=1, seed=5)
    ideal, _ = pd.shaky_clip(3, K, pd.D_0, w, h, n, sigma=0.004)
    bent, _ = pd.shaky_clip(3, K, pd.D_M, w, h, n, sigma=0.004)
    devi = [torch.from_numpy(f).to(cuda) for f in ideal]
    devb = [torch.from_numpy(f).to(cuda) for f in bent]
    a = vs.Stabilizer(devi, total=n, debug=1, pinhole=(None, pd.D_0), **cfg)
    z = vs.Stabilizer(devi, total=n, debug=1, **cfg)
    m = vs.Stabilizer(devb, total=n, debug=1, pinhole=(K, pd.D_M), **cfg)
    q = vs.Stabilizer(devb, total=n, pinhole=(K, pd.D_M), **cfg)
    marked = 0
    for i in range(n - 1):
        fa, fz, fm, fq = (s.pull().cpu().numpy() for s in (a, z, m, q))
        eq(fa, fz, ("D_0 markers", i))
        assert np.array_equal(m.warp_rotation(i), q.warp_rotation(i))
        diff = (fm != fq).any(axis=-1)
        assert (fm[diff] == (0, 255, 0)).all(), i              # vstab_draw_markers' colour 0x0000FF00, B G R bytes
        marked += int(diff.sum())
    assert marked > 0
    for s in (a, z, m, q):
        s.close()
