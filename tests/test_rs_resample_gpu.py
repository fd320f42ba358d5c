"""GPU tests of vstab_warp_nv12_rs_ex and vstab_set_readout_warp (include/vstab.h): every byte, BGR and plane-wise, against the numpy
definition (tests/warp_def.py: the per-row map fed to the resampler's own definition), against the older entry points wherever one
serves the combination, and through the pipeline.  Shapes: the smallest that reach the tile states tests/test_rs_resample_cpu.py asserts for
them (every tile staged, tiles wholly outside, boxes across all four edges, partial tiles; every tile gathered; one output row)."""
import ctypes

import numpy as np
import pytest

import distort_def as dd
import expect
import oracle
import synth
import warp_def as wd
from test_border_gpu import clip  # noqa: F401  (the module's fixture: 640 x 360 frames of a shaky clip)
from test_distort_gpu import H, K_CAL, LENS, OH, OW, W, refused

pytestmark = pytest.mark.gpu

CONSTANT, REPLICATE, REFLECT, REFLECT_101 = wd.CONSTANT, wd.REPLICATE, wd.REFLECT, wd.REFLECT_101
BORDERS = wd.ALL_BORDERS
RESAMPLE = wd.RESAMPLE
FORMATS = ("bgr", "planar")


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got != exp
    assert not bad.any(), (what, int(bad.sum()), "of", bad.size, "first at", tuple(int(v[0]) for v in np.nonzero(bad)))


def host(o):
    return tuple(x.cpu().numpy() for x in o) if isinstance(o, tuple) else o.cpu().numpy()


def call(vs, fd, p, dw, dh, mode, rb, D, resampler, border, fmt):
    return host(vs.warp_nv12_rs_ex(fd, p, dw, dh, rb, D, mode, RESAMPLE[resampler], border, vs.OUT_BGR8 if fmt == "bgr" else vs.OUT_NV12_PLANAR))


def same(got, exp, what):
    if isinstance(exp, tuple):
        eq(got[0], exp[0], what + ("luma",)), eq(got[1], exp[1], what + ("chroma",))
    else:
        eq(got, exp, what)


class Case:
    """One frame, parameter set, size and lens: the definition's map evaluated once, shared by every test that asks for the same key."""
    _made = {}

    def __init__(self, geometry, mode, D=None, r0=wd.R0, r_bottom=wd.R_BOTTOM, with_rot=True):
        self.sw, self.sh, self.dw, self.dh, fi, fo = geometry
        self.mode, self.D = mode, D
        self.p, rb = wd.case_params(self.sw, self.sh, self.dw, self.dh, fi, fo, r0, r_bottom)
        self.rb = rb if with_rot else None
        self.f = np.random.default_rng(700 + mode).integers(0, 256, (self.sh * 3 // 2, self.sw), dtype=np.uint8)     # seeded random NV12
        self.e = wd.Expected(self.f, *wd.maps(self.p, self.dw, self.dh, mode, self.rb, D))

    @classmethod
    def get(cls, *key, **kw):
        k = (key, tuple(sorted((a, str(b)) for a, b in kw.items())))
        if k not in cls._made:
            cls._made[k] = cls(*key, **kw)
        return cls._made[k]

    def expected(self, resampler, border, fmt):
        return self.e.bgr(resampler, border) if fmt == "bgr" else self.e.planar(resampler, border)

    def check(self, vs, cuda, resampler, border, fmt, what):
        got = call(vs, dev(self.f, cuda), self.p, self.dw, self.dh, self.mode, self.rb, self.D, resampler, border, fmt)
        same(got, self.expected(resampler, border, fmt), (what, resampler, border, fmt, self.mode))
        return got


# ---------------------------------------------------------------------------------------------------------------------
# (a) cubic / Lanczos with a rotation per row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("resampler", ["cubic", "lanczos4"])
@pytest.mark.parametrize("mode", [0, 1, 5])
def test_zoomed_out(vs, cuda, mode, resampler, fmt, border):
    """128 x 72 -> 200 x 100: every tile stages, some lie wholly outside the source, boxes cross all four edges, partial tiles; mode 5's
    map is the reference kernel's, run row by row on this GPU.  98.7 % of the quantised map entries differ from the map without rot_bottom
    (test_rs_resample_cpu.py), and on random content another tap or fraction is another byte nearly always: a fifth is a loose floor."""
    c = Case.get(wd.ZOOMED_OUT, mode)
    got = c.check(vs, cuda, resampler, border, fmt, "zoomed out")
    one = call(vs, dev(c.f, cuda), c.p, c.dw, c.dh, mode, None, None, resampler, border, fmt)     # the same call without rot_bottom
    a, b = (got[0], one[0]) if fmt == "planar" else (got, one)
    assert (a != b).mean() > 0.2, "the rotation per row moved too few bytes"


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("resampler", ["cubic", "lanczos4"])
def test_gathers(vs, cuda, resampler, fmt, border):
    """2048 x 512 -> 128 x 32: every tile of every plane is over the LDS budget, every pixel is sampled from global memory."""
    c = Case.get(wd.GATHERS, 1, r0=wd.GATHERS_R0, r_bottom=wd.GATHERS_R_BOTTOM)
    c.check(vs, cuda, resampler, border, fmt, "gathers")


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("resampler", ["cubic", "lanczos4"])
def test_one_row(vs, cuda, resampler, fmt, border):
    """128 x 72 -> 150 x 1: rs_den = 1 and t = 0, the bytes are those of the call without rot_bottom."""
    c = Case.get((128, 72, 150, 1, 60.0, 40.0), 1)
    got = c.check(vs, cuda, resampler, border, fmt, "one row")
    same(got, call(vs, dev(c.f, cuda), c.p, c.dw, c.dh, 1, None, None, resampler, border, fmt), ("one row, no rot_bottom", resampler, border, fmt))


# ---------------------------------------------------------------------------------------------------------------------
# (b) a calibrated lens with a rotation per row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("resampler", ["linear", "cubic", "lanczos4"])
@pytest.mark.parametrize("D", [dd.D_A, dd.D_B], ids=["D_A", "D_B"])
def test_dist_and_rot_bottom(vs, cuda, D, resampler, fmt, border):
    c = Case.get(wd.ZOOMED_OUT, 1, D=D)
    got = c.check(vs, cuda, resampler, border, fmt, "dist + rot_bottom")
    plain = Case.get(wd.ZOOMED_OUT, 1).expected(resampler, border, fmt)
    a, b = (got[0], plain[0]) if fmt == "planar" else (got, plain)
    assert (a != b).mean() > 0.2, "the distortion moved too few bytes"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("resampler", ["linear", "cubic", "lanczos4"])
def test_zero_distortion_is_the_ideal_lens(vs, cuda, resampler, fmt):
    c = Case.get(wd.ZOOMED_OUT, 1)
    fd = dev(c.f, cuda)
    for border in BORDERS:
        zero = call(vs, fd, c.p, c.dw, c.dh, 1, c.rb, dd.D_0, resampler, border, fmt)
        same(zero, call(vs, fd, c.p, c.dw, c.dh, 1, c.rb, None, resampler, border, fmt), ("D = 0", resampler, border, fmt))
        same(zero, c.expected(resampler, border, fmt), ("D = 0, definition", resampler, border, fmt))


# ---------------------------------------------------------------------------------------------------------------------
# where an older entry point serves the combination, the bytes are that entry point's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_equalities_with_the_older_entry_points(vs, cuda, fmt):
    c = Case.get((128, 72, 130, 70, 60.0, 40.0), 1)
    fd, p, dw, dh, rb = dev(c.f, cuda), c.p, c.dw, c.dh, c.rb
    of = vs.OUT_BGR8 if fmt == "bgr" else vs.OUT_NV12_PLANAR
    for mode in (0, 1, 3):
        # no rot_bottom, no dist
        same(call(vs, fd, p, dw, dh, mode, None, None, "linear", CONSTANT, fmt), host(vs.warp_nv12(fd, p, dw, dh, mode, of)), ("warp_nv12_ex", mode, fmt))
        same(call(vs, fd, p, dw, dh, mode, None, None, "cubic", CONSTANT, fmt), host(vs.warp_nv12_cubic(fd, p, dw, dh, mode, of)), ("cubic", mode, fmt))
        same(call(vs, fd, p, dw, dh, mode, None, None, "lanczos4", CONSTANT, fmt), host(vs.warp_nv12_lanczos4(fd, p, dw, dh, mode, of)), ("lanczos4", mode, fmt))
        for border in (REPLICATE, REFLECT, REFLECT_101):
            same(call(vs, fd, p, dw, dh, mode, None, None, "linear", border, fmt), host(vs.warp_nv12_border(fd, p, dw, dh, mode, of, border)), ("border", mode, border, fmt))
            same(call(vs, fd, p, dw, dh, mode, None, None, "cubic", border, fmt), host(vs.warp_nv12_cubic_border(fd, p, dw, dh, mode, of, border)),
                 ("cubic_border", mode, border, fmt))
            same(call(vs, fd, p, dw, dh, mode, None, None, "lanczos4", border, fmt), host(vs.warp_nv12_lanczos4_border(fd, p, dw, dh, mode, of, border)),
                 ("lanczos4_border", mode, border, fmt))
    # dist alone
    for mode in (1, 2):
        for resampler, border in (("linear", CONSTANT), ("linear", REFLECT), ("cubic", CONSTANT), ("cubic", REFLECT_101), ("lanczos4", REPLICATE)):
            same(call(vs, fd, p, dw, dh, mode, None, dd.D_A, resampler, border, fmt),
                 host(vs.warp_nv12_dist_ex(fd, p, dd.D_A, dw, dh, mode, RESAMPLE[resampler], border, of)), ("dist_ex", mode, resampler, border, fmt))
    # DEFAULT + rot_bottom: the border warp; with the constant border that is vstab_warp_nv12_rs
    for mode in (0, 1):
        for border in BORDERS:
            same(call(vs, fd, p, dw, dh, mode, rb, None, "linear", border, fmt), host(vs.warp_nv12_border(fd, p, dw, dh, mode, of, border, rot_bottom=rb)),
                 ("border + rot_bottom", mode, border, fmt))
        same(call(vs, fd, p, dw, dh, mode, rb, None, "linear", CONSTANT, fmt), host(vs.warp_nv12_rs(fd, p, rb, dw, dh, mode, of)), ("warp_nv12_rs", mode, fmt))


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------------------------------
READOUTS = [oracle.rodrigues((0.002 * (k % 3), -0.003, 0.001 * k)) for k in range(6)]


def pull_one(stab, how):
    return host(stab.pull() if how == "pull" else stab.pull_nv12(planar=True))


@pytest.mark.parametrize("how", ["pull", "planar"])
@pytest.mark.parametrize("resampler,border", [("cubic", CONSTANT), ("lanczos4", REFLECT_101)])
def test_pipeline_per_row_on_resampled_handles(vs, cuda, clip, resampler, border, how):
    """A cubic handle and a Lanczos handle with REFLECT_101 (map mode 0): with VSTAB_READOUT_PER_ROW every frame is delivered and equals
    the definition with the last row's rotation from readout @ W."""
    import torch
    K, Ko, cw, ch, frames = clip
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames[:6]], total=6, smooth_radius=1, tracking=0, readouts=READOUTS,
                         map_precision=expect.IEEE, resample=RESAMPLE[resampler], border_mode=border)
    stab.set_readout_warp(vs.READOUT_PER_ROW)
    for i in range(5):
        o = pull_one(stab, how)
        Wr = stab.warp_rotation(i)
        p, rb = oracle.map_params(K, Ko, Wr), oracle.map_params(K, Ko, READOUTS[i + 1] @ Wr)[8:]
        e = wd.Expected(frames[i + 1], *wd.maps(p, cw, ch, 0, rb))
        same(o, e.bgr(resampler, border) if how == "pull" else e.planar(resampler, border), ("pipeline", resampler, how, i))
    assert stab.pull() is None
    stab.close()


@pytest.mark.parametrize("how", ["pull", "planar"])
def test_pipeline_per_row_on_a_calibrated_cubic_handle(vs, cuda, how):
    import torch
    frames = [synth.nv12(60 + k, W, H) for k in range(6)]
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=6, readouts=READOUTS, calibration_ex=(K_CAL, dd.D_A),
                         resample=vs.RESAMPLE_CUBIC, **dict(LENS, smooth_radius=1, tracking=0))
    stab.set_readout_warp(vs.READOUT_PER_ROW)
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, OW, OH)
    for i in range(5):
        o = pull_one(stab, how)
        Wr = stab.warp_rotation(i)
        p, rb = oracle.map_params(K_CAL, Kout, Wr), oracle.map_params(K_CAL, Kout, READOUTS[i + 1] @ Wr)[8:]
        e = wd.Expected(frames[i + 1], *wd.maps(p, OW, OH, 1, rb, dd.D_A))
        same(o, e.bgr("cubic", CONSTANT) if how == "pull" else e.planar("cubic", CONSTANT), ("calibrated pipeline", how, i))
    assert stab.pull() is None
    stab.close()


def test_pipeline_default_refuses_and_the_mode_toggles_between_pulls(vs, cuda, clip):
    """Without the call a cubic handle refuses (and consumes) a frame with a read-out rotation, with today's message; the mode may change
    between pulls: frames pulled under PER_ROW are the definition's, those under REFUSE are refused."""
    import torch
    K, Ko, cw, ch, frames = clip
    msg = "VSTAB_RESAMPLE_CUBIC warps frames without a read-out rotation (vstab_frame.readout_rotation)"

    def handle():
        return vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames[:6]], total=6, smooth_radius=1, tracking=0, readouts=READOUTS,
                             map_precision=expect.IEEE, resample=vs.RESAMPLE_CUBIC)
    stab = handle()
    for i in range(5):
        assert refused(vs, stab.pull) == (vs.ERR_INVALID, msg), i
    assert stab.pull() is None
    stab.close()
    stab = handle()
    for i in range(5):
        per_row = i in (1, 2, 4)
        stab.set_readout_warp(vs.READOUT_PER_ROW if per_row else vs.READOUT_REFUSE)
        if not per_row:
            assert refused(vs, stab.pull) == (vs.ERR_INVALID, msg), i
            continue
        o = host(stab.pull())
        Wr = stab.warp_rotation(i)
        p, rb = oracle.map_params(K, Ko, Wr), oracle.map_params(K, Ko, READOUTS[i + 1] @ Wr)[8:]
        eq(o, wd.bgr(frames[i + 1], *wd.maps(p, cw, ch, 0, rb, None), "cubic", CONSTANT), ("toggled", i))
    # NV12 through BGR stays refused, before a frame is taken
    assert refused(vs, stab.pull_nv12)[0] == vs.ERR_INVALID
    assert stab.pull() is None
    stab.close()


def test_pipeline_frames_without_a_readout_keep_the_quantised_map(vs, cuda):
    """A calibrated RESAMPLE_DEFAULT handle, still camera: frames 1 and 3 alone carry a read-out rotation.  They are warped per row; every
    other frame is byte for byte what it is when no frame of the clip carries one (the quantised map neither used nor refreshed by them)."""
    import torch
    frames = [synth.nv12(60 + k, W, H) for k in range(7)]
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    cfg = dict(LENS, smooth_radius=1, tracking=0)
    plain = vs.Stabilizer(devf, total=7, calibration=(K_CAL, dd.D_A), **cfg)
    base = [host(plain.pull()) for _ in range(6)]
    plain.close()
    state = {"i": 0}
    dp = ctypes.POINTER(ctypes.c_double)
    rot = np.ascontiguousarray(READOUTS[2], np.float64)

    def fill(out, advance):
        i = state["i"]
        if i >= len(devf):
            return vs.EOF
        t, o = devf[i], out.contents
        o.y, o.uv = t.data_ptr(), t.data_ptr() + H * t.stride(0)
        o.pitch_y = o.pitch_uv = t.stride(0)
        o.width, o.height, o.mem, o.pts, o.hold, o.bit_depth = W, H, 0, i, 1 << 30, 8
        o.readout_rotation = rot.ctypes.data_as(dp) if i in (1, 3) else None
        if advance:
            state["i"] += 1
        return 0
    pull, peek = vs.PULL_FN(lambda u, o: fill(o, True)), vs.PULL_FN(lambda u, o: fill(o, False))
    src = vs.Source(pull, peek, None)
    c = vs.default_config(**cfg)
    h = ctypes.c_void_p()
    assert vs.lib.vstab_create(ctypes.byref(c), ctypes.byref(src), ctypes.byref(h)) == vs.OK, vs.lib.vstab_last_error()
    try:
        Kc, Dc = np.ascontiguousarray(K_CAL.reshape(9)), np.array(dd.D_A, np.float64)
        assert vs.lib.vstab_set_input_calibration(h, Kc.ctypes.data_as(dp), Dc.ctypes.data_as(dp)) == vs.OK, vs.lib.vstab_last_error()
        assert vs.lib.vstab_set_readout_warp(h, vs.READOUT_PER_ROW) == vs.OK, vs.lib.vstab_last_error()
        Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, OW, OH)
        p = oracle.map_params(K_CAL, Kout, np.eye(3))
        rb = oracle.map_params(K_CAL, Kout, READOUTS[2])[8:]
        per_row = None
        for k in range(1, 7):
            o = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
            assert vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0)) == vs.OK, (k, vs.lib.vstab_last_error())
            if k in (1, 3):
                per_row = per_row or wd.maps(p, OW, OH, 1, rb, dd.D_A)
                eq(o.cpu().numpy(), wd.bgr(frames[k], per_row[0], per_row[1], "linear", CONSTANT), ("per row", k))
                assert not np.array_equal(o.cpu().numpy(), base[k - 1])
            else:
                eq(o.cpu().numpy(), base[k - 1], ("untouched", k))
        assert vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0)) == vs.EOF
    finally:
        vs.lib.vstab_destroy(h)


def test_set_readout_warp_refusals(vs, cuda):
    import torch
    frames = [synth.nv12(60 + k, W, H) for k in range(3)]
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    n = "vstab_set_readout_warp: "
    s = vs.Stabilizer(devf, total=3, smooth_radius=1, tracking=0, resample=vs.RESAMPLE_CUBIC)
    for bad in (-1, 2, 7):
        assert refused(vs, s.set_readout_warp, bad) == (vs.ERR_INVALID, n + "mode must be VSTAB_READOUT_REFUSE (0) or VSTAB_READOUT_PER_ROW (1)")
    s.set_readout_warp(vs.READOUT_PER_ROW), s.set_readout_warp(vs.READOUT_REFUSE)
    s.close()
    unsupported = n + "served for 8-bit pixels with INTER_LINEAR, INTER_CUBIC or INTER_LANCZOS4"
    s = vs.Stabilizer(devf, total=3, smooth_radius=1, tracking=0, interpolation=0)
    assert refused(vs, s.set_readout_warp, vs.READOUT_PER_ROW) == (vs.ERR_UNSUPPORTED, unsupported)
    s.close()
    wide = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in frames]
    s = vs.Stabilizer(wide, total=3, bit_depth=10, pixel_depth=10, smooth_radius=1, tracking=0)
    assert refused(vs, s.set_readout_warp, vs.READOUT_PER_ROW) == (vs.ERR_UNSUPPORTED, unsupported)
    s.close()
    assert vs.lib.vstab_set_readout_warp(None, vs.READOUT_PER_ROW) == vs.ERR_INVALID
    assert vs.lib.vstab_last_error() == (n + "null handle").encode()
