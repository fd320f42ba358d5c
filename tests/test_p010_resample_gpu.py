"""GPU tests of vstab_warp_p010_planar_ex and vstab_set_resample10 (include/vstab.h, "Cubic and Lanczos resampling at 10 bits"): every
output word of luma and chroma against the numpy definition (tests/warp10_def.py), on fullrange.p010_extreme_frame (junk in the low six
bits) and on a seeded random frame.  Shapes: the smallest that reach the tile states tests/test_p010_resample_cpu.py asserts for them
(every box staged, tiles without a box, every tile gathered, no-box / staged / gathered tiles in one launch, boxes of exactly the budget
and one over it on either plane, tiles wholly outside and boxes across all four edges, partial tiles, the smallest source)."""
import numpy as np
import pytest

import expect
import fullrange
import oracle
import warp10_def as w10
import warp_def as wd
import warp_tiles as wt
from test_distort_gpu import refused

pytestmark = pytest.mark.gpu

CONSTANT, REPLICATE, REFLECT, REFLECT_101 = wd.CONSTANT, wd.REPLICATE, wd.REFLECT, wd.REFLECT_101
RESAMPLERS = w10.RESAMPLERS
RESAMPLE = wd.RESAMPLE


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint16)


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = got != exp
    assert not bad.any(), (what, int(bad.sum()), "of", bad.size, "first at", tuple(int(v[0]) for v in np.nonzero(bad)),
                           "got", int(got[bad][0]), "expected", int(exp[bad][0]))


def frames_of(sw, sh, seed):
    """-> {name: (y16, uv16)}: the extreme frame with junk below the ten bits, and a seeded random frame of whole words."""
    y16, uv16, _, _ = fullrange.p010_extreme_frame(seed, sw, sh)
    rng = np.random.default_rng(seed + 1)
    return {"extreme": (y16, uv16), "random": (rng.integers(0, 65536, (sh, sw)).astype(np.uint16), rng.integers(0, 65536, (sh // 2, sw)).astype(np.uint16))}


class Case:
    """One source size, parameter set and output size: the definition's map and the frames made once, shared by every test with the key."""
    _made = {}

    def __init__(self, sw, sh, dw, dh, params, mode, rb=None, seed=800):
        self.sw, self.sh, self.dw, self.dh, self.p, self.mode, self.rb = sw, sh, dw, dh, np.asarray(params, np.float32), mode, rb
        self.maps = wd.maps(self.p, dw, dh, mode, rb)
        self.frames = frames_of(sw, sh, seed + mode)
        self._dev, self._exp = {}, {}

    @classmethod
    def get(cls, key, make):
        if key not in cls._made:
            cls._made[key] = make()
        return cls._made[key]

    @classmethod
    def geometry(cls, geometry, mode, rot, r0=wd.R0, r_bottom=wd.R_BOTTOM):
        def make():
            sw, sh, dw, dh, fi, fo = geometry
            p, rb = wd.case_params(sw, sh, dw, dh, fi, fo, r0, r_bottom)
            return cls(sw, sh, dw, dh, p, mode, rb if rot else None)
        return cls.get((geometry, mode, rot, r0, r_bottom), make)

    @classmethod
    def tile_set(cls, kernel, name):
        def make():
            p, sw, sh, dw, dh, mode = wt.set_params(kernel, name)
            return cls(sw, sh, dw, dh, p, mode)
        return cls.get((kernel, name), make)

    def expected(self, frame, resampler, border):
        k = (frame, resampler, border)
        if k not in self._exp:
            self._exp[k] = w10.planar10(*self.frames[frame], *self.maps, resampler, border)
        return self._exp[k]

    def run(self, vs, cuda, frame, resampler, border):
        if frame not in self._dev:
            self._dev[frame] = tuple(dev(a, cuda) for a in self.frames[frame])
        y, uv = self._dev[frame]
        oy, ouv = vs.warp_p010_planar_ex(y, uv, self.p, self.dw, self.dh, self.rb, self.mode, RESAMPLE[resampler], border)
        return host(oy), host(ouv)

    def check(self, vs, cuda, resampler, border, what, frames=("extreme", "random")):
        for frame in frames:
            gy, guv = self.run(vs, cuda, frame, resampler, border)
            ey, euv = self.expected(frame, resampler, border)
            eq(gy, ey, (what, frame, resampler, border, self.mode, "luma"))
            eq(guv, euv, (what, frame, resampler, border, self.mode, "chroma"))
        return gy, guv


# ---------------------------------------------------------------------------------------------------------------------
# (a) ZOOMED_OUT: every box staged, under the constant border tiles without a box
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [False, True], ids=["one_rotation", "rot_bottom"])
@pytest.mark.parametrize("border", wd.ALL_BORDERS)
@pytest.mark.parametrize("resampler", RESAMPLERS)
@pytest.mark.parametrize("mode", [0, 1, 5])
def test_zoomed_out(vs, cuda, mode, resampler, border, rot):
    """128 x 72 -> 200 x 100; mode 5's map is the reference kernel's on this GPU."""
    Case.geometry(wd.ZOOMED_OUT, mode, rot).check(vs, cuda, resampler, border, "zoomed out")


def test_rot_bottom_moves_the_frame(vs, cuda):
    a, b = Case.geometry(wd.ZOOMED_OUT, 1, True), Case.geometry(wd.ZOOMED_OUT, 1, False)
    assert (a.expected("random", "cubic", REFLECT)[0] != b.expected("random", "cubic", REFLECT)[0]).mean() > 0.2


# ---------------------------------------------------------------------------------------------------------------------
# (b) the other map modes; an odd output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", wd.ALL_BORDERS)
@pytest.mark.parametrize("resampler", RESAMPLERS)
@pytest.mark.parametrize("mode", [2, 3, 4])
def test_other_map_modes(vs, cuda, mode, resampler, border):
    Case.geometry(wd.ZOOMED_OUT, mode, False).check(vs, cuda, resampler, border, "modes 2 - 4")


@pytest.mark.parametrize("border", wd.ALL_BORDERS)
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_odd_output(vs, cuda, resampler, border):
    """128 x 72 -> 199 x 99: the last column and row are odd, the chroma plane is ceil-sized."""
    c = Case.geometry((128, 72, 199, 99, 60.0, 40.0), 1, True)
    gy, guv = c.check(vs, cuda, resampler, border, "odd output")
    assert gy.shape == (99, 199) and guv.shape == (50, 200)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the larger sets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [False, True], ids=["one_rotation", "rot_bottom"])
@pytest.mark.parametrize("border", [CONSTANT, REFLECT_101])
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_gathers(vs, cuda, resampler, border, rot):
    """2048 x 512 -> 128 x 32: every tile of both planes is over the budget, every sample is blended from global memory."""
    Case.geometry(wd.GATHERS, 1, rot, wd.GATHERS_R0, wd.GATHERS_R_BOTTOM).check(vs, cuda, resampler, border, "gathers", ("extreme",))


# kernel (whose resampler and border mode the set is run under), set
SETS = [("cubic", "all_states"), ("lanczos4", "all_states"),
        ("cubic", "bgr_at_budget"), ("cubic", "bgr_at_budget_m0"), ("lanczos4", "bgr_at_budget"), ("cubic_border", "bgr_at_budget"),
        ("lanczos4_border", "bgr_at_budget"), ("cubic", "bgr_over_by_one")]


@pytest.mark.parametrize("kernel,name", SETS)
def test_tile_sets(vs, cuda, kernel, name):
    """No-box, staged and gathered tiles in one launch (4096 x 256 -> 1023 x 47); luma boxes of exactly 6144 words and of 6145."""
    resampler, border = wt.KERNELS[kernel]
    Case.tile_set(kernel, name).check(vs, cuda, resampler, border, (kernel, name), ("extreme",))


@pytest.mark.parametrize("border", [CONSTANT, REFLECT_101])
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_chroma_box_of_exactly_the_budget(vs, cuda, resampler, border):
    def make():
        p, sw, sh, dw, dh, mode = w10.chroma_set_params(resampler)
        return Case(sw, sh, dw, dh, p, mode)
    Case.get(("chroma_at_budget", resampler), make).check(vs, cuda, resampler, border, "chroma at budget", ("extreme",))


@pytest.mark.parametrize("border", wd.MODES)
@pytest.mark.parametrize("kernel", ["cubic_border", "lanczos4_border"])
def test_border_zoomed_out(vs, cuda, kernel, border):
    """96 x 64 -> 512 x 256, map mode 3: tiles wholly outside stage folded picture, boxes cross all four edges."""
    Case.tile_set(kernel, "zoomed_out").check(vs, cuda, wt.KERNELS[kernel][0], border, (kernel, "zoomed_out"), ("extreme",))


# ---------------------------------------------------------------------------------------------------------------------
# (d) the smallest source
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", wd.ALL_BORDERS)
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_smallest_source(vs, cuda, resampler, border):
    """8 x 2 -> 64 x 16: the chroma plane is 4 x 1 (REFLECT_101 of length 1)."""
    Case.geometry((8, 2, 64, 16, 6.0, 30.0), 1, True).check(vs, cuda, resampler, border, "8 x 2")


# ---------------------------------------------------------------------------------------------------------------------
# (e) layouts
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 0x5A5B


@pytest.mark.parametrize("border", [CONSTANT, REFLECT])
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_pitches_alignments_and_guard_words(vs, cuda, resampler, border):
    """Pitches wider than the rows; luma planes at addresses 2 mod 4, chroma planes at 4 mod 16; the words around both output planes, the
    row tails included, unchanged; the low six bits of every output word zero."""
    import torch
    c = Case.geometry((128, 72, 199, 99, 60.0, 40.0), 1, True)
    y16, uv16 = c.frames["extreme"]
    sw, sh, dw, dh = c.sw, c.sh, c.dw, c.dh

    def plane(a, pitch, offset):
        """a (rows, n) as a view with `pitch` words per row that starts `offset` words into a fresh buffer"""
        rows, n = a.shape
        buf = torch.full((offset + rows * pitch + 8,), 0x7777, dtype=torch.int16, device=cuda)
        v = buf[offset:offset + rows * pitch].view(rows, pitch)[:, :n]
        v.copy_(dev(a, cuda))
        return buf, v
    _, y = plane(y16, sw + 6, 1)
    _, uv = plane(uv16, sw + 10, 2)
    assert y.data_ptr() % 4 == 2 and uv.data_ptr() % 16 == 4
    cdw, cdh = 2 * ((dw + 1) // 2), (dh + 1) // 2
    guard = np.array(GUARD, np.uint16).view(np.int16).item()
    py, puv, oy_off, ouv_off = dw + 5, cdw + 6, 3, 2
    by = torch.full((oy_off + dh * py + 8,), guard, dtype=torch.int16, device=cuda)
    buv = torch.full((ouv_off + cdh * puv + 8,), guard, dtype=torch.int16, device=cuda)
    oy = by[oy_off:oy_off + dh * py].view(dh, py)[:, :dw]
    ouv = buv[ouv_off:ouv_off + cdh * puv].view(cdh, puv)[:, :cdw]
    assert oy.data_ptr() % 4 == 2 and ouv.data_ptr() % 16 == 4
    vs.warp_p010_planar_ex(y, uv, c.p, dw, dh, c.rb, c.mode, RESAMPLE[resampler], border, out_y=oy, out_uv=ouv)
    ey, euv = c.expected("extreme", resampler, border)
    for buf, off, rows, pitch, n, exp, what in ((by, oy_off, dh, py, dw, ey, "luma"), (buv, ouv_off, cdh, puv, cdw, euv, "chroma")):
        b = host(buf)
        inner = b[off:off + rows * pitch].reshape(rows, pitch)
        eq(inner[:, :n], exp, ("layout", what, resampler, border))
        assert not (inner[:, :n] & 63).any()
        assert (inner[:, n:] == GUARD).all() and (b[:off] == GUARD).all() and (b[off + rows * pitch:] == GUARD).all(), what


# ---------------------------------------------------------------------------------------------------------------------
# (f) against the 8-bit kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", wd.MODES)
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_bytes_shifted_up_give_the_8_bit_kernels_frames(vs, cuda, resampler, border):
    """A P010 frame made of an NV12 frame (word = byte << 6): min(out >> 6, 255) is the plane-wise output of vstab_warp_nv12_cubic_border /
    _lanczos4_border, byte for byte."""
    import torch
    sw, sh, dw, dh = 128, 72, 130, 70
    p, _ = wd.case_params(sw, sh, dw, dh, 60.0, 40.0)
    nv12 = np.random.default_rng(31).integers(0, 256, (sh * 3 // 2, sw), dtype=np.uint8)
    wide = nv12.astype(np.uint16) << 6
    warp8 = vs.warp_nv12_cubic_border if resampler == "cubic" else vs.warp_nv12_lanczos4_border
    for mode in (1, 3):
        y8, uv8 = (t.cpu().numpy() for t in warp8(torch.from_numpy(nv12).to(cuda), p, dw, dh, mode, vs.OUT_NV12_PLANAR, border))
        oy, ouv = vs.warp_p010_planar_ex(dev(wide[:sh], cuda), dev(wide[sh:], cuda), p, dw, dh, None, mode, RESAMPLE[resampler], border)
        eq(np.minimum(host(oy) >> 6, 255), y8, ("8-bit twin", resampler, border, mode, "luma"))
        eq(np.minimum(host(ouv) >> 6, 255), uv8, ("8-bit twin", resampler, border, mode, "chroma"))


# ---------------------------------------------------------------------------------------------------------------------
# (g) the pipeline
# ---------------------------------------------------------------------------------------------------------------------
W, H, N = 320, 180, 6
READOUTS = [oracle.rodrigues((0.002 * (k % 3), -0.003, 0.001 * k)) for k in range(N)]


@pytest.fixture(scope="module")
def clip10(cuda):
    K = oracle.get_preset_camera(4, W, H)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    wide = [np.concatenate(fullrange.p010_extreme_frame(70 + k, W, H)[:2]) for k in range(N)]
    return K, Ko, cw, ch, wide, [dev(f, cuda) for f in wide]


def out_planes(cw, ch, cuda):
    import torch
    return torch.empty((ch, cw), dtype=torch.int16, device=cuda), torch.empty(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device=cuda)


def handle(vs, devf, readouts=None):
    return vs.Stabilizer(devf, total=N, bit_depth=10, pixel_depth=10, smooth_radius=1, tracking=0, readouts=readouts, map_precision=expect.IEEE)


def test_pipeline_pulls_with_the_resampler_set_between_pulls(vs, cuda, clip10):
    """(LANCZOS4, REFLECT_101), then (CUBIC, CONSTANT), set between pulls: every plane-wise pull is the definition under warp_rotation(i),
    the frame's read-out rotation warped per row.  The converting pulls are refused before a frame is taken: the same frame then pulls
    plane-wise."""
    import torch
    K, Ko, cw, ch, wide, devf = clip10
    stab = handle(vs, devf, READOUTS)
    refusal = ("vstab_pull_frame: VSTAB_RESAMPLE_%s on a pixel_depth 10 handle (vstab_set_resample10) emits plane-wise P010 frames "
               "(vstab_pull_frame_p010_planar), not 16-bit BGR or P010 through BGR")
    for i in range(N - 1):
        resampler, border = ("lanczos4", REFLECT_101) if i < 2 else ("cubic", CONSTANT)
        stab.set_resample10(RESAMPLE[resampler], border)
        oy, ouv = out_planes(cw, ch, cuda)
        if i in (1, 3):
            bgr = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
            assert refused(vs, stab.pull_bgr16_into, bgr) == (vs.ERR_INVALID, refusal % resampler.upper()), i
            assert refused(vs, stab.pull_p010_into, oy, ouv) == (vs.ERR_INVALID, refusal % resampler.upper()), i
        assert stab.pull_p010_planar_into(oy, ouv), i
        Wr = stab.warp_rotation(i)
        p, rb = oracle.map_params(K, Ko, Wr), oracle.map_params(K, Ko, READOUTS[i + 1] @ Wr)[8:]
        ey, euv = w10.planar10(wide[i + 1][:H], wide[i + 1][H:], *wd.maps(p, cw, ch, 0, rb), resampler, border)
        eq(host(oy), ey, ("pipeline", i, resampler, "luma")), eq(host(ouv), euv, ("pipeline", i, resampler, "chroma"))
        one = w10.planar10(wide[i + 1][:H], wide[i + 1][H:], *wd.maps(p, cw, ch, 0), resampler, border)[0]
        assert (one != ey).mean() > 0.2, "the read-out rotation moved too few words"
    oy, ouv = out_planes(cw, ch, cuda)
    assert not stab.pull_p010_planar_into(oy, ouv)
    stab.close()


def test_pipeline_default_restores_the_handle(vs, cuda, clip10):
    """After (DEFAULT, CONSTANT) the frames are those of a handle that never made the call; the colour spec of the converting pulls is
    untouched by the calls."""
    import torch
    K, Ko, cw, ch, wide, devf = clip10
    a, b = handle(vs, devf), handle(vs, devf)
    a.set_colour10(vs.COLOUR_BT709, vs.RANGE_LIMITED), b.set_colour10(vs.COLOUR_BT709, vs.RANGE_LIMITED)
    a.set_resample10(vs.RESAMPLE_CUBIC, vs.BORDER_REPLICATE)
    for i in range(N - 1):
        if i == 1:
            a.set_resample10(vs.RESAMPLE_DEFAULT, vs.BORDER_CONSTANT)
        (ay, auv), (by, buv) = out_planes(cw, ch, cuda), out_planes(cw, ch, cuda)
        if i == 3:       # a converting pull, with the spec set before: served again, and the same on both handles
            ab, bb = (torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda) for _ in range(2))
            assert a.pull_bgr16_into(ab) and b.pull_bgr16_into(bb)
            eq(host(ab), host(bb), ("restored, bgr16", i))
            continue
        assert a.pull_p010_planar_into(ay, auv) and b.pull_p010_planar_into(by, buv), i
        same = np.array_equal(host(ay), host(by)) and np.array_equal(host(auv), host(buv))
        assert same == (i >= 1), i
        if i == 0:
            p = oracle.map_params(K, Ko, a.warp_rotation(0))
            ey, euv = w10.planar10(wide[1][:H], wide[1][H:], *wd.maps(p, cw, ch, 0), "cubic", REPLICATE)
            eq(host(ay), ey, "cubic before the restore, luma"), eq(host(auv), euv, "cubic before the restore, chroma")
    a.close(), b.close()


def test_set_resample10_refusals_on_live_handles(vs, cuda, clip10):
    import torch
    K, Ko, cw, ch, wide, devf = clip10
    n = "vstab_set_resample10: "
    s = handle(vs, devf)
    assert refused(vs, s.set_resample10, 3, 0) == (vs.ERR_INVALID, n + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)")
    assert refused(vs, s.set_resample10, vs.RESAMPLE_DEFAULT, vs.BORDER_REFLECT)[0] == vs.ERR_UNSUPPORTED
    # the handle is unchanged: the converting pull is served, the plane-wise one is the bilinear warp
    bgr = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
    assert s.pull_bgr16_into(bgr)
    s.close()
    nv12 = [torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device=cuda) for _ in range(3)]
    s8 = vs.Stabilizer(nv12, total=3, smooth_radius=1, tracking=0)
    assert refused(vs, s8.set_resample10, vs.RESAMPLE_CUBIC, vs.BORDER_CONSTANT) == (
        vs.ERR_UNSUPPORTED, n + "served for pixel_depth 10 handles; an 8-bit handle takes its resampler from vstab_config.resample and its border mode from "
                                "vstab_set_border_mode_ex")
    assert s8.pull() is not None
    s8.close()
