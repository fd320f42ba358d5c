"""GPU parity of the border modes of the cubic and Lanczos resamplers (include/vstab.h "Border modes of the cubic and Lanczos resamplers")
through the C ABI and the pipeline object: vstab_remap_{cubic,lanczos4}_border, vstab_warp_nv12_{cubic,lanczos4}_border (BGR8 and plane-wise
NV12) and vstab_set_border_mode_ex.  Bar: every byte equals the numpy definition (tests/warp_def.py) fed by the oracle's maps, and
every output plane is guarded by canary bytes (tests/layouts.py).  Under BORDER_CONSTANT the new entry points give the bytes of the pinned
ones (vstab_remap_cubic / _lanczos4, vstab_warp_nv12_cubic / _lanczos4)."""
import ctypes

import numpy as np
import pytest

import expect
import layouts
import oracle
import warp_def as wd
import warp_tiles as wt
from test_resample_border_cpu import TILE_KEYS
import synth
from test_border_gpu import PAST, ROT, cams, dev, eq, map_modes
from test_layouts_gpu import PITCH_UV_4G

pytestmark = pytest.mark.gpu

MODES = wd.MODES
RESAMPLERS = ("cubic", "lanczos4")
RESAMPLE = {"cubic": 2, "lanczos4": 4}   # vstab_config.resample


# ---- the C ABI with separate, canaried planes ---------------------------------------------------------------------------------------
def warp_rb(vs, resampler, s, params, dw, dh, mode, out_format, border_mode, cuda):
    """vstab_warp_nv12_{resampler}_border on layouts.Src s -> BGR (dh, dw, 3), or (y, uv) plane-wise NV12, read back after the canary check."""
    fn = f"vstab_warp_nv12_{resampler}_border"
    p, pp = layouts._f(params)
    if out_format == vs.OUT_BGR8:
        o = layouts.Plane(dh, 3 * dw, cuda)
        layouts._call(vs, fn, s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), int(border_mode), o.ptr, o.pitch, None, 0,
                      dw, dh, vs._stream())
        return o.host(shape=(dh, dw, 3))
    oy, ou = layouts.out_nv12(dw, dh, cuda)
    layouts._call(vs, fn, s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), int(border_mode), oy.ptr, oy.pitch, ou.ptr,
                  ou.pitch, dw, dh, vs._stream())
    return oy.host(), ou.host()


def remap_rb(vs, resampler, cuda, src, mx, my, border_mode, border=(0, 0, 0)):
    """vstab_remap_{resampler}_border into a canaried Plane -> (dh, dw[, cn]) uint8."""
    s = dev(src, cuda)
    cn = 1 if src.ndim == 2 else src.shape[2]
    dh, dw = mx.shape
    mxt, myt = dev(mx, cuda), dev(my, cuda)
    o = layouts.Plane(dh, dw * cn, cuda)
    bd = (ctypes.c_int * 3)(*border)
    layouts._call(vs, f"vstab_remap_{resampler}_border", s.data_ptr(), s.stride(0), src.shape[1], src.shape[0], cn, mxt.data_ptr(), mxt.stride(0) * 4,
                  myt.data_ptr(), myt.stride(0) * 4, int(border_mode), bd, o.ptr, o.pitch, dw, dh, vs._stream())
    return o.host(shape=(dh, dw, cn) if cn > 1 else (dh, dw))


def check_warp(vs, resampler, cuda, s, f, p, dw, dh, mode, border_mode, what):
    """BGR and plane-wise warps of Src s (packed NV12 f on the host) against the definition."""
    eq(warp_rb(vs, resampler, s, p, dw, dh, mode, vs.OUT_BGR8, border_mode, cuda), wd.bgr(f, *wd.maps(p, dw, dh, mode), resampler, border_mode),
       (what, resampler, "bgr", mode, border_mode))
    gy, guv = warp_rb(vs, resampler, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, border_mode, cuda)
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, mode), resampler, border_mode)
    eq(gy, ey, (what, resampler, "luma", mode, border_mode)), eq(guv, euv, (what, resampler, "chroma", mode, border_mode))


# ---- the stateless remap ------------------------------------------------------------------------------------------------------------
def test_remap_resample_border_golden_vectors(vs, cuda):
    import test_resample_border_cpu
    n = 0
    for k, resampler, src, mx, my, mode, out in test_resample_border_cpu.golden_cases():
        eq(remap_rb(vs, resampler, cuda, src, mx, my, mode), out, k)
        n += 1
    assert n >= 54


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_remap_resample_border_every_channel_count(vs, cuda, resampler):
    rng = np.random.default_rng(21)
    for sw, sh in ((1, 1), (2, 3), (3, 2), (37, 21), (300, 170)):
        for cn in (1, 2, 3):
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            dw, dh = (71, 33) if sw < 100 else (333, 190)
            mx = rng.uniform(-3.0 * sw - 5, 4.0 * sw + 5, (dh, dw)).astype(np.float32)
            my = rng.uniform(-3.0 * sh - 5, 4.0 * sh + 5, (dh, dw)).astype(np.float32)
            special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 32768.0, -32768.0, -0.0], np.float32)
            for m in (mx, my):
                pick = rng.random((dh, dw)) < 0.05
                m[pick] = rng.choice(special, int(pick.sum()))
            for mode in MODES:
                eq(remap_rb(vs, resampler, cuda, src, mx, my, mode), wd.remap(src, mx, my, resampler, mode), (sw, sh, cn, mode))


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_remap_resample_border_constant_equals_pinned_remap(vs, cuda, resampler):
    rng = np.random.default_rng(22)
    pinned = vs.remap_cubic if resampler == "cubic" else vs.remap_lanczos4
    mine = vs.remap_cubic_border if resampler == "cubic" else vs.remap_lanczos4_border
    for cn in (1, 2, 3):
        src = rng.integers(0, 256, (41, 57, cn) if cn > 1 else (41, 57), dtype=np.uint8)
        mx = rng.uniform(-70, 130, (45, 77)).astype(np.float32)
        my = rng.uniform(-50, 90, (45, 77)).astype(np.float32)
        mx[0, :5] = [np.nan, np.inf, -1e30, 32768.0, -32768.0]
        bd = (9, 130, 250)
        ref = pinned(dev(src, cuda), dev(mx, cuda), dev(my, cuda), bd).cpu().numpy()
        eq(remap_rb(vs, resampler, cuda, src, mx, my, vs.BORDER_CONSTANT, bd), ref, cn)
        eq(mine(dev(src, cuda), dev(mx, cuda), dev(my, cuda), vs.BORDER_CONSTANT, bd).cpu().numpy(), ref, ("binding", cn))
        eq(mine(dev(src, cuda), dev(mx, cuda), dev(my, cuda), vs.BORDER_REFLECT).cpu().numpy(),
           wd.remap(src, mx, my, resampler, vs.BORDER_REFLECT), ("binding reflect", cn))


# ---- the warp ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rv", [ROT, PAST])
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_warp_resample_border_every_map_mode(vs, cuda, resampler, rv):
    w, h = 320, 180
    f = synth.nv12(41, w, h, full_range=True)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    p, dw, dh, K, Ko = cams(w, h, rv)
    for mode in map_modes():
        for bm in MODES:
            check_warp(vs, resampler, cuda, s, f, p, dw - 3, dh - 1, mode, bm, ("modes", rv))


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_warp_resample_border_constant_equals_pinned_warps(vs, cuda, resampler):
    w, h = 320, 180
    f = synth.nv12(43, w, h, full_range=True)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    pinned = getattr(vs, f"warp_nv12_{resampler}")
    for rv in (ROT, PAST):
        p, dw, dh, K, Ko = cams(w, h, rv)
        for mode in range(6):
            got = warp_rb(vs, resampler, s, p, dw, dh, mode, vs.OUT_BGR8, vs.BORDER_CONSTANT, cuda)
            eq(got, pinned(dev(f, cuda), p, dw, dh, mode, vs.OUT_BGR8).cpu().numpy(), (rv, mode, "bgr"))
            gy, guv = warp_rb(vs, resampler, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, vs.BORDER_CONSTANT, cuda)
            ry, ruv = pinned(dev(f, cuda), p, dw, dh, mode, vs.OUT_NV12_PLANAR)
            eq(gy, ry.cpu().numpy(), (rv, mode, "y")), eq(guv, ruv.cpu().numpy(), (rv, mode, "uv"))


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_warp_resample_border_binding_and_tiny_source(vs, cuda, resampler):
    """The Python binding, and a 2 x 2 NV12 source (one chroma sample) warped to a larger output: every footprint folds."""
    fn = getattr(vs, f"warp_nv12_{resampler}_border")
    w, h = 128, 72
    f = synth.nv12(44, w, h)
    p, dw, dh, K, Ko = cams(w, h, PAST)
    eq(fn(dev(f, cuda), p, dw, dh, 0, vs.OUT_BGR8, vs.BORDER_REPLICATE).cpu().numpy(), wd.bgr(f, *wd.maps(p, dw, dh, 0), resampler, vs.BORDER_REPLICATE),
       "binding bgr")
    y, uv = fn(dev(f, cuda), p, dw, dh, 1, vs.OUT_NV12_PLANAR, vs.BORDER_REFLECT)
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, 1), resampler, vs.BORDER_REFLECT)
    eq(y.cpu().numpy(), ey, "binding y"), eq(uv.cpu().numpy(), euv, "binding uv")
    tiny = np.array([[10, 200], [90, 250], [60, 180]], np.uint8)
    s = layouts.place(tiny[:2], tiny[2:], "packed", cuda)
    Ki = np.array([[3.0, 0, 1.0], [0, 3.0, 1.0], [0, 0, 1]])
    Ko2 = np.array([[30.0, 0, 35.0], [0, 30.0, 20.0], [0, 0, 1]])
    pt = oracle.map_params(Ki, Ko2, oracle.rodrigues((0.05, -0.1, 0.3)))
    for bm in MODES:
        check_warp(vs, resampler, cuda, s, tiny, pt, 70, 41, 3, bm, "tiny")


@pytest.mark.parametrize("key", TILE_KEYS)
def test_resample_border_tile_sets(vs, cuda, key):
    """The sets of tests/warp_tiles.py for k_warp_cubic_border / k_warp_lanczos4_border: staged, gathered, exactly-the-budget, wholly-outside
    and edge-crossing tiles."""
    resampler, name = key
    p, sw, sh, dw, dh, mode = wt.set_params(key[0] + "_border", key[1])
    f = synth.nv12(sum(map(ord, name)), sw, sh, full_range=True)
    s = layouts.place(f[:sh], f[sh:], "packed", cuda)
    for bm in MODES:
        check_warp(vs, resampler, cuda, s, f, p, dw, dh, mode, bm, name)


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_resample_border_chroma_plane_past_4_gib(vs, cuda, resampler):
    """A 640 x 540 frame whose chroma rows from 257 on start past 2^32 bytes (one 4.5 GB allocation): chroma differs row by row."""
    import torch
    w, h = 640, 540
    f = synth.nv12(18, w, h)
    rows = np.arange(h // 2, dtype=np.uint16)[:, None]
    f[h:] = ((f[h:].astype(np.uint16) + 37 * rows) % 256).astype(np.uint8)
    assert PITCH_UV_4G * (h // 2 - 1) >= 1 << 32
    p, dw, dh, K, Ko = cams(w, h, PAST)
    s = layouts.place(f[:h], f[h:], None, cuda, spec=(w, PITCH_UV_4G, "one", 0, w * h))
    try:
        check_warp(vs, resampler, cuda, s, f, p, dw, dh, 0, vs.BORDER_REFLECT_101, "chroma 4g")
    finally:
        del s
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_resample_border_4k_config3_shape(vs, cuda, resampler):
    w, h = 3840, 2160
    f = synth.nv12(78, w, h)
    p, dw, dh, _, _ = cams(w, h, (0.01, -0.02, 0.015))
    assert (dw, dh) == (3524, 1999)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    check_warp(vs, resampler, cuda, s, f, p, dw, dh, 0, vs.BORDER_REFLECT_101, "4k")


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
W, H = 640, 360


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = synth.shaky_clip(6, K, W, H, 8, sigma=0.02)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    return K, Ko, cw, ch, frames


def expect_frame(resampler, f, K, Ko, R, cw, ch, out, how, border_mode, what):
    p = oracle.map_params(K, Ko, R)
    if how == "planar":
        ey, euv = wd.planar(f, *wd.maps(p, cw, ch, 0), resampler, border_mode)
        eq(out[0], ey, (what, "y")), eq(out[1], euv, (what, "uv"))
    else:
        eq(out, wd.bgr(f, *wd.maps(p, cw, ch, 0), resampler, border_mode), what)


@pytest.mark.parametrize("how", ["pull", "frames", "host", "peek", "planar"])
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_pipeline_resample_border_pulls(vs, cuda, clip, resampler, how):
    """A cubic / Lanczos handle with REFLECT_101 (set through vstab_set_border_mode_ex): each pull is the border warp of its frame."""
    from test_border_gpu import pulls
    K, Ko, cw, ch, frames = clip
    stab, outs = pulls(vs, cuda, frames, how, vs.BORDER_REFLECT_101, smooth_radius=2, resample=RESAMPLE[resampler], map_precision=expect.IEEE)
    assert len(outs) == len(frames) - 1
    for i, o in enumerate(outs):
        expect_frame(resampler, frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, o, how, vs.BORDER_REFLECT_101, (how, i))
    stab.close()


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_pipeline_resample_border_switches_and_refusals(vs, cuda, clip, resampler):
    """Modes changed between pulls (CONSTANT gives the constant-border resampler's bytes); NV12 through BGR is refused before a frame is taken,
    and no frame is lost; on the same handle vstab_set_border_mode still refuses while vstab_set_border_mode_ex accepts."""
    import torch
    K, Ko, cw, ch, frames = clip
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), smooth_radius=2, tracking=0,
                         resample=RESAMPLE[resampler], map_precision=expect.IEEE)
    for bm in MODES:
        assert vs.lib.vstab_set_border_mode(stab._h, bm) == vs.ERR_UNSUPPORTED
        assert vs.lib.vstab_set_border_mode_ex(stab._h, bm) == vs.OK
    for bad in (3, 5, -1, 8):
        assert vs.lib.vstab_set_border_mode_ex(stab._h, bad) == vs.ERR_INVALID
    stab.set_border_mode_ex(vs.BORDER_REFLECT_101)
    with pytest.raises(vs.VstabError, match="NV12 through BGR"):
        stab.pull_nv12(planar=False)
    seq = [4, 0, 1, 2, 0, 4, 1]
    for i, bm in enumerate(seq):
        stab.set_border_mode_ex(bm)
        planar = i % 3 == 2
        o = stab.pull_nv12(planar=True) if planar else stab.pull()
        assert o is not None, i
        o = tuple(x.cpu().numpy() for x in o) if planar else o.cpu().numpy()
        expect_frame(resampler, frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, o, "planar" if planar else "pull", bm, ("switch", bm, i))
    assert len(seq) == len(frames) - 1 and stab.pull() is None   # every frame was served: the refusal took none
    stab.close()
    p16 = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in frames[:5]]
    stab = vs.Stabilizer(p16, total=5, smooth_radius=1, bit_depth=10, pixel_depth=10)
    assert vs.lib.vstab_set_border_mode_ex(stab._h, vs.BORDER_REPLICATE) == vs.ERR_UNSUPPORTED
    stab.close()
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames[:5]], total=5, smooth_radius=1, interpolation=0)
    assert vs.lib.vstab_set_border_mode_ex(stab._h, vs.BORDER_REPLICATE) == vs.ERR_UNSUPPORTED
    assert vs.lib.vstab_set_border_mode_ex(stab._h, vs.BORDER_CONSTANT) == vs.OK
    stab.close()
