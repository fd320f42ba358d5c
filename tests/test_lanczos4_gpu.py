"""GPU parity of the Lanczos resampler (cv::remap INTER_LANCZOS4; include/vstab.h "Lanczos resampling") through the C ABI and the
pipeline object: vstab_remap_lanczos4, vstab_warp_nv12_lanczos4 (BGR8 and plane-wise NV12) and vstab_config.resample = 4.  Bar: every
byte equals the numpy definition (tests/warp_def.py) fed by the oracle's maps, and no byte around an output plane is written
(canary bands above, below and right of each plane, tests/layouts.py).  Covered:
  - the stateless remap for 1..3 channels: the KAT, pitched maps, an odd source address and pitch, NaN / +-inf / huge / tie entries, the
    int16 saturation edges and the refusal of 32768;
  - the fused and plane-wise warps for map modes 0..5 (both lens modes), several sizes and rotations;
  - the tile sets of tests/test_lanczos4_tiles_cpu.py (staged, gathered, at the LDS budget and just over it);
  - the seven plane layouts and planes past 4 GiB;
  - the pipeline's pulls: BGR, ring, plane-wise, host, peek, decoder-style, DMA-BUF, repeated parameters, refusals."""
import ctypes
import os

import numpy as np
import pytest

import expect
import layouts
import oracle
import synth
import warp_def as wd
import warp_tiles as wt
from test_cubic_gpu import special_maps
from test_cubic_paths_gpu import PITCH_Y_4G, W4, H4, _plane_past_4g, _release, drive, frames_4g, odd_source, pitched_map
from test_layouts_gpu import PITCH_UV_4G, run_pipeline

pytestmark = pytest.mark.gpu

ROT = (0.02, -0.03, 0.01)
ROTS = [(0.0, 0.0, 0.0), ROT, (-0.15, 0.1, 0.3)]
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lanczos4_kat.npz")


def cams(w, h, rvec=ROT):
    K = oracle.get_preset_camera(4, w, h)
    Ko, (dw, dh) = oracle.get_output_camera(K, w, h)
    return oracle.map_params(K, Ko, oracle.rodrigues(rvec)), dw, dh, K, Ko


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp).reshape(np.asarray(got).shape)
    assert np.array_equal(got, exp), (what, int((got != exp).sum()))


def modes_of(mode):
    """The set's own mode, and for mode 0 the reference kernel's map (mode 5) too where it is built."""
    return [mode, 5] if mode == 0 and oracle.ref_gfx950_available() else [mode]


def warp_c(vs, s, params, dw, dh, mode, out_format, cuda, out=None):
    """vstab_warp_nv12_lanczos4 on the planes of a layouts.Src -> BGR (dh, dw, 3), or (y, uv) plane-wise NV12, from canaried Planes
    (or the caller's `out`)."""
    p, pp = layouts._f(params)
    if out_format == vs.OUT_BGR8:
        o = out or layouts.Plane(dh, 3 * dw, cuda)
        layouts._call(vs, "vstab_warp_nv12_lanczos4", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), o.ptr, o.pitch,
                      None, 0, dw, dh, vs._stream())
        return o.host(shape=(dh, dw, 3))
    oy, ou = out or layouts.out_nv12(dw, dh, cuda)
    layouts._call(vs, "vstab_warp_nv12_lanczos4", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), oy.ptr, oy.pitch,
                  ou.ptr, ou.pitch, dw, dh, vs._stream())
    return oy.host(), ou.host()


def check(vs, cuda, s, f, p, dw, dh, mode, what, out_bgr=None, out_planar=None):
    """BGR and plane-wise Lanczos warps of Src s (packed NV12 f on the host) against the definition."""
    eq(warp_c(vs, s, p, dw, dh, mode, vs.OUT_BGR8, cuda, out_bgr), wd.bgr(f, *wd.maps(p, dw, dh, mode), "lanczos4"), (what, "bgr", mode))
    gy, guv = warp_c(vs, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, cuda, out_planar)
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, mode), "lanczos4")
    eq(gy, ey, (what, "luma", mode)), eq(guv, euv, (what, "chroma", mode))


def packed(f, h, cuda):
    return layouts.place(f[:h], f[h:], "packed", cuda)


# ---- the stateless remap -------------------------------------------------------------------------------------------------------
def remap_c(vs, cuda, src_ptr, pitch_src, sw, sh, cn, mx_t, my_t, border, dw, dh):
    """vstab_remap_lanczos4 through the C ABI, map planes as (possibly wider) float tensors with their own pitches, the output a
    canaried Plane -> (dh, dw[, cn]) uint8."""
    o = layouts.Plane(dh, dw * cn, cuda)
    b = (ctypes.c_int * 3)(*(list(border) + [0, 0, 0])[:3])
    st = vs.lib.vstab_remap_lanczos4(src_ptr, pitch_src, sw, sh, cn, mx_t.data_ptr(), mx_t.stride(0) * 4, my_t.data_ptr(), my_t.stride(0) * 4, b,
                                     o.ptr, o.pitch, dw, dh, vs._stream())
    if st != vs.OK:
        raise vs.VstabError(st, "vstab_remap_lanczos4")
    return o.host(shape=(dh, dw, cn) if cn > 1 else (dh, dw))


def test_remap_lanczos4_golden_vectors(vs, cuda):
    import torch
    kat = np.load(KAT)
    n = 0
    while f"case{n}_src" in kat:
        src, mx, my = kat[f"case{n}_src"], kat[f"case{n}_mapx"], kat[f"case{n}_mapy"]
        border = [int(v) for v in kat[f"case{n}_border"]]
        sh, sw = src.shape[:2]
        cn = 1 if src.ndim == 2 else src.shape[2]
        st = torch.from_numpy(np.ascontiguousarray(src)).to(cuda)
        got = remap_c(vs, cuda, st.data_ptr(), st.stride(0), sw, sh, cn, pitched_map(mx, 0, cuda), pitched_map(my, 0, cuda), border, *mx.shape[::-1])
        eq(got, kat[f"case{n}_out"], ("kat", n))
        # and through the binding
        eq(vs.remap_lanczos4(st, torch.from_numpy(mx).to(cuda), torch.from_numpy(my).to(cuda), border).cpu().numpy(), kat[f"case{n}_out"], ("kat binding", n))
        n += 1
    assert n >= 6


def test_remap_lanczos4_pitched_maps_odd_source_canaried_outputs(vs, cuda):
    """Map planes with pitches of their own (x and y differ), a source at an odd address with an odd pitch, odd sizes, 1, 2 and 3
    channels, NaN / +-inf / huge / tie map entries."""
    rng = np.random.default_rng(41)
    for sw, sh, dw, dh in ((1, 1, 13, 7), (3, 9, 29, 11), (203, 97, 131, 75)):
        for cn, border in ((1, (16,)), (2, (128, 128)), (3, (0, 9, 255))):
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            mx, my = special_maps(rng, sw, sh, dw, dh)
            mx[0, :4], my[0, :4] = (-4.0, -3.96875, sw + 3.0, sw + 2.984375), 0.5   # the footprint's outermost taps
            ptr, pitch, keep = odd_source(src, cuda)
            mxt, myt = pitched_map(mx, 5, cuda), pitched_map(my, 17, cuda)
            assert mxt.stride(0) != myt.stride(0)
            got = remap_c(vs, cuda, ptr, pitch, sw, sh, cn, mxt, myt, border, dw, dh)
            eq(got, wd.remap(src, mx, my, "lanczos4", wd.CONSTANT, border), ("remap", sw, cn))
            del keep


def test_remap_lanczos4_int16_saturation_edges(vs, cuda):
    """A 32767 x 2 source: map x of 32766.5, 32767.99 and 1e6 saturate X to 32767, whose footprint still holds columns 32764 .. 32766.
    The same for y on a 2 x 32767 source."""
    import torch
    rng = np.random.default_rng(42)
    xs = np.array([32766.5, 32767.99, 1e6, 32765.3, 32766.0, 32767.0, 32770.9, 32771.0], np.float32)
    ys = np.array([0.0, 0.5, 1.0, 1.7], np.float32)
    for cn, border in ((1, (16,)), (3, (1, 2, 3))):
        for tall in (False, True):
            sw, sh = (2, 32767) if tall else (32767, 2)
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            a, b = np.meshgrid(xs, ys)
            mx, my = (b, a) if tall else (a, b)
            mx, my = np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)
            dh, dw = mx.shape
            st = torch.from_numpy(src).to(cuda)
            got = remap_c(vs, cuda, st.data_ptr(), st.stride(0), sw, sh, cn, pitched_map(mx, 3, cuda), pitched_map(my, 0, cuda), border, dw, dh)
            exp = wd.remap(src, mx, my, "lanczos4", wd.CONSTANT, border)
            eq(got, exp, ("saturation", cn, tall))
            X, Y, _ = wd.quantise(mx, my)
            assert ((Y if tall else X) == 32767).sum() >= 2 * len(ys)


def test_lanczos4_sizes_of_32768_are_refused(vs, cuda):
    import torch
    src = torch.zeros((64, 64), dtype=torch.uint8, device=cuda)
    m = torch.zeros((4, 4), dtype=torch.float32, device=cuda)
    b = (ctypes.c_int * 3)(0, 0, 0)
    o = torch.zeros((4, 4), dtype=torch.uint8, device=cuda)
    for sw, sh, dw, dh in ((32768, 2, 4, 4), (2, 32768, 4, 4), (2, 2, 32768, 4), (2, 2, 4, 32768)):
        st = vs.lib.vstab_remap_lanczos4(src.data_ptr(), 1 << 16, sw, sh, 1, m.data_ptr(), 1 << 17, m.data_ptr(), 1 << 17, b, o.data_ptr(), 1 << 16,
                                         dw, dh, vs._stream())
        assert st == vs.ERR_INVALID, (sw, sh, dw, dh)
    p = np.ascontiguousarray(cams(640, 360)[0], np.float32)
    fp = p.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for sw, sh, dw, dh in ((32768, 2, 4, 4), (2, 32768, 4, 4), (2, 2, 32768, 4), (2, 2, 4, 32768)):
        for fmt in (vs.OUT_BGR8, vs.OUT_NV12_PLANAR, vs.OUT_NV12):
            st = vs.lib.vstab_warp_nv12_lanczos4(src.data_ptr(), 1 << 16, src.data_ptr(), 1 << 16, sw, sh, fp, 0, fmt, o.data_ptr(), 1 << 18,
                                                 o.data_ptr(), 1 << 18, dw, dh, vs._stream())
            assert st == vs.ERR_INVALID, (sw, sh, dw, dh, fmt)
    torch.cuda.synchronize()
    assert bool((o == 0).all())


# ---- the fused and plane-wise warps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(640, 360), (322, 182), (64, 32)])
def test_warp_lanczos4_sizes_and_rotations(vs, cuda, w, h):
    f = synth.nv12(w + h, w, h)
    s = packed(f, h, cuda)
    for rv in ROTS + [(0.6, -0.4, 0.2)]:
        p, dw, dh, _, _ = cams(w, h, rv)
        for m in modes_of(0):
            check(vs, cuda, s, f, p, dw, dh, m, (w, h, rv))
        # odd output sizes: partial tiles on both edges
        check(vs, cuda, s, f, p, dw - 7, dh - 3, 0, (w, h, rv, "odd"))


def test_warp_lanczos4_every_projection_pair(vs, cuda):
    """lens_mode 1's four projection pairs (map modes 1..4), wide and narrow fields of view."""
    w, h, dw, dh = 640, 360, 481, 271
    f = synth.nv12(9, w, h)
    s = packed(f, h, cuda)
    for pin in (oracle.PROJ_RECT, oracle.PROJ_FISH):
        for pout in (oracle.PROJ_RECT, oracle.PROJ_FISH):
            mode = oracle.map_mode(pin, pout)
            for din, dout in ((100.0, 90.0), (150.0, 300.0 if pout == oracle.PROJ_FISH else 120.0)):
                Kin, Kout = oracle.lens_camera(pin, din, w, h), oracle.lens_camera(pout, dout, dw, dh)
                for rv in ROTS[:2]:
                    check(vs, cuda, s, f, oracle.map_params(Kin, Kout, oracle.rodrigues(rv)), dw, dh, mode, (pin, pout, din, dout, rv))


def test_warp_lanczos4_refuses_other_formats(vs, cuda):
    w, h = 128, 72
    f = torch_dev(synth.nv12(1, w, h), cuda)
    p, dw, dh, _, _ = cams(w, h)
    for fmt in (vs.OUT_NV12, 5):
        with pytest.raises(vs.VstabError):
            vs.warp_nv12_lanczos4(f, p, dw, dh, vs.MAP_CREATEMAP_CL, fmt)
    with pytest.raises(vs.VstabError):
        vs.warp_nv12_lanczos4(f, p, dw, dh, 6, vs.OUT_BGR8)
    out = vs.warp_nv12_lanczos4(f, p, dw, dh)   # the binding's own path
    eq(out.cpu().numpy(), wd.bgr(synth.nv12(1, w, h), *wd.maps(p, dw, dh, 0), "lanczos4"), "binding")


def torch_dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- the tile sets: staged, gathered, at the budget and over it -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wt.TILE_SETS["lanczos4"]))
def test_lanczos4_tile_sets(vs, cuda, name):
    p, sw, sh, dw, dh, mode = wt.set_params("lanczos4", name)
    f = synth.nv12(sum(map(ord, name)), sw, sh, full_range=True)
    s = packed(f, sh, cuda)
    for m in modes_of(mode):
        check(vs, cuda, s, f, p, dw, dh, m, name)


# ---- the layout matrix -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["camera", "all_states"])
@pytest.mark.parametrize("name", layouts.LAYOUTS)
def test_lanczos4_every_layout(vs, cuda, name, cam):
    if cam == "camera":
        w, h = 640, 360
        p, dw, dh, _, _ = cams(w, h)
        mode = 0
    else:
        p, w, h, dw, dh, mode = wt.set_params("lanczos4", cam)
    f = synth.nv12(21, w, h)
    s = layouts.place(f[:h], f[h:], name, cuda)
    for m in modes_of(mode):
        check(vs, cuda, s, f, p, dw, dh, m, (name, cam))


def test_lanczos4_plane_alignment(vs, cuda):
    """A chroma plane at an odd address or with an odd pitch is refused, nothing written; a luma plane at an odd address with an odd
    pitch is read byte by byte."""
    w, h = 320, 180
    f = synth.nv12(22, w, h)
    p, dw, dh, _, _ = cams(w, h)
    for spec in ((w, w, "two", 0, 1), (w, w + 1, "two", 0, 0)):
        s = layouts.place(f[:h], f[h:], None, cuda, spec=spec)
        for fmt in (vs.OUT_BGR8, vs.OUT_NV12_PLANAR):
            o = layouts.Plane(dh, 3 * dw, cuda), layouts.out_nv12(dw, dh, cuda)
            with pytest.raises(vs.VstabError) as e:
                warp_c(vs, s, p, dw, dh, 0, fmt, cuda, o[0] if fmt == vs.OUT_BGR8 else o[1])
            assert e.value.status == vs.ERR_INVALID, spec
            for plane in (o[0], o[1][0], o[1][1]):
                assert bool((plane.buf == layouts.CANARY).all()), spec
    s = layouts.place(f[:h], f[h:], None, cuda, spec=(w + 1, w + 2, "two", 1, 2))
    check(vs, cuda, s, f, p, dw, dh, 0, "odd luma")


# ---- planes past 4 GiB -----------------------------------------------------------------------------------------------------------
def _sets_4g():
    """frames_4g's frame with the preset camera (every tile staged) and the set gather_540 (gathered tiles on every plane, and on the
    Lanczos footprint too: tests/test_lanczos4_tiles_cpu.py)."""
    f, sets, K, Ko = frames_4g()
    return f, sets, K, Ko


def _pipeline_4g(vs, cuda, s, f, K, Ko, what):
    for hold in (1 << 29, 0):
        for pulls in ("bgr", "planar"):
            outs = run_pipeline(vs, cuda, [s] * 4, mem=0, hold=hold, pulls=pulls, resample=vs.RESAMPLE_LANCZOS4, map_precision=expect.IEEE)
            for i, (o, R) in enumerate(outs):
                p = oracle.map_params(K, Ko, R)
                ch, cw = (o.shape[:2] if pulls == "bgr" else o[0].shape)
                if pulls == "bgr":
                    eq(o, wd.bgr(f, *wd.maps(p, cw, ch, 0), "lanczos4"), (what, "pipeline", hold, i))
                else:
                    ey, euv = wd.planar(f, *wd.maps(p, cw, ch, 0), "lanczos4")
                    eq(o[0], ey, (what, "pipeline y", hold, i)), eq(o[1], euv, (what, "pipeline uv", hold, i))


@pytest.mark.parametrize("plane", ["chroma", "luma"])
def test_lanczos4_source_plane_past_4_gib(vs, cuda, plane):
    f, sets, K, Ko = _sets_4g()
    spec = (W4, PITCH_UV_4G, "one", 0, W4 * H4) if plane == "chroma" else (PITCH_Y_4G, W4, "two", 0, 0)
    s = layouts.place(f[:H4], f[H4:], None, cuda, spec=spec)
    try:
        for p, dw, dh, label in sets:
            check(vs, cuda, s, f, p, dw, dh, 0, (plane, "4g", label))
        _pipeline_4g(vs, cuda, s, f, K, Ko, (plane, "4g"))
    finally:
        del s
        _release()


@pytest.mark.parametrize("plane", ["bgr", "luma", "chroma"])
def test_lanczos4_output_plane_past_4_gib(vs, cuda, plane):
    f, sets, _, _ = _sets_4g()
    s = packed(f, H4, cuda)
    for p, dw, dh, label in sets:
        cw2, ch2 = 2 * ((dw + 1) // 2), (dh + 1) // 2
        if plane == "bgr":
            o = _plane_past_4g(dh, 3 * dw, cuda)
            eq(warp_c(vs, s, p, dw, dh, 0, vs.OUT_BGR8, cuda, o), wd.bgr(f, *wd.maps(p, dw, dh, 0), "lanczos4"), (plane, label))
        else:
            o = (_plane_past_4g(dh, dw, cuda), layouts.Plane(ch2, cw2, cuda)) if plane == "luma" else \
                (layouts.Plane(dh, dw, cuda), _plane_past_4g(ch2, cw2, cuda))
            gy, guv = warp_c(vs, s, p, dw, dh, 0, vs.OUT_NV12_PLANAR, cuda, o)
            ey, euv = wd.planar(f, *wd.maps(p, dw, dh, 0), "lanczos4")
            eq(gy, ey, (plane, label, "luma")), eq(guv, euv, (plane, label, "chroma"))
        del o
        _release()


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------
W, H = 640, 360


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = synth.shaky_clip(4, K, W, H, 8, sigma=0.004)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    return K, Ko, cw, ch, frames


def expect_lz(frames, K, Ko, outs, pulls, what, mode=0):
    for i, (o, R) in enumerate(outs):
        p = oracle.map_params(K, Ko, R)
        if pulls == "bgr":
            ch, cw = o.shape[:2]
            eq(o, wd.bgr(frames[i + 1], *wd.maps(p, cw, ch, mode), "lanczos4"), (what, i))
        else:
            ch, cw = o[0].shape
            ey, euv = wd.planar(frames[i + 1], *wd.maps(p, cw, ch, mode), "lanczos4")
            eq(o[0], ey, (what, "y", i)), eq(o[1], euv, (what, "uv", i))


def stab_pulls(vs, cuda, frames, how, **cfg):
    """Stabilizer over device frames: how 'pull' (BGR), 'frames' (the ring pull), 'planar' -> (stab, [outputs])."""
    import torch
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), **cfg)
    outs = []
    if how == "frames":
        cw, ch = stab.out_size
        ring = [torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda) for _ in range(3)]
        while True:
            n = stab.pull_frames_into(ring, len(outs), 3)
            outs += [ring[(len(outs) + i) % 3].cpu().numpy() for i in range(n)]
            if n < 3:
                break
    else:
        while True:
            o = stab.pull_nv12(planar=True) if how == "planar" else stab.pull()
            if o is None:
                break
            outs.append(tuple(x.cpu().numpy() for x in o) if how == "planar" else o.cpu().numpy())
    return stab, outs


@pytest.mark.parametrize("tracking", [1, 0])
def test_pipeline_lanczos4_pulls(vs, cuda, clip, tracking):
    """BGR, ring and plane-wise pulls: rotations are the bilinear handle's, every frame the Lanczos warp."""
    K, Ko, cw, ch, frames = clip
    ref, _ = stab_pulls(vs, cuda, frames, "pull", smooth_radius=2, tracking=tracking, map_precision=expect.IEEE)
    for how in ("pull", "frames", "planar"):
        stab, outs = stab_pulls(vs, cuda, frames, how, smooth_radius=2, tracking=tracking, map_precision=expect.IEEE, resample=vs.RESAMPLE_LANCZOS4)
        assert len(outs) == len(frames) - 1
        rots = [stab.warp_rotation(i) for i in range(len(outs))]
        for i, R in enumerate(rots):
            assert np.array_equal(R, ref.warp_rotation(i)), (how, i)
        expect_lz(frames, K, Ko, list(zip(outs, rots)), "planar" if how == "planar" else "bgr", (how, tracking))
        stab.close()
    ref.close()


def test_pipeline_lanczos4_default_precision_and_lens_mode(vs, cuda, clip):
    K, Ko, cw, ch, frames = clip
    if oracle.ref_gfx950_available():
        stab, outs = stab_pulls(vs, cuda, frames[:5], "pull", smooth_radius=2, tracking=0, resample=vs.RESAMPLE_LANCZOS4)
        expect_lz(frames, K, Ko, [(o, stab.warp_rotation(i)) for i, o in enumerate(outs)], "bgr", "default precision", mode=5)
        stab.close()
    cfg = dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=480, out_height=270, smooth_radius=2)
    for how in ("pull", "planar"):
        stab, outs = stab_pulls(vs, cuda, frames[:5], how, resample=vs.RESAMPLE_LANCZOS4, **cfg)
        Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, 480, 270)
        for i, o in enumerate(outs):
            p = oracle.map_params(stab.K_in, Kout, stab.warp_rotation(i))
            if how == "pull":
                eq(o, wd.bgr(frames[i + 1], *wd.maps(p, 480, 270, oracle.MAP_FISH_TO_RECT), "lanczos4"), ("lens", i))
            else:
                ey, euv = wd.planar(frames[i + 1], *wd.maps(p, 480, 270, oracle.MAP_FISH_TO_RECT), "lanczos4")
                eq(o[0], ey, ("lens y", i)), eq(o[1], euv, ("lens uv", i))
        stab.close()


@pytest.mark.parametrize("mem,hold,name", [(0, 1 << 29, "decoder"), (0, 0, "decoder"), (1, 0, "uv_wider"), (0, 0, "chroma_first")])
def test_pipeline_lanczos4_decoder_style_frames(vs, cuda, clip, mem, hold, name):
    """Borrowed (hold large), copied (hold 0) and host-memory frames with decoder-style planes: the BGR and plane-wise pulls."""
    K, Ko, cw, ch, frames = clip
    srcs = [layouts.place(f[:H], f[H:], name, cuda, host=mem == 1) for f in frames]
    for pulls in ("bgr", "planar"):
        outs = run_pipeline(vs, cuda, srcs, mem, hold, pulls, resample=vs.RESAMPLE_LANCZOS4, map_precision=expect.IEEE)
        expect_lz(frames, K, Ko, outs, pulls, (name, mem, hold, pulls))


def test_pipeline_lanczos4_host_and_peek_pulls(vs, cuda, clip):
    """vstab_pull_frame_host and vstab_peek_frame alternate on one Lanczos handle."""
    import torch
    K, Ko, cw, ch, frames = clip
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), smooth_radius=2, resample=vs.RESAMPLE_LANCZOS4,
                         map_precision=expect.IEEE)
    outs, kinds = [], []
    while True:
        if len(outs) % 2:
            o = layouts.Plane(ch, 3 * cw, cuda)
            st = vs.lib.vstab_peek_frame(stab._h, o.ptr, o.pitch)
            if st == vs.EOF:
                break
            assert st == vs.OK, vs.lib.vstab_last_error()
            outs.append(o.host(shape=(ch, cw, 3)))
            kinds.append("peek")
        else:
            o = stab.pull_host()
            if o is None:
                break
            outs.append(o)
            kinds.append("host")
    rots = [stab.warp_rotation(i) for i in range(len(outs))]
    stab.close()
    assert len(outs) == len(frames) - 1 and "peek" in kinds and "host" in kinds
    expect_lz(frames, K, Ko, list(zip(outs, rots)), "bgr", "host / peek")


def test_pipeline_lanczos4_dmabuf_frames(vs, cuda, clip):
    """DMA-BUF frames used in place (hold forever) and copied (hold 0): the BGR and plane-wise pulls."""
    from test_pipeline_gpu import _DmaBufPool
    K, Ko, cw, ch, frames = clip
    n = len(frames)
    pool = _DmaBufPool(frames)
    try:
        for hold in (1 << 29, 0):
            for pulls in ("bgr", "planar"):
                state = {"i": 0}

                def fill(out, advance):
                    i = state["i"]
                    if i >= n:
                        return vs.EOF
                    o = out.contents
                    o.mem, o.dmabuf_fd, o.dmabuf_size, o.dmabuf_modifier = 2, pool.fds[i], pool.size, 0
                    o.y, o.uv, o.pitch_y, o.pitch_uv = 64, 64 + W * H, W, W
                    o.width, o.height, o.pts, o.hold, o.bit_depth = W, H, i, hold, 8
                    if advance:
                        state["i"] += 1
                    return 0
                outs = drive(vs, cuda, fill, pulls, resample=vs.RESAMPLE_LANCZOS4, map_precision=expect.IEEE)
                assert len(outs) == n - 1
                expect_lz(frames, K, Ko, outs, pulls, ("dmabuf", hold, pulls))
    finally:
        pool.close()


def test_pipeline_lanczos4_repeated_parameters(vs, cuda, clip):
    """Smoother FIXED and tracking off: the parameters repeat, the state in which a bilinear handle serves its warps from the cached
    quantised map.  The Lanczos handle evaluates its own map: every frame is the Lanczos warp."""
    import torch
    K, Ko, cw, ch, frames = clip
    cfg = dict(smooth_radius=2, tracking=0, smoother=vs.SMOOTHER_FIXED, map_precision=expect.IEEE)
    dev = [torch.from_numpy(f).to(cuda) for f in frames]
    for pulls in ("bgr", "planar"):
        lz = vs.Stabilizer(dev, total=len(frames), resample=vs.RESAMPLE_LANCZOS4, **cfg)
        n = 0
        while True:
            b = lz.pull() if pulls == "bgr" else lz.pull_nv12(planar=True)
            if b is None:
                break
            R = lz.warp_rotation(n)
            assert np.array_equal(R, lz.warp_rotation(0)), n
            o = b.cpu().numpy() if pulls == "bgr" else tuple(x.cpu().numpy() for x in b)
            expect_lz([frames[(n + 1) % len(frames)]] * 2, K, Ko, [(o, R)], pulls, ("repeated", n))
            n += 1
        assert n == len(frames) - 1
        lz.close()


def test_pipeline_lanczos4_refusals_keep_the_handle_serving(vs, cuda, clip):
    """NV12 through BGR is refused before a frame is taken; a frame with a read-out rotation is refused and consumed.  Either way the
    handle goes on serving every remaining frame, each the Lanczos warp."""
    import torch
    K, Ko, cw, ch, frames = clip
    fr = [torch.from_numpy(f).to(cuda) for f in frames[:6]]
    stab = vs.Stabilizer(fr, total=6, smooth_radius=1, resample=vs.RESAMPLE_LANCZOS4, map_precision=expect.IEEE)
    with pytest.raises(vs.VstabError, match="RESAMPLE_LANCZOS4"):
        stab.pull_nv12(planar=False)
    outs = []
    while True:
        o = stab.pull()
        if o is None:
            break
        outs.append(o.cpu().numpy())
    assert len(outs) == 5                       # no frame lost to the refusal
    expect_lz(frames, K, Ko, [(o, stab.warp_rotation(i)) for i, o in enumerate(outs)], "bgr", "after NV12 refusal")
    stab.close()
    # one frame of six carries a read-out rotation: its pull is refused (and the frame consumed), every other frame is served
    srcs = [layouts.place(f[:H], f[H:], "packed", cuda) for f in frames[:6]]
    ro = np.ascontiguousarray(oracle.rodrigues((0.0, 0.0, 0.001)), np.float64).reshape(9)
    ro_p = ro.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    state = {"i": 0}

    def fill(out, advance):
        k = state["i"]
        if k >= len(srcs):
            return vs.EOF
        s, o = srcs[k], out.contents
        o.y, o.uv, o.pitch_y, o.pitch_uv, o.width, o.height = s.y, s.uv, s.pitch_y, s.pitch_uv, s.w, s.h
        o.mem, o.pts, o.hold, o.bit_depth = 0, k, 1 << 29, 8
        o.readout_rotation = ro_p if k == 3 else None
        if advance:
            state["i"] += 1
        return 0
    pull, peek = vs.PULL_FN(lambda u, o: fill(o, True)), vs.PULL_FN(lambda u, o: fill(o, False))
    src = vs.Source(pull, peek, None)
    cfg = vs.default_config(smooth_radius=1, seed=7, resample=vs.RESAMPLE_LANCZOS4, map_precision=expect.IEEE)
    h = ctypes.c_void_p()
    assert vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(src), ctypes.byref(h)) == vs.OK, vs.lib.vstab_last_error()
    got, refused = {}, []
    try:
        for k in range(16):
            o = layouts.Plane(ch, 3 * cw, cuda)
            st = vs.lib.vstab_pull_frame(h, o.ptr, o.pitch)
            if st == vs.EOF:
                break
            if st == vs.ERR_INVALID:
                assert b"read-out" in vs.lib.vstab_last_error()
                assert bool((o.buf == layouts.CANARY).all())   # nothing written for the refused frame
                refused.append(k)
                continue
            assert st == vs.OK, vs.lib.vstab_last_error()
            R = np.zeros(9)
            assert vs.lib.vstab_get_warp_rotation(h, k, vs._dptr(R)) == vs.OK
            got[k] = (o.host(shape=(ch, cw, 3)), R.reshape(3, 3))
    finally:
        vs.lib.vstab_destroy(h)
    assert refused == [2] and sorted(got) == [0, 1, 3, 4], (refused, sorted(got))
    for k, (o, R) in got.items():
        eq(o, wd.bgr(frames[k + 1], *wd.maps(oracle.map_params(K, Ko, R), cw, ch, 0), "lanczos4"), ("after read-out refusal", k))
    for bad in (dict(pixel_depth=10), dict(interpolation=0)):
        with pytest.raises(vs.VstabError):
            vs.Stabilizer(fr, total=6, smooth_radius=1, **dict(dict(resample=vs.RESAMPLE_LANCZOS4), **bad))
    with pytest.raises(vs.VstabError):
        vs.Stabilizer(fr, total=6, smooth_radius=1, interpolation=4)
