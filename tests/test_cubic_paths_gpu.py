"""Every path of the bicubic kernels (vstab_warp_cubic.hip) against the numpy definition (tests/warp_def.py), byte for byte, with
canary bands above, below and right of every output plane (tests/layouts.py):
  - the tile sets of tests/warp_tiles.py (TILE_SETS["cubic"]; tests/test_cubic_tiles_cpu.py), whose model proves the luma / chroma / BGR
    tiles they gather, stage at exactly the LDS budget and one element over it, both output formats;
  - the seven plane layouts of the layout matrix;
  - source and output planes whose row offsets pass 2^32 bytes;
  - the pipeline's cubic pulls: decoder-style, host-memory and DMA-BUF frames, the host and peek pulls, repeated parameters;
  - the stateless remap with pitched map planes, an odd source address and pitch, and the int16 saturation edges."""
import ctypes

import numpy as np
import pytest

import expect
import layouts
import oracle
import synth
import warp_def as wd
import warp_tiles as wt
from test_layouts_gpu import PITCH_UV_4G, run_pipeline

pytestmark = pytest.mark.gpu

ROT = (0.02, -0.03, 0.01)


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


def check_cubic(vs, cuda, s, f, p, dw, dh, mode, what, out_bgr=None, out_planar=None):
    """BGR and plane-wise cubic warps of Src s (packed NV12 f on the host) against the definition."""
    eq(layouts.warp_nv12_cubic(vs, s, p, dw, dh, mode, vs.OUT_BGR8, cuda, out_bgr), wd.bgr(f, *wd.maps(p, dw, dh, mode), "cubic"), (what, "bgr", mode))
    gy, guv = layouts.warp_nv12_cubic(vs, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, cuda, out_planar)
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, mode), "cubic")
    eq(gy, ey, (what, "luma", mode)), eq(guv, euv, (what, "chroma", mode))


# ---- the tile sets: staged, gathered, at the budget and over it -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wt.TILE_SETS["cubic"]))
def test_cubic_tile_sets(vs, cuda, name):
    p, sw, sh, dw, dh, mode = wt.set_params("cubic", name)
    f = synth.nv12(sum(map(ord, name)), sw, sh, full_range=True)
    s = layouts.place(f[:sh], f[sh:], "packed", cuda)
    for m in modes_of(mode):
        check_cubic(vs, cuda, s, f, p, dw, dh, m, name)


# ---- the layout matrix -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["camera", "all_states"])
@pytest.mark.parametrize("name", layouts.LAYOUTS)
def test_cubic_every_layout(vs, cuda, name, cam):
    """A normal camera (every tile staged) and the set with no-box, staged and gathered tiles on every plane, in every layout;
    mode 0 and the reference kernel's map."""
    if cam == "camera":
        w, h = 640, 360
        p, dw, dh, _, _ = cams(w, h)
        mode = 0
    else:
        p, w, h, dw, dh, mode = wt.set_params("cubic", cam)
    f = synth.nv12(21, w, h)
    s = layouts.place(f[:h], f[h:], name, cuda)
    for m in modes_of(mode):
        check_cubic(vs, cuda, s, f, p, dw, dh, m, (name, cam))


def test_cubic_plane_alignment_refusals(vs, cuda):
    """Chroma is read as 2-byte pairs: a chroma plane at an odd address or with an odd pitch is refused (ERR_INVALID, nothing
    written); a luma plane at an odd address with an odd pitch is read byte by byte."""
    w, h = 320, 180
    f = synth.nv12(22, w, h)
    p, dw, dh, _, _ = cams(w, h)
    for spec in ((w, w, "two", 0, 1), (w, w + 1, "two", 0, 0)):
        s = layouts.place(f[:h], f[h:], None, cuda, spec=spec)
        for fmt in (vs.OUT_BGR8, vs.OUT_NV12_PLANAR):
            o = layouts.Plane(dh, 3 * dw, cuda), layouts.out_nv12(dw, dh, cuda)
            with pytest.raises(vs.VstabError) as e:
                layouts.warp_nv12_cubic(vs, s, p, dw, dh, 0, fmt, cuda, o[0] if fmt == vs.OUT_BGR8 else o[1])
            assert e.value.status == vs.ERR_INVALID, spec
            for plane in (o[0], o[1][0], o[1][1]):                          # nothing written, inside the planes or around them
                assert bool((plane.buf == layouts.CANARY).all()), spec
    s = layouts.place(f[:h], f[h:], None, cuda, spec=(w + 1, w + 2, "two", 1, 2))
    check_cubic(vs, cuda, s, f, p, dw, dh, 0, "odd luma")


# ---- planes past 4 GiB -----------------------------------------------------------------------------------------------------------
W4, H4 = 640, 540


def frames_4g():
    """The 640 x 540 frame of test_chroma_plane_past_4_gib (chroma differs row by row) and its two parameter sets: the preset
    camera (every tile staged) and the tile set gather_540 (no-box, staged and gathered tiles on every plane)
    -> f, [(params, dw, dh, label)], K, Ko."""
    f = synth.nv12(17, W4, H4)
    rows = np.arange(H4 // 2, dtype=np.uint16)[:, None]
    f[H4:] = ((f[H4:].astype(np.uint16) + 37 * rows) % 256).astype(np.uint8)
    p, dw, dh, K, Ko = cams(W4, H4)
    pg, sw, sh, gw, gh, _ = wt.set_params("cubic", "gather_540")
    assert (sw, sh) == (W4, H4)
    return f, [(p, dw, dh, "staged"), (pg, gw, gh, "gathered")], K, Ko


def _release():
    """Give a large buffer back to the device before the next one is allocated (the caller has dropped its references)."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _pipeline_4g(vs, cuda, s, f, K, Ko, what):
    """The pipeline with resample = CUBIC on a frame with planes past 4 GiB: borrowed (hold large) and copied (hold 0)."""
    for hold in (1 << 29, 0):
        for pulls in ("bgr", "planar"):
            outs = run_pipeline(vs, cuda, [s] * 5, mem=0, hold=hold, pulls=pulls, resample=vs.RESAMPLE_CUBIC, map_precision=expect.IEEE)
            for i, (o, R) in enumerate(outs):
                p = oracle.map_params(K, Ko, R)
                ch, cw = (o.shape[:2] if pulls == "bgr" else o[0].shape)
                if pulls == "bgr":
                    eq(o, wd.bgr(f, *wd.maps(p, cw, ch, 0), "cubic"), (what, "pipeline", hold, i))
                else:
                    ey, euv = wd.planar(f, *wd.maps(p, cw, ch, 0), "cubic")
                    eq(o[0], ey, (what, "pipeline y", hold, i)), eq(o[1], euv, (what, "pipeline uv", hold, i))


def test_cubic_chroma_plane_past_4_gib(vs, cuda):
    f, sets, K, Ko = frames_4g()
    assert PITCH_UV_4G * (H4 // 2 - 1) >= 1 << 32
    s = layouts.place(f[:H4], f[H4:], None, cuda, spec=(W4, PITCH_UV_4G, "one", 0, W4 * H4))
    try:
        for p, dw, dh, label in sets:
            check_cubic(vs, cuda, s, f, p, dw, dh, 0, ("chroma 4g", label))
        _pipeline_4g(vs, cuda, s, f, K, Ko, "chroma 4g")
    finally:
        del s
        _release()


PITCH_Y_4G = 8000000   # a multiple of 16: 540 luma rows span 4.32 GB, rows from 537 on start beyond 2^32


def test_cubic_luma_plane_past_4_gib(vs, cuda):
    f, sets, K, Ko = frames_4g()
    assert PITCH_Y_4G * (H4 - 1) >= 1 << 32 and PITCH_Y_4G * H4 < 1 << 33
    s = layouts.place(f[:H4], f[H4:], None, cuda, spec=(PITCH_Y_4G, W4, "two", 0, 0))
    try:
        for p, dw, dh, label in sets:
            check_cubic(vs, cuda, s, f, p, dw, dh, 0, ("luma 4g", label))
        _pipeline_4g(vs, cuda, s, f, K, Ko, "luma 4g")
    finally:
        del s
        _release()


def _plane_past_4g(rows, rb, cuda):
    """An output Plane whose last row starts past 2^32 bytes (one ~4.3 GB buffer)."""
    pitch = layouts._al((1 << 32) // (rows - 1) + 1, 16)
    o = layouts.Plane(rows, rb, cuda, pad=pitch - layouts._al(rb, 16))
    assert o.pitch * (rows - 1) >= 1 << 32
    return o


@pytest.mark.parametrize("plane", ["bgr", "luma", "chroma"])
def test_cubic_output_plane_past_4_gib(vs, cuda, plane):
    """pitch_dst of the BGR output, and the plane-wise luma pitch_dst / chroma pitch_dst_uv, with rows past 2^32 bytes: one large
    plane at a time, the other plane of the pair of normal size."""
    f, sets, _, _ = frames_4g()
    s = layouts.place(f[:H4], f[H4:], "packed", cuda)
    for p, dw, dh, label in sets:
        cw2, ch2 = 2 * ((dw + 1) // 2), (dh + 1) // 2
        if plane == "bgr":
            o = _plane_past_4g(dh, 3 * dw, cuda)
            eq(layouts.warp_nv12_cubic(vs, s, p, dw, dh, 0, vs.OUT_BGR8, cuda, o), wd.bgr(f, *wd.maps(p, dw, dh, 0), "cubic"), (plane, label))
        else:
            o = (_plane_past_4g(dh, dw, cuda), layouts.Plane(ch2, cw2, cuda)) if plane == "luma" else \
                (layouts.Plane(dh, dw, cuda), _plane_past_4g(ch2, cw2, cuda))
            gy, guv = layouts.warp_nv12_cubic(vs, s, p, dw, dh, 0, vs.OUT_NV12_PLANAR, cuda, o)
            ey, euv = wd.planar(f, *wd.maps(p, dw, dh, 0), "cubic")
            eq(gy, ey, (plane, label, "luma")), eq(guv, euv, (plane, label, "chroma"))
        del o
        _release()


# ---- the pipeline's cubic pulls ----------------------------------------------------------------------------------------------------
W, H = 640, 360


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = synth.shaky_clip(3, K, W, H, 8, sigma=0.004)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    return K, Ko, cw, ch, frames


def expect_cubic(frames, K, Ko, outs, pulls, what):
    for i, (o, R) in enumerate(outs):
        p = oracle.map_params(K, Ko, R)
        if pulls == "bgr":
            ch, cw = o.shape[:2]
            eq(o, wd.bgr(frames[i + 1], *wd.maps(p, cw, ch, 0), "cubic"), (what, i))
        else:
            ch, cw = o[0].shape
            ey, euv = wd.planar(frames[i + 1], *wd.maps(p, cw, ch, 0), "cubic")
            eq(o[0], ey, (what, "y", i)), eq(o[1], euv, (what, "uv", i))


@pytest.mark.parametrize("mem,hold,name", [(0, 1 << 29, "decoder"), (0, 0, "decoder"), (1, 0, "uv_wider"), (0, 1 << 29, "uv_narrower"),
                                           (0, 0, "chroma_first")])
def test_pipeline_cubic_decoder_style_frames(vs, cuda, clip, mem, hold, name):
    """Borrowed (hold large), copied (hold 0) and host-memory frames with decoder-style planes: the cubic BGR and plane-wise pulls."""
    K, Ko, cw, ch, frames = clip
    srcs = [layouts.place(f[:H], f[H:], name, cuda, host=mem == 1) for f in frames]
    for pulls in ("bgr", "planar"):
        outs = run_pipeline(vs, cuda, srcs, mem, hold, pulls, resample=vs.RESAMPLE_CUBIC, map_precision=expect.IEEE)
        expect_cubic(frames, K, Ko, outs, pulls, (name, mem, hold, pulls))


def test_pipeline_cubic_host_and_peek_pulls(vs, cuda, clip):
    """vstab_pull_frame_host and vstab_peek_frame (destructive, as in the reference) alternate on one cubic handle."""
    import torch
    K, Ko, cw, ch, frames = clip
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), smooth_radius=2, resample=vs.RESAMPLE_CUBIC,
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
    stab_rots = [stab.warp_rotation(i) for i in range(len(outs))]
    stab.close()
    assert len(outs) == len(frames) - 1 and "peek" in kinds and "host" in kinds
    expect_cubic(frames, K, Ko, list(zip(outs, stab_rots)), "bgr", "host / peek")


def test_pipeline_cubic_dmabuf_frames(vs, cuda, clip):
    """DMA-BUF frames (test_pipeline_gpu._DmaBufPool: device buffers exported as fds, planes at byte offset 64), used in place
    (hold forever) and copied (hold 0): the cubic BGR and plane-wise pulls are the warp of each frame."""
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
                outs = drive(vs, cuda, fill, pulls, resample=vs.RESAMPLE_CUBIC, map_precision=expect.IEEE)
                assert len(outs) == n - 1
                expect_cubic(frames, K, Ko, outs, pulls, ("dmabuf", hold, pulls))
    finally:
        pool.close()


def drive(vs, cuda, fill, pulls, **cfg_kw):
    """A handle over a vstab_source whose callbacks are fill(out, advance) -> [(output, warp rotation)] per emitted frame."""
    import torch
    pull, peek = vs.PULL_FN(lambda u, o: fill(o, True)), vs.PULL_FN(lambda u, o: fill(o, False))
    src = vs.Source(pull, peek, None)
    cfg = vs.default_config(smooth_radius=2, seed=7, **cfg_kw)
    h = ctypes.c_void_p()
    assert vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(src), ctypes.byref(h)) == vs.OK, vs.lib.vstab_last_error()
    ow, oh = ctypes.c_int(), ctypes.c_int()
    assert vs.lib.vstab_get_output_info(h, ctypes.byref(ow), ctypes.byref(oh), None, None) == vs.OK
    cw, ch = ow.value, oh.value
    outs = []
    try:
        while True:
            if pulls == "bgr":
                o = layouts.Plane(ch, 3 * cw, cuda)
                st = vs.lib.vstab_pull_frame(h, o.ptr, o.pitch)
                get = lambda: o.host(shape=(ch, cw, 3))
            else:
                oy, ou = layouts.out_nv12(cw, ch, cuda)
                st = vs.lib.vstab_pull_frame_nv12_planar(h, oy.ptr, oy.pitch, ou.ptr, ou.pitch)
                get = lambda: (oy.host(), ou.host())
            if st == vs.EOF:
                break
            assert st == vs.OK, vs.lib.vstab_last_error()
            R = np.zeros(9)
            assert vs.lib.vstab_get_warp_rotation(h, len(outs), vs._dptr(R)) == vs.OK
            outs.append((get(), R.reshape(3, 3)))
            torch.cuda.synchronize()
    finally:
        vs.lib.vstab_destroy(h)
    return outs


def test_pipeline_cubic_repeated_parameters(vs, cuda, clip):
    """smoother FIXED and tracking off: every frame is warped with the same 17 parameters, the state in which a bilinear handle
    serves its warps from the cached quantised map.  The cubic handle evaluates its own map: every frame is the cubic warp, and
    differs from the bilinear warp the cache would give."""
    import torch
    K, Ko, cw, ch, frames = clip
    cfg = dict(smooth_radius=2, tracking=0, smoother=vs.SMOOTHER_FIXED, map_precision=expect.IEEE)
    dev = [torch.from_numpy(f).to(cuda) for f in frames]
    lin = vs.Stabilizer(dev, total=len(frames), **cfg)
    cub = vs.Stabilizer(dev, total=len(frames), resample=vs.RESAMPLE_CUBIC, **cfg)
    for pulls in ("bgr", "planar"):
        n = 0
        while True:
            a = lin.pull() if pulls == "bgr" else lin.pull_nv12(planar=True)
            b = cub.pull() if pulls == "bgr" else cub.pull_nv12(planar=True)
            if a is None or b is None:
                assert a is None and b is None
                break
            i = n
            R = cub.warp_rotation(i)
            assert np.array_equal(R, lin.warp_rotation(i)) and np.array_equal(R, cub.warp_rotation(0)), i   # the same parameters, frame after frame
            p = oracle.map_params(K, Ko, R)
            f = frames[(i + 1) % len(frames)]
            if pulls == "bgr":
                a, b = a.cpu().numpy(), b.cpu().numpy()
                eq(a, expect.warp(f, p, cw, ch, expect.IEEE), ("bilinear", i))
                eq(b, wd.bgr(f, *wd.maps(p, cw, ch, 0), "cubic"), ("cubic", i))
                assert not np.array_equal(a, b), i
            else:
                ly, luv = expect.warp_planar(f, p, cw, ch, expect.IEEE)
                eq(a[0].cpu().numpy(), ly, ("bilinear y", i)), eq(a[1].cpu().numpy(), luv, ("bilinear uv", i))
                ey, euv = wd.planar(f, *wd.maps(p, cw, ch, 0), "cubic")
                eq(b[0].cpu().numpy(), ey, ("cubic y", i)), eq(b[1].cpu().numpy(), euv, ("cubic uv", i))
                assert not np.array_equal(ly, ey), i
            n += 1
        if pulls == "bgr":
            lin.close(), cub.close()
            lin = vs.Stabilizer(dev, total=len(frames), **cfg)
            cub = vs.Stabilizer(dev, total=len(frames), resample=vs.RESAMPLE_CUBIC, **cfg)
    lin.close(), cub.close()


# ---- the stateless remap's edges -----------------------------------------------------------------------------------------------------
def remap_c(vs, cuda, src_t, pitch_src, sw, sh, cn, mx_t, my_t, border, dw, dh):
    """vstab_remap_cubic through the C ABI, map planes as (possibly wider) float tensors with their own pitches, the output a
    canaried Plane -> (dh, dw[, cn]) uint8."""
    o = layouts.Plane(dh, dw * cn, cuda)
    b = (ctypes.c_int * 3)(*(list(border) + [0, 0, 0])[:3])
    st = vs.lib.vstab_remap_cubic(src_t, pitch_src, sw, sh, cn, mx_t.data_ptr(), mx_t.stride(0) * 4, my_t.data_ptr(), my_t.stride(0) * 4, b, o.ptr,
                                  o.pitch, dw, dh, vs._stream())
    if st != vs.OK:
        raise vs.VstabError(st, "vstab_remap_cubic")
    return o.host(shape=(dh, dw, cn) if cn > 1 else (dh, dw))


def odd_source(src, cuda):
    """src (h, w[, cn]) uint8 placed at an odd address with an odd pitch in a FILL-patterned buffer -> (pointer, pitch, buffer)."""
    import torch
    h, w = src.shape[:2]
    rb = src[0].size
    pitch = rb + (3 if rb % 2 == 0 else 2)
    buf = torch.full((h * pitch + 64,), layouts.FILL, dtype=torch.uint8, device=cuda)
    torch.as_strided(buf, (h, rb), (pitch, 1), 1).copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(h, rb)))
    assert (buf.data_ptr() + 1) % 2 == 1 and pitch % 2 == 1
    return buf.data_ptr() + 1, pitch, buf


def pitched_map(m, extra, cuda):
    """A (dh, dw) float32 map as the left columns of a wider NaN-filled tensor."""
    import torch
    dh, dw = m.shape
    big = torch.full((dh, dw + extra), float("nan"), dtype=torch.float32, device=cuda)
    big[:, :dw] = torch.from_numpy(m)
    return big[:, :dw]


def test_remap_cubic_pitched_maps_odd_source_canaried_outputs(vs, cuda):
    """Map planes with pitches of their own (x and y differ), a source at an odd address with an odd pitch, 1, 2 and 3 channels."""
    from test_cubic_gpu import special_maps
    rng = np.random.default_rng(23)
    sw, sh, dw, dh = 203, 97, 131, 75
    for cn, border in ((1, (16,)), (2, (128, 128)), (3, (0, 9, 255))):
        src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
        mx, my = special_maps(rng, sw, sh, dw, dh)
        ptr, pitch, keep = odd_source(src, cuda)
        mxt, myt = pitched_map(mx, 5, cuda), pitched_map(my, 17, cuda)
        assert mxt.stride(0) != myt.stride(0)
        got = remap_c(vs, cuda, ptr, pitch, sw, sh, cn, mxt, myt, border, dw, dh)
        eq(got, wd.remap(src, mx, my, "cubic", wd.CONSTANT, border), ("remap", cn))
        del keep


def test_remap_cubic_int16_saturation_edges(vs, cuda):
    """A 32767 x 2 source: map x of 32766.5, 32767.99 and 1e6 saturate X to 32767 (or stop just short of it), whose footprint still
    holds column 32766.  The same for y on a 2 x 32767 source."""
    import torch
    rng = np.random.default_rng(24)
    xs = np.array([32766.5, 32767.99, 1e6, 32765.3, 32766.0, 32767.0], np.float32)
    ys = np.array([0.0, 0.5, 1.0, 1.7], np.float32)
    for cn, border in ((1, (16,)), (3, (1, 2, 3))):
        for tall in (False, True):
            sw, sh = (2, 32767) if tall else (32767, 2)
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            a, b = np.meshgrid(xs, ys)                    # (len(ys), len(xs))
            mx, my = (b, a) if tall else (a, b)
            mx, my = np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)
            dh, dw = mx.shape
            st = torch.from_numpy(src).to(cuda)
            got = remap_c(vs, cuda, st.data_ptr(), st.stride(0), sw, sh, cn, pitched_map(mx, 3, cuda), pitched_map(my, 0, cuda), border, dw, dh)
            exp = wd.remap(src, mx, my, "cubic", wd.CONSTANT, border)
            eq(got, exp, ("saturation", cn, tall))
            X, Y, _ = wd.quantise(mx, my)
            assert ((Y if tall else X) == 32767).sum() >= 2 * len(ys)   # the saturated taps are there, and inside the source (column / row 32766)
            ins = exp != (np.array(border[:cn], np.uint8) if cn > 1 else border[0])
            assert ins.any()


def test_cubic_sizes_of_32768_are_refused(vs, cuda):
    import torch
    src = torch.zeros((64, 64), dtype=torch.uint8, device=cuda)
    m = torch.zeros((4, 4), dtype=torch.float32, device=cuda)
    b = (ctypes.c_int * 3)(0, 0, 0)
    o = torch.zeros((4, 4), dtype=torch.uint8, device=cuda)
    for sw, sh, dw, dh in ((32768, 2, 4, 4), (2, 32768, 4, 4), (2, 2, 32768, 4), (2, 2, 4, 32768)):
        st = vs.lib.vstab_remap_cubic(src.data_ptr(), 1 << 16, sw, sh, 1, m.data_ptr(), 1 << 17, m.data_ptr(), 1 << 17, b, o.data_ptr(), 1 << 16,
                                      dw, dh, vs._stream())
        assert st == vs.ERR_INVALID, (sw, sh, dw, dh)
    p = np.ascontiguousarray(cams(640, 360)[0], np.float32)
    fp = p.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for sw, sh, dw, dh in ((32768, 2, 4, 4), (2, 32768, 4, 4), (2, 2, 32768, 4), (2, 2, 4, 32768)):
        for fmt in (vs.OUT_BGR8, vs.OUT_NV12_PLANAR):
            st = vs.lib.vstab_warp_nv12_cubic(src.data_ptr(), 1 << 16, src.data_ptr(), 1 << 16, sw, sh, fp, 0, fmt, o.data_ptr(), 1 << 18,
                                              o.data_ptr(), 1 << 18, dw, dh, vs._stream())
            assert st == vs.ERR_INVALID, (sw, sh, dw, dh, fmt)
    torch.cuda.synchronize()
    assert bool((o == 0).all())
