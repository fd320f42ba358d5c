"""Every NV12 / P010 entry point with the planes laid out as decoders lay them out (tests/layouts.py): chroma in its own allocation,
before luma, at an aligned-height offset, at a wider or narrower pitch than luma, unaligned; the tiled kernels' wide flat source boxes
(anamorphic output cameras: tests/test_tile_boxes_cpu.py proves the tile states they reach); chroma planes whose row offsets pass
2^32 bytes; and the pipeline fed such frames.  Bar: every byte / word equals the oracle on compact copies of the same planes, and no
byte outside an output plane changes."""
import ctypes

import numpy as np
import pytest

import expect
import layouts
import oracle
import synth
from test_p010_cpu import p010_frame
from test_tile_boxes_cpu import WIDE_SETS, anamorphic

pytestmark = pytest.mark.gpu

ROT = (0.02, -0.03, 0.01)


def cams(w, h, rvec=ROT):
    K = oracle.get_preset_camera(4, w, h)
    Ko, (dw, dh) = oracle.get_output_camera(K, w, h)
    return oracle.map_params(K, Ko, oracle.rodrigues(rvec)), dw, dh, K, Ko


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp).reshape(np.asarray(got).shape)
    assert np.array_equal(got, exp), (what, int((got != exp).sum()))


def need_ref():
    if not oracle.ref_gfx950_available():
        pytest.fail("oracle/_ref/createMap.gfx950.co is missing: __graft_entry__.build() compiles it where /root/reference exists")


def check_nv12(vs, cuda, s, f, p, dw, dh, rb, what, opencl=True):
    """Every 8-bit entry point on Src s (frame f, packed NV12 on the host) against the oracle."""
    L = layouts
    eq(L.warp_nv12(vs, s, p, dw, dh, 0, vs.OUT_BGR8, cuda), oracle.warp_nv12_ex(f, p, dw, dh, 0, 0), (what, "bgr"))
    gy, guv = L.warp_nv12(vs, s, p, dw, dh, 1, vs.OUT_NV12, cuda)
    ey, euv = oracle.warp_nv12_ex(f, p, dw, dh, 1, 1)
    eq(gy, ey, (what, "nv12 y")), eq(guv, euv, (what, "nv12 uv"))
    for mode in (0, 1):
        gy, guv = L.warp_nv12(vs, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, cuda)
        ey, euv = oracle.warp_nv12_planar(f, p, dw, dh, mode)
        eq(gy, ey, (what, "planar y", mode)), eq(guv, euv, (what, "planar uv", mode))
    eq(L.warp_nv12(vs, s, p, dw, dh, 0, vs.OUT_BGR8, cuda, rb), oracle.warp_nv12_rs(f, p, rb, dw, dh, 0, 0), (what, "rs bgr"))
    gy, guv = L.warp_nv12(vs, s, p, dw, dh, 1, vs.OUT_NV12_PLANAR, cuda, rb)
    ey, euv = oracle.warp_nv12_planar(f, p, dw, dh, 1, rb)
    eq(gy, ey, (what, "rs planar y")), eq(guv, euv, (what, "rs planar uv"))
    q = vs.quantised_map(p, dw, dh, 0)
    eq(L.warp_nv12_mapped(vs, s, q, dw, dh, vs.OUT_BGR8, cuda), oracle.warp_nv12_ex(f, p, dw, dh, 0, 0), (what, "mapped"))
    gy, guv = L.warp_nv12_mapped(vs, s, q, dw, dh, vs.OUT_NV12, cuda)
    ey, euv = oracle.warp_nv12_ex(f, p, dw, dh, 0, 1)
    eq(gy, ey, (what, "mapped nv12 y")), eq(guv, euv, (what, "mapped nv12 uv"))
    eq(L.warp_nv12_nearest(vs, s, p, dw, dh, 0, cuda), oracle.remap_nearest(oracle.cvt_nv12_bgr(f), *oracle.create_map(p, dw, dh)), (what, "nearest"))
    if opencl:   # the default arithmetic: the reference's createMap kernel on this GPU
        eq(L.warp_nv12(vs, s, p, dw, dh, vs.MAP_CREATEMAP_CL_OPENCL, vs.OUT_BGR8, cuda), expect.warp(f, p, dw, dh, expect.OPENCL), (what, "ocl bgr"))
        gy, guv = L.warp_nv12(vs, s, p, dw, dh, vs.MAP_CREATEMAP_CL_OPENCL, vs.OUT_NV12_PLANAR, cuda)
        ey, euv = expect.warp_planar(f, p, dw, dh, expect.OPENCL)
        eq(gy, ey, (what, "ocl planar y")), eq(guv, euv, (what, "ocl planar uv"))


def check_p010(vs, cuda, s, y, uv, p, dw, dh, rb, what, planes_ok=True, opencl=True):
    L = layouts
    for blend in (vs.BLEND_EXACT, vs.BLEND_FP16):
        for r in (None, rb):
            exp = oracle.warp_p010(y, uv, p, dw, dh, r, 0, blend)
            eq(L.warp_p010(vs, s, p, dw, dh, 0, blend, cuda, r), exp, (what, "bgr16", blend, r is None))
            if planes_ok:
                gy, guv = L.warp_p010_planes(vs, s, p, dw, dh, 0, blend, cuda, r)
                ey, euv = oracle.cvt_bgr10_p010(exp)
                eq(gy, ey, (what, "planes y", blend)), eq(guv, euv, (what, "planes uv", blend))
            gy, guv = L.warp_p010_planes(vs, s, p, dw, dh, 1, blend, cuda, r, planar=True)
            ey, euv = oracle.warp_p010_planar(y, uv, p, dw, dh, 1, r, blend)
            eq(gy, ey, (what, "planar y", blend)), eq(guv, euv, (what, "planar uv", blend))
    if not planes_ok:
        with pytest.raises(vs.VstabError) as e:
            L.warp_p010_planes(vs, s, p, dw, dh, 0, 0, cuda)
        assert e.value.status == vs.ERR_UNSUPPORTED
    if opencl:
        for blend in (vs.BLEND_EXACT, vs.BLEND_FP16):
            eq(L.warp_p010(vs, s, p, dw, dh, vs.MAP_CREATEMAP_CL_OPENCL, blend, cuda), expect.warp_p010(y, uv, p, dw, dh, None, blend), (what, "ocl bgr16"))
            gy, guv = L.warp_p010_planes(vs, s, p, dw, dh, vs.MAP_CREATEMAP_CL_OPENCL, blend, cuda, planar=True)
            ey, euv = expect.warp_p010_planar(y, uv, p, dw, dh, None, blend)
            eq(gy, ey, (what, "ocl planar y")), eq(guv, euv, (what, "ocl planar uv"))


@pytest.mark.parametrize("name", layouts.LAYOUTS)
def test_nv12_every_entry_point_every_layout(vs, cuda, name):
    """64 x 16 tiles (a 583 x 331 output): BGR, NV12, plane-wise NV12, per row, quantised map, nearest, conversion and packing."""
    need_ref()
    w, h = 640, 360
    f = synth.nv12(11, w, h)
    p, dw, dh, K, Ko = cams(w, h)
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.05, -0.01, 0.02)))[8:]
    s = layouts.place(f[:h], f[h:], name, cuda)
    eq(layouts.cvt_nv12_bgr(vs, s, cuda), oracle.cvt_nv12_bgr(f), (name, "cvt"))
    eq(layouts.pack(vs, s, cuda), f, (name, "pack"))
    check_nv12(vs, cuda, s, f, p, dw, dh, rb, name)


@pytest.mark.parametrize("name", layouts.LAYOUTS)
def test_p010_every_entry_point_every_layout(vs, cuda, name):
    """BGR16, P010 planes and plane-wise P010, both blends, per row; the unaligned layout is refused by the planes output only."""
    need_ref()
    w, h = 640, 360
    y, uv, _, _ = p010_frame(12, w, h)
    p, dw, dh, K, Ko = cams(w, h)
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.05, -0.01, 0.02)))[8:]
    s = layouts.place(y, uv, name, cuda)
    eq(layouts.pack(vs, s, cuda, p010=True), oracle.pack_p010(y, uv), (name, "pack"))
    check_p010(vs, cuda, s, y, uv, p, dw, dh, rb, name, planes_ok=name != "unaligned")


@pytest.mark.parametrize("name", ["decoder", "uv_wider", "uv_narrower", "chroma_first"])
def test_large_outputs_take_the_tall_tiles_in_every_layout(vs, cuda, name):
    """A 2048 x 1536 output from 1920 x 1080: 1536 tiles of 64 x 32, the threshold of the 64 x 32-tile kernels (plane-wise and fused)."""
    w, h, dw, dh = 1920, 1080, 2048, 1536
    assert layouts.planar_launch(dw, dh, 8)[0] == 8
    K = oracle.get_preset_camera(4, w, h)
    Ko = np.array([[900.0, 0, dw / 2], [0, 900.0, dh / 2], [0, 0, 1]])
    p = oracle.map_params(K, Ko, oracle.rodrigues(ROT))
    f = synth.nv12(13, w, h)
    s = layouts.place(f[:h], f[h:], name, cuda)
    eq(layouts.warp_nv12(vs, s, p, dw, dh, 0, vs.OUT_BGR8, cuda), oracle.warp_nv12_ex(f, p, dw, dh, 0, 0), (name, "bgr"))
    gy, guv = layouts.warp_nv12(vs, s, p, dw, dh, 0, vs.OUT_NV12_PLANAR, cuda)
    ey, euv = oracle.warp_nv12_planar(f, p, dw, dh, 0)
    eq(gy, ey, (name, "planar y")), eq(guv, euv, (name, "planar uv"))
    y, uv, _, _ = p010_frame(14, w, h)
    s = layouts.place(y, uv, name, cuda)
    for blend in (0, 1):
        exp = oracle.warp_p010(y, uv, p, dw, dh, None, 0, blend)
        eq(layouts.warp_p010(vs, s, p, dw, dh, 0, blend, cuda), exp, (name, "bgr16", blend))
        gy, guv = layouts.warp_p010_planes(vs, s, p, dw, dh, 0, blend, cuda)
        ey, euv = oracle.cvt_bgr10_p010(exp)
        eq(gy, ey, (name, "planes y")), eq(guv, euv, (name, "planes uv"))
        gy, guv = layouts.warp_p010_planes(vs, s, p, dw, dh, 0, blend, cuda, planar=True)
        ey, euv = oracle.warp_p010_planar(y, uv, p, dw, dh, 0, None, blend)
        eq(gy, ey, (name, "planar y", blend)), eq(guv, euv, (name, "planar uv", blend))


@pytest.mark.parametrize("depth,dw,dh,sx,sy,rv,least", WIDE_SETS)
def test_wide_flat_source_boxes(vs, cuda, depth, dw, dh, sx, sy, rv, least):
    """Anamorphic output cameras whose tile boxes have rows of more than 64 16-byte chunks (and tiles wholly above / below the
    source): plane-wise NV12 or P010 with both blends and per row, and the same parameters through the fused kernels."""
    w, h = 1920, 1080
    p, K, Ko = anamorphic(sx, sy, rv, dw, dh)
    rb = oracle.map_params(K, Ko, oracle.rodrigues(np.asarray(rv) + np.array([0.01, -0.01, 0.005])))[8:]
    if depth == 8:
        f = synth.nv12(15, w, h)
        s = layouts.place(f[:h], f[h:], "decoder", cuda)
        for r in (None, rb):
            for mode in (0, 1):
                gy, guv = layouts.warp_nv12(vs, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, cuda, r)
                ey, euv = oracle.warp_nv12_planar(f, p, dw, dh, mode, r)
                eq(gy, ey, ("planar y", mode, r is None)), eq(guv, euv, ("planar uv", mode, r is None))
        eq(layouts.warp_nv12(vs, s, p, dw, dh, 0, vs.OUT_BGR8, cuda), oracle.warp_nv12_ex(f, p, dw, dh, 0, 0), "fused bgr")
        gy, guv = layouts.warp_nv12(vs, s, p, dw, dh, 0, vs.OUT_NV12, cuda)
        ey, euv = oracle.warp_nv12_ex(f, p, dw, dh, 0, 1)
        eq(gy, ey, "fused nv12 y"), eq(guv, euv, "fused nv12 uv")
    else:
        y, uv, _, _ = p010_frame(16, w, h)
        s = layouts.place(y, uv, "uv_wider", cuda)
        for blend in (0, 1):
            for r in (None, rb):
                gy, guv = layouts.warp_p010_planes(vs, s, p, dw, dh, 0, blend, cuda, r, planar=True)
                ey, euv = oracle.warp_p010_planar(y, uv, p, dw, dh, 0, r, blend)
                eq(gy, ey, ("planar y", blend, r is None)), eq(guv, euv, ("planar uv", blend, r is None))
            exp = oracle.warp_p010(y, uv, p, dw, dh, None, 0, blend)
            eq(layouts.warp_p010(vs, s, p, dw, dh, 0, blend, cuda), exp, ("fused bgr16", blend))
            gy, guv = layouts.warp_p010_planes(vs, s, p, dw, dh, 0, blend, cuda)
            ey, euv = oracle.cvt_bgr10_p010(exp)
            eq(gy, ey, ("fused planes y", blend)), eq(guv, euv, ("fused planes uv", blend))


# ---- chroma row offsets past 2^32 bytes ----------------------------------------------------------------------------------------------
PITCH_UV_4G = 16777200    # < 2^24, a multiple of 16: 270 chroma rows span 4.5 GB, rows from 257 on start beyond 2^32


def test_chroma_plane_past_4_gib(vs, cuda):
    """A 640 x 540 frame whose chroma pitch is just under 2^24: the staged loads' 32-bit chroma offsets would wrap for the bottom
    rows.  One 4.5 GB allocation (chroma behind a small luma plane), filled with a pattern first; chroma differs row by row."""
    import torch
    w, h = 640, 540
    f = synth.nv12(17, w, h)
    rows = np.arange(h // 2, dtype=np.uint16)[:, None]
    f[h:] = ((f[h:].astype(np.uint16) + 37 * rows) % 256).astype(np.uint8)   # chroma content differs row by row
    assert PITCH_UV_4G * (h // 2 - 1) >= 1 << 32 > PITCH_UV_4G * 256
    spec = (w, PITCH_UV_4G, "one", 0, w * h)
    p, dw, dh, K, Ko = cams(w, h)
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.05, -0.01, 0.02)))[8:]
    s = layouts.place(f[:h], f[h:], None, cuda, spec=spec)
    try:
        check_nv12(vs, cuda, s, f, p, dw, dh, rb, "4g", opencl=False)
        torch.cuda.synchronize()
        # the pipeline object borrowing such frames (hold large, device memory): what it emits is still the warp of the frame
        outs = run_pipeline(vs, cuda, [s] * 5, mem=0, hold=1 << 29, pulls="bgr")
        for i, (o, R) in enumerate(outs):
            eq(o, expect.warp(f, oracle.map_params(K, Ko, R), dw, dh), ("pipeline", i))
    finally:
        del s
        torch.cuda.empty_cache()
    # P010: luma 1280 bytes per row, the same chroma pitch
    y, uv, _, _ = p010_frame(18, w, h)
    uv = ((uv.astype(np.uint32) + (rows.astype(np.uint32) << 6)) & 0xffff).astype(np.uint16)
    s = layouts.place(y, uv, None, cuda, spec=(2 * w, PITCH_UV_4G, "one", 0, 2 * w * h))
    try:
        check_p010(vs, cuda, s, y, uv, p, dw, dh, rb, "4g", opencl=False)
        torch.cuda.synchronize()
    finally:
        del s
        torch.cuda.empty_cache()


# ---- the pipeline fed decoder-style frames ---------------------------------------------------------------------------------------
def run_pipeline(vs, cuda, srcs, mem, hold, pulls, bit_depth=0, **cfg_kw):
    """The pipeline object over raw vstab_source callbacks handing out the planes of `srcs` (layouts.Src) with the given mem / hold.
    -> [(output, warp rotation)] per emitted frame: pulls 'bgr' (8-bit BGR), 'planar' (NV12 plane-wise), 'p010_planar' / 'bgr16'."""
    import torch
    state = {"i": 0}

    def fill(out, advance):
        if state["i"] >= len(srcs):
            return vs.EOF
        s = srcs[state["i"]]
        o = out.contents
        o.y, o.uv, o.pitch_y, o.pitch_uv, o.width, o.height = s.y, s.uv, s.pitch_y, s.pitch_uv, s.w, s.h
        o.mem, o.pts, o.hold, o.bit_depth = mem, state["i"], hold, bit_depth
        if advance:
            state["i"] += 1
        return 0
    pull = vs.PULL_FN(lambda u, o: fill(o, True))
    peek = vs.PULL_FN(lambda u, o: fill(o, False))
    src = vs.Source(pull, peek, None)
    cfg = vs.default_config(smooth_radius=2, seed=7, **cfg_kw)
    h = ctypes.c_void_p()
    assert vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(src), ctypes.byref(h)) == vs.OK, vs.lib.vstab_last_error()
    ow, oh = ctypes.c_int(), ctypes.c_int()
    Ki, Ko = np.zeros(9), np.zeros(9)
    assert vs.lib.vstab_get_output_info(h, ctypes.byref(ow), ctypes.byref(oh), vs._dptr(Ki), vs._dptr(Ko)) == vs.OK
    cw, ch = ow.value, oh.value
    outs = []
    try:
        while True:
            if pulls == "bgr":
                o = layouts.Plane(ch, 3 * cw, cuda)
                st = vs.lib.vstab_pull_frame(h, o.ptr, o.pitch)
                get = lambda: o.host(shape=(ch, cw, 3))
            elif pulls == "bgr16":
                o = layouts.Plane(ch, 6 * cw, cuda)
                st = vs.lib.vstab_pull_frame_bgr16(h, o.ptr, o.pitch)
                get = lambda: o.host(np.uint16, (ch, cw, 3))
            elif pulls == "planar":
                oy, ou = layouts.out_nv12(cw, ch, cuda)
                st = vs.lib.vstab_pull_frame_nv12_planar(h, oy.ptr, oy.pitch, ou.ptr, ou.pitch)
                get = lambda: (oy.host(), ou.host())
            else:
                oy, ou = layouts.out_p010(cw, ch, cuda)
                st = vs.lib.vstab_pull_frame_p010_planar(h, oy.ptr, oy.pitch, ou.ptr, ou.pitch)
                get = lambda: (oy.host(np.uint16), ou.host(np.uint16))
            if st == vs.EOF:
                break
            assert st == vs.OK, vs.lib.vstab_last_error()
            R = np.zeros(9)
            assert vs.lib.vstab_get_warp_rotation(h, len(outs), vs._dptr(R)) == vs.OK
            outs.append((get(), R.reshape(3, 3)))
            torch.cuda.synchronize()
    finally:
        vs.lib.vstab_destroy(h)
    assert len(outs) == len(srcs) - 1
    return outs


@pytest.mark.parametrize("mem,hold,name", [(0, 1 << 29, "decoder"), (0, 0, "decoder"), (1, 0, "uv_wider"), (0, 1 << 29, "uv_narrower"),
                                           (0, 0, "chroma_first")])
def test_pipeline_with_decoder_style_frames(vs, cuda, mem, hold, name):
    """Frames whose chroma is not adjacent to luma (and whose pitches differ) borrowed in place (hold large), copied (hold 0), or in
    host memory: the BGR and plane-wise pulls are the warp of each frame under the rotation the handle reports."""
    W, H, n = 640, 360, 8
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = synth.shaky_clip(3, K, W, H, n, sigma=0.004)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    srcs = [layouts.place(f[:H], f[H:], name, cuda, host=mem == 1) for f in frames]
    for pulls in ("bgr", "planar"):
        for i, (o, R) in enumerate(run_pipeline(vs, cuda, srcs, mem, hold, pulls)):
            p = oracle.map_params(K, Ko, R)
            if pulls == "bgr":
                eq(o, expect.warp(frames[i + 1], p, cw, ch), (pulls, i))
            else:
                ey, euv = expect.warp_planar(frames[i + 1], p, cw, ch)
                eq(o[0], ey, (pulls, "y", i)), eq(o[1], euv, (pulls, "uv", i))


@pytest.mark.parametrize("name", ["decoder", "uv_wider", "uv_narrower"])
def test_pipeline_p010_frames_kept_forever_are_warped_in_place(vs, cuda, name):
    """pixel_depth 10 with HOLD_FOREVER: the warp reads upstream's 16-bit planes with their own pitches (S.pitch_uv16 = f.pitch_uv)."""
    W, H, n = 640, 360, 6
    K = oracle.get_preset_camera(4, W, H)
    frames8, _ = synth.shaky_clip(3, K, W, H, n, sigma=0.004)
    rng = np.random.default_rng(19)
    wide = [((f.astype(np.uint16) << 8) | (rng.integers(0, 256, f.shape, dtype=np.uint16))) for f in frames8]
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    srcs = [layouts.place(x[:H], x[H:], name, cuda) for x in wide]
    for blend in (0, 1):
        for pulls in ("p010_planar", "bgr16"):
            for i, (o, R) in enumerate(run_pipeline(vs, cuda, srcs, 0, 1 << 29, pulls, bit_depth=10, pixel_depth=10, blend=blend)):
                p = oracle.map_params(K, Ko, R)
                y, uv = wide[i + 1][:H], wide[i + 1][H:]
                if pulls == "bgr16":
                    eq(o, expect.warp_p010(y, uv, p, cw, ch, None, blend), (pulls, blend, i))
                else:
                    ey, euv = expect.warp_p010_planar(y, uv, p, cw, ch, None, blend)
                    eq(o[0], ey, (pulls, "y", blend, i)), eq(o[1], euv, (pulls, "uv", blend, i))
