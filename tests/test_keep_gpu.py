"""GPU parity of the keep-edge warp (include/vstab.h "Keep edges") through the C ABI and the pipeline object: vstab_remap_bilinear_keep,
vstab_warp_nv12_keep (BGR8 and plane-wise NV12, with and without a rotation per output row), vstab_pull_frame_keep and
vstab_pull_frame_nv12_planar_keep.  Bar: every byte equals the numpy definition (tests/warp_def.py) fed by the oracle's maps -- the reference
kernel's own map, run on this GPU, for VSTAB_MAP_CREATEMAP_CL_OPENCL; prev and dst are planes of their own inside canaried buffers, or one
plane (in place); after a call with a separate prev, prev is unchanged."""
import ctypes

import numpy as np
import pytest

import expect
import layouts
import oracle
import synth
import warp_def as wd
import warp_tiles as wt

pytestmark = pytest.mark.gpu

ROT = (0.02, -0.03, 0.01)
PAST = (0.35, -0.25, 0.2)   # looks past the source: wide kept areas, tiles with no written sample
G = layouts.GUARD_ROWS


def cams(w, h, rvec=ROT, preset=4):
    K = oracle.get_preset_camera(preset, w, h)
    Ko, (dw, dh) = oracle.get_output_camera(K, w, h)
    return oracle.map_params(K, Ko, oracle.rodrigues(rvec)), dw, dh, K, Ko


def eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp).reshape(np.asarray(got).shape)
    assert np.array_equal(got, exp), (what, int((got != exp).sum()))


def map_modes():
    """Map modes 0..4, and 5 (the reference kernel's map, run on this GPU) where its code object is built."""
    return list(range(5)) + ([5] if oracle.ref_gfx950_available() else [])


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class Held:
    """A plane holding `data` (rows, row bytes) inside a canaried device buffer: GUARD_ROWS rows above and below, the bytes right of every
    row, and `offset` bytes in front.  pitch / offset choose the alignment (default: both 16-byte aligned, the 16-byte copy is taken)."""

    def __init__(self, data, cuda, pitch=None, offset=0):
        import torch
        data = np.ascontiguousarray(data, np.uint8)
        self.rows, self.rb = data.shape
        self.pitch = pitch or layouts._al(self.rb, 16) + 48
        self.off = offset + G * self.pitch
        self.buf = torch.full((offset + (self.rows + 2 * G) * self.pitch,), layouts.CANARY, dtype=torch.uint8, device=cuda)
        layouts._rows_into(self.buf, self.off, self.pitch, data)
        self.ptr = self.buf.data_ptr() + self.off

    def host(self):
        """-> the plane's bytes, after checking every byte of the buffer outside it."""
        a = self.buf.cpu().numpy()
        body = a[self.off - G * self.pitch:].reshape(self.rows + 2 * G, self.pitch)
        bad = int((a[:self.off - G * self.pitch] != layouts.CANARY).sum() + (body[:G] != layouts.CANARY).sum() + (body[G + self.rows:] != layouts.CANARY).sum()
                  + (body[G:G + self.rows, self.rb:] != layouts.CANARY).sum())
        assert bad == 0, f"{bad} bytes written outside the plane"
        return np.ascontiguousarray(body[G:G + self.rows, :self.rb])


def history(seed, dw, dh):
    """Random frames to keep: BGR (dh, 3 dw), luma (dh, dw), chroma (ceil(dh / 2), 2 ceil(dw / 2))."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (dh, 3 * dw), dtype=np.uint8), rng.integers(0, 256, (dh, dw), dtype=np.uint8),
            rng.integers(0, 256, ((dh + 1) // 2, 2 * ((dw + 1) // 2)), dtype=np.uint8))


def warp_keep(vs, s, params, dw, dh, mode, fmt, prev, dst, rot_bottom=None):
    """vstab_warp_nv12_keep on layouts.Src s; prev, dst: Held planes (BGR) or pairs of them (plane-wise); dst may be prev."""
    p, pp = layouts._f(params)
    rb, rbp = layouts._f(np.asarray(rot_bottom).reshape(9)) if rot_bottom is not None else (None, None)
    if fmt == vs.OUT_BGR8:
        layouts._call(vs, "vstab_warp_nv12_keep", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, rbp, int(mode), int(fmt), prev.ptr, prev.pitch, None, 0,
                      dst.ptr, dst.pitch, None, 0, dw, dh, vs._stream())
    else:
        layouts._call(vs, "vstab_warp_nv12_keep", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, rbp, int(mode), int(fmt), prev[0].ptr, prev[0].pitch,
                      prev[1].ptr, prev[1].pitch, dst[0].ptr, dst[0].pitch, dst[1].ptr, dst[1].pitch, dw, dh, vs._stream())


def check_warp(vs, cuda, s, f, p, dw, dh, mode, what, rot_bottom=None, seed=1, place=None, formats=("bgr", "planar"), ways=("separate", "in_place")):
    """BGR and plane-wise keep warps of Src s (packed NV12 f on the host), prev separate and in place, against the definition (computed
    once per format).  place(data, role) -> Held chooses the layout of a plane (role 'prev' or 'dst'); default aligned planes."""
    place = place or (lambda data, role: Held(data, cuda))
    pb, py, puv = history(seed, dw, dh)
    other = lambda a: np.full_like(a, 0x3C)   # what dst holds before a call with a separate prev: every byte must be overwritten
    if "bgr" in formats:
        exp = wd.bgr(f, *wd.maps(p, dw, dh, mode, rot_bottom), "linear", wd.TRANSPARENT, pb)
        assert not np.array_equal(exp.reshape(pb.shape), pb), (what, "nothing written")
        for way in ways:
            prev = place(pb, "prev")
            dst = prev if way == "in_place" else place(other(pb), "dst")
            warp_keep(vs, s, p, dw, dh, mode, vs.OUT_BGR8, prev, dst, rot_bottom)
            eq(dst.host(), exp, (what, "bgr", mode, way))
            if way == "separate":
                eq(prev.host(), pb, (what, "bgr prev", mode))
    if "planar" in formats:
        ey, euv = wd.planar(f, *wd.maps(p, dw, dh, mode, rot_bottom), "linear", wd.TRANSPARENT, py, puv)
        for way in ways:
            prev = (place(py, "prev"), place(puv, "prev"))
            dst = prev if way == "in_place" else (place(other(py), "dst"), place(other(puv), "dst"))
            warp_keep(vs, s, p, dw, dh, mode, vs.OUT_NV12_PLANAR, prev, dst, rot_bottom)
            eq(dst[0].host(), ey, (what, "luma", mode, way)), eq(dst[1].host(), euv, (what, "chroma", mode, way))
            if way == "separate":
                eq(prev[0].host(), py, (what, "luma prev", mode)), eq(prev[1].host(), puv, (what, "chroma prev", mode))


# ---- the stateless remap ------------------------------------------------------------------------------------------------------------
def remap_keep(vs, cuda, src, mx, my, prev, in_place):
    """vstab_remap_bilinear_keep with canaried planes -> (output, prev afterwards), each (dh, dw[, cn])."""
    s = dev(src, cuda)
    cn = 1 if src.ndim == 2 else src.shape[2]
    dh, dw = mx.shape
    mxt, myt = dev(mx, cuda), dev(my, cuda)
    pv = Held(prev.reshape(dh, dw * cn), cuda)
    o = pv if in_place else Held(np.full((dh, dw * cn), 0x3C, np.uint8), cuda)
    layouts._call(vs, "vstab_remap_bilinear_keep", s.data_ptr(), s.stride(0), src.shape[1], src.shape[0], cn, mxt.data_ptr(), mxt.stride(0) * 4,
                  myt.data_ptr(), myt.stride(0) * 4, pv.ptr, pv.pitch, o.ptr, o.pitch, dw, dh, vs._stream())
    return o.host().reshape(prev.shape), pv.host().reshape(prev.shape)


def check_remap(vs, cuda, src, mx, my, prev, what):
    exp = wd.remap(src, mx, my, "linear", wd.TRANSPARENT, 0, prev)
    out, after = remap_keep(vs, cuda, src, mx, my, prev, False)
    eq(out, exp, (what, "separate")), eq(after, prev, (what, "prev"))
    out, _ = remap_keep(vs, cuda, src, mx, my, prev, True)
    eq(out, exp, (what, "in place"))


def test_remap_keep_golden_vectors(vs, cuda):
    import test_keep_cpu
    n = 0
    for k, src, mx, my, prev, out in test_keep_cpu.golden_cases():
        assert np.array_equal(wd.remap(src, mx, my, "linear", wd.TRANSPARENT, 0, prev), out)
        check_remap(vs, cuda, src, mx, my, prev, k)
        n += 1
    assert n == 9


def test_remap_keep_random_maps_every_channel_count(vs, cuda):
    rng = np.random.default_rng(11)
    for sw, sh, dw, dh in ((1, 1, 9, 5), (2, 2, 33, 7), (37, 23, 70, 9), (300, 170, 333, 190)):
        for cn in (1, 2, 3):
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            prev = rng.integers(0, 256, (dh, dw, cn) if cn > 1 else (dh, dw), dtype=np.uint8)
            mx = rng.uniform(-0.5 * sw - 2, 1.5 * sw + 2, (dh, dw)).astype(np.float32)
            my = rng.uniform(-0.5 * sh - 2, 1.5 * sh + 2, (dh, dw)).astype(np.float32)
            ties = ((rng.integers(-64, 32 * sw + 64, (dh, dw)) + 0.5) / 32.0).astype(np.float32)
            sel = rng.random((dh, dw)) < 0.2
            mx[sel] = ties[sel]
            special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 32768.0, -32768.0, -0.0], np.float32)
            for m in (mx, my):
                pick = rng.random((dh, dw)) < 0.05
                m[pick] = rng.choice(special, int(pick.sum()))
            check_remap(vs, cuda, src, mx, my, prev, (sw, sh, cn))


@pytest.mark.parametrize("sw", [5, 64])
def test_remap_keep_sweeps_every_position(vs, cuda, sw):
    """X over all of [-32768, 32767] (four rows of 16384), fx = 13 / 32, and the same sweep with fx = 0 (exact hits): written for X in
    [0, sw - 2] alone, whatever the fraction."""
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (3, sw, 3), dtype=np.uint8)
    X = np.arange(-32768, 32768, dtype=np.int64).reshape(4, 16384)
    prev = rng.integers(0, 256, X.shape + (3,), dtype=np.uint8)
    for fx in (13, 0):
        mx = ((X * 32 + fx) / 32.0).astype(np.float32)
        for my in (np.full(mx.shape, 1.25, np.float32), np.full(mx.shape, 0.5, np.float32), np.full(mx.shape, 2.0, np.float32)):
            m = wd.written(mx, my, sw, 3)
            assert int(m.sum()) == (0 if my[0, 0] == 2.0 else sw - 1)
            check_remap(vs, cuda, src, mx, my, prev, (sw, fx, float(my[0, 0])))


def test_remap_keep_binding(vs, cuda):
    rng = np.random.default_rng(13)
    src = rng.integers(0, 256, (21, 33, 2), dtype=np.uint8)
    prev = rng.integers(0, 256, (12, 40, 2), dtype=np.uint8)
    mx, my = rng.uniform(-10, 43, (12, 40)).astype(np.float32), rng.uniform(-8, 29, (12, 40)).astype(np.float32)
    exp = wd.remap(src, mx, my, "linear", wd.TRANSPARENT, 0, prev)
    pv = dev(prev, cuda)
    eq(vs.remap_bilinear_keep(dev(src, cuda), dev(mx, cuda), dev(my, cuda), pv).cpu().numpy(), exp, "binding")
    eq(pv.cpu().numpy(), prev, "binding prev")
    assert vs.remap_bilinear_keep(dev(src, cuda), dev(mx, cuda), dev(my, cuda), pv, out=pv) is pv
    eq(pv.cpu().numpy(), exp, "binding in place")


# ---- the warp: every map mode, both formats, prev separate and in place --------------------------------------------------------------
@pytest.mark.parametrize("rv", [ROT, PAST])
def test_warp_keep_every_map_mode(vs, cuda, rv):
    w, h = 256, 144
    f = synth.nv12(31, w, h, full_range=True)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    p, dw, dh, K, Ko = cams(w, h, rv)
    assert (dw, dh) == (230, 131)
    for mode in map_modes():
        check_warp(vs, cuda, s, f, p, dw, dh, mode, ("modes", rv), seed=mode)


def test_warp_keep_rotation_per_row(vs, cuda):
    w, h = 256, 144
    f = synth.nv12(32, w, h)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    p, dw, dh, K, Ko = cams(w, h, PAST)
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.38, -0.2, 0.26)))[8:]
    for mode in [m for m in map_modes() if m in (0, 1, 5)]:
        check_warp(vs, cuda, s, f, p, dw, dh, mode, "rs", rot_bottom=rb)
    pb, _, _ = history(1, dw, dh)
    for mode in (2, 3, 4):
        prev = Held(pb, cuda)
        with pytest.raises(vs.VstabError):
            warp_keep(vs, s, p, dw, dh, mode, vs.OUT_BGR8, prev, prev, rb)
        assert vs.lib.vstab_last_error().endswith(b"a rotation per output row (rot_bottom) is served for map modes 0, 1 and 5")
        eq(prev.host(), pb, ("refused", mode))


def test_warp_keep_binding(vs, cuda):
    w, h = 128, 72
    f = synth.nv12(34, w, h)
    p, dw, dh, K, Ko = cams(w, h, PAST)
    pb, py, puv = history(2, dw, dh)
    got = vs.warp_nv12_keep(dev(f, cuda), p, dw, dh, dev(pb.reshape(dh, dw, 3), cuda)).cpu().numpy()
    eq(got, wd.bgr(f, *wd.maps(p, dw, dh), "linear", wd.TRANSPARENT, pb), "binding bgr")
    prev = (dev(py, cuda), dev(puv, cuda))
    y, uv = vs.warp_nv12_keep(dev(f, cuda), p, dw, dh, prev, 1, vs.OUT_NV12_PLANAR, rot_bottom=p[8:], out=prev)
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, 1, p[8:]), "linear", wd.TRANSPARENT, py, puv)
    assert y is prev[0] and uv is prev[1]
    eq(y.cpu().numpy(), ey, "binding y"), eq(uv.cpu().numpy(), euv, "binding uv")


# ---- tile and layout paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wt.TILE_SETS["keep"]))
def test_keep_tile_sets(vs, cuda, name):
    """The sets of tests/warp_tiles.py for k_warp_keep: tiles with no written sample, written throughout, mixed; staged and gathered; cut by
    the image's edges."""
    p, sw, sh, dw, dh, mode = wt.set_params("keep", name)
    f = synth.nv12(sum(map(ord, name)), sw, sh, full_range=True)
    s = layouts.place(f[:sh], f[sh:], "packed", cuda)
    check_warp(vs, cuda, s, f, p, dw, dh, mode, name)


def test_keep_axis_pixel_is_kept(vs, cuda):
    """Map mode 0 with the identity rotation and the principal point on a pixel: that pixel's 0/0 quantises to X = Y = -32768 and is kept;
    it gives no anchor to its tile's box."""
    w, h = 256, 144
    f = synth.nv12(35, w, h)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    K = oracle.get_preset_camera(4, w, h)
    Ko = np.array([[100.0, 0, 64.0], [0, 100.0, 40.0], [0, 0, 1]])
    p = oracle.map_params(K, Ko, np.eye(3))
    mx, my = oracle.create_map_ex(p, 130, 70, 0)
    assert np.isnan(mx[40, 64]) and not wd.written(mx, my, w, h)[40, 64]
    check_warp(vs, cuda, s, f, p, 130, 70, 0, "axis")


@pytest.mark.parametrize("name", layouts.LAYOUTS)
def test_keep_every_source_layout(vs, cuda, name):
    w, h = 256, 144
    p, dw, dh, _, _ = cams(w, h, PAST)
    f = synth.nv12(36, w, h)
    s = layouts.place(f[:h], f[h:], name, cuda)
    check_warp(vs, cuda, s, f, p, dw, dh, 0, name)


@pytest.mark.parametrize("what", ["odd_pitches", "odd_prev", "odd_dst", "odd_both"])
def test_keep_odd_pitches_and_addresses(vs, cuda, what):
    """prev and dst at odd pitches and odd byte addresses: a tile with no written sample copies byte by byte unless both planes and both
    pitches are 16-byte aligned.  Odd output sizes: chroma has ceil(dw / 2) pairs in ceil(dh / 2) rows."""
    w, h = 256, 144
    p, dw, dh, _, _ = cams(w, h, PAST)
    dw, dh = dw - 1, dh - 2
    assert dw % 2 == 1 and dh % 2 == 1
    f = synth.nv12(37, w, h)
    s = layouts.place(f[:h], f[h:], None, cuda, spec=(w + 3, w + 6, "two", 1, 2))

    def place(data, role):
        rb = data.shape[1]
        if what == "odd_pitches":
            return Held(data, cuda, pitch=rb + (7 if role == "prev" else 13))
        odd = what == "odd_both" or what == "odd_" + role
        return Held(data, cuda, offset=5 if odd else 0)
    check_warp(vs, cuda, s, f, p, dw, dh, 0, what, place=place)


def test_keep_smallest_source_keeps_all_chroma(vs, cuda):
    """A 2 x 2 source: one luma footprint, and a 1 x 1 chroma plane, which keeps everything."""
    f = np.random.default_rng(38).integers(0, 256, (3, 2), dtype=np.uint8)
    s = layouts.place(f[:2], f[2:], "packed", cuda)
    Ki = np.array([[40.0, 0, 0.5], [0, 40.0, 0.5], [0, 0, 1]])
    Ko = np.array([[100.0, 0, 35.0], [0, 100.0, 10.0], [0, 0, 1]])
    p = oracle.map_params(Ki, Ko, np.eye(3))
    mx, my = wd.maps(p, 70, 21, 3)
    my_, mc = wd.written(mx, my, 2, 2), wd.written(*oracle.chroma_maps(mx, my), 1, 1)
    assert my_.any() and not my_.all() and not mc.any()
    check_warp(vs, cuda, s, f, p, 70, 21, 3, "2x2")


def test_keep_4k_config3_shape_in_place(vs, cuda):
    w, h = 3840, 2160
    f = synth.nv12(77, w, h)
    p, dw, dh, _, _ = cams(w, h, (0.01, -0.02, 0.015))
    assert (dw, dh) == (3524, 1999)
    s = layouts.place(f[:h], f[h:], "packed", cuda)
    check_warp(vs, cuda, s, f, p, dw, dh, 0, "4k", ways=("in_place",))


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
W, H = 640, 360


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames, _ = synth.shaky_clip(5, K, W, H, 7, sigma=0.02)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    return K, Ko, cw, ch, frames


def stabilizer(vs, cuda, frames, **cfg):
    import torch
    cfg.setdefault("smooth_radius", 2)
    return vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), **cfg)


def keep_pull(stab, cuda, planar, bufs, i, ring):
    """Frame i by a keep pull: ring: into bufs[i % 2] with bufs[(i + 1) % 2] as prev; else in place in bufs[0].  -> the output on the host."""
    dst = bufs[i % 2] if ring else bufs[0]
    prev = bufs[(i + 1) % 2] if ring else bufs[0]
    ok = stab.pull_nv12_planar_keep_into(dst[0], dst[1], prev[0], prev[1]) if planar else stab.pull_keep_into(dst, prev)
    assert ok
    return tuple(x.cpu().numpy() for x in dst) if planar else dst.cpu().numpy()


def first_history(cuda, cw, ch, planar):
    pb, py, puv = history(9, cw, ch)
    mk = (lambda: (dev(py, cuda), dev(puv, cuda))) if planar else (lambda: dev(pb.reshape(ch, cw, 3), cuda))
    return [mk(), mk()], ((py, puv) if planar else pb.reshape(ch, cw, 3))


def expect_keep(f, K, Ko, R, cw, ch, last, planar, mode=0, rot_bottom=None):
    p = oracle.map_params(K, Ko, R)
    if planar:
        return wd.planar(f, *wd.maps(p, cw, ch, mode, rot_bottom), "linear", wd.TRANSPARENT, last[0], last[1])
    return wd.bgr(f, *wd.maps(p, cw, ch, mode, rot_bottom), "linear", wd.TRANSPARENT, last)


def same(out, exp, planar, what):
    if planar:
        eq(out[0], exp[0], (what, "y")), eq(out[1], exp[1], (what, "uv"))
    else:
        eq(out, exp, what)


@pytest.mark.parametrize("tracking", [1, 0])
@pytest.mark.parametrize("planar", [False, True])
def test_pipeline_keep_pulls(vs, cuda, clip, planar, tracking):
    """A ring of two outputs, then the same stream in place: frame i is where(mask_i, warp(frame, warp_rotation(i)), frame i - 1), from a
    pattern-filled first prev.  Tracking off repeats the parameters frame after frame: no keep pull touches the quantised map."""
    K, Ko, cw, ch, frames = clip
    for ring in (True, False):
        stab = stabilizer(vs, cuda, frames, tracking=tracking, map_precision=expect.IEEE)
        bufs, last = first_history(cuda, cw, ch, planar)
        for i in range(len(frames) - 1):
            out = keep_pull(stab, cuda, planar, bufs, i, ring)
            last = expect_keep(frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, last, planar)
            same(out, last, planar, ("ring" if ring else "in place", tracking, i))
        assert stab.warps_from_cache() == 0
        assert not (stab.pull_nv12_planar_keep_into(*bufs[0], *bufs[1]) if planar else stab.pull_keep_into(bufs[0], bufs[1]))   # end of stream
        stab.close()


def test_pipeline_keep_and_plain_pulls_alternate(vs, cuda, clip):
    """Tracking off: the plain BGR pulls come from the cached quantised map from their second frame on, exactly as without keep pulls
    between them -- a keep pull neither reads nor updates that state."""
    K, Ko, cw, ch, frames = clip
    stab = stabilizer(vs, cuda, frames, tracking=0, map_precision=expect.IEEE)
    bufs, last = first_history(cuda, cw, ch, False)
    cached = []
    for i in range(len(frames) - 1):
        if i % 2 == 0:
            out = stab.pull().cpu().numpy()
            eq(out, expect.warp(frames[i + 1], oracle.map_params(K, Ko, stab.warp_rotation(i)), cw, ch, expect.IEEE), ("plain", i))
            bufs[0].copy_(dev(out, cuda))
            last = out
        else:
            before = stab.warps_from_cache()
            out = keep_pull(stab, cuda, False, bufs, 0, False)
            last = expect_keep(frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, last, False)
            eq(out, last, ("keep", i))
            assert stab.warps_from_cache() == before
        cached.append(stab.warps_from_cache())
    assert cached == [0, 0, 1, 1, 2, 2], cached      # plain pulls 0, 2, 4: the second writes the map down and reads it, the third reads it
    stab.close()


def test_pipeline_keep_readout_rotations(vs, cuda, clip):
    """Frames with read-out rotations (map mode 0): the keep warp takes the rotation of the last output row, readout * W."""
    K, Ko, cw, ch, frames = clip
    ro = [oracle.rodrigues((0.002 * (k % 3), -0.003, 0.001 * k)) for k in range(len(frames))]
    for planar in (False, True):
        stab = stabilizer(vs, cuda, frames, smooth_radius=1, tracking=0, readouts=ro, map_precision=expect.IEEE)
        bufs, last = first_history(cuda, cw, ch, planar)
        for i in range(4):
            out = keep_pull(stab, cuda, planar, bufs, i, True)
            W_rot = stab.warp_rotation(i)
            rb = oracle.map_params(K, Ko, ro[i + 1] @ W_rot)[8:]
            last = expect_keep(frames[i + 1], K, Ko, W_rot, cw, ch, last, planar, rot_bottom=rb)
            same(out, last, planar, ("readout", i))
        stab.close()


def test_pipeline_keep_default_precision(vs, cuda, clip):
    """The handle's default map arithmetic (the reference kernel's, map mode 5)."""
    if not oracle.ref_gfx950_available():
        pytest.skip("oracle/_ref/createMap.gfx950.co not built")
    K, Ko, cw, ch, frames = clip
    for planar in (False, True):
        stab = stabilizer(vs, cuda, frames[:5])
        bufs, last = first_history(cuda, cw, ch, planar)
        for i in range(4):
            out = keep_pull(stab, cuda, planar, bufs, i, i < 2)
            last = expect_keep(frames[i + 1], K, Ko, stab.warp_rotation(i), cw, ch, last, planar, mode=5)
            same(out, last, planar, ("default", i))
            if i == 1:       # from the ring to in place: the history moves into bufs[0]
                for a, b in zip(bufs[0] if planar else [bufs[0]], bufs[1] if planar else [bufs[1]]):
                    a.copy_(b)
        stab.close()


def test_pipeline_keep_refusals(vs, cuda, clip):
    """Every refusal comes before a frame is dequeued: after it the whole stream is delivered by plain pulls, frame for frame."""
    import torch
    K, Ko, cw, ch, frames = clip
    fr = frames[:4]
    out, prev = torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda), torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda)
    y, uv = vs.nv12_out_planes(cw, ch)
    py, puv = vs.nv12_out_planes(cw, ch)
    L = vs.lib
    bgr = lambda h, dst=out, pv=prev, pitch=None: L.vstab_pull_frame_keep(h, dst.data_ptr(), dst.stride(0), pv.data_ptr(), pv.stride(0) if pitch is None else pitch)
    nv = lambda h, a=py, b=puv: L.vstab_pull_frame_nv12_planar_keep(h, y.data_ptr(), y.stride(0), uv.data_ptr(), uv.stride(0), a.data_ptr(), a.stride(0),
                                                                    b.data_ptr(), b.stride(0))
    alias = ": prev must be dst itself (same pointer and pitch, every plane) or must not overlap it"
    ieee = dict(tracking=0, map_precision=expect.IEEE)
    first = lambda stab: oracle.map_params(K, Ko, stab.warp_rotation(0))
    table = [
        (dict(resample=vs.RESAMPLE_CUBIC, **ieee), None, vs.ERR_UNSUPPORTED, ": VSTAB_RESAMPLE_CUBIC has no keep-edge warp",
         lambda stab: wd.bgr(fr[1], *wd.maps(first(stab), cw, ch), "cubic")),
        (dict(resample=vs.RESAMPLE_LANCZOS4), None, vs.ERR_UNSUPPORTED, ": VSTAB_RESAMPLE_LANCZOS4 has no keep-edge warp", None),
        (dict(interpolation=0), None, vs.ERR_UNSUPPORTED, ": INTER_NEAREST has no keep-edge warp", None),
        (dict(border_mode=vs.BORDER_REFLECT_101, **ieee), None, vs.ERR_UNSUPPORTED,
         ": a border mode other than VSTAB_BORDER_CONSTANT is in force (vstab_set_border_mode)",
         lambda stab: wd.bgr(fr[1], *wd.maps(first(stab), cw, ch, 0), "linear", wd.REFLECT_101)),
        (dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=cw, out_height=ch, calibration=(None, 0)),
         None, vs.ERR_UNSUPPORTED, ": a calibrated handle (vstab_set_input_calibration) has no keep-edge warp", None),
        (ieee, "pitch", vs.ERR_INVALID, ": prev pitch smaller than row", lambda stab: expect.warp(fr[1], first(stab), cw, ch, expect.IEEE)),
        (ieee, "alias", vs.ERR_INVALID, alias, lambda stab: expect.warp(fr[1], first(stab), cw, ch, expect.IEEE)),
    ]
    for cfg, how, status, text, exp in table:
        stab = stabilizer(vs, cuda, fr, smooth_radius=1, **cfg)
        for fn, call in (("vstab_pull_frame_keep", bgr), ("vstab_pull_frame_nv12_planar_keep", nv)):
            if how == "pitch":
                got = bgr(stab._h, pitch=3 * cw - 1) if call is bgr else L.vstab_pull_frame_nv12_planar_keep(
                    stab._h, y.data_ptr(), y.stride(0), uv.data_ptr(), uv.stride(0), py.data_ptr(), py.stride(0), puv.data_ptr(), 2 * ((cw + 1) // 2) - 1)
            elif how == "alias":
                got = bgr(stab._h, pv=out[1:]) if call is bgr else nv(stab._h, a=y)     # BGR: prev one row into dst; planes: luma in place, chroma not
            else:
                got = call(stab._h)
            assert got == status and L.vstab_last_error() == (fn + text).encode(), (cfg, fn, L.vstab_last_error())
        outs = []
        while True:
            o = stab.pull()
            if o is None:
                break
            outs.append(o.cpu().numpy())
        assert len(outs) == len(fr) - 1, cfg                 # no frame was consumed by a refusal
        if exp is not None:
            eq(outs[0], exp(stab), ("after refusal", cfg))
        stab.close()
    p16 = [torch.from_numpy((f.astype(np.uint16) << 8).view(np.int16)).to(cuda) for f in fr]
    stab = vs.Stabilizer(p16, total=len(fr), smooth_radius=1, bit_depth=10, pixel_depth=10)
    for call in (bgr, nv):
        assert call(stab._h) == vs.ERR_INVALID and L.vstab_last_error().startswith(b"vstab_pull_frame: a pixel_depth 10 handle"), L.vstab_last_error()
    o16 = torch.zeros((ch, cw, 3), dtype=torch.int16, device=cuda)
    n = 0
    while stab.pull_bgr16_into(o16):
        n += 1
    assert n == len(fr) - 1
    stab.close()
