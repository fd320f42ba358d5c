"""Frames past 4K, portrait frames and extreme aspect ratios through every operator of the tracker and the warp, bit for bit against the
oracle (and, for the default map arithmetic, the reference's own createMap kernel built for gfx950).  Frame shape changes the warp's XCD
band / tile schedule and the launchers' choices of tile height, LDS and tail (modelled on the CPU by test_tile_schedule_cpu.py, which
shows that the outputs below reach every branch), the detector's scratch and key buffer (an 8K noise frame overflows the fused pass's 2^18 keys
into the two-pass detector), the pyramid's tiles and k_pack_pyr's groups, and the level sizes LK works from.  Every frame is generated
once per module; warp outputs go into canaried planes, so a tile written past dw or dh fails."""
import numpy as np
import pytest

import layouts
import lk_segments as M
import oracle
import synth
from test_lk_segments_gpu import check_records
from test_p010_cpu import p010_frame

pytestmark = pytest.mark.gpu

# name: (source width, source height, camera preset)
SHAPES = {
    "gopro53_169": (5312, 2988, oracle.GOPRO_H4B_WIDE169_MEASURED),    # past-4K landscape: tail / rwb branches
    "gopro53_87": (5312, 4648, oracle.GOPRO_H4B_WIDE43_MEASURED),      # near-square, the largest GoPro mode
    "uhd8k": (7680, 4320, oracle.GOPRO_H4B_WIDE169_MEASURED),          # the biggest grids; noise content overflows the fused detector
    "portrait1080": (1080, 1920, oracle.GOPRO_H4B_WIDE169_MEASURED),   # h > w everywhere; 64 x 16 tiles with a tail
    "portrait4k": (2160, 3840, oracle.GOPRO_H4B_WIDE169_MEASURED),     # portrait past the small-frame bound
    "ultrawide": (5760, 1080, oracle.GOPRO_H4B_WIDE169_MEASURED),      # few tile rows, many columns
    "strip": (7680, 256, oracle.GOPRO_H4B_WIDE169_MEASURED),           # one or two half-tile rows per XCD band
    "tower": (256, 4096, oracle.GOPRO_H4B_WIDE169_MEASURED),           # 4 - 5 tile columns
}
# the stateless warps with an explicit output below 8 half-tile rows (empty XCD bands) and one 1 - 2 tile columns wide
STATELESS_OUTPUTS = [(4000, 40), (4000, 37), (96, 4000)]
SMALL_ROT, BIG_ROT = (0.02, -0.03, 0.01), (0.1, 0.75, 0.2)    # BIG_ROT: whole tiles of every output map outside the source
SHIFT = (2.6, -1.9)


def warp_output(name):
    w, h, preset = SHAPES[name]
    K = oracle.get_preset_camera(preset, w, h)
    return oracle.get_output_camera(K, w, h)[1]


def cams(name, rvec):
    w, h, preset = SHAPES[name]
    K = oracle.get_preset_camera(preset, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    return oracle.map_params(K, Ko, oracle.rodrigues(rvec)), cw, ch, K, Ko


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.fixture(scope="module")
def frames():
    """name -> packed NV12 frame, generated on first use and kept for the module."""
    cache = {}

    def get(name):
        if name not in cache:
            w, h, _ = SHAPES[name]
            cache[name] = synth.nv12(100 + list(SHAPES).index(name), w, h)
        return cache[name]
    return get


def luma(frame, name):
    return np.ascontiguousarray(frame[:SHAPES[name][1]])


# ---- pyramid --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_pyr_down_and_two_levels(vs, cuda, frames, name):
    g = luma(frames(name), name)
    e1 = oracle.pyr_down(g)
    assert np.array_equal(vs.pyr_down(dev(g, cuda)).cpu().numpy(), e1), name
    mid, dst = vs.pyr_down_x2(dev(g, cuda))
    assert np.array_equal(mid.cpu().numpy(), e1), (name, "first level")
    assert np.array_equal(dst.cpu().numpy(), oracle.pyr_down(e1)), (name, "second level")


@pytest.mark.parametrize("name", ["portrait1080", "portrait4k", "gopro53_169", "gopro53_87", "tower"])
def test_pack_pyr(vs, cuda, frames, name):
    """k_pack_pyr (ring copy of the packed frame and pyramid level 1 in one launch) on a frame pair of the shape, as
    test_lk_segments_gpu.py::test_pack_pyr runs it: ring = oracle.pack_nv12, canaries behind it untouched, level 1 = oracle.pyr_down,
    the pyramid and the records those of the plain path, the records the oracle's."""
    import torch
    f = frames(name)
    w, h, _ = SHAPES[name]
    g0 = luma(f, name)
    fr = [g0, synth.shifted(g0, *SHIFT)]
    pts = oracle.good_features(g0, 60, 0.01, 20.0)
    uvs = [f[h:], np.ascontiguousarray(f[h:][::-1])]
    nbytes = w * h * 3 // 2
    ys, uvd, rings = [], [], []
    for y, u in zip(fr, uvs):
        ybig = torch.zeros((h, w + 64), dtype=torch.uint8, device=cuda)
        ybig[:, :w] = dev(y, cuda)
        ys.append(ybig[:, :w])
        uvd.append(dev(u, cuda))
        rings.append(torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=cuda))
    hrec, drec, pyr = vs.lk_segments(ys, pts, [1], uv=uvd, rings=rings, want_pyr=True)
    plain_h, plain_d, plain_pyr = vs.lk_segments([dev(y, cuda) for y in fr], pts, [1], want_pyr=True)
    assert np.array_equal(hrec, plain_h) and np.array_equal(drec, plain_d) and np.array_equal(pyr, plain_pyr), name
    check_records(M.expected(fr, pts, [1]), hrec, drec, name)
    l1 = (w + 1) // 2 * ((h + 1) // 2)
    for i, (y, u) in enumerate(zip(fr, uvs)):
        rb = rings[i].cpu().numpy()
        assert np.array_equal(rb[:nbytes].reshape(h * 3 // 2, w), oracle.pack_nv12(y, u)), (name, i)
        assert (rb[nbytes:] == 0xA5).all(), (name, i, "canary")
        assert np.array_equal(pyr[i, :l1].reshape((h + 1) // 2, (w + 1) // 2), oracle.pyr_down(y)), (name, i)


# ---- detector -------------------------------------------------------------------------------------------------------------------------
def detector_input(frames, name):
    """The shape's luma; at uhd8k white noise instead, whose 3x3 maxima above the threshold outnumber the fused pass's 2^18 keys."""
    if name == "uhd8k":
        w, h, _ = SHAPES[name]
        return np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)
    return luma(frames(name), name)


@pytest.mark.parametrize("name", list(SHAPES))
def test_good_features_both_detectors(vs, cuda, frames, name):
    """Defaults (200 corners, 30 px apart) with both detectors, and every candidate in order (max_corners 4000, min_distance 0) on
    the portrait and 5.3K shapes.  Every shape asserts the path it took: the fused pass everywhere except uhd8k, where the fused pass
    overflows and the two-pass detector grows its key buffer and compacts again."""
    g = detector_input(frames, name)
    gd = dev(g, cuda)
    fused_path = vs.DETECTOR_TWO_PASS if name == "uhd8k" else vs.DETECTOR_FUSED
    runs = [(200, 30.0)] + ([(4000, 0.0)] if name in ("portrait1080", "gopro53_169", "tower") else [])
    for mc, md in runs:
        exp = oracle.good_features(g, mc, 0.01, md)
        assert len(exp) >= min(mc, 100), (name, len(exp))
        for det, used in ((vs.DETECTOR_AUTO, fused_path), (vs.DETECTOR_TWO_PASS, vs.DETECTOR_TWO_PASS)):
            info = {}
            got = vs.good_features(gd, mc, 0.01, md, detector=det, info=info)
            assert info["detector_used"] == used, (name, det, info)
            assert np.array_equal(got, exp), (name, det, mc, md, len(got), len(exp))
    if name == "uhd8k":   # the content's claim, on the oracle's side: more candidates than the key buffer holds
        assert len(oracle.good_features(g, 0, 0.01, 0.0)) > 1 << 18


@pytest.mark.parametrize("name", ["gopro53_169", "portrait1080"])
def test_min_eig(vs, cuda, frames, name):
    g = luma(frames(name), name)
    got = vs.min_eig(dev(g, cuda)).cpu().numpy()
    exp = oracle.min_eig(g)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (name, int((got != exp).sum()))


# ---- LK -------------------------------------------------------------------------------------------------------------------------------
def edge_points(w, h):
    """Points within the 21 x 21 window of every edge and corner of the frame, and two outside it."""
    xs, ys = (1.0, 4.5, 9.0, w / 3, w / 2 + 0.25, w - 10.0, w - 5.5, w - 2.0), (1.0, 4.5, 9.0, h / 3, h / 2 + 0.25, h - 10.0, h - 5.5, h - 2.0)
    pts = [(x, y) for x in xs for y in ys if min(x, w - 1 - x) < 11 or min(y, h - 1 - y) < 11]
    return np.array(pts + [(-30.0, 10.0), (w + 40.0, h + 40.0)], np.float32)


@pytest.mark.parametrize("name", list(SHAPES))
def test_pyr_lk(vs, cuda, frames, name):
    g0 = luma(frames(name), name)
    h, w = g0.shape
    g1 = synth.shifted(g0, *SHIFT)
    corners = oracle.good_features(g0)
    pts = np.concatenate([corners, edge_points(w, h)])
    got, gst = vs.pyr_lk(dev(g0, cuda), dev(g1, cuda), pts)
    exp, est = oracle.pyr_lk(g0, g1, pts)
    assert np.array_equal(gst, est), (name, np.nonzero(gst != est)[0][:5])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (name, int((got != exp).sum()))
    ok = est[:len(corners)] > 0
    assert ok.sum() > 0.7 * len(corners)
    assert np.abs(np.median((exp - pts)[:len(corners)][ok], axis=0) - SHIFT).max() < 0.1


# ---- warp, 8 bits ---------------------------------------------------------------------------------------------------------------------
def some_tile_outside(bgr):
    """True if a whole 64 x 16 tile of the expected output is black (its pixels all map outside the source)."""
    dh, dw = bgr.shape[:2]
    t = bgr[:dh // 16 * 16, :dw // 64 * 64].reshape(dh // 16, 16, dw // 64, 64 * 3)
    return bool((t.max(axis=(1, 3)) == 0).any())


@pytest.mark.parametrize("name", list(SHAPES))
def test_warp_fused_and_plane_wise(vs, cuda, frames, name):
    """The fused NV12 -> BGR warp and the plane-wise NV12 warp (IEEE map) at the shape's output camera, a small rotation and one that
    puts whole tiles outside the source (uhd8k: the large one only), into canaried planes."""
    f = frames(name)
    w, h, _ = SHAPES[name]
    src = layouts.place(f[:h], f[h:], "packed", cuda)
    for rv in ((BIG_ROT,) if name == "uhd8k" else (SMALL_ROT, BIG_ROT)):
        p, cw, ch, _, _ = cams(name, rv)
        exp = oracle.warp_nv12(f, p, cw, ch)
        assert rv != BIG_ROT or some_tile_outside(exp), (name, rv)
        got = layouts.warp_nv12(vs, src, p, cw, ch, vs.MAP_CREATEMAP_CL, vs.OUT_BGR8, cuda)
        assert np.array_equal(got, exp), (name, rv, int((got != exp).any(axis=2).sum()))
        gy, guv = layouts.warp_nv12(vs, src, p, cw, ch, vs.MAP_CREATEMAP_CL, vs.OUT_NV12_PLANAR, cuda)
        ey, euv = oracle.warp_nv12_planar(f, p, cw, ch, 0)
        assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (name, rv, int((gy != ey).sum()), int((guv != euv).sum()))


@pytest.mark.parametrize("dw,dh", STATELESS_OUTPUTS)
def test_stateless_warps_flat_and_narrow_outputs(vs, cuda, frames, dw, dh):
    """Outputs of 5 half-tile rows or fewer (three or more XCD bands empty, the last one cut by dh) and of 2 tile columns, looking at the
    centre of the ultrawide source: fused BGR, plane-wise NV12 and plane-wise P010 with both blends."""
    name = "ultrawide"
    f = frames(name)
    w, h, preset = SHAPES[name]
    K = oracle.get_preset_camera(preset, w, h)
    Ko, _ = oracle.get_output_camera(K, w, h)
    Ko = Ko.copy()
    Ko[0, 2], Ko[1, 2] = (dw - 1) / 2, (dh - 1) / 2
    p = oracle.map_params(K, Ko, oracle.rodrigues(SMALL_ROT))
    src = layouts.place(f[:h], f[h:], "packed", cuda)
    got = layouts.warp_nv12(vs, src, p, dw, dh, vs.MAP_CREATEMAP_CL, vs.OUT_BGR8, cuda)
    assert np.array_equal(got, oracle.warp_nv12(f, p, dw, dh)), (dw, dh)
    gy, guv = layouts.warp_nv12(vs, src, p, dw, dh, vs.MAP_CREATEMAP_CL, vs.OUT_NV12_PLANAR, cuda)
    ey, euv = oracle.warp_nv12_planar(f, p, dw, dh, 0)
    assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (dw, dh)
    y, uv, _, _ = p010_frame(7, w, h)
    s10 = layouts.place(y, uv, "packed", cuda)
    for blend in (0, 1):
        gy, guv = layouts.warp_p010_planes(vs, s10, p, dw, dh, 0, blend, cuda, planar=True)
        ey, euv = oracle.warp_p010_planar(y, uv, p, dw, dh, 0, None, blend)
        assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (dw, dh, blend)
        assert np.array_equal(layouts.warp_p010(vs, s10, p, dw, dh, 0, blend, cuda), oracle.warp_p010(y, uv, p, dw, dh, None, 0, blend)), (dw, dh, blend)


# ---- warp, 10 bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gopro53_169", "portrait1080"])
def test_warp_p010(vs, cuda, name):
    """The plane-wise P010 warp with both blends, and (portrait1080) the fused P010 -> BGR16 warp, into canaried planes."""
    w, h, _ = SHAPES[name]
    y, uv, _, _ = p010_frame(20 + list(SHAPES).index(name), w, h)
    src = layouts.place(y, uv, "packed", cuda)
    p, cw, ch, _, _ = cams(name, SMALL_ROT)
    for blend in (0, 1):
        gy, guv = layouts.warp_p010_planes(vs, src, p, cw, ch, 0, blend, cuda, planar=True)
        ey, euv = oracle.warp_p010_planar(y, uv, p, cw, ch, 0, None, blend)
        assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (name, blend, int((gy != ey).sum()), int((guv != euv).sum()))
        if name == "portrait1080":
            got = layouts.warp_p010(vs, src, p, cw, ch, 0, blend, cuda)
            assert np.array_equal(got, oracle.warp_p010(y, uv, p, cw, ch, None, 0, blend)), (name, blend)


# ---- default map arithmetic -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refcl(cuda):
    if not oracle.ref_gfx950_available():
        pytest.fail("oracle/_ref/createMap.gfx950.co or its launcher is missing (run `make -C oracle` where /root/reference exists)")
    return oracle.create_map_ref_gfx950


def same_bits(a, b):
    """Bit-identical, NaNs matching NaNs (a NaN's payload is not part of the contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.mark.parametrize("name", ["gopro53_87", "portrait1080"])
def test_default_map_is_the_reference_kernel(refcl, vs, cuda, frames, name):
    """MAP_CREATEMAP_CL_OPENCL: the map planes bit-identical to the reference's createMap kernel on this GPU, and the fused warp in that
    mode equal to that kernel's map followed by the oracle's cv::remap."""
    f = frames(name)
    fd = dev(f, cuda)
    bgr = oracle.cvt_nv12_bgr(f)
    for rv in (SMALL_ROT, BIG_ROT):
        p, cw, ch, _, _ = cams(name, rv)
        rx, ry = refcl(p, cw, ch)
        mx, my = vs.create_map(p, cw, ch, mode=vs.MAP_CREATEMAP_CL_OPENCL)
        assert same_bits(mx.cpu().numpy(), rx) and same_bits(my.cpu().numpy(), ry), (name, rv)
        exp = oracle.remap_bilinear(bgr, rx, ry)
        got = vs.warp_nv12(fd, p, cw, ch, mode=vs.MAP_CREATEMAP_CL_OPENCL).cpu().numpy()
        assert np.array_equal(got, exp), (name, rv, int((got != exp).any(axis=2).sum()))
